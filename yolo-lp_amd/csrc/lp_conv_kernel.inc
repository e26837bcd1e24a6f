// Implicit-GEMM convolution for gfx950 (MI355X): NHWC activations, im2col-free, MFMA 32x32 tiles.
//
// GEMM view (per output tile):   D[cout][pixel] = sum_{tap, cin} Wp[tap][cout][cin] * X[pixel + tap][cin]
//   A operand = weights  (rows = output channels, K contiguous)
//   B operand = pixels   (cols = output pixels,   K = input channels, contiguous in NHWC)
// so the accumulator fragment of a lane holds 4 consecutive output channels of ONE pixel per register
// quad, which packs into 8-/16-byte LDS writes and comes back out as whole NHWC rows (16-B stores).
//
// Per K-chunk (KC input channels of one concat source) a workgroup stages
//   - the input halo of its TH x TW output tile  ( ((TH-1)S+KS) x ((TW-1)S+KS) pixels x KC )  and
//   - the weights of all KS*KS taps for its CB output channels ( KS*KS*CB x KC )
// in LDS (rows padded by one 16-B granule: conflict-free ds_read_b128 for the 32x32 operand maps), and
// every wave reads its A/B fragments from there for all taps: the halo is fetched once from HBM/L2 and
// reused 9x (no im2col buffer anywhere).  The next chunk's global loads are issued into registers before
// the MFMAs of the current chunk (issue-early / write-late staging).
//
// Concat inputs (BiFusion, SPPF, PAN, BepC3) are read straight from up to 4 source tensors: a K-chunk
// belongs to exactly one source, so torch.cat is never materialised.
//
// Epilogues:  MODE_ACT    bias + {none,ReLU,SiLU} (+ alpha*residual) -> NHWC activation dtype
//             MODE_PRED   bias + sigmoid -> fp32 columns [13, 13+n) of the [B,N,290] prediction tensor
//             MODE_DECODE bias (+ DFL softmax projection) + anchor-free decode -> fp32 columns [0,13)
//
// Reference semantics: RepVGGBlock deploy / Conv / SimConv forward_fuse (yolov6/layers/common.py:41-66,
// 258-259), Transpose (:186-187), Detect.forward eval (yolov6/models/effidehead.py:214-301), dist2bbox /
// dist2cor (yolov6/utils/general.py:29-66), generate_anchors (yolov6/assigners/anchor_generator.py:11-31).
#pragma once
#include "lp_internal.h"

namespace lp {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// One "K-block" is the 32 bytes of a row that one lane pair (lane, lane+32) consumes with one 16-B read
// each: 16 channels of a 16-bit type (one 32x32x16 MFMA) or 8 fp32 channels (four 32x32x2 MFMAs, lane half
// h taking channels 4h..4h+3 -- A and B use the same assignment, so the sum over K is complete).
template <typename T> struct Mma;
template <> struct Mma<f16> {
    typedef f16x8 V;
    static __device__ __forceinline__ f32x16 mma(V a, V b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mma<bf16> {
    typedef bf16x8 V;
    static __device__ __forceinline__ f32x16 mma(V a, V b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    typedef f32x4 V;
    static __device__ __forceinline__ f32x16 mma(V a, V b, f32x16 c) {
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], c, 0, 0, 0);
        return c;
    }
};

template <int CFG> struct Cfg;
template <> struct Cfg<CFG_A> { static constexpr int WC = 2, WP = 2, WGC = 2, WGP = 2; };
template <> struct Cfg<CFG_B> { static constexpr int WC = 2, WP = 2, WGC = 1, WGP = 4; };
template <> struct Cfg<CFG_C> { static constexpr int WC = 1, WP = 2, WGC = 1, WGP = 4; };
template <> struct Cfg<CFG_D> { static constexpr int WC = 2, WP = 2, WGC = 2, WGP = 4; };  // 8 waves: 128 couts x 256 px
template <> struct Cfg<CFG_E> { static constexpr int WC = 1, WP = 2, WGC = 2, WGP = 2; };  // 4 waves of 32 couts x 64 px: small footprint, more workgroups per CU
template <> struct Cfg<CFG_F> { static constexpr int WC = 1, WP = 2, WGC = 4, WGP = 2; };  // 8 waves of 32 x 64: 128 couts x 128 px with twice the waves of A

// LDS rows are unpadded (32 B for 3x3 chunks, 128 B for 1x1 chunks) because they are filled by LDS-DMA
// (global_load_lds_dwordx4: a wave writes 64 x 16 B contiguously); bank conflicts of the ds_read_b128 fragment
// reads are removed by an XOR swizzle of the 16-B granule position inside a row, applied to the SOURCE address
// of the DMA (weights: pre-swizzled when packed on the host) and again on the read.
__host__ __device__ __forceinline__ constexpr int swz(int row, int g, int gpr) {
    return gpr == 2 ? (g ^ ((row >> 3) & 1)) : (g ^ ((row >> 1) & 7));
}

template <typename T, int CFG, int KS, int S, int MODE, int NBUF> struct Geo {
    typedef Cfg<CFG> C;
    static constexpr int SZ = sizeof(T);
    static constexpr int EPG = 16 / SZ;                     // elements per 16-B granule
    static constexpr int KC = (KS == 1) ? 128 / SZ : 32 / SZ;  // channels per K-chunk: 1x1 -> 128 B rows, 3x3 -> 32 B rows
    static constexpr int GPR = KC / EPG;                    // granules per row (8 or 2)
    static constexpr int ROWB = KC * SZ;                    // LDS row bytes
    static constexpr int NKB = KC * SZ / 32;                // K-blocks per chunk
    static constexpr int NW = C::WGC * C::WGP;              // waves
    static constexpr int NT = 64 * NW;
    static constexpr int CB = 32 * C::WC * C::WGC;
    static constexpr int PB = 32 * C::WP * C::WGP;
    static constexpr int HPMAX = (KS == 1) ? PB : (S == 1 ? 2 * PB + 128 : 5 * PB + 128);  // halo pixels incl. pitch padding
    static constexpr int WROWS = KS * KS * CB;
    static constexpr int HS = HPMAX * GPR;                  // halo slots (16-B granules); multiple of 64
    static constexpr int WS = WROWS * GPR;                  // weight slots; multiple of 64
    static constexpr int NHI = (HS / 64 + NW - 1) / NW;     // halo DMA instructions per wave per chunk (max)
    static constexpr int NWI = (WS / 64 + NW - 1) / NW;     // weight DMA instructions per wave per chunk
    static constexpr int LDS_MAIN = (HPMAX + WROWS) * ROWB;
    static constexpr int OSZ = (MODE == MODE_ACT) ? SZ : 4;  // staged output element size
    static constexpr int STGB = CB * OSZ + 16;               // staging row bytes
    static constexpr int LDS_STG = PB * STGB;
    static constexpr int LDS = NBUF * LDS_MAIN > LDS_STG ? NBUF * LDS_MAIN : LDS_STG;
    static_assert(HS % 64 == 0 && WS % 64 == 0, "DMA instructions must not straddle the halo/weight regions");
    static_assert(LDS <= 160 * 1024, "LDS budget");
};

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

// Activation of the epilogue as a compile-time choice: the kernels branch ONCE per tile on the (uniform) runtime code and
// run a specialised copy of the conversion loop -- a per-element test costs a scalar branch per output value.
enum { ACT_SIGMOID = 3 };   // MODE_PRED; the other codes are lp_act
// sigmoid(v) = rcp(1 + exp(-v)) with the hardware reciprocal (v_rcp_f32, 1 ulp) instead of an IEEE division: the
// division expands to ~10 VALU instructions per output value, which made the sigmoid / SiLU epilogues VALU-bound
// (56 M sigmoids per step in the class predictors alone); 1 ulp is three orders below the parity tolerance.
__device__ __forceinline__ float sigmoid_fast(float v) { return __builtin_amdgcn_rcpf(1.f + __expf(-v)); }
template <int ACT> __device__ __forceinline__ float act_c(float v) {
    // IEEE 754-2019 maximum: NaN stays NaN (torch.relu's result; `v > 0.f ? v : 0.f` stored a NaN pre-activation as +0.0 and
    // hid a diverged layer from everything behind it), -0.0 and negatives give +0.0.  One v_maximum3_f32 on gfx950.
    if (ACT == LP_ACT_RELU) return __builtin_elementwise_maximum(v, 0.f);
    if (ACT == LP_ACT_SILU) {
        // The product is pinned in an fp32 register: otherwise some instantiations fold the multiply into the following
        // f32 -> f16 conversion (v_fma_mixlo_f16) and others do not, and kernel variants differ by one f16 ulp.
        float p = v * sigmoid_fast(v);
        asm volatile("" : "+v"(p));
        return p;
    }
    if (ACT == ACT_SIGMOID) return sigmoid_fast(v);
    return v;
}
template <int ACT> struct ActTag { static constexpr int value = ACT; };
// f(ActTag<code>{}) for the runtime activation code `act`
template <typename F> __device__ __forceinline__ void act_dispatch(int act, F&& f) {
    if (act == LP_ACT_RELU) f(ActTag<LP_ACT_RELU>{});
    else if (act == LP_ACT_SILU) f(ActTag<LP_ACT_SILU>{});
    else f(ActTag<LP_ACT_NONE>{});
}

template <typename T> __device__ __forceinline__ float to_f32(T v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f32(float v) { return (T)v; }

template <typename T, int CFG, int KS, int S, int MODE, int NBUF>
__global__ __launch_bounds__((Geo<T, CFG, KS, S, MODE, NBUF>::NT)) void conv_mfma_kernel(const ConvArgs a) {
    typedef Geo<T, CFG, KS, S, MODE, NBUF> G;
    typedef Cfg<CFG> C;
    typedef typename Mma<T>::V V;
    constexpr int NT = G::NT, NW = G::NW, CB = G::CB, PB = G::PB, KC = G::KC, GPR = G::GPR, ROWB = G::ROWB, EPG = G::EPG;
    __shared__ __attribute__((aligned(1024))) char smem[G::LDS];
    // buffer k of the NBUF-deep ring: halo rows at k*LDS_MAIN, weight rows behind them
    constexpr int WOFF = G::HPMAX * ROWB;

    // ---- block -> (pixel tile, cout tile): blocks sharing an input tile get ids equal mod 8, i.e. the same
    // XCD under round-robin dispatch, so the halo is served by that XCD's L2 for all cout tiles (speed only).
    const int bid = blockIdx.x;
    const int j = bid >> 3;
    const int ct = j % a.nct;
    const int pt = (j / a.nct) * 8 + (bid & 7);
    const int ntiles = a.B * a.tiles_y * a.tiles_x;
    if (pt >= ntiles) return;
    const int phase = blockIdx.y;
    const int b = pt / (a.tiles_y * a.tiles_x);
    const int trem = pt - b * (a.tiles_y * a.tiles_x);
    const int ty0 = (trem / a.tiles_x) * a.TH;
    const int tx0 = (trem % a.tiles_x) * a.TW;
    const int HH = (a.TH - 1) * S + KS, HW = (a.TW - 1) * S + KS;
    const int HP = a.hpitch;                       // LDS row pitch of the halo (>= HW; chosen on the host for conflict-free B reads)
    const int HWE = (HW + 1) >> 1;                 // even columns of a halo row (stride-2 layout: evens first, then odds)
    const int iy0 = ty0 * S - KS / 2, ix0 = tx0 * S - KS / 2;
    const int npix = a.TH * a.TW;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int wvc = wave % C::WGC, wvp = wave / C::WGC;

    // ---- per-lane halo DMA map (the same for every chunk): instruction i = wave + k*NW fills slots
    // [64 i, 64 i + 64); slot -> (halo pixel hp, stored granule position) -> source granule = swz(position)
    const int n_hg = HH * HP * GPR;
    const int n_hi = (n_hg + 63) >> 6;             // halo DMA instructions actually needed
    int hpix[G::NHI];                              // input pixel index of the slot, or -1 (zero padding)
    int hgc[G::NHI];                               // channel offset of the slot's source granule inside a chunk
#pragma unroll
    for (int k = 0; k < G::NHI; ++k) {
        const int slot = (wave + k * NW) * 64 + lane;
        const int hp = slot / GPR;
        const int hy = (int)(((unsigned)hp * a.hp_magic) >> 22), hxs = hp - hy * HP;
        // stride 2: a halo row is stored as its even columns followed by its odd columns, so that the pixels a tap reads
        // for consecutive output columns are consecutive in LDS (dense: no 2-way bank conflict of the stride-2 walk)
        const int hx = S == 2 ? (hxs < HWE ? 2 * hxs : 2 * (hxs - HWE) + 1) : hxs;
        const int iy = iy0 + hy, ix = ix0 + hx;
        const bool real = slot < n_hg && hxs < HW;                        // pitch-padding columns are never read
        const bool ok = real && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        hpix[k] = ok ? (b * a.H + iy) * a.W + ix : (real ? -1 : -2);       // -1: zero padding of the image, -2: no fetch
        hgc[k] = swz(hp, slot % GPR, GPR) * EPG;
    }
    const int nchunks = a.chunk_begin[a.nsrc];
#ifdef LP_STAMPS
    unsigned long long t_issue = 0, t_wait = 0, t_bar = 0, t_comp = 0, t_top = 0, t_mark = 0;
#define LP_STAMP(acc) do { unsigned long long _t; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t) :: "memory"); acc += _t - t_mark; t_mark = _t; } while (0)
#define LP_MARK() do { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_mark) :: "memory"); } while (0)
    const unsigned long long t_start = __builtin_readcyclecounter();
#else
#define LP_STAMP(acc) do {} while (0)
#define LP_MARK() do {} while (0)
#endif
    const T* wbase = (const T*)a.w + (long long)phase * a.w_phase_stride +
                     (long long)ct * nchunks * (G::WROWS * KC);

    // DMA of one K-chunk = NHI halo + NWI weight instructions per wave ("pieces").  The 2-deep ring spreads the pieces of
    // chunk q+1 over the K steps of chunk q, so that a wave never sits in the vector-memory issue queue (64 B/clk per
    // CU) for a whole chunk while its MFMAs could run.
    struct ChunkSrc { const T* sp; const char* ws; int c0, cs; };
    auto chunk_src = [&](int q) {
        int s = 0;
#pragma unroll
        for (int k = 1; k < LP_MAX_SRC; ++k)
            if (k < a.nsrc && q >= a.chunk_begin[k]) s = k;
        ChunkSrc c;
        c.c0 = (q - a.chunk_begin[s]) * KC;
        c.sp = (const T*)a.src[s].ptr;
        c.cs = a.src[s].cs;
        c.ws = (const char*)(wbase + (long long)q * (G::WROWS * KC));
        return c;
    };
    constexpr int NPIECE = G::NHI + G::NWI;
    auto issue_piece = [&](int jp, const ChunkSrc& cs_, char* buf) {
        char* const hlds = buf;
        char* const wlds = buf + WOFF;
        if (jp < G::NHI) {
            const int k = jp;
            const int i = wave + k * NW;
            if (i < n_hi) {                                   // wave-uniform
                const int c = cs_.c0 + hgc[k];
                const T* p = (hpix[k] >= 0 && c < cs_.cs) ? cs_.sp + (long long)hpix[k] * cs_.cs + c : (const T*)a.zero;
                if (hpix[k] != -2)   // lanes of padding columns are masked off: no request, nothing written
                    __builtin_amdgcn_global_load_lds((gbl_ptr_t)p, (lds_ptr_t)(hlds + i * 1024), 16, 0, 0);
            }
        } else {
            const int k = jp - G::NHI;
            const int i = wave + k * NW;
            if (i < G::WS / 64)                                // wave-uniform
                __builtin_amdgcn_global_load_lds((gbl_ptr_t)(cs_.ws + i * 1024 + lane * 16), (lds_ptr_t)(wlds + i * 1024), 16, 0, 0);
        }
    };
    auto issue_chunk = [&](int q, char* buf) {
        const ChunkSrc c = chunk_src(q);
#pragma unroll
        for (int jp = 0; jp < NPIECE; ++jp) issue_piece(jp, c, buf);
    };

    // ---- accumulators start at the bias of their output channel (row of D) ----
    f32x16 acc[C::WC][C::WP];
#pragma unroll
    for (int wc = 0; wc < C::WC; ++wc) {
        const float* bp = a.bias + ct * CB + (wvc * C::WC + wc) * 32 + 4 * h;
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            const f32x4 bv = *(const f32x4*)(bp + 8 * rg);
#pragma unroll
            for (int wp = 0; wp < C::WP; ++wp) {
                acc[wc][wp][4 * rg + 0] = bv[0];
                acc[wc][wp][4 * rg + 1] = bv[1];
                acc[wc][wp][4 * rg + 2] = bv[2];
                acc[wc][wp][4 * rg + 3] = bv[3];
            }
        }
    }

    // ---- per-lane fragment addresses (swizzled granule position folded in) ----
    int boff[C::WP][KS * KS][G::NKB];
#pragma unroll
    for (int wp = 0; wp < C::WP; ++wp) {
        int pl = (wvp * C::WP + wp) * 32 + r;
        if (pl >= npix) pl = 0;  // padding columns of the tile: computed, never stored
        const int ty = (int)(((unsigned)pl * a.tw_magic) >> 22), tx = pl - ty * a.TW;
        const int hp0 = (ty * S) * HP + (S == 2 ? tx : tx * S);
#pragma unroll
        for (int t = 0; t < KS * KS; ++t) {
            // stride 2: column 2 tx + kx sits at tx + (kx >> 1) of the even (kx even) or odd half of the stored row
            const int hp = hp0 + (t / KS) * HP + (S == 2 ? ((t % KS) & 1) * HWE + ((t % KS) >> 1) : (t % KS));
#pragma unroll
            for (int kb = 0; kb < G::NKB; ++kb) boff[wp][t][kb] = hp * ROWB + swz(hp, 2 * kb + h, GPR) * 16;
        }
    }
    int aoff[G::NKB];
#pragma unroll
    for (int kb = 0; kb < G::NKB; ++kb) aoff[kb] = ((wvc * C::WC) * 32 + r) * ROWB + swz(r, 2 * kb + h, GPR) * 16;

    if (NBUF == 2) issue_chunk(0, smem);
    for (int q = 0; q < nchunks; ++q) {
        char* const buf = smem + (NBUF == 2 ? (q & 1) * G::LDS_MAIN : 0);
        if (NBUF == 1) {
            LP_MARK();
            __syncthreads();  // previous chunk's fragment reads are done
            LP_STAMP(t_top);
            issue_chunk(q, buf);
            LP_STAMP(t_issue);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's LDS-DMA has landed ...
            LP_STAMP(t_wait);
            __syncthreads();                                   // ... and so has everyone else's
            LP_STAMP(t_bar);
        } else {
            // one barrier per chunk: it retires chunk q's DMA (vmcnt(0)) and proves every wave has finished
            // reading chunk q-1, whose buffer the next DMA overwrites while chunk q is being multiplied
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        const bool prefetch = NBUF == 2 && q + 1 < nchunks;                 // block-uniform
        const ChunkSrc nxt = chunk_src(prefetch ? q + 1 : q);
        char* const nbuf_ptr = smem + ((q + 1) & 1) * G::LDS_MAIN;
        const char* const hlds = buf;
        const char* const wlds = buf + WOFF;
        // K steps of the chunk (tap x K-block), software-pipelined over two register sets: the fragments of step
        // s+1 are requested from LDS before the MFMAs of step s are issued, so LDS latency hides under them
        constexpr int NS = KS * KS * G::NKB;
        V fa[2][C::WC], fb[2][C::WP];
        auto load_frags = [&](int st, V(&af)[C::WC], V(&bf)[C::WP]) {
            const int t = st / G::NKB, kb = st % G::NKB;
#pragma unroll
            for (int wc = 0; wc < C::WC; ++wc) af[wc] = *(const V*)(wlds + aoff[kb] + (t * CB + wc * 32) * ROWB);
#pragma unroll
            for (int wp = 0; wp < C::WP; ++wp) bf[wp] = *(const V*)(hlds + boff[wp][t][kb]);
        };
        load_frags(0, fa[0], fb[0]);
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            if (st + 1 < NS) load_frags(st + 1, fa[(st + 1) & 1], fb[(st + 1) & 1]);
            if (NBUF == 2 && prefetch) {       // this step's share of the next chunk's DMA pieces
#pragma unroll
                for (int jp = st; jp < NPIECE; jp += NS) issue_piece(jp, nxt, nbuf_ptr);
            }
            __builtin_amdgcn_sched_barrier(0);   // keep the next step's ds_reads ahead of this step's MFMAs
#pragma unroll
            for (int wc = 0; wc < C::WC; ++wc)
#pragma unroll
                for (int wp = 0; wp < C::WP; ++wp) acc[wc][wp] = Mma<T>::mma(fa[st & 1][wc], fb[st & 1][wp], acc[wc][wp]);
            __builtin_amdgcn_sched_barrier(0);
        }
        LP_STAMP(t_comp);
    }
#ifdef LP_STAMPS
    if (a.stamps && lane == 0) {
        unsigned long long* o = a.stamps + ((long long)(blockIdx.x * NW + wave)) * 8;
        o[0] = t_top; o[1] = t_issue; o[2] = t_wait; o[3] = t_bar; o[4] = t_comp;
        o[5] = __builtin_readcyclecounter() - t_start; o[6] = nchunks; o[7] = 1;
    }
#endif

    // ---- epilogue: activation in registers, transpose through LDS, whole-row stores ----
    __syncthreads();
    char* const stg = smem;
    auto stage_out = [&](auto tag) {
        constexpr int ACT = decltype(tag)::value;
#pragma unroll
        for (int wc = 0; wc < C::WC; ++wc)
#pragma unroll
            for (int wp = 0; wp < C::WP; ++wp) {
                const int pl = (wvp * C::WP + wp) * 32 + r;
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const int cl = (wvc * C::WC + wc) * 32 + 8 * rg + 4 * h;
                    float v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = act_c<ACT>(acc[wc][wp][4 * rg + k]);
                    char* dst = stg + pl * G::STGB + cl * G::OSZ;
                    if (MODE == MODE_ACT && sizeof(T) == 2) {
                        typedef T T4 __attribute__((ext_vector_type(4)));
                        T4 o;
                        o[0] = from_f32<T>(v[0]); o[1] = from_f32<T>(v[1]);
                        o[2] = from_f32<T>(v[2]); o[3] = from_f32<T>(v[3]);
                        *(T4*)dst = o;
                    } else {
                        f32x4 o = {v[0], v[1], v[2], v[3]};
                        *(f32x4*)dst = o;
                    }
                }
            }
    };
    if (MODE == MODE_ACT) act_dispatch(a.act, stage_out);
    else if (MODE == MODE_PRED) stage_out(ActTag<ACT_SIGMOID>{});
    else stage_out(ActTag<LP_ACT_NONE>{});
    __syncthreads();

    const int OW = a.Wo * a.out_scale;
    const int ody = phase >> 1, odx = phase & 1;
    if (MODE == MODE_ACT) {
        constexpr int GPP = CB / EPG;  // granules per staged pixel row
        T* const out = (T*)a.out + (long long)b * a.out_img_stride;
        // two sibling layers as one launch (a.out2): channels >= out_split belong to the second tensor; the offset below is
        // relative to `out` either way (both tensors live in the arena: the difference of two pointers into it)
        const long long out2_rel = a.out2 ? ((T*)a.out2 + (long long)b * a.out2_img_stride) - out : 0;
        const T* const res = a.res ? (const T*)a.res + (long long)b * a.Ho * a.Wo * a.res_cs : nullptr;
        // The residual is a branch around the whole loop, not inside it: a load inside the store loop makes the compiler
        // wait for vmcnt(0) before every store, which also waits for the previous STORE -- the rows would go out one
        // memory round trip at a time.  Without a residual the stores are fire-and-forget; with one, all residual rows
        // are requested first.
        constexpr int NIT = (PB * GPP + NT - 1) / NT;
        constexpr long long NO_STORE = -0x7fffffffffffffffLL - 1;
        long long ooff[NIT];      // element offset of the row piece relative to `out` (negative for a second tensor placed below it), or NO_STORE
        long long roff[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int g = tid + it * NT;
            const int pl = g / GPP, cg = g - pl * GPP;
            const int c = ct * CB + cg * EPG;
            const int ty = (int)(((unsigned)pl * a.tw_magic) >> 22), tx = pl - ty * a.TW;
            const int oy = ty0 + ty, ox = tx0 + tx;
            const bool ok = g < PB * GPP && pl < npix && c < a.out_c && oy < a.Ho && ox < a.Wo;
            const long long opix = (long long)(oy * a.out_scale + ody) * OW + (ox * a.out_scale + odx);
            const bool second = a.out2 && c >= a.out_split;
            ooff[it] = !ok ? NO_STORE : second ? out2_rel + opix * a.out2_pix_stride + (c - a.out_split) : opix * a.out_pix_stride + c;
            roff[it] = ok ? ((long long)oy * a.Wo + ox) * a.res_cs + c : 0;   // invalid lanes read element 0: valid memory, unused
        }
        if (res) {
            uint4 rv[NIT];
#pragma unroll
            for (int it = 0; it < NIT; ++it) rv[it] = *(const uint4*)(res + roff[it]);   // unconditional: all in flight together
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (ooff[it] == NO_STORE) continue;
                const int g = tid + it * NT;
                const int pl = g / GPP, cg = g - pl * GPP;
                uint4 v = *(const uint4*)(stg + pl * G::STGB + cg * 16);
                T* pv = (T*)&v;
                const T* pr = (const T*)&rv[it];
#pragma unroll
                for (int k = 0; k < EPG; ++k) pv[k] = from_f32<T>(to_f32(pv[k]) + a.alpha * to_f32(pr[k]));
                *(uint4*)(out + ooff[it]) = v;
            }
        } else {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (ooff[it] == NO_STORE) continue;
                const int g = tid + it * NT;
                const int pl = g / GPP, cg = g - pl * GPP;
                *(uint4*)(out + ooff[it]) = *(const uint4*)(stg + pl * G::STGB + cg * 16);
            }
        }
    } else if (MODE == MODE_PRED) {
        float* const out = (float*)a.out + (long long)b * a.out_img_stride;
        for (int idx = tid; idx < PB * CB; idx += NT) {
            const int pl = idx / CB, cl = idx - pl * CB;
            const int c = ct * CB + cl;
            if (pl >= npix || c >= a.out_c) continue;
            const int ty = (int)(((unsigned)pl * a.tw_magic) >> 22), tx = pl - ty * a.TW;
            const int oy = ty0 + ty, ox = tx0 + tx;
            if (oy >= a.Ho || ox >= a.Wo) continue;
            out[((long long)oy * a.Wo + ox) * a.out_pix_stride + c] = *(const float*)(stg + pl * G::STGB + cl * 4);
        }
    } else {  // MODE_DECODE: four threads per pixel, one per box side (round 3: the DFL softmax -- 2 x 17 exponentials and 17 divisions per
        // side -- ran on one thread per pixel, half the workgroup idle: 72 us for yolov6m's 160x160 level).  Thread (pixel, k) computes
        // side k with the same operations as before, the quad exchanges the four distances, every thread decodes two corner values.
        float* const out = (float*)a.out + (long long)b * a.out_img_stride;
        const int nb = a.reg_bins;
        for (int item0 = 0; item0 < npix * 4; item0 += NT) {     // (NT % 64 == 0: whole waves take part in the exchange)
            const int item = item0 + tid;
            const int plr = item >> 2, k = item & 3;
            const int pl = plr < npix ? plr : npix - 1;
            const int ty = (int)(((unsigned)pl * a.tw_magic) >> 22), tx = pl - ty * a.TW;
            const int oy = ty0 + ty, ox = tx0 + tx;
            const bool ok = plr < npix && oy < a.Ho && ox < a.Wo;
            const float* z = (const float*)(stg + pl * G::STGB);
            float dk;
            if (nb == 1) {
                dk = z[k];
            } else {  // softmax over the bins of side k, projected by proj[]
                const float* zk = z + k * nb;
                float m = zk[0];
                for (int i = 1; i < nb; ++i) m = fmaxf(m, zk[i]);
                float sum = 0.f;
                for (int i = 0; i < nb; ++i) sum += expf(zk[i] - m);
                float acc2 = 0.f;
                for (int i = 0; i < nb; ++i) acc2 += (expf(zk[i] - m) / sum) * a.proj[i];
                dk = acc2;
            }
            const int q0 = (tid & 63) & ~3;
            const float d0 = __shfl(dk, q0), d1 = __shfl(dk, q0 + 1), d2 = __shfl(dk, q0 + 2), d3 = __shfl(dk, q0 + 3);
            if (!ok) continue;
            const float* cz = z + 4 * nb;
            const float ax = (float)ox + 0.5f, ay = (float)oy + 0.5f;
            const float x1 = ax - d0, y1 = ay - d1, x2 = ax + d2, y2 = ay + d3;
            const float sp = a.stride_px;
            float* o = out + ((long long)oy * a.Wo + ox) * a.out_pix_stride;
            // corners 2k (an x coordinate) and 2k + 1 (a y coordinate): dist2cor's signs (utils/general.py:47-66)
            const float cx_ = cz[2 * k], cy_ = cz[2 * k + 1];
            const float kx = (k < 2 ? ax - cx_ : ax + cx_) * sp;
            const float ky = ((k == 0 || k == 3) ? ay - cy_ : ay + cy_) * sp;
            if (a.det_mode) {
                // detections-only forward: columns 0..11 of the anchor's candidate row = what score_kernel (lp_nms.hip) derives
                // from prediction columns 0..12, in its operation order: xyxy = (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)
                if (k == 0) {
                    const float cx = ((x1 + x2) / 2.f) * sp, cy = ((y1 + y2) / 2.f) * sp, bw = (x2 - x1) * sp, bh = (y2 - y1) * sp;
                    o[0] = cx - bw / 2;
                    o[1] = cy - bh / 2;
                    o[2] = cx + bw / 2;
                    o[3] = cy + bh / 2;
                }
                o[4 + 2 * k] = kx;
                o[5 + 2 * k] = ky;
                continue;
            }
            if (k == 0) {
                o[0] = ((x1 + x2) / 2.f) * sp;
                o[1] = ((y1 + y2) / 2.f) * sp;
                o[2] = (x2 - x1) * sp;
                o[3] = (y2 - y1) * sp;
                o[4] = 1.f;
            }
            o[5 + 2 * k] = kx;
            o[6 + 2 * k] = ky;
        }
    }
}

template <typename T, int CFG, int KS, int S, int MODE, int NBUF>
static inline int launch_one(const ConvArgs& a, hipStream_t st) {
    typedef Geo<T, CFG, KS, S, MODE, NBUF> G;
    const int ntiles = a.B * a.tiles_y * a.tiles_x;
    dim3 grid((unsigned)(a.nct * round_up(ntiles, 8)), (unsigned)a.nphase);
    hipLaunchKernelGGL((conv_mfma_kernel<T, CFG, KS, S, MODE, NBUF>), grid, dim3(G::NT), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LP_ERR_HIP, std::string("conv launch: ") + hipGetErrorString(e));
    return LP_OK;
}

template <typename T>
static inline int launch_dtype(int cfg, int mode, int ks, int s, int nbuf, const ConvArgs& a, hipStream_t st) {
    if (mode == MODE_PRED) {
        if (cfg == CFG_B && ks == 1 && s == 1) return launch_one<T, CFG_B, 1, 1, MODE_PRED, 1>(a, st);
        if (cfg == CFG_C && ks == 1 && s == 1) return launch_one<T, CFG_C, 1, 1, MODE_PRED, 1>(a, st);
    } else if (mode == MODE_DECODE) {
        if (cfg == CFG_A && ks == 1 && s == 1) return launch_one<T, CFG_A, 1, 1, MODE_DECODE, 1>(a, st);
        if (cfg == CFG_C && ks == 1 && s == 1) return launch_one<T, CFG_C, 1, 1, MODE_DECODE, 1>(a, st);
    } else {
#define LP_CASE(CF, NB)                                                                     \
    if (cfg == CF && nbuf == NB) {                                                          \
        if (ks == 1 && s == 1) return launch_one<T, CF, 1, 1, MODE_ACT, NB>(a, st);         \
        if (ks == 3 && s == 1) return launch_one<T, CF, 3, 1, MODE_ACT, NB>(a, st);         \
        if (ks == 3 && s == 2) return launch_one<T, CF, 3, 2, MODE_ACT, NB>(a, st);         \
    }
        LP_CASE(CFG_A, 1) LP_CASE(CFG_A, 2)
        LP_CASE(CFG_B, 1) LP_CASE(CFG_B, 2)
        LP_CASE(CFG_C, 1)
        LP_CASE(CFG_D, 1) LP_CASE(CFG_D, 2)
        LP_CASE(CFG_E, 1) LP_CASE(CFG_E, 2)
        LP_CASE(CFG_F, 1) LP_CASE(CFG_F, 2)
#undef LP_CASE
    }
    return fail(LP_ERR_UNSUPPORTED, "conv: no kernel for this (cfg, mode, ksize, stride, nbuf)");
}

}  // namespace lp
