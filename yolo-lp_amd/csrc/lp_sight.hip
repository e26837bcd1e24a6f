// A device-resident log of sightings: lp_sight_update (include/lp_hip.h) matches every read that ends in a tracker call against
// the recent reads of all streams, then appends it to the ring it has just scanned.  The same weighted Hamming distance as
// lp_watch_match (lp_watch.hip), but symmetric: an entry is itself a voted read with weights of its own, which entries may match
// depends on the pair of streams and on the entry's age, and among equally cheap entries the most recent wins.  The reference has
// nothing here; the written-down specification is yolov6/utils/sight.py (sight_update_np), which these kernels match on every int32
// of sight_i and of the log (tests/test_sight_gpu.py).  Everything is integer except one fp32 product per read and position; the
// reductions are an unsigned minimum and an integer sum, so the result does not depend on the order in which workgroups arrive.
// The record layout, the weight of a position (read_weight, also of the stored weights), where the confusion table keeps a pair's
// cost (confuse_offset), the prefix sum and the host's limit checks are lp_read_match.inc's, shared with lp_watch.hip.  The table
// loop (bytes, no WILD column; the default of 16, the clamp at 16 and "own id costs nothing" restated in it), the staging (qp
// transposed, the reads' streams), the flush of a block and the scoring loop stay this file's own: sight_scan_kernel sits on a
// register edge (35 spilled at two workgroups per CU), and with the table's cost rule, the flush and the quantiser's test taken
// from shared functions it kept its 35 spills but reloaded three more registers in front of every table build and lp_sight_update
// was 3 % slower (profiles/read_match_codegen.txt).  As it stands the kernel is the one it was before the sharing.
//
// sight_prep_kernel (one workgroup): every thread owns a run of lines, counts its reads (a line below its stream's clamped count
//   whose hits reach min_hits), the counts are prefix-summed in LDS, read k of the call gets its line in qlist[k] and every line its
//   read number (or -1) in kidx; keys and counts are cleared; the header's total is copied into the workspace, so that no later
//   kernel reads the word the append kernel writes.
// sight_scan_kernel: one workgroup of 256 threads per LP_SIGHT_BLOCK_ENTRIES slots; workgroups past the filled part leave at once.
//   Every lane owns four slots, each two 16-byte loads (lane t takes slots base + r * 256 + t), and parks them in LDS: the stored
//   ids as table columns (0..63 the id, 64 "matches nothing"), the weights, the stream, and one word (in window) << 31 | age rank.
//   So the log is read from memory once per call, however many reads end.  The workgroup walks the call's reads in blocks of
//   LP_SIGHT_QUERY_BLOCK = 16.  Per block it builds the LDS table
//     T[position][column][read] = one byte: 0 for the read's own id, else 0x20 | confusion weight
//   (16 bytes per column: one LDS read fetches a column's bytes for all sixteen reads), and a (slot, read) pair is then, per
//   position, one byte extract, a min of the two weights and a multiply-add into (cost << 4 | mismatches).  A slot outside the
//   window is skipped before any of it; the pair mask is looked up only for a slot that passed both limits.  A lane keeps, per
//   read, the 64-bit minimum of cost << 32 | age rank << 4 | mismatches over its accepted slots and their number; a wave that
//   accepted something combines by shuffles, its first lane combines into LDS (64-bit minimum, integer add), and one thread per
//   read with a hit issues one global atomicMin and one atomicAdd.  Blocks of four and eight reads run the same code on that many
//   table bytes only (template Q4).
// sight_tail_kernel: one thread per line turns key and count into the sight_i row: the age rank names seq, seq the slot, and the
//   four prev_* words are copied out of the log, which nothing has written yet.
// sight_append_kernel: one thread per read writes its slot (two 16-byte vector stores) -- the last C reads of the call only -- and
//   thread 0 writes the new total.  It runs behind the tail in stream order: the tail has read the old rows by then.
#include "lp_internal.h"
#include "lp_streams.h"
#include "lp_read_match.inc"

namespace lp {

namespace {

constexpr int G_T = 256;                                   // threads of a scan workgroup
constexpr int G_E = LP_SIGHT_BLOCK_ENTRIES;
constexpr int G_R = G_E / G_T;                             // slots per lane
constexpr int G_QB = LP_SIGHT_QUERY_BLOCK;
constexpr int G_COLS = 65;                                 // 0..63 ids, 64 matches nothing
constexpr int G_PREP_T = 1024;
constexpr int G_WORDS = 8;                                 // int32 words of a row of the log and of sight_i
constexpr unsigned G_RANK_MASK = 0xfffffffu;               // 28 bits of the key hold the age rank (< capacity <= 2^24)
static_assert(G_R == 4 && G_QB == 16, "lp_sight.hip is written for 4 slots per lane and blocks of 16 reads");
static_assert(LP_TRACK_MAX_CLS == 64, "the table has 64 id columns");

struct SightWs {                                           // carve-up of the caller's workspace, L = n_streams * max_ended
    unsigned long long* keys;                              // [L] by read number
    int32_t* cnts;                                         // [L] by read number
    int32_t* qlist;                                        // [L] line of read k
    int32_t* kidx;                                         // [L] read number of line l, -1: the line is no read
    int32_t* hdr;                                          // [4] reads of the call, total before the call, 0, 0
    size_t bytes;
};
SightWs sight_carve(void* base, size_t S, size_t max_ended) {
    const size_t L = S * max_ended;
    char* p = (char*)base;
    SightWs w;
    w.keys = (unsigned long long*)p;
    w.cnts = (int32_t*)(p + 8 * L);
    w.qlist = (int32_t*)(p + 12 * L);
    w.kidx = (int32_t*)(p + 16 * L);
    w.hdr = (int32_t*)(p + 20 * L);
    w.bytes = (20 * L + 16 + 15) & ~(size_t)15;
    return w;
}

// grid (1), block (1024); per = ceil(L / 1024) lines per thread
__global__ __launch_bounds__(G_PREP_T) void sight_prep_kernel(const int32_t* __restrict__ state, const int32_t* __restrict__ ended_i,
                                                              const int32_t* __restrict__ ended_count, int S, int max_ended, int min_hits,
                                                              int per, SightWs ws) {
    __shared__ int s_scan[G_PREP_T];
    const int tid = threadIdx.x;
    const int L = S * max_ended;
    const long long l0 = (long long)tid * per;
    const int lo = l0 < L ? (int)l0 : L, hi = l0 + per < L ? (int)(l0 + per) : L;
    int c = 0;
    for (int l = lo; l < hi; ++l) {
        const int s = l / max_ended, j = l - s * max_ended;
        c += (j < clamp_count(ended_count[s], max_ended) && ended_i[(long long)l * RM_REC_WORDS + RM_W_HITS] >= min_hits) ? 1 : 0;
    }
    s_scan[tid] = c;
    block_prefix_sum<G_PREP_T>(s_scan);
    int k = s_scan[tid] - c;                                           // number of this thread's first read: k + c <= L
    if (tid == 0) {
        ws.hdr[0] = s_scan[G_PREP_T - 1];
        ws.hdr[1] = state[0];
        ws.hdr[2] = 0;
        ws.hdr[3] = 0;
    }
    for (int l = lo; l < hi; ++l) {
        const int s = l / max_ended, j = l - s * max_ended;
        const bool read = j < clamp_count(ended_count[s], max_ended) && ended_i[(long long)l * RM_REC_WORDS + RM_W_HITS] >= min_hits;
        ws.keys[l] = ~0ull;
        ws.cnts[l] = 0;
        ws.kidx[l] = read ? k : -1;
        if (read) ws.qlist[k++] = l;
    }
}

// ids of four stored bytes -> table columns
__device__ __forceinline__ unsigned to_columns(unsigned x) {
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned b = (x >> (8 * k)) & 0xffu;
        out |= (b < 64u ? b : 64u) << (8 * k);
    }
    return out;
}

struct __attribute__((aligned(16))) SightLds {
    unsigned char T[8 * G_COLS * G_QB];                    // 8 positions x 65 columns x 16 reads = 8320 bytes
    unsigned qp[8 * G_QB];                                 // weight of read q at position p: [p][q]
    uint2 ids[G_E];                                        // the workgroup's slots, slot r of lane t at r * 256 + t: ids as columns,
    uint2 qw[G_E];                                         // the weights minus 1 as bytes,
    uint2 meta[G_E];                                       // (stream, in window << 31 | age rank)
    int best[G_QB * 8];                                    // id of read q at position p: [q][p]
    int rstream[G_QB];
    unsigned long long key[G_QB];
    int cnt[G_QB];
};

// One block of 4 * Q4 reads (the reads k0 .. k0 + nq - 1, nq <= 4 * Q4), from the staged best / qp to the global atomics.
template <int Q4>
__device__ __forceinline__ void sight_block(SightLds& lds, const unsigned char* __restrict__ confuse, const unsigned char* __restrict__ pair,
                                            int S, unsigned mm, unsigned mc, int k0, int nq, const SightWs& ws) {
    constexpr int NQ = 4 * Q4;
    const int tid = threadIdx.x;
    // ---- the table: one unit = (position, four id columns or the special one, read) -------------------------------------------------
    for (int u = tid; u < 8 * 17 * NQ; u += G_T) {
        const int q = u % NQ, pc = u / NQ, p = pc / 17, c4 = pc - p * 17;
        const int b = lds.best[q * 8 + p];
        const bool inr = (unsigned)b < 64u;
        unsigned char* col0 = lds.T + (p * G_COLS + c4 * 4) * G_QB + q;
        if (c4 == 16) {
            col0[0] = 0x20u | 16u;                                     // a stored id that matches nothing
            continue;
        }
        unsigned cw = 0x10101010u;                                     // the cost rule of the watch table (build_read_table), in bytes   
        if (confuse != nullptr && inr) cw = *(const unsigned*)(confuse + confuse_offset(p, b, c4));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned c = (cw >> (8 * k)) & 0xffu;
            c = c > 16u ? 16u : c;                                     // a table the host did not check cannot leave its five bits
            col0[k * G_QB] = (inr && c4 * 4 + k == b) ? 0u : (0x20u | c);
        }
    }
    __syncthreads();
    // ---- the scan --------------------------------------------------------------------------------------------------------------
    unsigned long long best[NQ];
    unsigned cnt[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { best[q] = ~0ull; cnt[q] = 0u; }
#pragma unroll 1
    for (int r = 0; r < G_R; ++r) {
        const uint2 meta = lds.meta[r * G_T + tid];
        if ((meta.y >> 31) == 0u) continue;                            // empty, outside the window, or past the log
        const uint2 ids = lds.ids[r * G_T + tid], qw = lds.qw[r * G_T + tid];
        unsigned acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = 0u;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const unsigned col = ((p < 4 ? ids.x : ids.y) >> (8 * (p & 3))) & 0xffu;
            const unsigned qe = (((p < 4 ? qw.x : qw.y) >> (8 * (p & 3))) & 0xffu) + 1u;
            const unsigned* row = (const unsigned*)(lds.T + (p * G_COLS + col) * G_QB);
            const unsigned* qr = lds.qp + p * G_QB;
#pragma unroll
            for (int g = 0; g < Q4; ++g) {
                const unsigned w = row[g];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned b = (w >> (8 * k)) & 0xffu;
                    const unsigned m = qr[4 * g + k] < qe ? qr[4 * g + k] : qe;
                    acc[4 * g + k] += ((m * (b & 31u)) << 4) + (b >> 5);
                }
            }
        }
        const unsigned rank = meta.y & G_RANK_MASK;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            bool ok = (acc[q] >> 4) <= mc && (acc[q] & 15u) <= mm;
            if (ok && pair != nullptr) ok = meta.x < (unsigned)S && pair[(size_t)lds.rstream[q] * S + meta.x] != 0;
            const unsigned long long key = ((unsigned long long)(acc[q] >> 4) << 32) | ((unsigned long long)rank << 4) | (acc[q] & 15u);
            best[q] = ok && key < best[q] ? key : best[q];
            cnt[q] += ok ? 1u : 0u;
        }
    }
    // a wave combines in registers first (a log that holds the same plates many times makes every lane a hit, and 256 atomics on one
    // LDS word run one after the other); then one lane per wave and read goes to LDS
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        if (__any(cnt[q] != 0u)) {                                     // (wave-uniform)
            unsigned long long k = best[q];
            unsigned c = cnt[q];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(k, off);
                k = o < k ? o : k;
                c += __shfl_xor(c, off);
            }
            if ((tid & 63) == 0) {
                atomicMin(&lds.key[q], k);
                atomicAdd(&lds.cnt[q], (int)c);
            }
        }
    }
    __syncthreads();
    if (tid < nq && lds.cnt[tid] > 0) {
        atomicMin(&ws.keys[k0 + tid], lds.key[tid]);
        atomicAdd(&ws.cnts[k0 + tid], lds.cnt[tid]);
    }
}

// grid (ceil(C / LP_SIGHT_BLOCK_ENTRIES)), block (256).  Two workgroups per CU: left to itself the compiler keeps all 128 read weights
// of a block in registers (256 VGPRs, one workgroup per CU); held to 128 it spills 35 of them and a log of 2^20 slots is still
// scanned a third faster.
__global__ __launch_bounds__(G_T, 2) void sight_scan_kernel(const int32_t* __restrict__ state, int C, const unsigned char* __restrict__ confuse,
                                                         const unsigned char* __restrict__ pair, int S, int max_ended,
                                                         const int32_t* __restrict__ ended_i, const float* __restrict__ ended_f,
                                                         const int32_t* __restrict__ now, int window, unsigned mm, unsigned mc, SightWs ws) {
    __shared__ SightLds lds;
    const int tid = threadIdx.x;
    const int nv = ws.hdr[0], total = ws.hdr[1];
    const int fill = total < 0 ? 0 : (total < C ? total : C);
    const int base = blockIdx.x * G_E;                                 // < 2^24 + 1024
    if (nv <= 0 || base >= fill) return;                               // (block-uniform)
    const long long nw = now[0];
#pragma unroll
    for (int r = 0; r < G_R; ++r) {
        const int idx = base + r * G_T + tid;
        uint2 ids = make_uint2(0u, 0u), qw = make_uint2(0u, 0u), meta = make_uint2(0u, 0u);
        if (idx < fill) {                                              // fill <= C: row 1 + idx is inside the log
            const uint4* row = (const uint4*)(state + (size_t)(1 + idx) * G_WORDS);
            const uint4 a = row[0], b = row[1];
            const long long age = nw - (long long)(int)b.z;
            const unsigned in_window = (age >= 0 && age <= (long long)window) ? 1u : 0u;
            ids = make_uint2(to_columns(a.x), to_columns(a.y));
            qw = make_uint2(a.z, a.w);
            meta = make_uint2(b.x, (in_window << 31) | ((unsigned)(total - 1 - (int)b.w) & G_RANK_MASK));
        }
        lds.ids[r * G_T + tid] = ids;                                  // read back by this lane alone
        lds.qw[r * G_T + tid] = qw;
        lds.meta[r * G_T + tid] = meta;
    }
    for (int k0 = 0; k0 < nv; k0 += G_QB) {                            // nv <= n_streams * max_ended: k0 + q indexes qlist, keys, cnts
        const int nq = nv - k0 < G_QB ? nv - k0 : G_QB;
        if (tid < G_QB * 8) {
            const int q = tid >> 3, p = tid & 7;
            int b = -1, line = 0;
            unsigned qp = 1u;
            if (q < nq) {
                line = ws.qlist[k0 + q];
                b = ended_i[(long long)line * RM_REC_WORDS + RM_W_IDS + p];
                const float share = ended_f[(long long)line * RM_REC_WORDS + RM_F_SHARES + p];
                if (share > 0.f) qp = read_weight(share);
            }
            lds.best[tid] = b;
            lds.qp[p * G_QB + q] = qp;
            if (p == 0) lds.rstream[q] = line / max_ended;             // < n_streams
        }
        if (tid < G_QB) { lds.key[tid] = ~0ull; lds.cnt[tid] = 0; }
        __syncthreads();
        if (nq <= 4) sight_block<1>(lds, confuse, pair, S, mm, mc, k0, nq, ws);
        else if (nq <= 8) sight_block<2>(lds, confuse, pair, S, mm, mc, k0, nq, ws);
        else sight_block<4>(lds, confuse, pair, S, mm, mc, k0, nq, ws);
        __syncthreads();                                               // the next block stages over best / qp / key / cnt and the table
    }
}

// grid (ceil(L / 256)), block (256)
__global__ __launch_bounds__(256) void sight_tail_kernel(const int32_t* __restrict__ state, int C, int L, SightWs ws, int32_t* __restrict__ sight_i) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    int4 lo = make_int4(-1, 0, 0, 0), hi = make_int4(-1, -1, 0, 0);
    const int k = ws.kidx[l];
    if (k >= 0) {
        const int n = ws.cnts[k];
        if (n > 0) {
            const unsigned long long key = ws.keys[k];
            const long long seq = (long long)ws.hdr[1] - 1 - (long long)((key >> 4) & G_RANK_MASK);
            const int slot = (int)(((seq % C) + C) % C);               // in 0..C-1 whatever the log held
            hi = *(const int4*)(state + (size_t)(1 + slot) * G_WORDS + 4);
            lo = make_int4(slot, (int)(key & 15ull), (int)(key >> 32), n);
        }
    }
    int4* out = (int4*)(sight_i + (size_t)l * G_WORDS);
    out[0] = lo;
    out[1] = hi;
}

// grid (ceil(max(L, 1) / 256)), block (256)
__global__ __launch_bounds__(256) void sight_append_kernel(int32_t* __restrict__ state, int C, int max_ended, const int32_t* __restrict__ ended_i,
                                                           const float* __restrict__ ended_f, const int32_t* __restrict__ now, SightWs ws) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int V = ws.hdr[0], total = ws.hdr[1];
    if (k == 0) state[0] = (int)((unsigned)total + (unsigned)V);
    if (k >= V || V - k > C) return;                                   // of V > C reads the last C are written
    const int line = ws.qlist[k];                                      // k < V <= L
    unsigned idw[2] = {0u, 0u}, qw[2] = {0u, 0u};
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int b = ended_i[(long long)line * RM_REC_WORDS + RM_W_IDS + p];
        const unsigned qp = read_weight(ended_f[(long long)line * RM_REC_WORDS + RM_F_SHARES + p]);
        idw[p >> 2] |= ((unsigned)b < 64u ? (unsigned)b : 254u) << (8 * (p & 3));
        qw[p >> 2] |= (qp - 1u) << (8 * (p & 3));
    }
    const long long t = (long long)total + k;
    const int slot = (int)(((t % C) + C) % C);                         // in 0..C-1
    int4* row = (int4*)(state + (size_t)(1 + slot) * G_WORDS);
    row[0] = make_int4((int)idw[0], (int)idw[1], (int)qw[0], (int)qw[1]);
    row[1] = make_int4(line / max_ended, ended_i[(long long)line * RM_REC_WORDS + RM_W_TRACK], now[0], (int)t);
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" size_t lp_sight_state_bytes(int capacity) {
    if (capacity < 1 || capacity > LP_SIGHT_MAX_CAPACITY) return 0;
    return ((size_t)capacity + 1) * G_WORDS * 4;
}

extern "C" size_t lp_sight_workspace_bytes(int n_streams, int max_ended) {
    if (!ended_dims_fault(n_streams, max_ended).empty()) return 0;
    return sight_carve(nullptr, (size_t)n_streams, (size_t)max_ended).bytes;
}

extern "C" int lp_sight_update(int32_t* state, int capacity, const unsigned char* confuse, const unsigned char* pair, const int32_t* ended_i,
                               const float* ended_f, const int32_t* ended_count, int n_streams, int max_ended, const int32_t* now, int window,
                               int min_hits, int max_mismatch, int max_cost, int32_t* sight_i, void* workspace, size_t workspace_bytes,
                               void* stream) {
    const std::string fn = "lp_sight_update: ";
    if (capacity < 1 || capacity > LP_SIGHT_MAX_CAPACITY)
        return fail(LP_ERR_ARG, fn + "capacity " + std::to_string(capacity) + " (need 1.." + std::to_string(LP_SIGHT_MAX_CAPACITY) + ")");
    if (const std::string f = ended_dims_fault(n_streams, max_ended); !f.empty()) return fail(LP_ERR_ARG, fn + f);
    if (window < 0 || min_hits < 1) return fail(LP_ERR_ARG, fn + "need window >= 0 and min_hits >= 1");
    if (const std::string f = match_limits_fault(max_mismatch, max_cost); !f.empty()) return fail(LP_ERR_ARG, fn + f);
    if (max_ended == 0) return LP_OK;                                  // no line: no read, nothing to write
    if (!state || !ended_i || !ended_f || !ended_count || !now || !sight_i || !workspace) return fail(LP_ERR_ARG, fn + "null pointer");
    if (((uintptr_t)state & 15) != 0 || ((uintptr_t)sight_i & 15) != 0 || ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)confuse & 3) != 0 ||
        ((uintptr_t)now & 3) != 0)
        return fail(LP_ERR_ARG, fn + "state, sight_i and the workspace must be 16-byte, confuse and now 4-byte aligned");
    const SightWs ws = sight_carve(workspace, (size_t)n_streams, (size_t)max_ended);
    if (workspace_bytes < ws.bytes)
        return fail(LP_ERR_ARG, fn + "workspace of " + std::to_string(workspace_bytes) + " bytes, need " + std::to_string(ws.bytes));
    const size_t L = (size_t)n_streams * max_ended;
    {   // the log, sight_i and the workspace may overlap neither an input nor each other
        const Region reg[] = {{state, lp_sight_state_bytes(capacity), true},
                              {confuse, confuse ? (size_t)3 * 64 * 64 : 0, false},
                              {pair, pair ? (size_t)n_streams * n_streams : 0, false},
                              {ended_i, L * RM_REC_WORDS * 4, false},
                              {ended_f, L * RM_REC_WORDS * 4, false},
                              {ended_count, (size_t)n_streams * 4, false},
                              {now, 4, false},
                              {sight_i, L * G_WORDS * 4, true},
                              {workspace, ws.bytes, true}};
        if (regions_clash(reg, (int)(sizeof(reg) / sizeof(reg[0]))))
            return fail(LP_ERR_ARG, fn + "the log, sight_i and the workspace may overlap neither an input nor each other");
    }

    hipStream_t st = (hipStream_t)stream;
    const int Li = (int)L;
    hipLaunchKernelGGL(sight_prep_kernel, dim3(1), dim3(G_PREP_T), 0, st, state, ended_i, ended_count, n_streams, max_ended, min_hits,
                       ceil_div(Li, G_PREP_T), ws);
    LP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sight_scan_kernel, dim3((unsigned)ceil_div(capacity, G_E)), dim3(G_T), 0, st, state, capacity, confuse, pair, n_streams,
                       max_ended, ended_i, ended_f, now, window, (unsigned)max_mismatch, (unsigned)max_cost, ws);
    LP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sight_tail_kernel, dim3((unsigned)ceil_div(Li, 256)), dim3(256), 0, st, state, capacity, Li, ws, sight_i);
    LP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sight_append_kernel, dim3((unsigned)ceil_div(Li, 256)), dim3(256), 0, st, state, capacity, max_ended, ended_i, ended_f, now,
                       ws);
    LP_HIP_CHECK(hipGetLastError());
    return LP_OK;
}
