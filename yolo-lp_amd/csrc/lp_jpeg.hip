// lp_jpeg_encode_batch (include/lp_hip.h): baseline JPEG files of B frames, written whole on the device.  The reference has nothing
// here; yolov6/utils/jpeg.py states the format and restates every step in numpy, byte for byte (tests/test_jpeg_gpu.py).
//
// Four launches per LP_JPEG_PER_LAUNCH frames, descriptors and quantisation tables by value in the kernel arguments:
//   jpeg_dct_kernel<SRC>        one wave per MCU (4 per workgroup): lane (cy, cx) reads the 2 x 2 pixels of chroma site (cy, cx),
//                               makes 4 Y and the Cb, Cr of the site; the six 8 x 8 blocks go through LDS for the row pass, the
//                               column pass and the quantiser, and leave as int16 [mcu][6][64] in zig-zag order (coalesced).
//   jpeg_entropy_kernel<false>  one workgroup per restart interval, one lane per block: the bits of every block, a workgroup scan
//                               for the blocks' bit offsets, the codes merged into an LDS bit buffer with atomicOr, the 1-bit
//                               padding, a second scan over the 0xFF bytes; leaves the interval's stuffed length.
//   jpeg_scan_kernel            one workgroup per frame: exclusive scan of (length + 2) over the intervals in blocks of 256 with a
//                               carry, from the header's length; if the file fits `cap` it copies the header, writes RSTm / EOI
//                               and nbytes, else nbytes = -needed and every interval's offset is -1.
//   jpeg_entropy_kernel<true>   the same coder again, writing the stuffed bytes at the interval's offset (offset -1: nothing).
// The coder runs twice instead of parking a worst case of 2496 bytes per MCU in memory.
#include "lp_internal.h"
#include <vector>

namespace lp {

namespace {

constexpr int JP_SLOTS = LP_JPEG_PER_LAUNCH;
constexpr int JP_NV12_JFIF = 2;                         // the matrix whose planes are JFIF already (bt601f)
constexpr int JP_SCAN = 256;                            // intervals per step of the scan kernel
constexpr int JP_BLOCKS = LP_JPEG_MAX_RESTART * 6;      // blocks of the longest interval
constexpr int JP_BLOCK_BITS = 22 + 63 * 26;             // DC: code <= 11 bits + 11; AC: code <= 16 bits + 10
constexpr int JP_WORDS = (JP_BLOCKS * JP_BLOCK_BITS + 31) / 32 + 2;
static_assert(JP_WORDS * 4 + 4096 < 64 * 1024, "the bit buffer of an interval lives in static LDS");

struct JpFrame {
    const unsigned char* p0;
    const unsigned char* p1;
    int pitch0, pitch1, h, w;
    int format, mcux, n_mcu, n_int;
    long long mcu_base;                 // the frame's first MCU in the coefficient area
    int int_base, pad_;                 // ... first interval in the length and offset tables
};
struct JpTable { JpFrame f[JP_SLOTS]; };
struct JpQuant { unsigned short q[2][64]; unsigned rcp[2][64]; };      // natural order; rcp = ceil(2^20 / q)
static_assert(sizeof(JpTable) + sizeof(JpQuant) < 4096, "the tables travel as kernel arguments: under 4 KiB");

// M[k][n] = rint(4096 a(k) cos((2n + 1) k pi / 16))
__constant__ int JP_M[64] = {
    1448, 1448, 1448, 1448, 1448, 1448, 1448, 1448, 2009, 1703, 1138, 400, -400, -1138, -1703, -2009,
    1892, 784, -784, -1892, -1892, -784, 784, 1892, 1703, -400, -2009, -1138, 1138, 2009, 400, -1703,
    1448, -1448, -1448, 1448, 1448, -1448, -1448, 1448, 1138, -2009, 400, 1703, -1703, -400, 2009, -1138,
    784, -1892, 1892, -784, -784, 1892, -1892, 784, 400, -1138, 1703, -2009, 2009, -1703, 1138, -400};
__constant__ unsigned char JP_ZZ[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.1 / K.2 (natural order) and K.3 (counts per code length, then the symbols)
const int JP_BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
     72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

struct JpSpec { unsigned char counts[16]; unsigned char values[162]; };
constexpr JpSpec JP_DC_L = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JpSpec JP_DC_C = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JpSpec JP_AC_L = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa}};
constexpr JpSpec JP_AC_C = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa}};

// The canonical codes of Annex C, by symbol: code << 5 | length (0: no such symbol).  [0] luma, [1] chroma.
struct JpHuff { unsigned dc[2][16]; unsigned ac[2][256]; };
constexpr int JP_HUFF_WORDS = sizeof(JpHuff) / 4;
constexpr void jp_fill(unsigned* t, const JpSpec& s) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.counts[len - 1]; ++i) t[s.values[k++]] = (code++ << 5) | (unsigned)len;
        code <<= 1;
    }
}
constexpr JpHuff jp_make_huff() {
    JpHuff h = {};
    jp_fill(h.dc[0], JP_DC_L);
    jp_fill(h.dc[1], JP_DC_C);
    jp_fill(h.ac[0], JP_AC_L);
    jp_fill(h.ac[1], JP_AC_C);
    return h;
}
constexpr JpHuff JP_HUFF_HOST = jp_make_huff();
__constant__ JpHuff JP_HUFF = JP_HUFF_HOST;

__device__ __forceinline__ int jp_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// A pixel source: the 2 x 2 pixels at (i0, j0) (both even) of the frame padded by replication -> four Y, one Cb, one Cr.
struct JpBgrSrc {
    static constexpr int FORMAT = 0;
    static __device__ __forceinline__ void quad(const JpFrame& f, int i0, int j0, int* y4, int* cb, int* cr) {
        int sb = 0, sr = 0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = i0 + r < f.h ? i0 + r : f.h - 1;
            const unsigned char* row = f.p0 + (long long)i * f.pitch0;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int j = j0 + c < f.w ? j0 + c : f.w - 1;
                const unsigned char* p = row + (long long)j * 3;
                const int B = p[0], G = p[1], R = p[2];
                y4[r * 2 + c] = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
                sb += -11059 * R - 21709 * G + 32768 * B;
                sr += 32768 * R - 27439 * G - 5329 * B;
            }
        }
        *cb = jp_clamp255(((sb + (1 << 17)) >> 18) + 128);
        *cr = jp_clamp255(((sr + (1 << 17)) >> 18) + 128);
    }
};
struct JpNv12Src {                      // bt601f: the planes are JFIF already
    static constexpr int FORMAT = 1;
    static __device__ __forceinline__ void quad(const JpFrame& f, int i0, int j0, int* y4, int* cb, int* cr) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = i0 + r < f.h ? i0 + r : f.h - 1;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int j = j0 + c < f.w ? j0 + c : f.w - 1;
                y4[r * 2 + c] = f.p0[(long long)i * f.pitch0 + j];
            }
        }
        const int ci = (i0 < f.h ? i0 : f.h - 1) >> 1, cj = (j0 < f.w ? j0 : f.w - 1) >> 1;
        const unsigned pair = *reinterpret_cast<const unsigned short*>(f.p1 + (long long)ci * f.pitch1 + cj * 2);
        *cb = (int)(pair & 255u);
        *cr = (int)(pair >> 8);
    }
};

// grid (ceil(most MCUs of a frame / 4), frames of this launch), block 256: wave v of workgroup x owns MCU 4x + v of its frame.
template <typename SRC>
__global__ __launch_bounds__(256) void jpeg_dct_kernel(const JpTable tab, const JpQuant qt, short* __restrict__ coef) {
    __shared__ int s_a[4][6][64];
    __shared__ int s_b[4][6][64];
    const JpFrame f = tab.f[blockIdx.y];
    if (f.format != SRC::FORMAT || (int)blockIdx.x * 4 >= f.n_mcu) return;         // uniform over the workgroup
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int mcu_raw = blockIdx.x * 4 + wave;
    const bool valid = mcu_raw < f.n_mcu;
    const int mcu = valid ? mcu_raw : f.n_mcu - 1;      // a spare wave repeats the last MCU and stores nothing
    const int my = mcu / f.mcux, mx = mcu - my * f.mcux;
    {
        const int cy = l >> 3, cx = l & 7;
        int y4[4], cb, cr;
        SRC::quad(f, my * 16 + 2 * cy, mx * 16 + 2 * cx, y4, &cb, &cr);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int rr = 2 * cy + r, cc = 2 * cx + c;
                s_a[wave][(rr >> 3) * 2 + (cc >> 3)][(rr & 7) * 8 + (cc & 7)] = y4[r * 2 + c] - 128;
            }
        s_a[wave][4][l] = cb - 128;
        s_a[wave][5][l] = cr - 128;
    }
    __syncthreads();
    const int hi = l >> 3, lo = l & 7;
    int mrow[8], mcol[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) { mrow[n] = JP_M[lo * 8 + n]; mcol[n] = JP_M[hi * 8 + n]; }
#pragma unroll
    for (int b = 0; b < 6; ++b) {       // row pass: t[r = hi][k = lo]
        int acc = 0;
#pragma unroll
        for (int n = 0; n < 8; ++n) acc += s_a[wave][b][hi * 8 + n] * mrow[n];
        s_b[wave][b][l] = (acc + 128) >> 8;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 6; ++b) {       // column pass: coef[k = hi][c = lo]
        int acc = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) acc += mcol[r] * s_b[wave][b][r * 8 + lo];
        s_a[wave][b][l] = (acc + 32768) >> 16;
    }
    __syncthreads();
    const int nat = JP_ZZ[l];
    short* o = coef + (f.mcu_base + mcu) * 384 + l;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const int c = s_a[wave][b][nat], t = b >> 2;
        const unsigned a = (unsigned)(c < 0 ? -c : c);
        const int v = (int)(((a + (qt.q[t][nat] >> 1)) * qt.rcp[t][nat]) >> 20);     // == (a + q / 2) / q (tests/test_jpeg_cpu.py)
        if (valid) o[b * 64] = (short)(c < 0 ? -v : v);
    }
}

// Exclusive scan of one int per lane over the 256 lanes of a workgroup; *total = the sum.  Every lane must call it.
__device__ __forceinline__ int jp_scan256(int v, int* s, int tid, int* total) {
    __syncthreads();                    // the last use of s is over
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int t = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    *total = s[255];
    return s[tid] - v;
}

// The bits of a block, merged into the LDS bit buffer: bit p of the stream is bit 31 - p % 32 of word p / 32.
struct JpEmit {
    unsigned* buf;
    unsigned long long acc;
    int n, w;
    __device__ __forceinline__ JpEmit(unsigned* b, int bit0) : buf(b), acc(0), n(bit0 & 31), w(bit0 >> 5) {}
    __device__ __forceinline__ void put(unsigned code, int len) {        // len <= 26
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            n -= 32;
            if (w < JP_WORDS) atomicOr(&buf[w], (unsigned)(acc >> n));
            ++w;
            acc &= (1ull << n) - 1ull;
        }
    }
    __device__ __forceinline__ void flush() {
        if (n > 0 && w < JP_WORDS) atomicOr(&buf[w], (unsigned)(acc << (32 - n)));
    }
};
struct JpCount {
    int bits = 0;
    __device__ __forceinline__ void put(unsigned, int len) { bits += len; }
};

__device__ __forceinline__ int jp_size(int v) { return 32 - __clz(v < 0 ? -v : v); }        // 0 for 0
__device__ __forceinline__ unsigned jp_value(int v, int s) { return (unsigned)(v > 0 ? v : v + (1 << s) - 1) & ((1u << s) - 1u); }

// One block: the DC difference against `pred`, then the AC run/size symbols (hdc, hac: the component's tables in LDS).
template <typename SINK>
__device__ __forceinline__ void jp_code_block(const short* blk, int pred, const unsigned* hdc, const unsigned* hac, SINK& out) {
    const uint4* src = reinterpret_cast<const uint4*>(blk);
    int run = 0;
    for (int g = 0; g < 8; ++g) {
        const uint4 q = src[g];
        const unsigned wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = (int)(short)(wd[e >> 1] >> (16 * (e & 1)));
            if (g == 0 && e == 0) {
                const int d = c - pred;
                int s = jp_size(d);
                s = s > 11 ? 11 : s;
                const unsigned h = hdc[s];
                out.put(h >> 5, (int)(h & 31u));
                if (s) out.put(jp_value(d, s), s);
            } else if (c == 0) {
                ++run;
            } else {
                while (run >= 16) {
                    out.put(hac[0xF0] >> 5, (int)(hac[0xF0] & 31u));
                    run -= 16;
                }
                int s = jp_size(c);
                s = s > 10 ? 10 : s;
                const unsigned h = hac[(run << 4) | s];
                out.put(h >> 5, (int)(h & 31u));
                out.put(jp_value(c, s), s);
                run = 0;
            }
        }
    }
    if (run > 0) out.put(hac[0] >> 5, (int)(hac[0] & 31u));      // EOB, unless coefficient 63 is nonzero
}

// grid (most intervals of a frame, frames of this launch), block 256: interval x of frame y; lane t < 6 * MCUs codes block t.
template <bool WRITE>
__global__ __launch_bounds__(256) void jpeg_entropy_kernel(const JpTable tab, int restart, const short* __restrict__ coef,
                                                          int* __restrict__ lens, const int* __restrict__ offs,
                                                          unsigned char* __restrict__ out, long long cap) {
    __shared__ unsigned s_bits[JP_WORDS];
    __shared__ unsigned s_huff[JP_HUFF_WORDS];
    __shared__ int s_scan[256];
    const JpFrame f = tab.f[blockIdx.y];
    const int it = blockIdx.x, tid = threadIdx.x;
    if (it >= f.n_int) return;
    int off = 0;
    if (WRITE) {
        off = offs[f.int_base + it];
        if (off < 0) return;            // the file does not fit: nothing of it is written
    }
    const int m0 = it * restart;
    const int nm = f.n_mcu - m0 < restart ? f.n_mcu - m0 : restart;
    const int nb = nm * 6;
    for (int i = tid; i < JP_HUFF_WORDS; i += 256) s_huff[i] = reinterpret_cast<const unsigned*>(&JP_HUFF)[i];
    __syncthreads();

    const short* blk = coef + (f.mcu_base + m0) * 384 + tid * 64;
    const int b = tid % 6, comp = b >> 2;       // comp: 0 luma tables, 1 chroma tables
    const unsigned* hdc = s_huff + comp * 16;
    const unsigned* hac = s_huff + 32 + comp * 256;
    int pred = 0;
    if (tid < nb) {                     // the DC of the block before it in its component, 0 at the interval's start
        if (b >= 1 && b <= 3) pred = blk[-64];
        else if (tid >= 6) pred = b == 0 ? blk[-3 * 64] : blk[-6 * 64];
    }
    JpCount cnt;
    if (tid < nb) jp_code_block(blk, pred, hdc, hac, cnt);
    int total_bits;
    const int bit0 = jp_scan256(cnt.bits, s_scan, tid, &total_bits);
    const int n_bytes = (total_bits + 7) >> 3;
    for (int i = tid; i < (n_bytes + 3) / 4 && i < JP_WORDS; i += 256) s_bits[i] = 0u;
    __syncthreads();
    if (tid < nb) {
        JpEmit em(s_bits, bit0);
        jp_code_block(blk, pred, hdc, hac, em);
        em.flush();
    }
    if (tid == 0) {                     // 1-bits up to the byte boundary
        const int pad = (8 - (total_bits & 7)) & 7, w = total_bits >> 5;
        if (pad && w < JP_WORDS) atomicOr(&s_bits[w], ((1u << pad) - 1u) << (32 - (total_bits & 31) - pad));
    }
    __syncthreads();
    // stuffing: lane t owns bytes [t * chunk, (t + 1) * chunk)
    const int chunk = (n_bytes + 255) / 256;
    const int i0 = tid * chunk < n_bytes ? tid * chunk : n_bytes;
    const int i1 = i0 + chunk < n_bytes ? i0 + chunk : n_bytes;
    int ff = 0;
    for (int i = i0; i < i1; ++i) ff += ((s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u) == 255u;
    int total_ff;
    const int ff0 = jp_scan256(ff, s_scan, tid, &total_ff);
    if (!WRITE) {
        if (tid == 0) lens[f.int_base + it] = n_bytes + total_ff;
    } else {
        unsigned char* dst = out + (long long)blockIdx.y * cap + off + i0 + ff0;
        for (int i = i0; i < i1; ++i) {
            const unsigned v = (s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
            *dst++ = (unsigned char)v;
            if (v == 255u) *dst++ = 0;
        }
    }
}

// grid (frames of this launch), block 256.
__global__ __launch_bounds__(256) void jpeg_scan_kernel(const JpTable tab, const int* __restrict__ lens, int* __restrict__ offs,
                                                       const unsigned char* __restrict__ headers, int header_len,
                                                       unsigned char* __restrict__ out, long long cap, int* __restrict__ nbytes) {
    __shared__ int s_scan[256];
    const JpFrame f = tab.f[blockIdx.x];
    const int tid = threadIdx.x;
    const int* len = lens + f.int_base;
    int* of = offs + f.int_base;
    long long carry = header_len;       // where the next block of intervals begins
    for (int base = 0; base < f.n_int; base += JP_SCAN) {
        const int i = base + tid;
        const int v = i < f.n_int ? len[i] + 2 : 0;     // every interval is followed by RSTm or EOI
        int total;
        const int e = jp_scan256(v, s_scan, tid, &total);
        const long long at = carry + e;
        if (i < f.n_int) of[i] = at > 0x7fffffffLL ? 0x7fffffff : (int)at;
        carry += total;
    }
    unsigned char* o = out + (long long)blockIdx.x * cap;
    if (carry > cap) {
        for (int i = tid; i < f.n_int; i += 256) of[i] = -1;
        if (tid == 0) nbytes[blockIdx.x] = carry > 0x7fffffffLL ? -0x7fffffff : -(int)carry;
        return;
    }
    const unsigned char* h = headers + (long long)blockIdx.x * header_len;
    for (int i = tid; i < header_len; i += 256) o[i] = h[i];
    for (int i = tid; i < f.n_int; i += 256) {          // this lane wrote of[i] itself
        unsigned char* m = o + of[i] + len[i];
        m[0] = 0xFF;
        m[1] = (unsigned char)(i < f.n_int - 1 ? 0xD0 + (i & 7) : 0xD9);
    }
    if (tid == 0) nbytes[blockIdx.x] = (int)carry;
}

// The frames of a call as table entries, and the workspace: int16 [MCUs][6][64], int32 lengths [intervals], int32 offsets
// [intervals].  An empty string: fine.
struct JpLayout {
    std::vector<JpFrame> f;
    long long mcus = 0, ints = 0;
    size_t bytes = 0;
};
std::string jp_layout(const lp_jpeg_desc* desc, int n, int restart, JpLayout* L) {
    if (n < 0 || (n > 0 && !desc)) return "bad arguments (need n_frames >= 0 and desc)";
    if (restart < 1 || restart > LP_JPEG_MAX_RESTART)
        return "restart must be in 1.." + std::to_string(LP_JPEG_MAX_RESTART) + ", got " + std::to_string(restart);
    L->f.resize((size_t)n);
    for (int b = 0; b < n; ++b) {
        const lp_jpeg_desc& d = desc[b];
        const std::string what = " (frame " + std::to_string(b) + ")";
        if (d.h0 < 1 || d.w0 < 1 || d.h0 > 65535 || d.w0 > 65535) return "h0 and w0 must be in 1..65535" + what;
        if (d.format == 0) {
            if (!d.p0 || d.p1) return "a BGR frame needs p0 and a null p1" + what;
            if (d.pitch0 < 3 * d.w0) return "pitch0 < 3 * w0" + what;
        } else if (d.format == 1) {
            const std::string why = plane_fault(d.p0, d.p1, d.pitch0, d.pitch1, d.h0, d.w0, d.matrix);
            if (!why.empty()) return why + what;
            if (d.matrix != JP_NV12_JFIF) return "an NV12 frame must be bt601f (matrix 2): convert the others with lp_nv12_to_bgr_batch" + what;
        } else {
            return "unknown format" + what;
        }
        JpFrame& e = L->f[b];
        e.p0 = d.p0; e.p1 = d.p1; e.pitch0 = d.pitch0; e.pitch1 = d.pitch1; e.h = d.h0; e.w = d.w0; e.format = d.format;
        e.mcux = ceil_div(d.w0, 16);
        e.n_mcu = e.mcux * ceil_div(d.h0, 16);
        e.n_int = ceil_div(e.n_mcu, restart);
        e.mcu_base = L->mcus;
        e.pad_ = 0;
        if (L->ints + e.n_int > 0x7fffffffLL) return "too many restart intervals in one call" + what;
        e.int_base = (int)L->ints;
        L->mcus += e.n_mcu;
        L->ints += e.n_int;
    }
    L->bytes = (size_t)L->mcus * 768 + (((size_t)L->ints * 8 + 15) & ~(size_t)15);
    return "";
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" size_t lp_jpeg_workspace_bytes(const lp_jpeg_desc* desc, int n_frames, int restart) {
    JpLayout L;
    return jp_layout(desc, n_frames, restart, &L).empty() ? L.bytes : 0;
}

extern "C" int lp_jpeg_encode_batch(const lp_jpeg_desc* desc, int n_frames, const lp_jpeg_params* params, const unsigned char* headers,
                                    int header_len, unsigned char* out, size_t cap, int32_t* nbytes, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const std::string fn = "lp_jpeg_encode_batch: ";
    if (!params) return fail(LP_ERR_ARG, fn + "null params");
    if (params->quality < 1 || params->quality > 100)
        return fail(LP_ERR_ARG, fn + "quality must be in 1..100, got " + std::to_string(params->quality));
    JpLayout L;
    const std::string why = jp_layout(desc, n_frames, params->restart, &L);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    if (n_frames == 0) return LP_OK;
    if (!headers || header_len < 1 || !out || !nbytes || cap < 1 || cap > 0x7fffffffULL)
        return fail(LP_ERR_ARG, fn + "bad arguments (need headers, header_len >= 1, out, nbytes, 1 <= cap < 2^31)");
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < L.bytes)
        return fail(LP_ERR_ARG, fn + "the workspace must be 16-byte aligned and hold " + std::to_string(L.bytes) + " bytes");

    JpQuant qt;
    const int q = params->quality, s = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            int v = (JP_BASE[t][i] * s + 50) / 100;
            v = v < 1 ? 1 : (v > 255 ? 255 : v);
            qt.q[t][i] = (unsigned short)v;
            qt.rcp[t][i] = (unsigned)(((1 << 20) + v - 1) / v);
        }
    short* coef = (short*)workspace;
    int* lens = (int*)((char*)workspace + (size_t)L.mcus * 768);
    int* offs = lens + L.ints;
    hipStream_t st = (hipStream_t)stream;
    const int restart = params->restart;
    for (int b0 = 0; b0 < n_frames; b0 += JP_SLOTS) {
        const int nf = n_frames - b0 < JP_SLOTS ? n_frames - b0 : JP_SLOTS;
        JpTable tab = {};
        int most_mcu = 1, most_int = 1;
        bool any[2] = {false, false};
        for (int j = 0; j < nf; ++j) {
            tab.f[j] = L.f[b0 + j];
            most_mcu = tab.f[j].n_mcu > most_mcu ? tab.f[j].n_mcu : most_mcu;
            most_int = tab.f[j].n_int > most_int ? tab.f[j].n_int : most_int;
            any[tab.f[j].format] = true;
        }
        unsigned char* o = out + (size_t)b0 * cap;
        const dim3 gd((unsigned)ceil_div(most_mcu, 4), (unsigned)nf), ge((unsigned)most_int, (unsigned)nf);
        if (any[0]) hipLaunchKernelGGL(jpeg_dct_kernel<JpBgrSrc>, gd, dim3(256), 0, st, tab, qt, coef);
        if (any[1]) hipLaunchKernelGGL(jpeg_dct_kernel<JpNv12Src>, gd, dim3(256), 0, st, tab, qt, coef);
        hipLaunchKernelGGL(jpeg_entropy_kernel<false>, ge, dim3(256), 0, st, tab, restart, (const short*)coef, lens, (const int*)offs, o,
                           (long long)cap);
        hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)nf), dim3(256), 0, st, tab, (const int*)lens, offs,
                           headers + (size_t)b0 * header_len, header_len, o, (long long)cap, nbytes + b0);
        hipLaunchKernelGGL(jpeg_entropy_kernel<true>, ge, dim3(256), 0, st, tab, restart, (const short*)coef, lens, (const int*)offs, o,
                           (long long)cap);
        LP_HIP_CHECK(hipGetLastError());
    }
    return LP_OK;
}
