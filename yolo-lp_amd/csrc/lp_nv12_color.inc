// The NV12 colour rule of lp_frames.hip (the letterbox's NV12 source) and lp_nv12.hip (the converter); include inside an
// unnamed namespace of namespace lp.  The specification is yolov6/utils/nv12.py.  For pixel (i, j) of an h0 x w0 frame (both
// even) with planes y [h0][pitch_y] and uv [h0/2][pitch_uv] (U, V pairs):
//     Y = y[i][j], U = uv[i >> 1][2 (j >> 1)], V = uv[i >> 1][2 (j >> 1) + 1]        (chroma replicated, not interpolated)
//     c = max(Y - yoff, 0) * CY;  d = U - 128;  e = V - 128;  half = 1 << 19         (int32, arithmetic shifts)
//     R = clamp255((c + half + CVR e) >> 20), G = clamp255((c + half + CVG e + CUG d) >> 20), B = clamp255((c + half + CUB d) >> 20)
// with the integers of NV_MAT below (|accumulator| < 5.9e8 over all 2^24 triples).
constexpr int NV_SHIFT = 20;
constexpr int NV_HALF = 1 << (NV_SHIFT - 1);
constexpr int NV_MATRICES = 4;

struct NvMat { int yoff, cy, cub, cug, cvg, cvr; };
__constant__ NvMat NV_MAT[NV_MATRICES] = {
    {16, 1220542, 2116026, -409993, -852492, 1673527},      // 0 bt601, limited range (OpenCV's COLOR_YUV2BGR_NV12 table)
    {16, 1220945, 2215014, -223607, -558796, 1879825},      // 1 bt709, limited range
    {0, 1048576, 1858077, -360853, -748826, 1470104},       // 2 bt601, full range
    {0, 1048576, 1945738, -196424, -490864, 1651297},       // 3 bt709, full range
};

struct Chroma { int b, g, r; };         // the chroma terms of one UV pair

__device__ __forceinline__ Chroma chroma_of(unsigned pair, const NvMat& m) {     // pair: U | V << 8
    const int d = (int)(pair & 255u) - 128, e = (int)(pair >> 8) - 128;
    return {m.cub * d, m.cvg * e + m.cug * d, m.cvr * e};
}
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ void bgr_of(int Y, const Chroma& ch, const NvMat& m, int* bgr) {
    const int c0 = Y - m.yoff;
    const int c = (c0 < 0 ? 0 : c0) * m.cy + NV_HALF;
    bgr[0] = clamp255((c + ch.b) >> NV_SHIFT);
    bgr[1] = clamp255((c + ch.g) >> NV_SHIFT);
    bgr[2] = clamp255((c + ch.r) >> NV_SHIFT);
}
__device__ __forceinline__ unsigned ld16(const unsigned char* p) { return *reinterpret_cast<const unsigned short*>(p); }
