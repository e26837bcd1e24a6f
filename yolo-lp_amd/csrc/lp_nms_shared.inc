// Device pieces of the NMS that lp_nms.hip (per-image NMS) and lp_tiles.hip (cross-tile merge) share: the compare-exchange step of the
// bitonic sort over 64-bit candidate keys, and torchvision's IoU predicate.
#pragma once
#include "lp_internal.h"

namespace lp {

static constexpr int SORT_LDS_KEYS = 16384;  // keys per LDS block of the sort (128 KiB)
static constexpr int SORT_T = 1024;
template <typename P>
__device__ __forceinline__ void bitonic_step(P d, int count, int g0, int k, int j) {   // one compare-exchange step over d[0 .. count)
    for (int p = threadIdx.x; p < count / 2; p += SORT_T) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), ixj = i | j;
        const unsigned long long a = d[i], c = d[ixj];
        const bool up = ((g0 + i) & k) == 0;
        if ((a > c) == up) { d[i] = c; d[ixj] = a; }
    }
}

// torchvision's predicate `inter / (area_i + area_j - inter) > iou_threshold`, fp32 op by op, without the division for
// (nearly) every pair.  With U = fl(fl(area_i + area_j) - inter), t = thr_f (the largest fp32 <= the double threshold, so that
// (double)ovr > iou_thres <=> ovr > t) and ovr = fl(inter / U) (round to nearest): ovr > t  <=>  inter / U >= m (resp. > m),
// m = the midpoint of t and the next fp32 above it, i.e. m = t (1 + e) with 0 < e <= 2^-24.  Let p = fl(t U) = t U (1 + d),
// |d| <= 2^-24, p and t normal and positive (then U > 0):
//   inter > fl(p (1 + 2^-20))  =>  inter > t U (1 - 2^-24)^2 (1 + 2^-20) > t U (1 + 2^-21) > m U   =>  ovr > t;
//   inter < fl(p (1 - 2^-20))  =>  inter < t U (1 + 2^-24)^2 (1 - 2^-20) < t U < m U               =>  not.
// Only inside that 2^-19-wide band -- and for U <= 0, NaN, infinities, a zero threshold or a subnormal product, where every
// comparison below is false -- the IEEE division decides, as before.  An fp32 division is ~11 dependent VALU instructions, the
// two products and compares are 5.  lp_check_iou_predicate runs both forms side by side (tests/test_hip_kernels.py).
template <bool EXACT_ONLY = false>
__device__ __forceinline__ bool iou_gt(float ix1, float iy1, float ix2, float iy2, float iarea, float jx1, float jy1,
                                      float jx2, float jy2, float thr_f) {
    const float xx1 = ix1 > jx1 ? ix1 : jx1;
    const float yy1 = iy1 > jy1 ? iy1 : jy1;
    const float xx2 = ix2 < jx2 ? ix2 : jx2;
    const float yy2 = iy2 < jy2 ? iy2 : jy2;
    float w = xx2 - xx1;
    if (!(w > 0.f)) w = 0.f;
    float h = yy2 - yy1;
    if (!(h > 0.f)) h = 0.f;
    // disjoint boxes (most pairs): inter = 0 * h or w * 0 is 0 (or NaN for an infinite side), the quotient 0, -0 or NaN, and
    // none of them is > thr_f >= 0 -- the same answer without the division
    if (w == 0.f || h == 0.f) return false;
    const float inter = w * h;
    const float jarea = (jx2 - jx1) * (jy2 - jy1);
    const float u = iarea + jarea - inter;
    if (!EXACT_ONLY) {
        const float p = thr_f * u;
        const bool normal = p >= 1.17549435e-38f && thr_f >= 1.17549435e-38f;   // FLT_MIN: the bounds on p and on m need normal numbers
        if (normal && inter > p * 1.00000095367431640625f) return true;      // 1 + 2^-20
        if (normal && inter < p * 0.99999904632568359375f) return false;     // 1 - 2^-20
    }
    const float ovr = inter / u;
    return ovr > thr_f;   // thr_f = largest fp32 <= the double threshold  <=>  (double)ovr > iou_thres
}

}  // namespace lp
