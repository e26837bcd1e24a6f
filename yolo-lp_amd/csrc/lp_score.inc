// The per-anchor arithmetic of non_max_suppression's candidate selection (yolov6/utils/nms.py:76-96,120), shared by
// score_kernel (lp_nms.hip: reads the [B,N,290] prediction tensor) and the detections-only class-predictor kernel
// (lp_head_rows.inc: reads the sigmoids it has just staged in LDS).  Everything is fp32, op by op in the reference's order.
#pragma once
#include "lp_internal.h"

namespace lp {

// (value, index) max with torch.max's tie rule: the smaller index wins among equal values.  NAN_AWARE: a NaN beats every number, and
// among NaNs the smaller index wins (ATen: the first NaN sticks).  Either form is commutative, associative and idempotent.
template <bool NAN_AWARE> __device__ __forceinline__ void argmax_combine(float& v, int& i, float ov, int oi) {
    if (NAN_AWARE) {
        const bool on = ov != ov, vn = v != v;
        if (on ? (!vn || oi < i) : (!vn && (ov > v || (ov == v && oi < i)))) { v = ov; i = oi; }
    } else {
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// Rotate-within-16-lanes DPP move (row_ror:n): lane j of each 16-lane row receives lane (j - n) mod 16.
template <int N> __device__ __forceinline__ float ror16f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + N, 0xf, 0xf, false));
}
template <int N> __device__ __forceinline__ int ror16i(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x120 + N, 0xf, 0xf, false); }

// 16 lanes own one anchor row: lane j holds v[k] = column COL0 + j + 16 k (0 where that is past column 289).  Eight
// (max, FIRST arg-max) reductions over the heads' column groups [13,44) [44,68) [68,105) ... [253,290): every lane folds
// its own columns in ascending order (first maximum wins), then four rotate steps (1,2,4,8) of a (value, index)
// max-combine leave every lane of the group with the head's result (the combine is commutative, associative and idempotent,
// so a rotate all-reduce is exact).  NAN_AWARE: a NaN column wins its head and the first one sticks, as in torch.max.
template <int COL0, int NK, bool NAN_AWARE>
__device__ __forceinline__ void score_heads_fold(const float (&v)[NK], int j, float (&cf)[8], int (&ci)[8]) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        constexpr int SEGS[9] = {13, 44, 68, 105, 142, 179, 216, 253, 290};
        const int a = SEGS[s] - COL0, b = SEGS[s + 1] - COL0;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            if (16 * k + 15 < a || 16 * k >= b) continue;            // compile-time: slot k cannot touch head s
            const int c = j + 16 * k;
            const bool take = NAN_AWARE ? bv == bv && (v[k] > bv || v[k] != v[k]) : v[k] > bv;
            if (c >= a && c < b && take) { bv = v[k]; bi = c - a; }   // ascending columns: first maximum stays
        }
        { const float ov = ror16f<1>(bv); const int oi = ror16i<1>(bi); argmax_combine<NAN_AWARE>(bv, bi, ov, oi); }
        { const float ov = ror16f<2>(bv); const int oi = ror16i<2>(bi); argmax_combine<NAN_AWARE>(bv, bi, ov, oi); }
        { const float ov = ror16f<4>(bv); const int oi = ror16i<4>(bi); argmax_combine<NAN_AWARE>(bv, bi, ov, oi); }
        { const float ov = ror16f<8>(bv); const int oi = ror16i<8>(bi); argmax_combine<NAN_AWARE>(bv, bi, ov, oi); }
        cf[s] = bv;
        ci[s] = bi;
    }
}
// NaN: torch.max returns the FIRST NaN of a head and its index, where `v > bv` drops it.  A second compare per column would
// double the fold's compares, so the wave first learns whether any of its class columns MAY be NaN from the unsigned maximum of
// their bit patterns -- one v_max3_u32 per two columns and one ballot: a pattern above +inf's is a NaN or has the sign bit set (a
// negative value or -0, which a probability times obj = 1 never is) -- and takes the NaN-aware fold only then: never, on the
// head's own output.  The choice is wave-uniform (every lane of a row group takes part in the rotates of either fold), and the
// NaN-aware fold is right for every input, so a false alarm costs time only.
template <int COL0, int NK>
__device__ __forceinline__ void score_heads(const float (&v)[NK], int j, float (&cf)[8], int (&ci)[8]) {
    unsigned top = 0u;
#pragma unroll
    for (int k = 0; k < NK; k += 2) {
        unsigned u0 = __float_as_uint(v[k]), u1 = k + 1 < NK ? __float_as_uint(v[k + 1]) : 0u;
        if (16 * k < 13 - COL0) u0 = j + 16 * k >= 13 - COL0 ? u0 : 0u;     // (the box / corner columns in front of the heads do not count)
        if (16 * (k + 1) < 13 - COL0) u1 = j + 16 * (k + 1) >= 13 - COL0 ? u1 : 0u;
        const unsigned m = u0 > u1 ? u0 : u1;
        top = top > m ? top : m;
    }
    if (__builtin_expect(__ballot(top > 0x7f800000u) != 0ull, 0)) score_heads_fold<COL0, NK, true>(v, j, cf, ci);
    else score_heads_fold<COL0, NK, false>(v, j, cf, ci);
}
// keep-mask value (ad4 twice, ad5 omitted: the reference's quirk) and score: plain left-to-right sums, then / 8
__device__ __forceinline__ float score_mask_value(const float (&cf)[8]) {
    float m = cf[0] + cf[1]; m = m + cf[2]; m = m + cf[3]; m = m + cf[4]; m = m + cf[5];
    m = m + cf[6]; m = m + cf[6]; m = m / 8.0f;
    return m;
}
__device__ __forceinline__ float score_value(const float (&cf)[8]) {
    float sc = cf[0] + cf[1]; sc = sc + cf[2]; sc = sc + cf[3]; sc = sc + cf[4]; sc = sc + cf[5];
    sc = sc + cf[6]; sc = sc + cf[7]; sc = sc / 8.0f;
    return sc;
}
// sort key of a candidate: descending score, then ascending anchor index
__device__ __forceinline__ unsigned long long score_key(float sc, int anchor) {
    unsigned u = __float_as_uint(sc);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // ascending-orderable bits
    if (sc != sc) u = 0xffffffffu;                    // a NaN of either sign sorts before every number, as in torch's descending sort
    return ((unsigned long long)(~u) << 32) | (unsigned)anchor;
}

}  // namespace lp
