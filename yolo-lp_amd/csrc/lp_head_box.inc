// Box / corner predictors of the detections-only forward as a streaming kernel (round 3): reg_preds + cor_preds (one 1x1 conv,
// <= 32 output channels: 4 box distances + 8 corner offsets), anchor-free decode, columns 0..11 of EVERY anchor's candidate row.
//
// The generic kernel (conv_mfma_kernel<CFG_C, 1, 1, MODE_DECODE>) gives this op -- 26 MB in, 10 MB out and 0.3 GFLOP at the
// 80x80 level -- one short-lived workgroup per 256 anchors whose DMA -> barrier -> MFMA -> LDS staging -> decode phases do not
// overlap: 22 / 11 / 10.5 us for the three levels of yololps at batch 32.  Here a wave owns 32 anchors at a time: the weights of
// all K steps stay in its registers (A fragments), the pixel operand comes straight from memory into the B registers as in
// conv1x1_stream_kernel, and every lane decodes and stores what the accumulator layout leaves it with -- lane (anchor, 0): box
// distances (couts 0..3) and corners 4..7 (couts 8..11), lane (anchor, 1): corners 0..3 (couts 4..7) -- as 16-byte stores.  No LDS,
// no barrier.
// Same bits as the generic kernel (tested: route "det" against route "pred"): accumulators start at the bias, the K steps come in
// the same order (chunk-major, 32-byte K-steps) with the same operand positions, K-steps beyond the stored channels multiply the
// zero page by zero weights, and the decode arithmetic is its det_mode branch op by op (-ffp-contract=off).
// SPARSE form (round 4): the same computation for the anchors that PASSED the class predictors' confidence mask only.  The class kernel of
// the level (head_det_kernel / score_kernel) has run before this one on the same stream and has appended its candidates to the images' key
// lists; the entries [det_prev[b], det_cnt[b]) of image b are this level's (det_prev = the snapshot the box kernel of the level before
// left in det_snap; the first level starts at 0).  A wave gathers 32 of those anchors (the anchor index is the low word of the sort key) as
// the pixel operand: a column of an MFMA tile does not depend on its neighbours, so the rows written are bit for bit the dense form's -- the
// rows of anchors that did not pass are never read by lp_nms_candidates and stay unwritten.  26 MB in / 23 MB out at the 80x80 level become
// ~0.3 MB each at the bench's pass rate (3.5 %).
// Reference semantics: Detect.forward eval branch, reg_preds / cor_preds + dist2bbox / dist2cor (effidehead.py:262-301,
// utils/general.py:29-66), followed by non_max_suppression's xywh2xyxy (nms.py:100-101).
#pragma once
#include "lp_conv_kernel.inc"

namespace lp {

template <typename T, int NCH, bool SPARSE>
__global__ __launch_bounds__(256) void head_box_det_kernel(const ConvArgs a, const int cb_pack, const int gpi) {
    typedef typename Mma<T>::V V;
    constexpr int SZ = sizeof(T), EPG = 16 / SZ, ROWB = 128, NKB = 4, GPR = 8, NK = NCH * NKB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int HW = a.Ho * a.Wo;
    const long long M = (long long)a.B * HW;
    long long ntiles = (M + 31) / 32;
    long long t0 = (long long)blockIdx.x * 4 + wave, tstride = (long long)gridDim.x * 4;
    [[maybe_unused]] int sb = 0, slo = 0, sn = 0;                 // SPARSE: image of this workgroup, first entry and number of entries of this level in its key list
    if constexpr (SPARSE) {
        sb = blockIdx.x / gpi;
        const int gi = blockIdx.x - sb * gpi;
        int hi = a.det_cnt[sb];
        hi = hi > a.det_np ? a.det_np : hi;                       // (keys beyond the list's capacity were dropped by the class kernel)
        slo = a.det_prev ? a.det_prev[sb] : 0;
        slo = slo < 0 ? 0 : (slo > hi ? hi : slo);
        sn = hi - slo;
        if (gi == 0 && threadIdx.x == 0) a.det_snap[sb] = hi;     // where the next level's entries begin
        ntiles = (sn + 31) / 32;
        t0 = (long long)gi * 4 + wave;
        tstride = (long long)gpi * 4;
    } else if (a.det_snap) {                                      // dense form in front of a level that may run sparse: the same snapshot, one thread per image
        const int b = blockIdx.x * 256 + threadIdx.x;
        if (b < a.B) { const int c = a.det_cnt[b]; a.det_snap[b] = c > a.det_np ? a.det_np : c; }
    }
    if (t0 >= ntiles) return;

    V wa[NK];                                   // A fragments of all K steps: row r of the 32-cout tile, K half h
#pragma unroll
    for (int k = 0; k < NK; ++k)
        wa[k] = *(const V*)((const char*)a.w + ((long long)(k / NKB) * cb_pack + r) * ROWB + swz(r, 2 * (k % NKB) + h, GPR) * 16);
    f32x16 bias;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg)
#pragma unroll
        for (int j = 0; j < 4; ++j) bias[4 * rg + j] = a.bias[8 * rg + 4 * h + j];
    const char* const src = (const char*)a.src[0].ptr;
    const int cs = a.src[0].cs;
    const int ngran = cs / EPG;                 // 16-byte granules that exist in a source row; a lane's granule beyond them reads the zero page
    const float sp = a.stride_px;

    for (long long t = t0; t < ntiles; t += tstride) {
        long long m = t * 32 + r;
        bool live = m < M;
        if constexpr (SPARSE) {
            live = m < sn;
            const unsigned long long key = a.det_keys[(long long)sb * a.det_np + slo + (live ? m : 0)];
            const int n_ = (int)(unsigned)key - a.det_anchor0;            // anchor of this level (the key's low word is the image's anchor index)
            live = live && n_ >= 0 && n_ < HW;
            m = (long long)sb * HW + (live ? n_ : 0);
        }
        const char* const row = src + (live ? m : M - 1) * (long long)cs * SZ + h * 16;
        V vb[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) vb[k] = *(const V*)(2 * k + h < ngran ? row + k * 32 : (const char*)a.zero);
        __builtin_amdgcn_sched_barrier(0);      // all K steps' loads in flight together (left alone the compiler sent them one by one
        f32x16 acc = bias;                      // through a single register quad: load -> wait -> MFMA, a memory round trip per K step)
#pragma unroll
        for (int k = 0; k < NK; ++k) acc = Mma<T>::mma(wa[k], vb[k], acc);
        if (!live) continue;
        const int b = (int)(m / HW), n = (int)(m - (long long)b * HW);
        const int oy = n / a.Wo, ox = n - oy * a.Wo;
        const float ax = (float)ox + 0.5f, ay = (float)oy + 0.5f;
        float* const o = (float*)a.out + (long long)b * a.out_img_stride + (long long)n * a.out_pix_stride;
        if (h == 0) {
            // what score_kernel (lp_nms.hip) derives from prediction columns 0..3, in its operation order (see MODE_DECODE, det_mode)
            const float x1 = ax - acc[0], y1 = ay - acc[1], x2 = ax + acc[2], y2 = ay + acc[3];
            const float cx = ((x1 + x2) / 2.f) * sp, cy = ((y1 + y2) / 2.f) * sp, bw = (x2 - x1) * sp, bh = (y2 - y1) * sp;
            const f32x4 v0 = {cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2};
            const f32x4 v2 = {(ax + acc[4]) * sp, (ay + acc[5]) * sp, (ax + acc[6]) * sp, (ay - acc[7]) * sp};
            *(f32x4*)o = v0;
            *(f32x4*)(o + 8) = v2;
        } else {
            const f32x4 v1 = {(ax - acc[0]) * sp, (ay - acc[1]) * sp, (ax - acc[2]) * sp, (ay + acc[3]) * sp};
            *(f32x4*)(o + 4) = v1;
        }
    }
}

template <typename T, int NCH>
static inline int head_box_det_launch_one(const ConvArgs& a, int cb_pack, hipStream_t st) {
    const long long ntiles = ((long long)a.B * a.Ho * a.Wo + 31) / 32;
    long long grid = (ntiles + 3) / 4;
    if (grid > 2048) grid = 2048;               // eight workgroups per CU; beyond that a wave re-uses its weight fragments for several tiles
    if (a.det_keys) {                           // SPARSE: gpi workgroups per image, each taking 128 entries of the image's list at a time
        long long gpi = (ntiles / a.B + 3) / 4; // (enough for every anchor of the level; a workgroup without entries returns at once)
        const long long cap = 2048 / a.B;
        if (gpi > cap) gpi = cap;
        if (gpi < 1) gpi = 1;
        hipLaunchKernelGGL((head_box_det_kernel<T, NCH, true>), dim3((unsigned)(gpi * a.B)), dim3(256), 0, st, a, cb_pack, (int)gpi);
    } else
    hipLaunchKernelGGL((head_box_det_kernel<T, NCH, false>), dim3((unsigned)grid), dim3(256), 0, st, a, cb_pack, 1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LP_ERR_HIP, std::string("head box launch: ") + hipGetErrorString(e));
    return LP_OK;
}

template <typename T>
static inline int head_box_det_launch_dtype(const ConvArgs& a, int cb_pack, hipStream_t st) {
    switch (a.chunk_begin[a.nsrc]) {
        case 1: return head_box_det_launch_one<T, 1>(a, cb_pack, st);
        case 2: return head_box_det_launch_one<T, 2>(a, cb_pack, st);
        case 3: return head_box_det_launch_one<T, 3>(a, cb_pack, st);
        case 4: return head_box_det_launch_one<T, 4>(a, cb_pack, st);
    }
    return fail(LP_ERR_UNSUPPORTED, "head box: more than four K-chunks");
}

}  // namespace lp
