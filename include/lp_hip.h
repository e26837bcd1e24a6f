/* lp_hip.h -- C ABI of libyololp_hip.so: the MI355X (gfx950) implementation of YOLO-LP's detection
 * forward + decode + NMS hot path, with the frame pre- and post-processing around it (letterbox, rescale, plate crops).
 *
 * The reference (KyleHuang9/YOLO-LP) is pure Python/PyTorch and has no FFI of its own; its boundary for this
 * path is the Python module API.  This header is the C-ABI a binding for that API
 * sits on: plain pointers and sizes, no torch types.  Each entry point names the reference interface it
 * replaces (file:line relative to the reference repository).
 *
 * Conventions
 *   - every function returns LP_OK (0) or a negative lp_status; lp_last_error() gives the message of the
 *     last failure on the calling thread.  Nothing here falls back to a CPU path.
 *   - all device pointers are caller-owned (the Python host allocates them as torch tensors); the library
 *     allocates no device memory.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - activations inside an engine are NHWC with the channel count padded to a multiple of 8; the element
 *     type is the engine's activation dtype (lp_dtype).  Accumulation is always fp32 (MFMA).
 *   - what an op writes (tests/test_containment_gpu.py): ALL stored channels of every pixel of its destination tensors, the
 *     padding channels (logical count up to the next multiple of 8; the space-to-depth input: 12 up to 16) as zero whatever
 *     the memory held before -- consumers multiply them by zero-packed weights, and a stale Inf there would become NaN --
 *     and no other byte: not of the arena (other tensors, the up to 255 bytes between a tensor's end and the next 256-byte
 *     boundary, the arena's last 256 bytes), not in front of or behind it, not in the caller's frame.  A tensor whose op a
 *     fused form carries (fused stem, fused 1x1 + 3x3 stride 2, fused BiFusion, the planar stem's space-to-depth input) is
 *     not written at all.  lp_engine_forward writes all B * num_anchors * LP_PRED_COLS floats of pred and nothing around
 *     them.  lp_engine_forward_det writes inside `workspace` (and, for levels whose class predictors do not fit the row
 *     kernel, the prediction scratch behind the arena's last tensor): of an anchor that does not pass the confidence mask,
 *     columns 12..27 of its candidate row are never written, and columns 0..11 only where the level's box predictors run
 *     in the dense form (LP_VARIANT_BOX_DENSE, or a level that does not fit the streaming box kernel, e.g. a DFL head),
 *     which computes the box columns of every anchor.  lp_nms / lp_nms_candidates write det, count, keep (every element:
 *     rows past count[b] zero, keep -1 there) and the workspace; lp_nms also the obj * cls products into pred.
 */
#ifndef LP_HIP_H
#define LP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { LP_OK = 0, LP_ERR_ARG = -1, LP_ERR_STATE = -2, LP_ERR_HIP = -3, LP_ERR_UNSUPPORTED = -4 } lp_status;
typedef enum { LP_F16 = 0, LP_BF16 = 1, LP_F32 = 2 } lp_dtype;
typedef enum { LP_ACT_NONE = 0, LP_ACT_RELU = 1, LP_ACT_SILU = 2 } lp_act;

#define LP_PRED_COLS 290   /* 4 xywh + 1 obj + 8 corners + 31 + 24 + 6*37 (effidehead.py:283-301) */
#define LP_DET_COLS 28     /* xyxy + 8 corners + 8 conf + 8 idx (nms.py:94-96) */
#define LP_MAX_SRC 4       /* inputs of one conv that are read as a channel concat without materialising it */

typedef struct lp_engine lp_engine;

const char* lp_version(void);
const char* lp_last_error(void);

/* ---------------------------------------------------------------------------------------------------
 * Engine: a static graph of fused conv kernels over NHWC tensors, built once per model by the host from the
 * model's folded weights, then run per batch.  Replaces Model.forward = backbone -> neck -> detect
 * (yolov6/models/yolo.py:32-40) and everything below it (layers/common.py, models/efficientrep.py,
 * models/reppan.py, models/effidehead.py:214-301, assigners/anchor_generator.py:11-31,
 * utils/general.py:29-66).
 * ------------------------------------------------------------------------------------------------- */
int lp_engine_create(lp_engine** out, int act_dtype /* lp_dtype */);
void lp_engine_destroy(lp_engine* e);

/* Declare an activation tensor with `channels` channels at 1/2^stride_log2 of the input resolution.
 * Returns its id (>= 0) or a negative lp_status. */
int lp_engine_tensor(lp_engine* e, int channels, int stride_log2);

/* Execution lane (0..4) of the ops added from now on.  Lane 0 is the caller's stream; lanes 1..4 are side
 * streams of the engine.  Ops on different lanes may overlap; the engine derives every cross-lane dependency from
 * the tensors the ops read and write and forks / joins the side streams inside lp_engine_forward, so callers still
 * see one in-order forward on `stream`.  Used for the independent branches of BiFusion (common.py:523-527) and the
 * per-level towers of the head (effidehead.py:228-245), which a builder may add right behind the neck layer that feeds them so
 * that they run under the rest of the neck. */
int lp_engine_set_lane(lp_engine* e, int lane);

/* The network input: caller's NCHW image batch [B,3,H,W] -> tensor `dst` (declared with 3 channels,
 * stride_log2 0).  Must be the first op. */
int lp_engine_add_input(lp_engine* e, int dst);

typedef struct lp_conv_desc {
    int n_src;              /* 1..LP_MAX_SRC; the sources are concatenated along channels in this order */
    int src[LP_MAX_SRC];
    int dst;
    int ksize;              /* 1 or 3 (padding ksize/2) */
    int stride;             /* 1 or 2 */
    int act;                /* lp_act, applied after bias */
    int res;                /* tensor id added after the activation (out = act(conv+b) + res_alpha*res), or -1 */
    float res_alpha;
    const float* weight;    /* host, fp32, [Cout][Cin_total][k][k]  (torch Conv2d.weight, BN already folded) */
    const float* bias;      /* host, fp32, [Cout] */
    int dst2;               /* <= 0 (tensor 0 is the network input, never a destination): none; else a second destination: TWO sibling layers of the reference that read the same input with the same
                             * kernel size, stride and activation (the class and box towers of a head level, effidehead.py:232-244; cv1 /
                             * cv2 of SimCSPSPPF and BepC3, common.py:139-141,497-500) run as ONE launch: weight / bias hold the rows of the
                             * first layer (dst's channels, a multiple of 8) followed by those of the second (dst2's).  No residual. */
} lp_conv_desc;

/* act(conv(cat(src...)) + bias) [+ alpha*res].  Replaces RepVGGBlock deploy forward (common.py:258-259),
 * Conv/SimConv/Conv_C3.forward_fuse (common.py:41-42,65-66,475-476), the torch.cat feeding them
 * (common.py:146-147,499,527; reppan.py:227-232) and BottleRep's residual (common.py:455). */
int lp_engine_add_conv(lp_engine* e, const lp_conv_desc* d);

/* 2x2 stride-2 transposed conv with bias: Transpose.forward (common.py:186-187).
 * weight: host fp32 [Cin][Cout][2][2] (torch ConvTranspose2d.weight), bias [Cout]. */
int lp_engine_add_deconv2x2(lp_engine* e, int src, int dst, const float* weight, const float* bias);

/* Three chained 5x5 stride-1 pad-2 max pools (windows 5/9/13): the `self.m` calls of
 * SimCSPSPPF/SimSPPF.forward (common.py:101-103,144-146).  dst1 = m(src), dst2 = m(dst1), dst3 = m(dst2). */
int lp_engine_add_pool5_chain(lp_engine* e, int src, int dst1, int dst2, int dst3);

/* Classification predictors of one pyramid level: the eight 1x1 convs + sigmoid of Detect.forward
 * (effidehead.py:235-242,251-258) as ONE contraction; writes columns [13,13+n_cls) of the level's rows of
 * pred.  weight: host fp32 [n_cls][C] (the eight predictor weights stacked in head order), bias [n_cls]. */
int lp_engine_add_head_cls(lp_engine* e, int src, int level, int n_cls, const float* weight, const float* bias);

/* Box + corner predictors of one level and the anchor-free decode: reg_preds / cor_preds 1x1 convs
 * (effidehead.py:244-245), optional DFL softmax-projection (:247-249, reg_bins = reg_max+1 = 17, proj =
 * proj_conv.weight[17]), generate_anchors (anchor_generator.py:11-31), dist2bbox 'xywh' and dist2cor
 * (general.py:29-40,51-66), * stride (effidehead.py:285-286) and the objectness column of ones (:290).
 * Writes columns [0,13) of the level's rows.  weight: host fp32 [4*reg_bins + 8][C], bias likewise.
 * reg_bins = 1 means plain ltrb distances (use_dfl False). */
int lp_engine_add_head_box(lp_engine* e, int src, int level, int reg_bins, const float* weight, const float* bias,
                           const float* proj);

/* Freeze the graph and pack the weights for the MFMA kernels (host side). */
int lp_engine_finalize(lp_engine* e, int n_levels);
size_t lp_engine_weight_bytes(const lp_engine* e);
/* Copy the packed weights into caller-owned device memory (>= lp_engine_weight_bytes, 256-B aligned).  The buffer must
 * stay alive and writable while the engine is used: its first 256 bytes are the kernels' zero page and a 16-byte scratch
 * granule (target of stores that must not land anywhere else). */
int lp_engine_upload(lp_engine* e, void* dev_weights, void* stream);

/* Activation arena for a given input shape (H, W multiples of 32). */
size_t lp_engine_arena_bytes(const lp_engine* e, int B, int H, int W);
int lp_engine_bind(lp_engine* e, void* dev_arena, size_t bytes, int B, int H, int W);
/* Placement of tensor `id` inside the bound arena: byte offset, logical channels, stored channels (padded
 * to 8), height, width.  Layout is [B][h][w][c_stored] of the activation dtype. */
int lp_engine_tensor_info(const lp_engine* e, int id, size_t* offset, int* c, int* c_stored, int* h, int* w);
/* Rows of pred per image (sum over levels of h*w) for the bound shape. */
int lp_engine_num_anchors(const lp_engine* e);

/* Run the graph on the bound shape.  x: device [B,3,H,W] of x_dtype (lp_dtype); pred: device fp32
 * [B, num_anchors, LP_PRED_COLS].  Model.forward's first return value (yolo.py:40); the second one (the
 * three neck maps) stays in the arena (lp_engine_tensor_info). */
int lp_engine_forward(lp_engine* e, const void* x, int x_dtype, float* pred, void* stream);

/* Detections-only forward for callers that go straight on to NMS (Inferer, Evaler.predict, the benchmark): the head does not
 * write the [B,N,290] prediction tensor -- its class-predictor kernels apply non_max_suppression's candidate selection
 * (nms.py:76-96: obj * cls, eight (max, first arg-max), the confidence mask, the score) to the sigmoids while they are still
 * on chip and append the passing anchors to the candidate lists in `workspace` (lp_nms_workspace_bytes(B, N) bytes, 256-byte
 * aligned).  lp_nms_candidates(workspace, ...) on the same stream finishes the job; det / count / keep are bit-identical to
 * lp_nms on the prediction tensor lp_engine_forward would have written.  Replaces Model.forward + the first half of
 * non_max_suppression (yolo.py:32-40, effidehead.py:283-301, nms.py:68-96). */
int lp_engine_forward_det(lp_engine* e, const void* x, int x_dtype, double conf_thres, void* workspace, size_t workspace_bytes,
                          void* stream);

/* enable != 0: lp_engine_forward / lp_engine_forward_det capture their launches into a hipGraph on first use with a given
 * (x, pred or workspace + threshold, dtype, launch geometry) and replay it afterwards; any other pointers re-capture.  For
 * launch-bound shapes (batch 1). */
int lp_engine_set_graph(lp_engine* e, int enable);

/* enable != 0 (default): the forwards issue every kernel on the caller's stream in op order; 0: independent branches of the
 * graph (lp_engine_set_lane) run on side streams forked from / joined into the caller's stream.  With several forwards in flight
 * on several streams the fork / join events cost more than the lanes hide (six batches in flight: 16.2 k images/s on one lane
 * each against 14.9 k; profiles/r03_inflight_lanes.txt); with ONE forward in flight the lanes were worth +2.6 % until the head
 * kernels got shorter -- final state of round 3: one lane +1.2 % at batch 32, +4.5 % at batch 1, lanes +1.8 % on yolov6m 1280x1280
 * (profiles/r03_round_ab.txt).  Results do not depend on it. */
int lp_engine_set_single_lane(lp_engine* e, int enable);

/* MFMA family of the 3x3 layers (call before lp_engine_finalize; default: enabled, LP_NO_MFMA16=1 in the environment
 * disables; stride-2 layers: LP_VARIANT_PIPE16_S2* below).  enable != 0: every 16-bit 3x3 stride-1 MODE_ACT layer whose 16-channel K-chunks are a multiple of four (input channels
 * a multiple of 64) and whose weights are packed in 128-row cout tiles (more than 64 stored output channels) runs on v_mfma_f32_16x16x32 (LP_VARIANT_PIPE16_*:
 * tiles of any number of 16-pixel blocks fill the 256 CUs evenly where 256-pixel tiles leave 22 % of the MFMA slots empty).  That
 * family adds the products in another fp32 order than all other variants: results agree to rounding, not bit for bit.  The choice is
 * a function of the layer alone -- never of the batch size, the input size or a timing -- so image k of a batch equals image k
 * alone, and inside the family the autotuner's variants are bit-identical.  enable == 0: every layer on the 32x32x16 family. */
int lp_engine_set_mfma16(lp_engine* e, int enable);

/* Introspection for benchmarks: ops of the frozen graph and per-op device time (hipEvent pairs on
 * `stream`, one untimed warm run first).  op_ms has lp_engine_num_ops() entries (milliseconds). */
int lp_engine_num_ops(const lp_engine* e);
/* kind: 0 input, 1 conv, 2 deconv, 3 pool, 4 head_cls, 5 head_box.  flops = 2*MAC of the op on the bound
 * shape; bytes = algorithmic activation bytes read + written (each tensor once) + weight bytes. */
int lp_engine_op_info(const lp_engine* e, int op, int* kind, int* ksize, int* cin, int* cout, double* flops,
                      double* bytes);
int lp_engine_profile(lp_engine* e, const void* x, int x_dtype, float* pred, void* stream, float* op_ms, int reps);
/* Same, with `inner` back-to-back launches of every op between its two events (op_ms = event time / inner): the cost of
 * the event pair itself is amortised, so op_ms approaches the kernel duration a rocprofv3 kernel trace reports. */
int lp_engine_profile_ops(lp_engine* e, const void* x, int x_dtype, float* pred, void* stream, float* op_ms, int reps, int inner);

/* Pick, per conv op and for the bound shape, the fastest of the kernel variants (workgroup tile / LDS ring depth)
 * that share the op's weight packing, by timing each in place (hipEvent pairs on `stream`).  The choice is
 * remembered per (B,H,W) and re-applied by lp_engine_bind.  Variants differ only in tiling: every output element
 * is the same fp32 sum in the same K order, so results do not depend on the choice.  lp_engine_op_variant reports
 * the current choice of an op: cfg = a workgroup tile of the implicit-GEMM kernel (0..5 = A..F) with
 * nbuf = LDS ring depth 1 or 2, or LP_VARIANT_STREAM64 / LP_VARIANT_STREAM128 (streaming 1x1 kernel with 64 / 128 output
 * channels per wave, nbuf 2), or LP_VARIANT_ROWS (row-writer form of a head_cls op, nbuf 1), or LP_VARIANT_PIPE_* (pipelined
 * 3x3 stride-1 kernel, nbuf 3).  LP_VARIANT_PIPE_P belongs to the stem only (op 1, over the space-to-depth image the input op
 * writes): with it the stem gathers its pixels from the caller's NCHW frame itself and the input op is skipped, whenever the
 * frame passed to lp_engine_forward has the engine's 16-bit dtype (other dtypes: input op + the stem's other variant).
 * lp_engine_set_op_variant forces one (tests, experiments): LP_ERR_UNSUPPORTED if it does not fit the op, and then nothing changes:
 * the variants and fused forms that were on, the remembered tuning and the prepared launches stay as they were. */
enum { LP_VARIANT_STREAM64 = 16, LP_VARIANT_STREAM128 = 17, LP_VARIANT_ROWS = 18,
       /* pipelined 3x3 stride-1 kernel (persistent, 3-slot LDS ring, nbuf 3): 128 couts x 256 px, 64 x 512, 128 x 128, 32 x 512 */
       LP_VARIANT_PIPE_D = 32, LP_VARIANT_PIPE_B = 33, LP_VARIANT_PIPE_F = 34, LP_VARIANT_PIPE_C = 35,
       LP_VARIANT_PIPE_P = 36 /* 32 x 512, the stem reading the NCHW frame (see above) */,
       LP_VARIANT_PIPE16_D = 39, LP_VARIANT_PIPE16_F = 41 /* PIPE_D / PIPE_F on v_mfma_f32_16x16x32 (128-row packing, layers with a multiple of four
                                       * number of 16-channel K-chunks; nbuf 3).  ANOTHER fp32 summation order: equal to the other variants to
                                       * rounding, not bit for bit -- see lp_engine_set_mfma16 */,
       LP_VARIANT_PIPE16_V0 = 42, LP_VARIANT_PIPE16_V1 = 43 /* the same sums as PIPE16_* with tiles of any number of 16-pixel blocks (128 couts x
                                       * <= 448 px as 2 x 4 waves, 128 x <= 224 as 4 x 2): tiles that fill the persistent grid evenly */,
       LP_VARIANT_FUSED_STEM2 = 37 /* op 2 only (3x3 stride 2 behind the stem, <= 64 channels): input op + stem + this layer as ONE kernel
                                      whenever the frame has the engine's 16-bit dtype; the stem's output never reaches memory */,
       LP_VARIANT_FUSED_PW_S2 = 38 /* a 3x3 stride-2 layer (<= 64 channels) whose input comes from a 1x1 layer (64 -> <= 64 channels) that nobody
                                      else reads (BiFusion's downsample(cv2(x)), common.py:504-527): the two as ONE kernel; the 1x1 op is skipped */ };
/* LP_VARIANT_FUSED_BIFUSION (45): the cv3 of a 64-channel BiFusion level (common.py:504-527: 1x1 ReLU over [upsample(x0), cv1(x1), d]) together with
 * the transposed convolution and cv1 as ONE kernel (lp_bifusion_fused.inc): their outputs never reach memory; the two carried ops are skipped.
 * Bit-identical to the three launches.  lp_engine_op_carrier: index of the op whose kernel currently carries `op` (fused stem, fused 1x1 + 3x3
 * stride 2, fused BiFusion; frame_direct != 0: the caller's frame has the engine's dtype), or -1: the op launches its own kernel. */
enum { LP_VARIANT_FUSED_BIFUSION = 45 };
/* LP_VARIANT_BOX_SPARSE (46, the default) / LP_VARIANT_BOX_DENSE (47): a head_box op in the detections-only forward (lp_engine_forward_det) computes
 * reg_preds / cor_preds + dist2bbox / dist2cor (effidehead.py:262-301, general.py:29-66) for the anchors the level's class predictors let pass only,
 * or for every anchor.  The candidate rows lp_nms_candidates reads are the same bits either way; the sparse form needs one execution lane and the
 * op order cls(level), box(level) per level (else the dense form runs whatever is set).  nbuf is ignored. */
enum { LP_VARIANT_BOX_SPARSE = 46, LP_VARIANT_BOX_DENSE = 47 };
/* LP_VARIANT_PIPE16_S2A (48) / _S2B (49): a 3x3 STRIDE-2 layer with 128-row weight packing (more than 64 stored output channels, one
 * destination, 16-bit) on v_mfma_f32_16x16x32: persistent workgroups, three halo + two weight LDS slots (the halo requested two chunks ahead, counted vmcnt), tiles of any number of 16-pixel blocks (128 couts x
 * <= 256 px as 2 x 4 waves, 128 x <= 224 as 4 x 2), nbuf 3 (lp_conv3x3_s2p16.inc; reference: efficientrep.py:57-117, common.py:258-259).
 * Another fp32 summation order than conv_mfma_kernel<KS=3,S=2>'s (equal to rounding, not bit for bit).  Measured 0-9 % faster than that
 * kernel per layer and equal over the whole step (profiles/r04_s2p16_convbench.txt, r04_experiments.txt 15): NOT a default and never picked by the autotuner -- lp_engine_set_op_variant selects it for
 * one op; an engine created under LP_S2P16=1 runs every eligible layer on it (by rule, never by timing). */
enum { LP_VARIANT_PIPE16_S2A = 48, LP_VARIANT_PIPE16_S2B = 49 };
int lp_engine_op_carrier(const lp_engine* e, int op, int frame_direct);
/* The library's own view of the frozen graph (tests): the tensor ids op `op` reads -- src[0..n_src), -1 behind them; res, or -1 --
 * and writes -- dst[0..2], -1 for none (the second destination of a two-destination conv, the three of a pool chain; head ops
 * write pred, not a tensor) -- as they stand after lp_engine_finalize, i.e. after the space-to-depth rewrite of the stem: the input
 * op then writes a tensor of 12 channels at half resolution that the host never declared, the stem reads it, and the declared
 * input tensor is unused.  Any pointer may be NULL.  No other effect. */
int lp_engine_op_io(const lp_engine* e, int op, int* src /*[LP_MAX_SRC]*/, int* n_src, int* res, int* dst /*[3]*/);
int lp_engine_autotune(lp_engine* e, const void* x, int x_dtype, float* pred, void* stream, int reps);
int lp_engine_op_variant(const lp_engine* e, int op, int* cfg, int* nbuf);
int lp_engine_set_op_variant(lp_engine* e, int op, int cfg, int nbuf);
/* Test hook: the output-tile choice (0 = the planner's best, 1, 2, ... = the next candidates; the autotuner times 0..2) of whatever
 * variant the op currently has -- the implicit-GEMM, pipelined and block-tiled kernels, and the planar stem, the fused stem and the
 * fused 1x1 + 3x3 stride-2 form while one of those is switched on.  Invalidates what lp_engine_set_op_variant invalidates.  A choice
 * past the last candidate repeats the last one (conv kernels) or is LP_ERR_UNSUPPORTED and changes nothing (stem / fused forms).
 * lp_engine_op_tile reports the choice and the TH x TW output tile prepared for the bound shape.  LP_ERR_UNSUPPORTED: the op's
 * kernel has no output tiles (input, pooling, head ops, the streaming 1x1 kernel, the fused BiFusion kernel). */
int lp_engine_set_op_tile(lp_engine* e, int op, int choice);
int lp_engine_op_tile(const lp_engine* e, int op, int* choice, int* TH, int* TW);
/* Copy the tuned choices (all shapes) of an engine built from the same graph and dtype, e.g. to the other engines of a
 * several-batches-in-flight pipeline, instead of tuning each. */
int lp_engine_copy_tuning(lp_engine* dst, const lp_engine* src);

/* ---------------------------------------------------------------------------------------------------
 * Post-processing.  Replaces non_max_suppression (yolov6/utils/nms.py:31-130) including its call of
 * torchvision.ops.nms (:121).  All images of the batch are processed by one set of launches.
 *   pred      device fp32 [B,N,290]; columns 13.. are multiplied by column 4 IN PLACE (nms.py:76)
 *   conf/iou  thresholds as the python floats the reference receives (conf is compared in fp32, iou in
 *             double, as torch / torchvision do)
 *   det       device fp32 [B,max_det,28] (16-byte aligned), rows in descending-score order; rows >= count[b] are zero
 *   count     device int32 [B]
 *   keep      device int32 [B,max_det] anchor index of every kept row, or NULL
 *   workspace device scratch of at least lp_nms_workspace_bytes(B,N) bytes
 * Ties and NaN (lp_nms and lp_engine_forward_det + lp_nms_candidates alike; torch.max's and torch's descending sort's rules):
 *   - the arg-max of a head (det columns 20..27) is the FIRST column whose probability equals the head's largest one.  Two logits
 *     whose fp32 sigmoids are the same number tie: from about 17 up every sigmoid is 1.0f and the first such column wins, not
 *     the one with the largest logit;
 *   - a NaN probability wins its head: the maximum (det columns 12..19) is NaN and the index that of the head's first NaN;
 *   - a NaN in one of the first seven heads makes the masked mean NaN, the comparison with conf false: no candidate;
 *   - a NaN only in the last head (the mask does not read it) leaves the anchor a candidate with a NaN score.  NaN scores, of
 *     either sign, sort before every number, among themselves by ascending anchor; equal scores by ascending anchor.
 * ------------------------------------------------------------------------------------------------- */
size_t lp_nms_workspace_bytes(int B, int N);
int lp_nms(float* pred, int B, int N, double conf_thres, double iou_thres, int max_det, float* det, int32_t* count,
           int32_t* keep, void* workspace, size_t workspace_bytes, void* stream);

/* Second half of lp_nms for candidate lists already in `workspace` (written by lp_engine_forward_det): stable descending sort,
 * the > 30000 cut (nms.py:115-116), greedy IoU suppression (torchvision.ops.nms), max_det (nms.py:121-125). */
int lp_nms_candidates(int B, int N, double iou_thres, int max_det, float* det, int32_t* count, int32_t* keep, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Device int32 [B] inside `workspace`: how many anchors of each image passed the confidence mask (nms.py:90-96) in the last
 * lp_nms / lp_engine_forward_det that used it (valid once that call's stream work is done).  Callers use it as a cheap
 * estimate of the candidate density when choosing between the two forms of the path; nothing in the results depends on it. */
const int32_t* lp_nms_candidate_counts(const void* workspace, int B, int N);

/* ---------------------------------------------------------------------------------------------------
 * Callers either side of the path.
 *
 * lp_preprocess_letterbox: Inferer.precess_image (yolov6/core/inferer.py:191-201) with letterbox
 * (yolov6/data/data_augment.py:30-61) for one frame.  img: device uint8 [h0,w0,3] BGR (cv2.imread layout);
 * out: device [3,H,W] of out_dtype, RGB, /255.  The frame is resized (bilinear, OpenCV INTER_LINEAR fixed-point
 * scheme) to rh x rw, placed at (top,left) and surrounded by 114.  rh == h0 && rw == w0 means no resize.
 *
 * lp_rescale_round: Inferer.rescale (inferer.py:203-228) + .round() (:100) on columns 0..11 of n detection rows
 * (row stride 28 floats), in place: v = round_half_even(clamp((v - pad) / ratio, 0, img_w | img_h)).
 * ------------------------------------------------------------------------------------------------- */
int lp_preprocess_letterbox(const unsigned char* img, int h0, int w0, void* out, int out_dtype, int H, int W, int rh, int rw,
                            int top, int left, void* stream);
int lp_rescale_round(float* det, int n, double ratio, double padx, double pady, int img_w, int img_h, void* stream);

/* Batched forms of the two entry points above for B frames of any source sizes (the same restatement of inferer.py:191-228
 * and data_augment.py:30-61, one launch per LP_FRAMES_PER_LAUNCH frames; descriptors travel as kernel arguments, so neither
 * call uploads anything and both may be captured in a graph).
 *
 * lp_preprocess_letterbox_batch: out [B,3,H,W] of out_dtype.  Slot b < n_frames is bit-identical to lp_preprocess_letterbox
 * with desc[b] into [3,H,W]; slots n_frames <= b < B are padding (114/255 everywhere).  desc is a HOST array of n_frames
 * entries; every entry is checked with the single-frame rules before anything is launched (LP_ERR_ARG names the frame).
 *
 * lp_rescale_round_batch: det [B,max_det,28] in place; for image b, rows r < min(count[b], max_det) (count: DEVICE int32 [B],
 * read by the kernel: no host sync) are rescaled exactly as lp_rescale_round(det[b], n, desc[b]...) would.  Rows at or beyond
 * the count and columns 12..27 are left untouched.  desc is a HOST array of B entries. */
#define LP_FRAMES_PER_LAUNCH 64
typedef struct lp_frame_desc {
    const unsigned char* img;   /* device uint8 [h0,w0,3] BGR, any alignment */
    int h0, w0, rh, rw, top, left;
} lp_frame_desc;
typedef struct lp_rescale_desc { double ratio, padx, pady; int img_w, img_h; } lp_rescale_desc;
int lp_preprocess_letterbox_batch(const lp_frame_desc* desc, int n_frames, int B, void* out, int out_dtype, int H, int W,
                                  void* stream);
int lp_rescale_round_batch(float* det, const int32_t* count, int B, int max_det, const lp_rescale_desc* desc, void* stream);

/* Tiled detection of large frames: a 3840x2160 frame letterboxed to one 640x640 input is shrunk 6x and its plates with it.  The
 * reference has nothing here (Inferer shrinks every frame, inferer.py:191-201); these two entry points put the work around
 * the forward on the device: cutting letterboxed tiles out of device frames, and merging the per-tile detections per frame.
 *
 * lp_preprocess_tiles_batch extends lp_preprocess_letterbox_batch (same kernel, same conventions: descriptors by value in the
 * kernel arguments, one launch per LP_FRAMES_PER_LAUNCH tiles, nothing uploaded, no host sync): slot b < n_tiles of out
 * [B,3,H,W] is bit-identical to what lp_preprocess_letterbox_batch writes for a CONTIGUOUS COPY of the region
 * frame[y0:y0+th, x0:x0+tw] with the same (rh, rw, top, left) -- the bilinear taps clamp at the region's edges, not the
 * frame's; slots n_tiles <= b < B are padding (114/255).  The region is read in place: its first pixel and the frame's row
 * pitch of w0*3 bytes.  desc is a HOST array of n_tiles entries, all checked before the first launch (LP_ERR_ARG names the
 * tile): img, h0, w0 >= 1, region inside the frame with th, tw >= 1, geometry inside H x W. */
typedef struct lp_tile_desc {
    const unsigned char* img;   /* the device frame, uint8 [h0,w0,3] BGR, any alignment */
    int h0, w0;
    int y0, x0, th, tw;         /* the region of it */
    int rh, rw, top, left;      /* letterbox geometry of a (th, tw) image */
} lp_tile_desc;
int lp_preprocess_tiles_batch(const lp_tile_desc* desc, int n_tiles, int B, void* out, int out_dtype, int H, int W, void* stream);

/* NV12 video frames.  Decoders deliver NV12, not BGR: an h0 x w0 frame (both even) is a luma plane y, uint8 [h0][w0] with rows
 * pitch_y >= w0 bytes apart, and a half-resolution chroma plane uv, uint8 [h0/2][w0/2][2] (U first) with rows pitch_uv >= w0 bytes
 * apart, pitch_uv even, base 2-byte aligned.  The reference has nothing here; yolov6/utils/nv12.py states the rule and restates
 * both entry points in numpy, bit for bit.  For pixel (i, j): Y = y[i][j], U = uv[i>>1][j>>1][0], V = uv[i>>1][j>>1][1] (chroma
 * is replicated, not interpolated), and in int32 with arithmetic right shifts
 *     c = max(Y - yoff, 0) * CY;  d = U - 128;  e = V - 128;  half = 1 << 19
 *     R = clamp255((c + half + CVR*e) >> 20);  G = clamp255((c + half + CVG*e + CUG*d) >> 20);  B = clamp255((c + half + CUB*d) >> 20)
 * with (yoff, CY, CUB, CUG, CVG, CVR) of `matrix`:
 *     0 bt601  (limited range; the table of OpenCV's COLOR_YUV2BGR_NV12)  16, 1220542, 2116026, -409993, -852492, 1673527
 *     1 bt709  (limited range)                                            16, 1220945, 2215014, -223607, -558796, 1879825
 *     2 bt601f (full range)                                                0, 1048576, 1858077, -360853, -748826, 1470104
 *     3 bt709f (full range)                                                0, 1048576, 1945738, -196424, -490864, 1651297
 *
 * lp_preprocess_nv12_batch: the letterbox of lp_preprocess_tiles_batch (same kernel, reading NV12 planes through another pixel
 * source) with the conversion fused in; no BGR frame exists on the device.  Slot b < n of out [B,3,H,W] is bit-identical to what lp_preprocess_tiles_batch writes for the region (y0, x0, th, tw)
 * and the geometry (rh, rw, top, left) of the BGR frame the rule gives for the WHOLE frame: the bilinear taps clamp at the region's
 * edges, chroma is indexed by the absolute frame coordinate (odd y0, x0 are legal), rh == th && rw == tw means no resize; a whole
 * frame is the region (0, 0, h0, w0).  Slots n <= b < B are padding (114/255).  Descriptors travel by value in the kernel
 * arguments, one launch per LP_NV12_PER_LAUNCH slots: nothing is uploaded, no host sync, capturable in a graph.  desc is a HOST
 * array of n entries, all checked before the first launch; LP_ERR_ARG names the entry for: a null plane, odd (or < 2) h0 or w0,
 * pitch_y < w0, pitch_uv < w0 or odd, uv not 2-byte aligned, an unknown matrix, a region outside the frame, geometry outside H x W.
 *
 * lp_nv12_to_bgr_batch: the frame itself for the callers that need it (plate crops, the best-shot gallery, saving images):
 * out = uint8 [h0,w0,3] BGR, contiguous, any alignment, by the rule above; one launch per LP_FRAMES_PER_LAUNCH frames, the
 * table in the kernel arguments.  The same plane checks, and a null out, are LP_ERR_ARG naming the entry before any launch. */
#define LP_NV12_PER_LAUNCH 32
typedef struct lp_nv12_desc {
    const unsigned char* y;     /* device luma plane */
    const unsigned char* uv;    /* device chroma plane */
    int pitch_y, pitch_uv;
    int h0, w0;
    int y0, x0, th, tw;         /* the region of the frame */
    int rh, rw, top, left;      /* letterbox geometry of a (th, tw) image */
    int matrix;
} lp_nv12_desc;
typedef struct lp_nv12_bgr_desc {
    const unsigned char* y;
    const unsigned char* uv;
    int pitch_y, pitch_uv;
    int h0, w0;
    int matrix;
    unsigned char* out;         /* device uint8 [h0,w0,3] */
} lp_nv12_bgr_desc;
int lp_preprocess_nv12_batch(const lp_nv12_desc* desc, int n, int B, void* out, int out_dtype, int H, int W, void* stream);
int lp_nv12_to_bgr_batch(const lp_nv12_bgr_desc* desc, int n, void* stream);

/* lp_merge_tiles: per-frame merge of per-tile detections; one workgroup per frame, at most 64 tiles (whole frames) per launch,
 * the tile table travels as kernel arguments: nothing is uploaded, no host sync.
 *   det_t [n_tiles,max_det_t,28] fp32 + count_t [n_tiles] int32 (DEVICE): the tiles' detections as lp_nms leaves them, in
 *   tile-local source pixels, rounded, i.e. after lp_rescale_round_batch with each tile's (th, tw) as its source image.
 *   tiles: HOST array, tile t belongs to frame tiles[t].frame and covers (y0, x0, th, tw) of it; the tiles of a frame are
 *   contiguous, frames ascending.  frame_hw: HOST int [n_frames][2] = (h, w).
 *   det [n_frames,max_det,28], count [n_frames], src [n_frames,max_det] int32 (tile index x max_det_t + row of every kept row,
 *   tiles counted from 0 over the whole call; -1 past the count).  Rows at or past count[f] are zero, as lp_nms leaves them.
 * Per frame, in this order (yolov6/utils/tiles.py::merge_tiles_np restates it bit for bit):
 *   1. candidates: rows r < min(max(count_t[t], 0), max_det_t) of the frame's tiles, in (tile, row) order;
 *   2. cut-plate filter (border >= 0; negative: off): with the tile-local box (x1,y1,x2,y2) = columns 0..3 a row is dropped if
 *      x0 > 0 && x1 <= border, or y0 > 0 && y1 <= border, or x0 + tw < w && x2 >= tw - border, or y0 + th < h && y2 >= th - border
 *      (a box touching a tile side that is not a frame side is a plate cut by the slicing; the neighbouring tile sees it whole);
 *   3. shift: columns 0,2,..,10 += (float)x0, columns 1,3,..,11 += (float)y0; columns 12..27 are copied;
 *   4. score = (c12 + c13 + ... + c19) / 8.0f, summed left to right in fp32 (nms.py:120); order: descending score (-0 = +0; NaNs
 *      by their bit pattern, as the keys of lp_nms order them), ties in candidate order;
 *   5. greedy suppression ACROSS tiles only: in that order a candidate is kept unless an already kept candidate of ANOTHER tile
 *      overlaps it by more than thres.  metric 0 (IoU): torchvision's predicate as lp_nms evaluates it (fp32 op by op, the
 *      quotient compared against the double threshold); metric 1 (IoS): inter / min(area_i, area_j) > thres, the same fp32 ops
 *      with that denominator (IEEE division: a zero area gives NaN = not suppressed, or +inf = suppressed);
 *   6. the first max_det kept rows, in order.
 * A frame covered by one tile therefore comes out as that tile's rows, unchanged and in order.
 * Limits (LP_ERR_ARG, with the numbers in the message): at most 64 tiles per frame, and tiles_of_frame * max_det_t <= 16384
 * candidate slots per frame (they are sorted in LDS).  workspace: DEVICE, 16-byte aligned, lp_merge_tiles_workspace_bytes
 * bytes (kept lists that outgrow LDS).  Every argument is checked before the first launch. */
typedef struct lp_tile_ref { int frame, y0, x0, th, tw; } lp_tile_ref;
size_t lp_merge_tiles_workspace_bytes(int n_frames, int max_det);
int lp_merge_tiles(const float* det_t, const int32_t* count_t, const lp_tile_ref* tiles, int n_tiles, int max_det_t,
                   const int* frame_hw, int n_frames, double thres, int metric /* 0 IoU, 1 IoS */, int border, int max_det,
                   float* det, int32_t* count, int32_t* src, void* workspace, size_t workspace_bytes, void* stream);

/* lp_track_update: plate tracking across video frames with a per-track vote over the eight character heads; a small
 * device-resident tracker per stream, one workgroup per stream, at most LP_FRAMES_PER_LAUNCH frames per launch (a longer call is
 * several launches on `stream`, a stream's frames may span them); the frame table travels as kernel arguments: nothing is
 * uploaded, no host sync, so the call can be enqueued behind lp_rescale_round_batch.  The reference has nothing here (Inferer
 * treats video frames independently, inferer.py); yolov6/utils/track.py::PlateTrackerNp restates the rules below bit for bit.
 *   state: DEVICE, 16-byte aligned, lp_track_state_bytes(n_streams, max_tracks) bytes, all zero = no tracks (the caller zeroes
 *   it once; zeroing a stream's lp_track_state_bytes(1, max_tracks) bytes resets that stream).  max_tracks: 1..LP_TRACK_MAX_TRACKS.
 *   det [B,max_det,28] fp32 + count [B] int32 (DEVICE): the frames' detections as lp_nms / lp_rescale_round_batch leave them;
 *   only the first n = min(max(count, 0), max_det, LP_TRACK_MAX_DETS) rows of a frame take part.
 *   stream_of: HOST int [B], the stream of frame b, or -1: the frame is not tracked (padding slots of a batch).  The frames of a
 *   stream are taken in ascending b; streams need not be contiguous.  flush: HOST [n_streams] or NULL; after its frames (there
 *   may be none) a stream with flush[s] != 0 ends all its live tracks in slot order.
 *   det_out [B,max_det,28] (may not alias det), tid [B,max_det] int32; ended_i / ended_f [n_streams,max_ended,12], ended_count
 *   [n_streams] int32: per stream the first max_ended records of the tracks that ended in this call, in the order they ended
 *   (records past them are zero), and the number that ended (it may exceed max_ended).  ended_i = id, first, last, hits,
 *   best_0..7; ended_f = share_0..7, x1, y1, x2, y2 (the last matched box).
 * Per frame of a stream, fp32 op by op (no fused multiply-add), every live slot holding id, first, last (frame index of the last
 * match), hits, misses, the box and corners of the last matched row, a velocity (vx, vy), votes[8][LP_TRACK_MAX_CLS] and total[8]:
 *   1. predict: the box shifted by (vx * k, vy * k), k = (float)(misses + 1); the product is rounded, then the add;
 *   2. expand, for the predicted box and every row's box: e = (float)expand * (x2 - x1), x1 -= e, x2 += e; the same in y;
 *   3. pairs: the IoU of every (slot, row) on the expanded boxes, inter / (area_i + area_j - inter) with the fp32 ops of lp_nms's
 *      IoU predicate (torchvision's, the quotient computed: it is the sort key); the pair exists iff (double)iou > match_thres
 *      (not for NaN).  Order: descending IoU, ties by slot, then row; in that order a pair is taken iff its slot and its row are
 *      both still free (global greedy matching);
 *   4. a matched slot: vx = (cx_new - cx_old) / k with cx = (x1 + x2) * 0.5f on the stored, unexpanded box, vy likewise; box and
 *      corners = the row's columns 0..11; hits += 1, misses = 0, last = frame; it votes (7);
 *   5. an unmatched live slot: misses += 1; misses > max_age ends the track (record appended, slot zeroed), in slot order;
 *   6. unmatched rows in row order: score = (c12 + ... + c19) / 8.0f summed left to right (nms.py:120); iff (double)score >=
 *      new_thres (not for NaN) the lowest free slot -- those freed in 5 included -- becomes a new track: id = next_id++, first =
 *      last = frame, hits = 1, misses = 0, zero velocity, zero votes, then it votes.  With no free slot the row stays untracked
 *      and the stream's `dropped` counter goes up;
 *   7. vote, per head p: v = c[20+p], conf = c[12+p]; iff conf > 0 && 0 <= v < ncls[p] (float compares, false for NaN):
 *      votes[p][(int)v] += conf, total[p] += conf;
 *   8. read of a track: best_p = the first index of the largest votes[p][0..ncls[p]) (strict >: 0 for an all-zero head),
 *      share_p = total[p] > 0 ? votes[p][best_p] / total[p] : 0.0f;
 *   9. tid[r] = the id of a matched or new row's track, -1 for every other r < max_det; det_out[r] = the row with columns
 *      12..19 replaced by the track's shares and 20..27 by (float)best_p, read after this frame's vote: the layout everything
 *      downstream takes (lp_plate_crops_batch).  Other rows r < min(max(count, 0), max_det) are copied unchanged (so are all
 *      such rows of a frame with stream_of -1, whose tid is -1), rows at or past it are zero;
 *  10. the stream's frame counter goes up.  Frame counter and next_id start at 0.
 * `dropped` (int32, rows that found no free slot since the state was zeroed) is read from the state itself: it lives
 * lp_track_dropped_offset(max_tracks, s) bytes into it.
 * Every argument is checked before the first launch (LP_ERR_ARG names the offending frame or head; nothing is launched):
 * match_thres in [0, 1], |new_thres| <= 3e38, expand in [0, 1e6], max_age >= 0, ncls[p] in 1..LP_TRACK_MAX_CLS (the model's
 * npro, nalp, nads x 6), B >= 0, max_det >= 1, max_ended >= 0, stream_of[b] in -1..n_streams-1. */
#define LP_TRACK_MAX_TRACKS 128
#define LP_TRACK_MAX_DETS 128   /* 128 x 128 pair keys are sorted in LDS: the budget of lp_merge_tiles */
#define LP_TRACK_MAX_CLS 64
typedef struct lp_track_params { double match_thres, new_thres, expand; int max_age; int ncls[8]; } lp_track_params;
size_t lp_track_state_bytes(int n_streams, int max_tracks);   /* 0: bad arguments */
size_t lp_track_dropped_offset(int max_tracks, int stream_index);
int lp_track_update(void* state, int n_streams, int max_tracks, const lp_track_params* p,
                    const float* det, const int32_t* count, int B, int max_det,
                    const int* stream_of /* HOST [B] */, const unsigned char* flush /* HOST [n_streams] or NULL */,
                    float* det_out, int32_t* tid, int32_t* ended_i, float* ended_f, int32_t* ended_count,
                    int max_ended, void* stream);
/* lp_track_update_slots: lp_track_update (which is this call with slot = NULL) that also reports where each row's track lives:
 * slot [B,max_det] int32 (DEVICE, may be NULL), slot[r] = the tracker slot (0..max_tracks-1) of a matched or new row's track, -1
 * wherever tid[r] is -1.  A slot holds one track at a time, so it indexes per-track side tables (lp_best_shot_update). */
int lp_track_update_slots(void* state, int n_streams, int max_tracks, const lp_track_params* p,
                          const float* det, const int32_t* count, int B, int max_det,
                          const int* stream_of /* HOST [B] */, const unsigned char* flush /* HOST [n_streams] or NULL */,
                          float* det_out, int32_t* tid, int32_t* slot, int32_t* ended_i, float* ended_f, int32_t* ended_count,
                          int max_ended, void* stream);
/* lp_track_update_hold: lp_track_update_slots (which is this call with hp = NULL: the hold outputs are then ignored) that also
 * emits, per frame, the rows redaction has to cover: the frame's own rows followed by one predicted row for every track the
 * frame missed, so that a plate the detector loses for a frame is not stored readable (lp_redact_plates_batch takes det_hold,
 * count_hold as they are).  The hold reads the state and never writes it: det_out, tid, slot, the ended records, `dropped` and
 * every state byte are what they are without it.
 *  11. hold: in a tracked frame, after step 5, a slot is held iff it was live at the start of the frame, was not matched, did
 *      not end in this frame, has hits >= min_hits and, after the increment of 5, misses <= max_misses (values above max_age
 *      behave as max_age: the track ends first).  A slot that ended in this frame and was re-used by a new track is not held.
 *      The held row of a slot, fp32 op by op: k = (float)misses, dx = vx * k, dy = vy * k (the k and the rounded products of
 *      step 1 of this frame); columns 0..3 = the stored box + (dx, dy, dx, dy), bit for bit the box step 1 predicted before the
 *      expansion; columns 4..11 = the stored corners, x columns (4, 6, 8, 10) + dx, y columns (5, 7, 9, 11) + dy; columns
 *      12..19 the track's shares and 20..27 its voted ids (8; the slot cast no vote in this frame).
 *   Per frame b, nc = min(max(count[b], 0), max_det): det_hold [B, max_det + max_tracks, 28] = rows 0..nc-1 of det_out[b] (all of
 *   them, those past LP_TRACK_MAX_DETS included), then the held rows in slot order, every later row zero; count_hold [B] = nc +
 *   the number of held rows (never capped: max_tracks extra rows always fit); tid_hold [B, max_det + max_tracks] int32 = tid
 *   for the first nc rows, the track id for held rows, -1 elsewhere.  A frame with stream_of -1 gets its copied rows,
 *   count_hold = nc and no held row.  Flushing happens after the frames and changes nothing here.  The hold does not grow the
 *   box with the track's age, has no model beyond the constant velocity of step 1 and holds nothing past max_age.
 * Also checked before the first launch with hp != NULL: min_hits >= 1, max_misses >= 0, the three hold pointers non-null (B > 0),
 * det_hold overlapping neither det nor det_out, (max_det + max_tracks) * 28 below 2^31. */
typedef struct lp_track_hold_params { int min_hits, max_misses; } lp_track_hold_params;
int lp_track_update_hold(void* state, int n_streams, int max_tracks, const lp_track_params* p,
                         const float* det, const int32_t* count, int B, int max_det,
                         const int* stream_of /* HOST [B] */, const unsigned char* flush /* HOST [n_streams] or NULL */,
                         float* det_out, int32_t* tid, int32_t* slot, int32_t* ended_i, float* ended_f, int32_t* ended_count,
                         int max_ended, const lp_track_hold_params* hp, float* det_hold, int32_t* count_hold, int32_t* tid_hold,
                         void* stream);

/* lp_plate_crops_batch: perspective-rectified plate crops of B frames' detections (the inverse of the warp of the reference's
 * plate generator, yolov6/data/generate/generate.py:566-586), one launch per LP_FRAMES_PER_LAUNCH frames; descriptors travel
 * as kernel arguments, so nothing is uploaded and the call may be captured in a graph.
 *   det [n_frames,max_det,28] fp32 in source-frame pixels (as lp_rescale_round_batch leaves it); count: DEVICE int32
 *   [n_frames], read by the kernel (no host sync).  Frame b crops its rows r < n_b = clamp(count[b], 0, min(max_det,
 *   max_crops_b)) into slot out_slot_b + r of out [n_slots,crop_h,crop_w,3] uint8 BGR (the frames' pixel format), and writes
 *   status[out_slot_b + r] for every r < max_crops_b: 1 = cropped along the corners, 2 = along the box, 3 = neither is
 *   usable (crop filled with 0), 0 = not cropped (r >= n_b; those crop pixels are left untouched).  Nothing outside the
 *   frames' slot ranges is written.
 *   Quad: corners TL (c4,c5), TR (c10,c11), BR (c8,c9), BL (c6,c7) if all finite, strictly convex in label orientation (the
 *   cross products of consecutive edges along TL->BL->BR->TR all < 0, y down) and of area >= 1; else the box (x1,y1)-(x2,y2)
 *   if finite with x2-x1 >= 1 and y2-y1 >= 1.  Map: the fp64 square-to-quad projective map (Heckbert), (0,0)->TL, (1,0)->TR,
 *   (1,1)->BR, (0,1)->BL.  Output pixel (i,j) samples the map at ((j+0.5)/crop_w, (i+0.5)/crop_h), source point
 *   clamp(X-0.5, 0, w0-1), clamp(Y-0.5, 0, h0-1) (edge replicated), fp32 bilinear blend, rounded half to even: what
 *   grid_sample(bilinear, border, align_corners=False) gives at the mapped points.  yolov6/utils/plate_crop.py restates it
 *   bit for bit.
 *   desc is a HOST array of n_frames entries; every entry (img, h0, w0 >= 1, max_crops, out_slot >= 0, out_slot + max_crops <=
 *   n_slots, no two frames' slot ranges overlapping) and 1 <= crop_h, crop_w <= 1024 are checked before anything is launched
 *   (LP_ERR_ARG names the frame); the pointers must be non-null when any frame has max_crops > 0.  Nothing to do: LP_OK. */
typedef struct lp_crop_desc {
    const unsigned char* img;   /* device uint8 [h0,w0,3] BGR, any alignment (as lp_frame_desc) */
    int h0, w0;
    int max_crops;              /* slots reserved for this frame */
    int out_slot;               /* first output slot of this frame */
} lp_crop_desc;
int lp_plate_crops_batch(const lp_crop_desc* desc, int n_frames, const float* det, const int32_t* count, int max_det,
                         unsigned char* out, int32_t* status, int n_slots, int crop_h, int crop_w, void* stream);

/* lp_crop_sharpness: the Laplacian energy of plate crops, an integer per crop that ranks the frames of one track by focus.
 *   crops [n_slots,crop_h,crop_w,3] uint8 BGR + status [n_slots] int32 as lp_plate_crops_batch leaves them (DEVICE); sharp
 *   [n_slots] unsigned 64-bit (DEVICE, 8-byte aligned).  For a slot with status 1 or 2:
 *     g = (29 * B + 150 * G + 77 * R + 128) >> 8 per pixel;
 *     L = 4 g(i,j) - g(i-1,j) - g(i+1,j) - g(i,j-1) - g(i,j+1) on the interior 1 <= i <= crop_h-2, 1 <= j <= crop_w-2;
 *     sharp = the sum of L * L (|L| <= 1020: a 64 x 192 checkerboard of 0 / 255 gives 12255912000 > 2^32).
 *   sharp = 0 for status 0 or 3, or when a side is shorter than 3.  One workgroup per slot, no atomics; all integer, so the
 *   result does not depend on the order of the sum.  yolov6/utils/best_shot.py::crop_sharpness_np restates it.
 *   Sensor noise raises the measure as focus does: it ranks the frames of one track and is not comparable across cameras. */
int lp_crop_sharpness(const unsigned char* crops, const int32_t* status, int n_slots, int crop_h, int crop_w,
                      unsigned long long* sharp, void* stream);

/* lp_best_shot_update: the sharpest rectified crop of every live plate track, kept on the device and handed out next to the
 * track's record when the track ends.  Called right behind lp_track_update_slots, lp_plate_crops_batch and lp_crop_sharpness
 * of the same frames; the frame table travels as kernel arguments (one launch per LP_FRAMES_PER_LAUNCH frames, one workgroup per
 * stream, plus one closing launch): nothing is uploaded, no host sync, capturable in a graph.  The reference has nothing here;
 * yolov6/utils/best_shot.py::BestShotNp restates the rules below bit for bit.
 *   state: DEVICE, 16-byte aligned, lp_best_shot_state_bytes(n_streams, max_tracks, crop_h, crop_w) bytes, all zero = empty (the
 *   caller zeroes it once; zeroing a stream's lp_best_shot_state_bytes(1, ...) bytes resets that stream).  Per stream: its own
 *   frame counter and max_tracks entries indexed by the tracker's slot, each id + 1 (0 = empty), a has-shot flag, a 64-bit key,
 *   the frame, row and status of the shot, its det row and the crop bytes (16-byte aligned).
 *   det [B,max_det,28] + count [B]: the rows GIVEN to the tracker (their raw per-frame confidences); tid, slot [B,max_det] as
 *   lp_track_update_slots wrote them; crops [B,max_crops,crop_h,crop_w,3], status [B,max_crops], sharp [B,max_crops] as
 *   lp_plate_crops_batch (frame b's slots at b * max_crops) and lp_crop_sharpness wrote them; stream_of: HOST int [B], as given to
 *   the tracker; ended_i [n_streams,max_ended,12] + ended_count [n_streams] as that tracker call wrote them (all DEVICE).
 *   Outputs (DEVICE): shot_crops [n_streams,max_ended,crop_h,crop_w,3] uint8, shot_i [n_streams,max_ended,4] int32 = frame, row,
 *   status, valid; shot_q [n_streams,max_ended] unsigned 64-bit = the shot's sharpness; shot_det [n_streams,max_ended,28] fp32 =
 *   its det row.  The call first zeroes shot_i, shot_q and shot_det; the crop bytes of a record without a shot are left as
 *   they were (the convention of lp_plate_crops_batch's status 0).
 * Per stream the frames are taken in ascending b (stream_of -1: skipped):
 *   1. rows r < min(max(count, 0), max_det, max_crops, LP_TRACK_MAX_DETS) with tid[r] >= 0 take part, g = slot[r] (a row whose
 *      slot is outside 0..max_tracks-1 is skipped);
 *   2. if entry g holds another id it is retired (5); an entry that does not hold id becomes {id + 1, no shot};
 *   3. the row is eligible iff status[r] is 1 or 2 and (double)score >= min_score, score = (c12 + ... + c19) / 8.0f summed left
 *      to right in fp32 as lp_track_update's rule 6 (false for NaN);
 *   4. key = ((status == 1) << 63) | sharp[r]: a crop cut along the corners beats one cut along the box.  The row becomes the
 *      entry's shot iff the entry has none or key > the entry's key (strict: the earlier frame keeps a tie); that copies the crop,
 *      the det row, the stream's frame counter, r, status and key into the entry;
 *   5. retire entry g: e = the first index < min(ended_count[s], max_ended) with ended_i[s][e][0] == the entry's id; if there is
 *      one and the entry has a shot: shot_crops[s][e] = its crop, shot_i[s][e] = (frame, row, status, 1), shot_q[s][e] = the key
 *      without its top bit, shot_det[s][e] = its det row.  Either way the entry becomes empty (an occupant whose record was cut
 *      off by max_ended is dropped silently);
 *   6. the stream's frame counter goes up.  After the stream's last frame (also for a stream without frames in the call) every
 *      non-empty entry whose id is among the call's records is retired, in slot order.  Live tracks stay.
 * Every argument is checked before the first launch (LP_ERR_ARG): n_streams >= 1, max_tracks in 1..LP_TRACK_MAX_TRACKS, crop
 * sides in 1..1024, B >= 0, max_det >= 1, max_crops >= 0, max_ended >= 0, |min_score| <= 3e38, stream_of[b] in -1..n_streams-1,
 * the alignment of state, sharp and shot_q, and the pointers (crops, status, sharp may be NULL when B == 0 or max_crops == 0; the
 * record arrays when max_ended == 0). */
size_t lp_best_shot_state_bytes(int n_streams, int max_tracks, int crop_h, int crop_w);   /* 0: bad arguments */
int lp_best_shot_update(void* state, int n_streams, int max_tracks, int crop_h, int crop_w,
                        const float* det, const int32_t* count, int B, int max_det, const int32_t* tid, const int32_t* slot,
                        const unsigned char* crops, const int32_t* status, const unsigned long long* sharp, int max_crops,
                        const int* stream_of /* HOST [B] */, const int32_t* ended_i, const int32_t* ended_count, int max_ended,
                        double min_score, unsigned char* shot_crops, int32_t* shot_i, unsigned long long* shot_q, float* shot_det,
                        void* stream);

/* lp_stack_update: one denoised picture per plate track.  The rectified crops a track shows are aligned to their running sum by
 * an integer shift and summed on the device; when the track ends, the rounded mean is handed out next to its record: n crops
 * divide the noise variance by n.  Called behind lp_best_shot_update with the same arguments (it shares the crops, status and
 * sharp buffers); the frame table travels as kernel arguments (one launch per LP_FRAMES_PER_LAUNCH frames, one workgroup per
 * (stream, slot), plus one closing launch): nothing is uploaded, no host sync, no allocation, capturable in a graph.  The
 * reference has nothing here; yolov6/utils/stack.py::StackNp restates the rules below bit for bit.  All sums are integer, so the
 * result does not depend on their order.
 *   state: DEVICE, 16-byte aligned, lp_stack_state_bytes(n_streams, max_tracks, crop_h, crop_w) bytes, all zero = empty (the
 *   caller zeroes it once; zeroing a stream's lp_stack_state_bytes(1, ...) bytes resets that stream).  Per stream: its own frame
 *   counter and max_tracks entries indexed by the tracker's slot, each id + 1 (0 = empty), n, first_frame, last_frame and acc,
 *   uint16 [crop_h,crop_w,3] (16-byte aligned): the sum of the n aligned crops.
 *   det, count, tid, slot, crops, status, sharp, stream_of, ended_i, ended_count: as for lp_best_shot_update.
 *   p: search 0..4, max_frames 1..255, min_score and min_width finite (|x| <= 3e38), min_sharp.
 *   Outputs (DEVICE): stack_crops [n_streams,max_ended,crop_h,crop_w,3] uint8, stack_i [n_streams,max_ended,4] int32 = n,
 *   first_frame, last_frame, valid.  The call first zeroes stack_i; the crop bytes of a record without a stack are left as they
 *   were.
 * Per stream the frames are taken in ascending b (stream_of -1: skipped):
 *   1. rows r < min(max(count, 0), max_det, max_crops, LP_TRACK_MAX_DETS) with tid[r] >= 0 take part, in ascending r, g = slot[r]
 *      (a row whose slot is outside 0..max_tracks-1 is skipped);
 *   2. if entry g holds another id it is retired (5); an entry that does not hold id becomes {id + 1, n = 0};
 *   3. the row is eligible iff status[r] == 1 (a crop cut along the box is not rectified and is never mixed in), (double)score >=
 *      min_score with score = (c12 + ... + c19) / 8.0f summed left to right in fp32 (false for NaN), (double)(det[2] - det[0]) >=
 *      min_width, one fp32 subtraction (false for NaN; the plate's width in frame pixels), sharp[r] >= min_sharp, and the entry's
 *      n < max_frames;
 *   4. align: y(p) = 29 B + 150 G + 77 R, un-rounded.  With n == 0, search == 0, crop_h <= 2 search or crop_w <= 2 search the
 *      shift d is (0, 0).  Otherwise the candidates (dy, dx) of [-search, search]^2 are numbered k = 0.. in the order of
 *      (dy^2 + dx^2, dy, dx) (k = 0 is (0, 0)), cost_k = the sum over i in [R, crop_h-R), j in [R, crop_w-R) of
 *      | n * y(crop[i+dy][j+dx]) - y(acc[i][j]) | (the new crop against the running SUM, no division; every term is below 2^24,
 *      the sum over a 1024 x 1024 crop needs 44 bits: unsigned 64-bit), and d is the candidate of the smallest (cost, k).
 *      accumulate: acc[i][j][c] += crop[clamp(i+dy, 0, crop_h-1)][clamp(j+dx, 0, crop_w-1)][c] (an entry with n == 0 starts from
 *      zero), n += 1, first_frame is set when n was 0, last_frame = the stream's frame counter.  255 * 255 = 65025 fits uint16:
 *      that is why max_frames <= 255;
 *   5. retire entry g: e = the first index < min(ended_count[s], max_ended) with ended_i[s][e][0] == the entry's id; if there is
 *      one and n >= 1: stack_crops[s][e] = (acc + (n >> 1)) / n per channel, stack_i[s][e] = (n, first_frame, last_frame, 1).
 *      Either way the entry becomes empty (id + 1 = 0, n = 0; an occupant whose record was cut off by max_ended is dropped
 *      silently);
 *   6. the stream's frame counter goes up.  After the stream's last frame (also for a stream without frames in the call) every
 *      non-empty entry whose id is among the call's records is retired, in slot order.  Live tracks stay.
 * What the rule does not do: the shift is an integer translation of at most `search` pixels, with no rotation, scale or
 * sub-pixel step; every frame has the same weight; a track whose plate really changes (an occlusion) is averaged through it;
 * min_sharp compares Laplacian energies, which are not comparable across cameras.
 * Every argument is checked before the first launch (LP_ERR_ARG): the rules of lp_best_shot_update for the shared arguments, p and
 * its ranges, the alignment of state and sharp, and that the state, stack_crops and stack_i overlap neither an input nor each
 * other. */
typedef struct lp_stack_params { double min_score, min_width; unsigned long long min_sharp; int search, max_frames; } lp_stack_params;
size_t lp_stack_state_bytes(int n_streams, int max_tracks, int crop_h, int crop_w);   /* 0: bad arguments */
int lp_stack_update(void* state, int n_streams, int max_tracks, int crop_h, int crop_w,
                    const float* det, const int32_t* count, int B, int max_det, const int32_t* tid, const int32_t* slot,
                    const unsigned char* crops, const int32_t* status, const unsigned long long* sharp, int max_crops,
                    const int* stream_of /* HOST [B] */, const int32_t* ended_i, const int32_t* ended_count, int max_ended,
                    const lp_stack_params* p, unsigned char* stack_crops, int32_t* stack_i, void* stream);

/* lp_redact_plates_batch: make the plates of B frames unreadable IN PLACE, by a mosaic or a fill, in BGR frames or in the planes of
 * NV12 frames; at most LP_FRAMES_PER_LAUNCH frames per launch, descriptors by value in the kernel arguments: nothing is uploaded,
 * no host sync, capturable in a graph, so the call can be enqueued behind lp_rescale_round_batch.  It goes LAST: whatever reads the
 * frames (lp_plate_crops_batch, the best-shot gallery) must be enqueued before it.  The reference has nothing here;
 * yolov6/utils/redact.py::redact_plates_np restates the rules below bit for bit.
 *   det [n_frames,max_det,28] fp32 in frame pixels + count [n_frames] int32 (DEVICE, read by the kernels).  For frame b every row
 *   r < n_b = clamp(count[b], 0, max_det) is redacted: there is no cap on the plates of a frame.
 *   Quad of a row: the rule of lp_plate_crops_batch (corners if finite, strictly convex and of area >= 1, else the box if finite
 *   and >= 1 px on each side).  status [n_frames,max_det] int32: 1 corners, 2 box, 3 neither (nothing is written for the row),
 *   0 for r >= n_b.
 *   Expanded quad, fp64 op by op (no fused multiply-add): cx = 0.25 * (((x0 + x1) + x2) + x3), cy likewise, s = 1.0 + margin,
 *   x'_k = cx + s * (x_k - cx), y'_k = cy + s * (y_k - cy).
 *   Pixel (i, j) belongs to the row iff j in [clamp(floor(min x'), 0, w0), clamp(ceil(max x'), 0, w0)), i likewise in y and h0
 *   (clamped in double, then converted), and its centre P = (j + 0.5, i + 0.5) satisfies ex * (P.y - a.y) - ey * (P.x - a.x) <= 0,
 *   e = b - a, for the four edges a -> b along p0 -> p3 -> p2 -> p1 -> p0 (the label orientation; an edge belongs to the quad).
 *   A quad partly or wholly outside the frame redacts what is inside.
 *   Mosaic: the cell grid is anchored to the frame, cell (I, J) = rows [I * cell, min((I + 1) * cell, h0)) x the same in columns;
 *   its value per channel is (2 * sum + n) / (2 * n) in integers over its n pixels (the mean, rounded half up) OF THE FRAME AS IT
 *   WAS BEFORE THE CALL; a pixel that belongs to any row is replaced by its cell's value.  So the result does not depend on the
 *   order of the rows, overlapping plates store the same bytes, and a second call with the same rows changes only bytes the first changed.
 *   NV12: the luma plane takes the same cells on Y; the chroma plane cells of cell/2 x cell/2 samples, U and V averaged
 *   separately by the same formula; chroma sample (ci, cj) is replaced iff any of its four luma pixels (2ci..2ci+1, 2cj..2cj+1)
 *   belongs to a row.  The matrix plays no part (the result is not the BGR result of the converted frame).
 *   Fill: the same pixels and chroma samples get fill[0..2], bytes in the frame's own format.
 *   No other byte changes: pitch padding, pixels of no row, rows at or past n_b, frames whose count is <= 0.
 * Two kernels: the first reads the frames and writes, for every cell that the bounding rectangle of a row touches, one packed
 * entry (c0, c1, c2, 0) into the workspace (per frame a table of ceil(h0 / cell) x ceil(w0 / cell) 4-byte entries, each table at
 * a 16-byte multiple); the second reads det, count and those entries and writes the frames.  The second looks up only entries the
 * first wrote in the same call, so the workspace may hold anything on entry.  Fill is the second kernel alone (workspace unused).
 * Every argument is checked before the first launch (LP_ERR_ARG names the frame; nothing is launched): null desc, p or status,
 * null det or count with n_frames > 0, format, p0 null, p1 null (NV12) or non-null (BGR), the NV12 plane rules of lp_nv12_desc,
 * pitch0 < 3 * w0 (BGR), h0 or w0 < 1, mode, cell odd or outside 2..LP_REDACT_MAX_CELL (mosaic), margin outside [0, 4] or NaN,
 * max_det < 1, and in mosaic mode a workspace that is null, not 16-byte aligned or smaller than lp_redact_workspace_bytes.
 * n_frames == 0: LP_OK. */
#define LP_REDACT_MAX_CELL 64
typedef struct lp_redact_desc {
    unsigned char* p0;      /* BGR: the frame, uint8 [h0][w0][3], rows pitch0 >= 3*w0 bytes apart, any alignment.  NV12: the luma plane */
    unsigned char* p1;      /* BGR: NULL.  NV12: the chroma plane (2-byte aligned, U first) */
    int pitch0, pitch1;     /* NV12: pitch0 >= w0, pitch1 >= w0 and even (the plane rules of lp_nv12_desc) */
    int h0, w0;             /* NV12: both even, >= 2 */
    int format;             /* 0 BGR, 1 NV12 */
} lp_redact_desc;
typedef struct lp_redact_params {
    int mode;               /* 0 mosaic, 1 fill */
    int cell;               /* mosaic: side of a cell in pixels, even, 2..LP_REDACT_MAX_CELL (64) */
    double margin;          /* the quad is scaled by 1 + margin about its centre; 0 <= margin <= 4 */
    unsigned char fill[3];  /* fill: the bytes written, in the frame's own format: (B,G,R), or (Y,U,V) */
} lp_redact_params;
size_t lp_redact_workspace_bytes(const lp_redact_desc* desc, int n_frames, const lp_redact_params* p);  /* 0 for fill (and for bad arguments) */
int lp_redact_plates_batch(const lp_redact_desc* desc, int n_frames, const float* det, const int32_t* count, int max_det,
                           const lp_redact_params* p, int32_t* status /* [n_frames,max_det] */,
                           void* workspace, size_t workspace_bytes, void* stream);

/* lp_redact_gauss_batch: the third redaction, a Gaussian blur.  The pixel set is that of lp_redact_plates_batch to the letter (rows,
 * quad, margin, scan rectangle, edge tests, status codes, the NV12 "chroma sample iff any of its four luma pixels" rule); only the
 * value written is new: a pixel of any row takes G(frame) at that pixel, where G is the frame AS IT WAS BEFORE THE CALL under the
 * integer separable blur below.  G depends on the frame alone, so the result does not depend on the order of the rows and
 * overlapping plates store the same bytes; no byte outside the union of the masks changes.  Unlike the mosaic a second call is
 * NOT idempotent inside the mask: it blurs again.  yolov6/utils/redact.py::redact_plates_np (mode 'gauss') restates it bit for bit.
 *   Taps are data (yolov6/utils/redact.py::gauss_taps computes them in float64; the device evaluates no exponential):
 *   t[0..radius], non-increasing, t[0] + 2 * (t[1] + ... + t[radius]) = 16384, radius in 1..LP_REDACT_MAX_RADIUS.
 *   Blur of one plane of bytes p, indices clamped to the plane (replicate border), int32 throughout:
 *     hq[i][j]  = (sum_k t[|k|] * p[i][clamp(j + k)] + 32) >> 6          (k = -radius..radius; at most 65280)
 *     out[i][j] = (sum_k t[|k|] * hq[clamp(i + k)][j] + (1 << 21)) >> 22  (the sum stays below 2^31)
 *   A constant plane comes out unchanged.  BGR: the three channels, the same taps.  NV12: Y with taps / radius; U and V with
 *   taps_c / radius_c, each on the half-resolution chroma plane in chroma coordinates (the clamp too); the matrix plays no part.
 * Two kernels: the first only reads the frames and writes the workspace: per frame a table of h0 x w0 4-byte entries
 * (c0, c1, c2, 0), one per pixel (NV12: the pixel's blurred luma and its block's blurred U, V), each table at a 16-byte
 * multiple; it fills every frame-anchored 32 x 32 tile that the scan rectangle of a row touches, one workgroup per tile, the tile
 * and its halo staged through LDS once.  The second (the write kernel of lp_redact_plates_batch at cell 1) reads det, count and
 * entries the first wrote in the same call, and writes the frames; the workspace may hold anything on entry.  Every blur launch
 * of a call precedes its first write launch.  At most LP_FRAMES_PER_LAUNCH frames of one format per launch, descriptors and taps
 * by value in the kernel arguments: nothing is uploaded, no host sync, capturable in a graph.
 * Every argument is checked before the first launch (LP_ERR_ARG; nothing is launched): whatever lp_redact_plates_batch rejects for
 * descriptors, det, count, status, margin and max_det; radius outside 1..LP_REDACT_MAX_RADIUS; taps that increase; a tap total
 * other than 16384; with an NV12 frame the same three on radius_c and taps_c; a workspace that is null, not 16-byte aligned or
 * smaller than lp_redact_gauss_workspace_bytes.  n_frames == 0: LP_OK. */
#define LP_REDACT_MAX_RADIUS 48
typedef struct lp_redact_gauss_params {
    double margin;                                  /* as lp_redact_params */
    int radius, radius_c;                           /* of taps (BGR, Y) and of taps_c (U, V; read only with an NV12 frame) */
    uint16_t taps[LP_REDACT_MAX_RADIUS + 1];        /* t[0..radius] */
    uint16_t taps_c[LP_REDACT_MAX_RADIUS + 1];
} lp_redact_gauss_params;
size_t lp_redact_gauss_workspace_bytes(const lp_redact_desc* desc, int n_frames, const lp_redact_gauss_params* p);  /* 0 for bad arguments */
int lp_redact_gauss_batch(const lp_redact_desc* desc, int n_frames, const float* det, const int32_t* count, int max_det,
                          const lp_redact_gauss_params* p, int32_t* status /* [n_frames,max_det] */,
                          void* workspace, size_t workspace_bytes, void* stream);

/* lp_overlay_draw_batch: draw the detections of B frames onto them IN PLACE -- box outline, corner-quad outline, a label plate and
 * the label's glyphs (track id and the eight heads' characters) -- in BGR frames or in the planes of NV12 frames (no BGR copy of an
 * NV12 frame exists); at most LP_FRAMES_PER_LAUNCH frames of one format per launch pair, descriptors, styles and palette by value
 * in the kernel arguments: nothing is uploaded, no host sync, capturable in a graph.  It goes LAST on a stream: crops and best
 * shots read the frames first, redaction comes next, the overlay after it, so outlines sit on top of a mosaic.  The reference
 * draws nothing; yolov6/utils/overlay.py::draw_plates_np restates the rules below byte for byte.
 *   det [n_frames,max_det,28] fp32 in frame pixels + count [n_frames] int32 (DEVICE).  Rows r < n_b = clamp(count[b], 0, max_det)
 *   are painted in row order, a later row over an earlier one; a row paints up to four layers in the order box outline, quad
 *   outline, label plate, label glyphs.  Every layer is a blend that ends in a byte: one call with n rows equals n calls of one row.
 *   tid [n_frames,max_det] int32 (DEVICE, may be NULL): the track id of a row, < 0 for none.  style [n_frames,max_det] int32
 *   (DEVICE, may be NULL: style 0): the row's entry of p->styles; < 0 skips the row (status 0); >= n_styles takes the last.
 *   Which shape: the quad rule of lp_plate_crops_batch.  status [n_frames,max_det] int32: 1 corners: the box outline in the box
 *   colour (only with p->draw_box and a box, columns 0..3, that is finite with sides >= 1 px), then the quad outline in the quad
 *   colour; 2 box: the box outline alone, in the box colour, whatever draw_box says; 3: nothing is drawn, no label either; 0 for
 *   r >= n_b and for a skipped row.
 *   Outline of thickness t (0: none) of the closed polygon p0 -> p3 -> p2 -> p1 -> p0: pixel (i, j) belongs iff the squared
 *   distance from its centre P = (j + 0.5, i + 0.5) to any of the four segments is <= (t / 2)^2 (round joins; a zero-length
 *   segment is a point).  fp64 on the row's fp32 values, op by op (no fused multiply-add), no division; per segment a -> b:
 *     ex = bx - ax, ey = by - ay, L = ex * ex + ey * ey, dx = px - ax, dy = py - ay, d = dx * ex + dy * ey
 *     d <= 0: dx * dx + dy * dy <= hw2;  d >= L: fx = px - bx, fy = py - by, fx * fx + fy * fy <= hw2;
 *     else cr = dx * ey - dy * ex, cr * cr <= hw2 * L;     hw = 0.5 * t, hw2 = hw * hw.
 *   Scan rectangle: rows [clamp(floor(min y - hw), 0, h0), clamp(ceil(max y + hw), 0, h0)), columns likewise in x and w0 (clamped
 *   in double, then converted, as lp_redact_plates_batch clamps).
 *   Label (p->label): glyphs '#', the decimal digits of tid, ' ' (only with tid >= 0 and p->show_id), then for head h = 0..7:
 *   v = row[20 + h]; glyph_of[h][(int)v] when v is finite and 0 <= v < 64, the '?' glyph otherwise and for an entry >= n_glyphs
 *   (0xFFFF by convention); at most LP_OVERLAY_MAX_GLYPHS.  atlas (DEVICE) uint8 [n_glyphs][gh][gw] coverage with the fixed
 *   indices 0..9 digits, 10 '#', 11 ' ', 12 '?'; glyph_of (DEVICE) uint16 [8][64].  W = n * gw + 2 * pad, H = gh + 2 * pad.  With
 *   the quad's integer bounds bx0 = floor(min x), by0 = floor(min y), by1 = ceil(max y), each clamped to +-2^20 in double and then
 *   converted, and q = (t + 1) / 2: ly = by0 - q - H, and ly = by1 + q when that is < 0; lx = max(min(bx0, w0 - W), 0).  The
 *   rectangle [ly, ly + H) x [lx, lx + W) is clipped to the frame.  Plate layer: every pixel of it at coverage 255.  Glyph layer:
 *   coverage atlas[g_k][i - ly - pad][j - lx - pad - k * gw] for the pixels of cell k.
 *   Blend of opacity a (0..256) and coverage c (255 for outlines and the plate): w = a * c <= 65280 and, per channel in int32,
 *   out = (fg * w + dst * (65280 - w) + 32640) / 65280: w = 0 leaves the byte, w = 65280 stores fg exactly.
 *   NV12: Y per pixel; a chroma sample once per layer with wbar = (w00 + w01 + w10 + w11 + 2) >> 2 over its four luma pixels,
 *   U and V separately.  Colours are bytes in the frame's own format: (B,G,R), or (Y,U,V); no matrix plays a part.
 *   Palette: a row with tid >= 0 takes palette[tid % n_palette] as its quad and plate colours (n_palette 0: none).
 *   No other byte changes: pitch padding, pixels of no layer, rows at or past n_b, frames whose count is <= 0.
 * Two kernels per launch pair (lp_overlay.hip): the first, a thread per (frame, row), writes a fixed-size record and a bounding
 * rectangle per row into the workspace, and status; the second, a 256-thread workgroup per frame-anchored 32 x 32 tile and a thread
 * per 2 x 2 pixel block, culls the rows against its tile into an LDS list in row order, returns before reading a pixel when the
 * list is empty, and otherwise loads its block once, blends the listed rows in order in registers and stores the block once: every
 * pixel has one owner, so the in-place painter's order needs no atomics.  The workspace may hold anything on entry.
 * Every argument is checked before the first launch (LP_ERR_ARG names the frame; nothing is launched): whatever
 * lp_redact_plates_batch rejects for descriptors, det, count, status and max_det; null p, atlas or glyph_of; n_styles outside
 * 1..LP_OVERLAY_MAX_STYLES; t or pad outside 0..16 or an opacity outside 0..256 in a used style; n_palette outside
 * 0..LP_OVERLAY_MAX_PALETTE; n_glyphs outside 13..LP_OVERLAY_MAX_ATLAS; gh or gw outside 1..LP_OVERLAY_MAX_CELL; a workspace that is
 * null, not 16-byte aligned or smaller than lp_overlay_workspace_bytes.  n_frames == 0: LP_OK. */
#define LP_OVERLAY_MAX_STYLES 8
#define LP_OVERLAY_MAX_GLYPHS 20
#define LP_OVERLAY_MAX_THICKNESS 16
#define LP_OVERLAY_MAX_PAD 16
#define LP_OVERLAY_MAX_PALETTE 64
#define LP_OVERLAY_MAX_ATLAS 1024
#define LP_OVERLAY_MAX_CELL 64
typedef struct lp_overlay_style {
    unsigned char box[3], quad[3], plate[3], text[3];   /* the colours of the four layers, bytes in the frame's own format */
    int t;                                              /* outline thickness in pixels, 0..16 (0: no outline) */
    int a_line, a_plate, a_text;                        /* opacity 0..256 of the outlines, the label plate, the glyphs */
    int pad;                                            /* pixels between the label's edge and its glyphs, 0..16 */
} lp_overlay_style;
typedef struct lp_overlay_params {
    int n_styles;                                       /* 1..LP_OVERLAY_MAX_STYLES */
    lp_overlay_style styles[LP_OVERLAY_MAX_STYLES];
    int n_palette;                                      /* 0..LP_OVERLAY_MAX_PALETTE */
    unsigned char palette[LP_OVERLAY_MAX_PALETTE][3];
    int n_glyphs, gh, gw;                               /* the atlas: [n_glyphs][gh][gw] */
    int show_id, label, draw_box;                       /* booleans */
} lp_overlay_params;
size_t lp_overlay_workspace_bytes(int n_frames, int max_det);      /* 288 bytes per (frame, row); 0 for bad arguments */
int lp_overlay_draw_batch(const lp_redact_desc* desc, int n_frames, const float* det, const int32_t* count, int max_det,
                          const int32_t* tid /* may be NULL */, const int32_t* style /* may be NULL */, const lp_overlay_params* p,
                          const unsigned char* atlas, const uint16_t* glyph_of, int32_t* status /* [n_frames,max_det] */,
                          void* workspace, size_t workspace_bytes, void* stream);

/* lp_overlay_scene_batch: draw what the tracker knows about the scene onto B frames IN PLACE -- the zones of lp_zone_update as a
 * translucent fill plus an outline, its directed lines with a marker on their +1 side, a label per line with its running +/-
 * totals, a label per zone with its occupancy (in an alert colour while a dwell alert fires), and a km/h tag beside every drawn
 * plate whose track has a speed estimate of lp_speed_update -- in BGR frames or in the planes of NV12 frames, from DEVICE-resident
 * inputs with no host read.  On a stream it goes after the redaction and BEFORE lp_overlay_draw_batch, so zone fills lie under the
 * plate outlines.  The reference draws nothing; yolov6/utils/scene.py::draw_scene_np restates the rules below byte for byte.  The
 * picture agrees with lp_zone_update: a filled pixel is an anchor it would call inside, the marker sits on the side it counts +1.
 *   stream_of (HOST, may be NULL: frame b is stream b) int32 [n_frames]: the stream of a frame; an entry outside [0, n_streams)
 *   skips the frame (no byte changes, status 0).  packed (DEVICE) int32 [n_streams][LP_ZONE_MAP_WORDS]: the map lp_zone_update
 *   takes (the caller has validated it: a zone whose vertex count is outside 3..16 is not drawn).  Three optional groups, each
 *   all given or all NULL: totals [n_streams][2][16] + occ [n_streams][8] (absent: no labels, no zone is busy); zone_ev
 *   [n_streams][max_events][12] + zone_count [n_streams] (absent: no alert colour); speed_i [n_streams][max_tracks][8] + det
 *   [n_frames][max_det][28] + count [n_frames] + tid [n_frames][max_det] + status [n_frames][max_det] (absent: no tags); all
 *   DEVICE int32 (det fp32) as lp_zone_update, lp_speed_update and lp_track_update leave them.  names (DEVICE, may be NULL: empty
 *   names) uint16 [n_streams][24][LP_SCENE_MAX_NAME]: lines 0..15, then zones 0..7, glyph indices, 0xFFFF ends a name.
 *   Layers of a frame of stream s, in this order, each one blend of lp_overlay_draw_batch that ends in a byte (one call equals
 *   the layers applied one at a time):
 *   1. zone fills, z ascending: pixel (i, j) belongs iff the crossing number over the zone's edges (Vk, Vk+1 mod n) at P = (j + 0.5,
 *      i + 0.5) is odd; an edge toggles iff (yi > py) != (yj > py) and, with t = (xj - xi) * (py - yi) - (px - xi) * (yj - yi),
 *      t > 0 if yj > yi, else t < 0: fp64 on the fp32 vertices, op by op, no fused multiply-add, no division -- lp_zone_update's
 *      test.  Scan rectangle: the vertices' bounds, clamped as an outline's.  Opacity a_fill, or a_fill_busy when occ[s][z] > 0;
 *      colour zone, or alert when one of the first min(max(zone_count[s], 0), max_events) event lines has kind 4 and index z.
 *   2. zone outlines, z ascending: the closed polygon V0 -> V1 -> ... -> V0 by the segment test of lp_overlay_draw_batch at
 *      thickness t (0: none), opacity a_line, the fill's colour; scan rectangle: the bounds grown by t / 2.
 *   3. lines, l ascending: the segment A -> B likewise in the line colour; then, as its own layer in the mark colour at a_line, the
 *      marker: M = ((ax + bx) * 0.5, (ay + by) * 0.5), e = B - A, L = ex * ex + ey * ey, dx = px - Mx, dy = py - My,
 *      s = ex * dy - ey * dx, u = dx * ex + dy * ey, q = |u| + s; the pixel belongs iff L > 0, s >= 0 and q * q <= (m * m) * L,
 *      m = marker (0: none): a right isosceles triangle of height m, base on the line, apex on the +1 side.  fp64 op by op, no
 *      division, no square root.  Scan rectangle: M grown by m, clamped.
 *   4. zone labels z ascending, then line labels l ascending: plate (plate colour, a_plate) and glyphs (text colour, a_text) as
 *      lp_overlay_draw_batch blends a label.  Zone: the name, ' ', the digits of occ[s][z]; line: the name, ' ', '+', the digits of
 *      totals[s][0][l], ' ', '-', the digits of totals[s][1][l]; a value < 0 prints as its 32-bit unsigned value (the totals wrap);
 *      a name glyph >= n_glyphs shows '?'; at most LP_SCENE_MAX_GLYPHS.  atlas (DEVICE) uint8 [n_glyphs][gh][gw] with the fixed
 *      indices of lp_overlay_draw_batch and 13 '+', 14 '-', 15 '.', 16 ':'.  Placement: the anchor (x, y) is vertex 0 of a zone, B of
 *      a line; ax = floor(x), ay0 = floor(y), ay1 = ceil(y), each clamped to +-2^20 in double and converted; W = n * gw + 2 * pad,
 *      H = gh + 2 * pad, q = (t + 1) / 2; ly = ay0 - q - H, and ly = ay1 + q when that is < 0; lx = max(min(ax, w0 - W), 0); the
 *      rectangle [ly, ly + H) x [lx, lx + W) is clipped to the frame.
 *   5. speed tags, rows in row order: row r < clamp(count[b], 0, max_det) with tid >= 0 whose quad status (lp_plate_crops_batch's
 *      rule) is not 3 gets a tag iff speed_i[s] has a slot with id == tid and speed >= 0, the lowest such slot; kmh = (speed * 36 +
 *      5000) / 10000 in int64; the tag is a label of the digits of kmh on a plate in the tag colour with bx1 = ceil(max x), by0 =
 *      floor(min y) of the quad (clamped to +-2^20), ly = by0, lx = max(min(bx1 + q, w0 - W), 0), clipped.  status = 1 for a row
 *      that gets a tag, else 0.
 *   NV12: Y per pixel, a chroma sample once per layer with wbar = (w00 + w01 + w10 + w11 + 2) >> 2.  Colours are bytes in the frame's
 *   own format.  No other byte changes: pitch padding, pixels of no layer, skipped frames.
 * Two kernels per launch pair of at most LP_FRAMES_PER_LAUNCH frames of one format (lp_overlay_scene.hip), in the ownership
 * structure of lp_overlay_draw_batch: a setup kernel, a thread per (frame, shape) and per (frame, row), writes fixed-size records
 * with clamped scan rectangles into the workspace (which may hold anything on entry); the draw kernel, a 256-thread workgroup per
 * 32 x 32 tile and a thread per 2 x 2 block, culls the frame's 72 shape layers and its tags into an LDS list in layer order, returns
 * before reading a pixel when the list is empty, and otherwise loads its block once, blends in registers and stores once.  The fill
 * tests every pixel.  Descriptors, streams and style travel by value in the kernel arguments: nothing is uploaded, no host sync,
 * capturable in a graph.  Every argument is checked before the first launch (LP_ERR_ARG names the frame; nothing is launched):
 * whatever lp_redact_plates_batch rejects for descriptors; null desc, packed, p or atlas; n_streams < 1; a group that is half
 * given; max_events < 1 with events, max_tracks or max_det < 1 with tags; t or pad outside 0..16, marker outside
 * 0..LP_SCENE_MAX_MARKER, an opacity outside 0..256; n_glyphs outside LP_SCENE_FIXED_GLYPHS..LP_OVERLAY_MAX_ATLAS (an atlas too small
 * for the fixed glyphs); gh or gw outside 1..LP_OVERLAY_MAX_CELL; a workspace that is null, not 16-byte aligned or smaller than
 * lp_overlay_scene_workspace_bytes(n_frames, max_det with tags, else 0).  n_frames == 0: LP_OK. */
#define LP_SCENE_MAX_GLYPHS 36   /* a 12-glyph name, " +", 10 digits, " -", 10 digits */
#define LP_SCENE_MAX_NAME 12
#define LP_SCENE_MAX_MARKER 64
#define LP_SCENE_FIXED_GLYPHS 17
typedef struct lp_scene_style {
    unsigned char zone[3], alert[3], line[3], mark[3], plate[3], text[3], tag[3];   /* bytes in the frame's own format */
    int t;                                              /* thickness of outlines and lines, 0..16 (0: none) */
    int marker;                                         /* height m of a line's direction marker, 0..64 (0: none) */
    int a_fill, a_fill_busy, a_line, a_plate, a_text;   /* opacities 0..256 */
    int pad;                                            /* pixels between a label's edge and its glyphs, 0..16 */
    int n_glyphs, gh, gw;                               /* the atlas: [n_glyphs][gh][gw] */
} lp_scene_style;
size_t lp_overlay_scene_workspace_bytes(int n_frames, int max_det);      /* 4640 bytes per frame + 48 per (frame, row); 0 for bad arguments */
int lp_overlay_scene_batch(const lp_redact_desc* desc, int n_frames, const int32_t* stream_of /* HOST, may be NULL */, int n_streams,
                           const int32_t* packed, const int32_t* totals, const int32_t* occ, const int32_t* zone_ev,
                           const int32_t* zone_count, int max_events, const int32_t* speed_i, int max_tracks, const float* det,
                           const int32_t* count, const int32_t* tid, int max_det, const lp_scene_style* p, const unsigned char* atlas,
                           const uint16_t* names /* may be NULL */, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* lp_jpeg_encode_batch: complete baseline JPEG files of B frames, written on the device: no pixel crosses PCIe, only the files do.
 * The reference has nothing here; yolov6/utils/jpeg.py states the format and restates it in numpy byte for byte:
 * SOF0, 8 bits, 4:2:0 (MCU 16 x 16: four Y blocks, Cb, Cr), the Annex K quantisation tables scaled by quality 1..100 as libjpeg
 * scales them, the Annex K.3 Huffman tables, restart intervals of `restart` MCUs along the linear MCU order (each byte aligned with
 * 1-bits, DC predictors 0 at its start, RSTm with m modulo 8 between them), 0x00 after every 0xFF of entropy data, sizes that are
 * no multiple of 16 padded by replication, SOF0 carrying the true size.
 *   Sources (the descriptor style of lp_redact_desc, plus the NV12 matrix).  format 0: a BGR frame, uint8 [h0][w0][3], rows pitch0 >=
 *   3 * w0 bytes apart, any alignment, converted by the integer JFIF rule of jpeg.py.  format 1: an NV12 frame under the plane rules
 *   of lp_nv12_desc whose matrix is 2 (bt601f): its planes are JFIF already and feed the transform as they are.  Any other matrix
 *   is LP_ERR_ARG here: convert such a frame with lp_nv12_to_bgr_batch first.  1 <= h0, w0 <= 65535.
 *   headers (DEVICE) uint8 [n_frames][header_len]: SOI .. SOS of each frame as jpeg.py::jpeg_header makes them (equal lengths; they
 *   must state the quality and restart of `params`, which the kernels derive their tables from).
 *   out (DEVICE) uint8 [n_frames][cap], nbytes (DEVICE) int32 [n_frames].  On return out[f][0 .. nbytes[f]) is the whole file,
 *   EOI included.  A file that needs more than cap bytes leaves nbytes[f] = -needed and writes nothing of frame f; no byte at or
 *   beyond out[f] + cap is ever written.  1 <= cap < 2^31.
 *   workspace (DEVICE, 16-byte aligned, lp_jpeg_workspace_bytes): 768 bytes per MCU (the int16 coefficients, 3 bytes per padded
 *   pixel) + 8 bytes per restart interval (stuffed length, offset), rounded up to 16; it may hold anything on entry.
 * Four launches per LP_JPEG_PER_LAUNCH frames (lp_jpeg.hip), descriptors and tables by value in the kernel arguments: nothing is
 * uploaded, no host read, no allocation.  Every argument is checked before the first launch (LP_ERR_ARG names the frame;
 * nothing is launched or written): null desc, params, headers, out, nbytes; quality outside 1..100; restart outside
 * 1..LP_JPEG_MAX_RESTART; the frame rules above; cap or header_len < 1; a workspace that is null, misaligned or too small.
 * n_frames == 0: LP_OK.  lp_jpeg_workspace_bytes returns 0 for arguments lp_jpeg_encode_batch would reject. */
#define LP_JPEG_MAX_RESTART 32
#define LP_JPEG_PER_LAUNCH 32
typedef struct lp_jpeg_desc {
    const unsigned char* p0;    /* BGR: the frame.  NV12: the luma plane */
    const unsigned char* p1;    /* BGR: NULL.  NV12: the chroma plane (2-byte aligned, U first) */
    int pitch0, pitch1;
    int h0, w0;
    int format;                 /* 0 BGR, 1 NV12 */
    int matrix;                 /* NV12: must be 2 (bt601f); BGR: ignored */
} lp_jpeg_desc;
typedef struct lp_jpeg_params {
    int quality;                /* 1..100 */
    int restart;                /* MCUs per restart interval, 1..LP_JPEG_MAX_RESTART */
} lp_jpeg_params;
size_t lp_jpeg_workspace_bytes(const lp_jpeg_desc* desc, int n_frames, int restart);
int lp_jpeg_encode_batch(const lp_jpeg_desc* desc, int n_frames, const lp_jpeg_params* params, const unsigned char* headers,
                         int header_len, unsigned char* out, size_t cap, int32_t* nbytes, void* workspace, size_t workspace_bytes,
                         void* stream);

/* lp_lookback_update: the look-back delay of redaction.  lp_track_update_hold covers a tracked plate from its first detection on; a
 * plate enters the picture small or blurred and is detected a few frames later, and those first frames would be stored readable.
 * A small device-resident delay line keeps, per stream, the redaction rows of the last `depth` frames, adds rows to those past
 * frames once a new track's second detection has fixed its velocity, and hands the rows of a frame out `depth` frames later, when
 * the frame itself is redacted (lp_redact_plates_batch takes rel_det, rel_count as they are; its result does not depend on the
 * order of the rows).  Called right behind lp_track_update_hold of the same frames; the frame table travels as kernel arguments (one
 * launch per LP_FRAMES_PER_LAUNCH frames, one workgroup per stream, plus one closing launch per 64 streams): nothing is uploaded, no
 * host sync, capturable in a graph.  The reference has nothing here; yolov6/utils/lookback.py::LookbackNp restates the rules
 * below bit for bit.
 *   Parameters: depth D in 1..LP_LOOKBACK_MAX_DEPTH; max_back >= 0: the frames before a track's first detection that are covered;
 *   back_cap >= 0: the back rows a stored frame can take.  hold_rows = max_det + max_tracks as lp_track_update_hold lays det_hold
 *   out (any hold_rows >= max_det is taken), rows = hold_rows + back_cap: every stored entry is [rows,28] fp32 plus a count.
 *   state: DEVICE, 16-byte aligned, lp_lookback_state_bytes(n_streams, max_tracks, depth, rows) bytes, all zero = empty (the caller
 *   zeroes it once; zeroing a stream's lp_lookback_state_bytes(1, ...) bytes resets that stream, together with the tracker's).
 *   Per stream, in 4-byte words: f (the counter of tracked frames), base (every frame below it has been released), dropped (the
 *   back rows that found no room), one unused; per tracker slot 16 words: id + 1 (0 = empty), seen (0, 1 or 2), first (the stream
 *   frame of the first detection), one unused, the twelve geometry words of that detection; the D counts of the ring padded to a
 *   multiple of 4 words; the ring of D entries of rows * 28 floats, frame g living in entry g % D.  D * rows * 112 bytes plus
 *   16 + 64 * max_tracks + 4 * D (rounded up to 16) of tables.
 *   Inputs (DEVICE) are what lp_track_update_hold of the same frames left: det_hold [B,hold_rows,28] (16-byte aligned), count_hold
 *   [B], tid [B,max_det], slot [B,max_det] (a slot names at most one row of a frame); stream_of and flush: HOST, as given to the
 *   tracker.  Outputs (DEVICE): rel_det [B,rows,28] fp32 (16-byte aligned), rel_count [B], rel_frame [B] int32; tail_det
 *   [n_streams,D,rows,28] fp32 (16-byte aligned), tail_count [n_streams,D], tail_frame [n_streams,D] int32.  Every element of
 *   rel_* and tail_* is written exactly once per call, so the buffers need no clearing.
 * The frames of a stream are taken in ascending b.  Per tracked frame, its stream counter at f:
 *   A. follow: every row r < min(max_det, LP_TRACK_MAX_DETS) with slot[b][r] = t in 0..max_tracks-1 and tid[b][r] = id >= 0, in
 *      ascending r; the row is det_hold[b][r], which is det_out[b][r] (rule 11).  The entry of t holds another id, or is empty:
 *      it becomes {id + 1, seen = 1, first = f, geometry = columns 0..11}.  It holds id with seen == 1: the row CONFIRMS the
 *      track (B) and seen = 2.  seen == 2: nothing happens.
 *   B. back rows of a confirming row, fp32 op by op, no fused multiply-add: k = (float)(f - first),
 *      vx = ((x1' + x2') * 0.5f - (x1 + x2) * 0.5f) / k and vy likewise (step 4 of lp_track_update; primes mark the confirming
 *      row, the unprimed values are the stored first geometry).  Targets: every frame g with
 *      max(base, f - D, first - max_back, 0) <= g < f and g != first, in ascending g.  The back row for g: m = (float)(g - first)
 *      (negative before the first detection, positive in the gap between the two), dx = vx * m, dy = vy * m (rounded products);
 *      columns 0..3 = the first box + (dx, dy, dx, dy); columns 4..11 = the first corners, x columns (4, 6, 8, 10) + dx, y
 *      columns (5, 7, 9, 11) + dy; columns 12..27 those of the confirming row (the track's shares and voted ids after this
 *      frame's vote).  The row is appended to the ring entry of g behind the rows already there; within one frame the appended
 *      rows come in ascending r.  An entry that already holds `rows` rows does not take the row and dropped goes up.  A track
 *      with only one detection gets no back rows.
 *   C. release: if f - D >= base: rel_det[b] = the entry of frame f - D (its rows, then zero rows), rel_count[b] its count,
 *      rel_frame[b] = f - D, then base = f - D + 1.  Otherwise rel_det[b] is all zero, rel_count[b] = 0, rel_frame[b] = -1.
 *   D. store: the entry f % D becomes the first min(max(count_hold[b], 0), hold_rows) rows of det_hold[b] followed by zero
 *      rows, with that count.  Then f goes up.
 * A frame with stream_of -1 is released at once: rel_det[b] = its own det_hold rows below the clamped count, then zero rows,
 * rel_count[b] that count, rel_frame[b] = -2; it touches no state.
 * After a stream's frames, with flush[s]: every frame still in the ring, base .. f - 1, goes to tail_det[s], tail_count[s] and
 * tail_frame[s] in ascending frame order; the remaining tail entries are zero rows, count 0, frame -1; then base = f.  The slot
 * entries stay: the tracker has ended those tracks, and new ids replace them by rule A.  A stream without a flush gets an
 * all-empty tail.  B == 0 with a flush is valid and gives tails only.
 * What it does not do: the model is constant velocity from two detections only; a plate visible for more than depth frames before
 * its confirmation is covered for depth of them; a track that is never confirmed adds nothing; the delay is depth frames of
 * latency, and depth frames that the caller's frame memory stays occupied.
 * Every argument is checked before the first launch (LP_ERR_ARG, nothing launched): depth in 1..LP_LOOKBACK_MAX_DEPTH, max_back >= 0,
 * back_cap >= 0, n_streams >= 1, max_tracks in 1..LP_TRACK_MAX_TRACKS, B >= 0, max_det >= 1, hold_rows >= max_det, rows * 28 below
 * 2^31, stream_of[b] in -1..n_streams-1, the alignment of state, det_hold, rel_det and tail_det, the pointers (the per-frame ones
 * may be NULL when B == 0; flush may be NULL: no stream is flushed), and that no output (rel_*, tail_*) overlaps the state, an
 * input or another output.  Not checked: that a slot names at most one row of a frame (the tracker's outputs do). */
#define LP_LOOKBACK_MAX_DEPTH 32
size_t lp_lookback_state_bytes(int n_streams, int max_tracks, int depth, int rows);   /* 0: bad arguments */
int lp_lookback_update(void* state, int n_streams, int max_tracks, int depth, int max_back, int back_cap,
                       const float* det_hold, const int32_t* count_hold, const int32_t* tid, const int32_t* slot,
                       int B, int max_det, int hold_rows,
                       const int* stream_of /* HOST [B] */, const unsigned char* flush /* HOST [n_streams] or NULL */,
                       float* rel_det, int32_t* rel_count, int32_t* rel_frame,
                       float* tail_det, int32_t* tail_count, int32_t* tail_frame, void* stream);

/* lp_watch_match: look the reads of the tracks that ended in a tracker call up in a device-resident watchlist (stolen vehicles,
 * permits, subscribers), tolerating misreads: a weighted Hamming distance over the eight heads that charges less for a position the
 * vote itself was unsure about and for pairs of characters listed as confusable.  Called right behind lp_track_update (any of its
 * forms) on the same stream; all pointers are DEVICE pointers; nothing is uploaded or read back, nothing is allocated, capturable
 * in a graph.  The reference has nothing here; yolov6/utils/watch.py::watch_match_np restates the rules below on every int32.
 *   entries: uint8 [n_entries,8], 8-byte aligned, 0 <= n_entries <= LP_WATCH_MAX_ENTRIES, one row per plate, one id per head: 0..63
 *   a class id, 255 the wildcard (the position is not compared), 64..254 match nothing (the host constructors refuse them; the
 *   kernel treats them as a mismatch of weight 16).
 *   confuse: uint8 [3,64,64] in sixteenths, 0..16 (larger values are read as 16), 4-byte aligned, or NULL for 16 everywhere; group
 *   0 is head 0, group 1 head 1, group 2 heads 2..7; the row is the read id, the column the entry id; the diagonal is never read.
 *   ended_i, ended_f [n_streams,max_ended,12], ended_count [n_streams]: as lp_track_update left them.  The reads are, per stream s,
 *   the lines j < min(max(ended_count[s], 0), max_ended): best[p] = ended_i[s][j][4 + p], share[p] = ended_f[s][j][p].
 * Per read, entry e and position p, w = entries[e][p]:
 *   1. q_p = share[p] > 0 ? min((int)(share[p] * 255.0f), 255) + 1 : 1 (the fp32 product, truncated; false for NaN): 1..256;
 *   2. w == 255: cost 0, no mismatch; 0 <= best[p] < 64 and w == best[p]: cost 0, no mismatch; otherwise one mismatch of cost
 *      q_p * c, c = confuse[g(p)][best[p]][w] when best[p] and w are both in 0..63, else 16;
 *   3. mism(e) and cost(e) are the int32 sums over the eight positions (cost <= 8 * 256 * 16 = LP_WATCH_MAX_COST); e is accepted iff
 *      mism(e) <= max_mismatch and cost(e) <= max_cost.
 *   match_i: int32 [n_streams,max_ended,4], line-parallel to ended_i: (entry, mismatches, cost, n_hits) = the accepted entry with
 *   the smallest (cost, index), its two sums, and the number of accepted entries (above 1: ambiguous; duplicates count, the lowest
 *   index wins).  (-1, 0, 0, 0) for a line without an accepted entry, for every line at or past its stream's count and for every
 *   line when n_entries == 0.  Every line is written by every call.  All reductions are an unsigned minimum or an integer sum: the
 *   result does not depend on the order of the workgroups.
 * Three launches: a one-workgroup kernel numbers the valid reads (a prefix sum over the clamped counts) and clears their keys; the
 * scan, one workgroup per LP_WATCH_BLOCK_ENTRIES entries, holds its entries in registers (the list is read from memory once per
 * call) and walks the reads in blocks of LP_WATCH_QUERY_BLOCK, each block through an LDS table (position, entry id, read) ->
 * (cost, mismatch), then one atomic minimum and one atomic add per workgroup and read with a hit; a tail kernel writes match_i.
 * max_ended == 0 launches nothing; n_entries == 0 launches the tail alone.
 *   workspace: 16-byte aligned, lp_watch_workspace_bytes(n_streams, max_ended) bytes; it may hold anything on entry.
 * What it does not do: no insertions or deletions (lp_watch_match_indel below tolerates one); no alert while a track is live (ended
 * records only: lp_watch_live does that); one best entry plus a count, not a ranked list; no update in place of the list.
 * Every argument is checked before the first launch (LP_ERR_ARG, nothing launched): n_entries outside 0..LP_WATCH_MAX_ENTRIES,
 * n_streams < 1, max_ended < 0, n_streams * max_ended * 12 at or above 2^31, max_mismatch outside 0..8, max_cost outside
 * 0..LP_WATCH_MAX_COST; with max_ended > 0: ended_count or match_i null; with n_entries > 0 as well: entries, ended_i, ended_f or the
 * workspace null, the three alignments, a workspace that is too small; match_i or the workspace overlapping an input or each other. */
#define LP_WATCH_MAX_ENTRIES (1 << 24)
#define LP_WATCH_MAX_COST 32768
#define LP_WATCH_BLOCK_ENTRIES 2048   /* entries per workgroup of the scan: 256 lanes x 8 */
#define LP_WATCH_QUERY_BLOCK 16       /* reads per LDS table */
size_t lp_watch_workspace_bytes(int n_streams, int max_ended);   /* 0: bad arguments */
int lp_watch_match(const unsigned char* entries, int n_entries, const unsigned char* confuse /* NULL: all 16 */,
                   const int32_t* ended_i, const float* ended_f, const int32_t* ended_count, int n_streams, int max_ended,
                   int max_mismatch, int max_cost, int32_t* match_i, void* workspace, size_t workspace_bytes, void* stream);

/* lp_watch_match_indel: lp_watch_match that survives one lost or gained character.  When two narrow glyphs merge, a rivet is read as a
 * character or a 7-character plate is read as 8, every later head moves by one and the positional distance charges four or five
 * mismatches for one error.  Heads 2..7 share one alphabet and one confusion group, so read head p is also compared with entry head
 * p + 1 and p - 1.  Arguments, reads and rules 1 and 2 are lp_watch_match's; yolov6/utils/watch.py::watch_match_np(..., indel,
 * gap_cost, align=True) restates the rules below on every int32.
 * Per read, entry e and position p let U[p] be the (cost, mismatch) pair of rule 2 for w = entries[e][p], L[p] (p in 2..6) the pair for
 * w = entries[e][p + 1] and R[p] (p in 3..7) the pair for w = entries[e][p - 1]; 255, ids 64..254 and a best[p] outside 0..63 behave
 * in L and R as in U.  With indel == 1 an entry is scored under 12 alignments, each U[0] + U[1] plus
 *   code 0        unshifted: sum U[2..7];
 *   codes 1..5    the read lost the character at entry head k = 2..6 (code k - 1): sum U[2..k-1] + sum L[k..6]; read head 7 is not
 *                 compared;
 *   codes 6..10   the read gained a character at read head k = 2..6 (code k + 4): sum U[2..k-1] + sum R[k+1..7]; read head k and
 *                 entry head 7 are not compared;
 *   code 11       the error is at the end: sum U[2..6]; head 7 is compared on neither side;
 * codes 1..11 add gap_cost (cost units, 0..LP_WATCH_MAX_GAP_COST = one fully confident mismatch) to the cost and 1 to the
 * mismatches, so the cost stays <= LP_WATCH_MAX_COST.  The entry's score is the alignment with the smallest (cost, mismatches,
 * code); e is accepted iff THAT alignment has mismatches <= max_mismatch and cost <= max_cost.  Across entries as lp_watch_match:
 * the smallest (cost, index) wins, n_hits counts the accepted entries.
 *   match_i: as lp_watch_match; its mismatches count the gap.
 *   match_align: int32 [n_streams,max_ended]: the winning entry's code; 0 on every line without a hit.  Every line is written.
 * With indel == 0 only code 0 exists: match_i is lp_watch_match's on every int32 (its scan kernel runs) and match_align is 0.
 * With max_mismatch == 1 a shifted read must be otherwise exact.
 * Three launches as lp_watch_match, with the same prep kernel and workspace (lp_watch_workspace_bytes).  The scan builds the same LDS
 * table in blocks of LP_WATCH_INDEL_QUERY_BLOCK reads; per (entry, read) it does 18 lookups, 8 for U and 5 each for L and R (row p
 * of the table at the column of the entry's head p + 1 / p - 1), and takes the minimum over the 12 alignments in one pass over the
 * positions: the prefix sum of U, the best deletion opened so far plus L[p], the best insertion opened so far plus R[p], all on the
 * word (cost << 12 | mismatches << 4 | code), whose unsigned order is the (cost, mismatches, code) order.  The code travels with the
 * lane's best entry into the 64-bit key (cost << 32 | index << 8 | code << 4 | mismatches; the index above the code keeps the order
 * across entries (cost, index)).
 * What it does not do: more than one gap; gaps in heads 0 and 1 (other alphabets); the sightings log (lp_sight_update stays
 * positional); a ranked list of matches.
 * Checked before the first launch (LP_ERR_ARG, nothing launched): everything lp_watch_match checks, indel outside 0..1, gap_cost
 * outside 0..LP_WATCH_MAX_GAP_COST, match_align null (max_ended > 0), and match_i, match_align or the workspace overlapping an
 * input or each other. */
#define LP_WATCH_MAX_GAP_COST 4096
#define LP_WATCH_INDEL_QUERY_BLOCK 16 /* reads per LDS table of lp_watch_match_indel's scan */
int lp_watch_match_indel(const unsigned char* entries, int n_entries, const unsigned char* confuse /* NULL: all 16 */,
                         const int32_t* ended_i, const float* ended_f, const int32_t* ended_count, int n_streams, int max_ended,
                         int max_mismatch, int max_cost, int indel /* 0 or 1 */, int gap_cost, int32_t* match_i, int32_t* match_align,
                         void* workspace, size_t workspace_bytes, void* stream);

/* lp_watch_live: look the reads of the tracks that are still LIVE up in a watchlist, once per track and read.  lp_watch_match answers
 * when a track has ended, max_age frames after the plate was last seen; a permit holder waiting at a barrier, or a stolen vehicle
 * still in the picture, needs the answer while its track lives.  A memo per tracker slot keeps the answer, so that a track is looked
 * up when it reaches min_hits detections and again only when its voted read changes: a stream of 25 frames a second with a handful of
 * cars causes a handful of scans of the list per car, not 25 a second.  Called behind lp_track_update (any of its forms; behind
 * lp_watch_match of the ended records if that runs too) on the same stream; all pointers but ncls are DEVICE pointers; nothing is
 * uploaded or read back, nothing is allocated, capturable in a graph.  The tracker state is read, never written.  The reference has
 * nothing here; yolov6/utils/watch_live.py::LiveWatchNp restates the rules below on every int32.
 *   track_state: the state of lp_track_update (16-byte aligned) as its last call left it; ncls: HOST int [8], the tracker's.
 *   memo: int32 [n_streams,max_tracks,8], 16-byte aligned, lp_watch_live_state_bytes bytes, all zero = empty (the caller zeroes it
 *   once, zeroes a stream's part together with the tracker's, and zeroes all of it when the list or a limit changes):
 *   id + 1, key_lo, key_hi, entry, mismatches, cost, n_hits, last_at_lookup.
 * Every stream s < n_streams is processed, whether or not the tracker call gave it a frame; every slot t < max_tracks, in order:
 *   1. a slot is live iff hits > 0; a slot that is not live gets a zero memo line;
 *   2. its read is rule 8 of lp_track_update unchanged: best_p = the first index of the largest votes[p][0..ncls[p]) (0 for an
 *      all-zero head), share_p = votes[p][best_p] / total[p] if total[p] > 0 else 0 (one fp32 division); key = the eight best_p as
 *      bytes, best_0..3 in key_lo and best_4..7 in key_hi, least significant byte first;
 *   3. it is a candidate iff it is live and hits >= min_hits (a missed slot, misses > 0, is a candidate like any other), and fresh
 *      iff it is a candidate and (memo.id != id + 1 or memo.key != key);
 *   4. the fresh slots of stream s in ascending slot order are its queries j = 0, 1, ..., in the ended-record layout (the record
 *      the track would leave if it ended now): q_i[s][j] = (id, first, last, hits, best_0..7), q_f[s][j] = (share_0..7, box x1, y1,
 *      x2, y2), q_slot[s][j] = t, q_count[s] = their number; lines past the count are zero, with q_slot -1
 *      (q_i int32 / q_f fp32 [n_streams,max_tracks,12], q_slot int32 [n_streams,max_tracks], q_count int32 [n_streams]);
 *   5. m = lp_watch_match(entries, confuse, q_i, q_f, q_count, max_ended = max_tracks, max_mismatch, max_cost), unchanged;
 *   6. every fresh slot: memo[s][t] = (id + 1, key_lo, key_hi, m.entry, m.mismatches, m.cost, m.n_hits, last); a lookup that found
 *      nothing is memoised too (entry -1), so it is not repeated;
 *   7. live_i int32 [n_streams,max_tracks,8], 16-byte aligned, one row per slot: for a live slot whose memo holds its id
 *      (id, entry, mismatches, cost, n_hits, fresh ? 1 : 0, hits, last_at_lookup); for every other slot (-1, -1, 0, 0, 0, 0, 0, 0).
 * An alert is a row with fresh == 1 and entry >= 0; fresh == 0 and entry >= 0 is a standing hit.  A new track in a reused slot
 * never inherits the memo (its id differs).  Every word of q_*, live_i is written by every call.
 * Five launches: live_gather_kernel (one workgroup per stream, steps 1 to 4: thread t reads slot t's first 16 bytes and memo line;
 * a slot that is not a candidate is not read further, nor is one whose memo holds its id with last == last_at_lookup, since votes
 * change only on a match and a match sets last; the other candidates' heads are read by one thread per (slot, head); the fresh
 * slots are numbered by ballot and prefix count), the three of lp_watch_match with its match_i in the workspace, and
 * live_scatter_kernel (one workgroup per stream, steps 6 and 7).
 *   workspace: 16-byte aligned, lp_watch_live_workspace_bytes(n_streams, max_tracks) bytes; it may hold anything on entry.
 * What it does not do: the read is the one at the end of the tracker call (several frames of a stream in one call: at most one
 * lookup per track); the memoised cost is as of the lookup (a read whose key stays while its shares move is not scored again; the
 * ended-record match stays the final word); and, as lp_watch_match, no insertions or deletions (lp_watch_live_indel below tolerates
 * one), one best entry plus a count.
 * Every argument is checked before the first launch (LP_ERR_ARG, nothing launched): n_streams < 1, max_tracks outside
 * 1..LP_TRACK_MAX_TRACKS, n_streams * max_tracks * 12 at or above 2^31, ncls null or a width outside 1..LP_TRACK_MAX_CLS,
 * min_hits < 1, n_entries outside 0..LP_WATCH_MAX_ENTRIES, max_mismatch outside 0..8, max_cost outside 0..LP_WATCH_MAX_COST, a null
 * pointer (entries only with n_entries > 0; confuse may be NULL), track_state, memo, live_i or the workspace not 16-byte aligned,
 * entries not 8-byte or confuse not 4-byte aligned (n_entries > 0), a workspace that is too small, and a written buffer (memo, q_*,
 * live_i, workspace) that overlaps the state, the list or another one. */
size_t lp_watch_live_state_bytes(int n_streams, int max_tracks);       /* of the memo; 0: bad arguments */
size_t lp_watch_live_workspace_bytes(int n_streams, int max_tracks);   /* 0: bad arguments */
int lp_watch_live(const void* track_state, int n_streams, int max_tracks, const int* ncls /* HOST [8] */, int min_hits, int32_t* memo,
                  const unsigned char* entries, int n_entries, const unsigned char* confuse /* NULL: all 16 */,
                  int max_mismatch, int max_cost, int32_t* q_i, float* q_f, int32_t* q_slot, int32_t* q_count, int32_t* live_i,
                  void* workspace, size_t workspace_bytes, void* stream);

/* lp_watch_live_indel: lp_watch_live whose step 5 is lp_watch_match_indel(..., indel, gap_cost).  Everything else -- the memo and its
 * eight words, the "look up once per read" rule, the queries, live_i -- is lp_watch_live's, and with indel == 0 every word of them is
 * what lp_watch_live writes.  One output more:
 *   8. live_align: int32 [n_streams,max_tracks], one alignment code per slot.  It is STATE beside the memo, in a tensor the caller
 *      (the tracker) owns and zeroes once together with the memo: a fresh slot gets the code of its lookup, a slot whose row of
 *      live_i is a standing one (live, memo holds its id, not fresh) keeps the code it has, every other slot gets 0.  So the
 *      alignment code of a standing hit is the one of its lookup, and a stream whose memo is zeroed needs no zeroing of live_align.
 *   workspace: 16-byte aligned, lp_watch_live_indel_workspace_bytes(n_streams, max_tracks) bytes (lp_watch_live's plus the
 *   match_align of step 5).
 * Checked before the first launch: everything lp_watch_live checks, indel outside 0..1, gap_cost outside
 * 0..LP_WATCH_MAX_GAP_COST, live_align null or overlapping another buffer. */
size_t lp_watch_live_indel_workspace_bytes(int n_streams, int max_tracks);   /* 0: bad arguments */
int lp_watch_live_indel(const void* track_state, int n_streams, int max_tracks, const int* ncls /* HOST [8] */, int min_hits,
                        int32_t* memo, const unsigned char* entries, int n_entries, const unsigned char* confuse /* NULL: all 16 */,
                        int max_mismatch, int max_cost, int indel /* 0 or 1 */, int gap_cost, int32_t* q_i, float* q_f, int32_t* q_slot,
                        int32_t* q_count, int32_t* live_i, int32_t* live_align, void* workspace, size_t workspace_bytes, void* stream);

/* lp_sight_update: a device-resident log of sightings.  Every read that ends in a tracker call is matched against the recent reads
 * of all streams -- the car the exit camera reads now is the car the entry camera read 40 minutes ago; a plate hidden for longer than
 * max_age comes back as a new track of the vehicle whose track has just ended -- and is then appended to the ring the call has just
 * scanned.  Called behind lp_track_update (any of its forms; behind lp_watch_match / lp_watch_live if they run too) on the same stream;
 * all pointers are DEVICE pointers; nothing is uploaded or read back, nothing is allocated, capturable in a graph.  The reference has
 * nothing here; yolov6/utils/sight.py::sight_update_np restates the rules below on every int32 of sight_i and of the log.
 *   state: int32 [1 + capacity,8], 16-byte aligned, lp_sight_state_bytes(capacity) bytes, 1 <= capacity <= LP_SIGHT_MAX_CAPACITY; all
 *   zero = empty (the caller zeroes it once, and again to clear the log).  Row 0 is the header (total, 0, 0, 0, 0, 0, 0, 0), total = the
 *   reads appended since the last clear (the caller keeps it below 2^31); row 1 + slot holds w0, w1 = the eight ids as bytes (position p
 *   in byte p & 3 of word p >> 2), w2, w3 = the eight position weights minus 1 as bytes, w4 = stream, w5 = track id, w6 = stamp, w7 =
 *   seq = the value of total when the read was appended.  Append number t lives in slot t % capacity; fill = min(total, capacity).
 *   confuse: as lp_watch_match (uint8 [3,64,64] sixteenths, 4-byte aligned, or NULL for 16 everywhere).
 *   pair: uint8 [n_streams,n_streams] or NULL: pair[s_read][s_entry] != 0 means that entries logged from stream s_entry are candidates
 *   for the reads of stream s_read (NULL: every pair, the same stream included; with a pair, a stored stream outside 0..n_streams-1 is
 *   allowed nowhere).
 *   ended_i, ended_f [n_streams,max_ended,12], ended_count [n_streams]: as lp_track_update left them, exactly as lp_watch_match takes them.
 *   now: int32 [1] on the DEVICE, 4-byte aligned, >= 0: the caller's clock (seconds, a frame or call number; the log does not interpret
 *   it), so that the call can sit in a captured graph while the caller bumps the value in place.  window >= 0, min_hits >= 1.
 *   1. A read is a line j < min(max(ended_count[s], 0), max_ended) whose hits (ended_i[s][j][3]) are >= min_hits; other lines are neither
 *      looked up nor appended, and their row of sight_i is the empty row.
 *   2. Every read is matched against the log as it stood before the call (the reads of one call do not see each other).  Per position p:
 *      q_r = rule 1 of lp_watch_match on share[p], q_e = the stored weight; id_r = best[p] if 0 <= best[p] < 64, else "matches nothing";
 *      equal ids in 0..63 cost 0; anything else is one mismatch of cost min(q_r, q_e) * c, c = confuse[g(p)][id_r][id_e] when both ids are
 *      in 0..63, else 16 (symmetric in the two uncertainties: both sides are voted reads; there are no wildcards).
 *   3. An entry is accepted iff its slot is filled, pair allows it, 0 <= now - stamp <= window (the difference in 64 bits), mism <=
 *      max_mismatch and cost <= max_cost.  Among the accepted entries the winner has the smallest (cost, age rank), age rank = total - 1 -
 *      seq: 0 is the newest.
 *   4. sight_i: int32 [n_streams,max_ended,8], 16-byte aligned, line-parallel to ended_i: (slot, mismatches, cost, n_hits, prev_stream,
 *      prev_id, prev_stamp, prev_seq), n_hits = the number of accepted entries; the empty row is (-1, 0, 0, 0, -1, -1, 0, 0).  The prev_*
 *      words are copied out because the winning slot may be overwritten by this same call's appends.  Every line is written by every call.
 *   5. After all matching, read k of the call, in (stream, line) order over the reads, is append number total + k with stamp now: a stored
 *      id is best[p] if it is in 0..63, else 254; a stored weight is q_r - 1; the track id is ended_i[s][j][0].  Of V > capacity reads only
 *      the last capacity are written.  total grows by V.
 * All reductions are an unsigned minimum or an integer sum: the result does not depend on the order of the workgroups.
 * Four launches: a one-workgroup kernel numbers the reads (a prefix sum), clears their keys and copies total into the workspace; the scan,
 * one workgroup per LP_SIGHT_BLOCK_ENTRIES slots, holds its slots in LDS (the log is read from memory once per call) and walks the reads in
 * blocks of LP_SIGHT_QUERY_BLOCK through an LDS table (position, stored id, read) -> confusion weight, then one atomic minimum of
 * cost << 32 | age rank << 4 | mismatches and one atomic add per workgroup and read with a hit; a tail kernel writes sight_i from the old
 * rows; only then an append kernel writes the new slots (plain vector stores) and total.  max_ended == 0 launches nothing.
 *   workspace: 16-byte aligned, lp_sight_workspace_bytes(n_streams, max_ended) bytes; it may hold anything on entry.
 * What it does not do: no insertions or deletions (the reads stay positional); one best earlier sighting plus a count, not a chain; now
 * must not run backwards (entries stamped after now simply do not match); fewer than 2^31 appends between clears; the log is not a part
 * of the tracker's state (it survives a reset of the tracker, where track ids restart: prev_seq, not prev_id, names a sighting).
 * Every argument is checked before the first launch (LP_ERR_ARG, nothing launched): capacity outside 1..LP_SIGHT_MAX_CAPACITY,
 * n_streams < 1, max_ended < 0, n_streams * max_ended * 12 at or above 2^31, window < 0, min_hits < 1, max_mismatch outside 0..8, max_cost
 * outside 0..LP_WATCH_MAX_COST; with max_ended > 0: a null pointer (confuse and pair may be NULL), the five alignments, a workspace that is
 * too small; the log, sight_i or the workspace overlapping an input or each other. */
#define LP_SIGHT_MAX_CAPACITY (1 << 24)
#define LP_SIGHT_BLOCK_ENTRIES 1024   /* slots per workgroup of the scan: 256 lanes x 4 */
#define LP_SIGHT_QUERY_BLOCK 16       /* reads per LDS table */
size_t lp_sight_state_bytes(int capacity);                          /* 0: bad arguments */
size_t lp_sight_workspace_bytes(int n_streams, int max_ended);      /* 0: bad arguments */
int lp_sight_update(int32_t* state, int capacity, const unsigned char* confuse /* NULL: all 16 */, const unsigned char* pair /* NULL: all */,
                    const int32_t* ended_i, const float* ended_f, const int32_t* ended_count, int n_streams, int max_ended,
                    const int32_t* now /* DEVICE [1] */, int window, int min_hits, int max_mismatch, int max_cost, int32_t* sight_i,
                    void* workspace, size_t workspace_bytes, void* stream);

/* lp_zone_update: tripwires and zones on the LIVE plate tracks -- line crossings with a direction, zone entry and exit, dwell alerts,
 * occupancy and in / out counts.  The tracker, the watchlists and the sightings log say which plate; a gate, a car park or a street also
 * asks which way it went and how long it has been there.  Called behind lp_track_update (any of its forms; behind lp_watch_match,
 * lp_watch_live and lp_sight_update if they run too) on the same stream; all pointers but ncls are DEVICE pointers; nothing is uploaded or
 * read back, nothing is allocated, capturable in a graph.  The tracker state is read, never written.  The reference has nothing here;
 * yolov6/utils/zones.py::ZoneEventsNp restates the rules below on every int32 of the four outputs and of the memo.
 *   track_state: the state of lp_track_update (16-byte aligned) as its last call left it; ncls: HOST int [8], the tracker's.
 *   zone_map: int32 [n_streams, LP_ZONE_MAP_WORDS], 16-byte aligned, the packed geometry of every stream, in pixels of its frames, all
 *   values finite: words 0, 1 = n_lines (0..LP_ZONE_MAX_LINES), n_zones (0..LP_ZONE_MAX_ZONES); 2..15 = 0; 16 + 4 l .. = line l, the
 *   directed segment A -> B, as fp32 bits ax, ay, bx, by; 80 + 4 z .. = zone z as n_verts (3..LP_ZONE_MAX_VERTS), min_dwell (>= 0, 0: no
 *   dwell alert), 0, 0; 112 + 32 z + 2 v .. = vertex v of zone z, a simple polygon (convex or not), as fp32 bits x, y; everything past
 *   a count is 0.  The caller validates it (yolov6/utils/zones.py::check_packed); the kernel clamps the three counts to their ranges.
 *   memo: int32 [n_streams, max_tracks + 2, 16], 16-byte aligned, lp_zone_state_bytes bytes, all zero = empty (the caller zeroes it
 *   once, zeroes a stream's part together with the tracker's, and all of it when the map changes).  Row t < max_tracks, one per slot:
 *   id + 1, last (the track's last matched frame when the anchor was taken), the anchor's x and y as fp32 bits, inside_mask |
 *   alerted_mask << 8, enter_frame[8], 0, 0, 0.  Row max_tracks: the +1 totals per line; row max_tracks + 1: the -1 totals (int32, wrap).
 * Arithmetic: a point or vertex is widened from fp32 to fp64; every later operation is one IEEE fp64 subtract or multiply, rounded on
 * its own, in the written order (no fused multiply-add, no division): cross(P, Q, R) = (Qx - Px) * (Ry - Py) - (Qy - Py) * (Rx - Px).
 * Every comparison is a plain float compare, false for NaN.  Anchor of a slot: ((x1 + x2) * 0.5f, (y1 + y2) * 0.5f) of the stored box in
 * fp32 (the tracker's cx, cy); an anchor with |x| <= FLT_MAX and |y| <= FLT_MAX is finite, any other crosses no line and is in no zone.
 * Crossing of line l by the move P0 -> P1: d0 = cross(A, B, P0), d1 = cross(A, B, P1); direction +1 iff d0 <= 0 and d1 > 0, -1 iff
 * d0 > 0 and d1 <= 0 (a point on the line is on the negative side: a stop on the line is counted once); and the move must pass between
 * the ends: e0 = cross(P0, P1, A), e1 = cross(P0, P1, B), (e0 <= 0 and e1 > 0) or (e0 > 0 and e1 <= 0).  Inside a zone: the crossing
 * number over the edges (Vi, Vj), j = (i + 1) % n: an edge toggles iff (yi > py) != (yj > py) and, with t = (xj - xi) * (py - yi) -
 * (px - xi) * (yj - yi), t > 0 if yj > yi, else t < 0.
 * Every stream s < n_streams is processed, whether or not the tracker call gave it a frame; every slot t < max_tracks, in order; now =
 * the stream's frame counter:
 *   1. a slot is eligible iff hits > 0 and hits >= min_hits;
 *   2. a non-empty memo line whose slot is not eligible or holds another id is gone: for every zone of its inside mask, ascending, an
 *      event of kind 5 (ended inside) with frame = memo.last, value = memo.last - enter_frame[z], the memo's anchor, key 0, hits 0; the
 *      line is zeroed;
 *   3. an eligible slot with an empty memo line starts a track: no crossing is tested; every zone it is inside emits kind 2 (enter) with
 *      enter_frame[z] = last;
 *   4. an eligible slot whose memo holds its id: the lines, ascending: a crossing of memo anchor -> current anchor emits kind 1 with
 *      value +1 / -1, and that total goes up by one; the zones, ascending: outside -> inside emits kind 2, sets enter_frame[z] = last and
 *      clears the zone's alerted bit; inside -> outside emits kind 3 (left) with value = last - enter_frame[z]; the memo takes the new
 *      anchor, last and inside mask;
 *   5. behind each zone's transition in 3 and 4: iff the track is inside z, min_dwell[z] > 0, the alerted bit is clear and now -
 *      enter_frame[z] >= min_dwell[z]: kind 4 (dwell) with value = now - enter_frame[z], and the bit is set (a missed but live track
 *      keeps dwelling);
 *   6. an event line, int32 [12]: kind, the line or zone index, id, slot, frame (last for kinds 1..4), value, the anchor's x and y as fp32
 *      bits, key_lo, key_hi (the eight voted ids of rule 8 of lp_track_update, packed as the memo of lp_watch_live packs them; 0 for
 *      kind 5), hits, 0;
 *   7. zone_ev [n_streams, max_events, 12]: a stream's events in the order produced (by slot; within a slot step 2, the lines, then the
 *      zones with each transition followed by its alert); zone_count [n_streams]: the number produced, not capped -- lines at or past
 *      max_events are not written, lines from the count to max_events are zero; zone_occ [n_streams, 8]: the eligible tracks inside each
 *      zone after the call; zone_totals [n_streams, 2, 16]: a copy of the two total rows.  All int32, 16-byte aligned; every word of the
 *      four is written by every call.  The int32 differences wrap.
 * One launch, one workgroup of 128 threads per stream, lane t = slot t: the stream's geometry is staged in LDS once; a lane reads its
 * slot's first 16 bytes, its box and its memo line; the votes are read only for a slot that emits an event of kind 1 to 4; the events are
 * counted per lane, numbered by a prefix sum over the workgroup and written by their lane; zone_occ and the totals are integer
 * reductions in LDS.
 * What it does not do: positions are those at the end of the tracker call (several frames of a stream in one call are tested on the
 * chord; a track born and ended inside one call is unseen); a track that touches a line and turns back yields +1 then -1; a track that
 * ends inside a zone is kind 5, not kind 3; everything stays in pixels (lp_speed_update has the calibrated plane); the anchor is the plate, not
 * the vehicle's footprint.
 * Every argument is checked before the launch (LP_ERR_ARG, nothing launched): n_streams < 1, max_tracks outside
 * 1..LP_TRACK_MAX_TRACKS, max_events < 0, the words of the state, of the map or of zone_ev at or above 2^31, ncls null or a width
 * outside 1..LP_TRACK_MAX_CLS, min_hits < 1, a null pointer (zone_ev only with max_events > 0), the state, the map, the memo or an
 * output not 16-byte aligned, and a written buffer (memo, the four outputs) that overlaps the state, the map or another one. */
#define LP_ZONE_MAX_LINES 16
#define LP_ZONE_MAX_ZONES 8
#define LP_ZONE_MAX_VERTS 16
#define LP_ZONE_MAP_WORDS 368   /* 16 + 4 * 16 + 4 * 8 + 2 * 16 * 8 */
size_t lp_zone_state_bytes(int n_streams, int max_tracks);             /* of the memo; 0: bad arguments */
int lp_zone_update(const void* track_state, int n_streams, int max_tracks, const int* ncls /* HOST [8] */,
                   const void* zone_map /* DEVICE, the packed geometry */, int min_hits, int32_t* memo,
                   int32_t* zone_ev, int32_t* zone_count, int max_events, int32_t* zone_occ, int32_t* zone_totals,
                   void* stream);

/* lp_speed_update: the speed of the LIVE plate tracks on a calibrated ground plane, with an alert over a limit.  lp_zone_update works in
 * pixels of the frame, where a pixel near the horizon is many metres; this maps the tracker's anchor through a per-stream homography to
 * millimetres on a plane and differences the positions over time.  Called behind lp_track_update (any of its forms; behind the other
 * add-ons if they run too) on the same stream; all pointers but ncls are DEVICE pointers; nothing is uploaded or read back, nothing is
 * allocated, capturable in a graph.  The tracker state is read, never written.  The reference has nothing here;
 * yolov6/utils/speed.py::SpeedNp restates the rules below on every int32 of the three outputs and of the memo.
 *   track_state: the state of lp_track_update (16-byte aligned) as its last call left it; ncls: HOST int [8], the tracker's.
 *   ground_map: int32 [n_streams, LP_SPEED_MAP_WORDS], 16-byte aligned: words 0..17 = H, a 3x3 fp64 homography, row-major h0..h8, as bit
 *   pairs (lo, hi), all finite, frame pixels -> metres on the plane the plates move in (calibrated at plate height); 18 = period_us
 *   (1..10^7), the nominal frame period; 19 = limit_mm_s (>= 0, 0: no alert); 20 = min_gap_us (>= 0); 21 = min_span_us (>= 1); 22 =
 *   enabled (0 / 1; a stream without a plane is all zero: "none" rows, no events); the rest 0.  The caller validates it
 *   (yolov6/utils/speed.py::check_packed).
 *   clock_us: NULL, or int64 [n_streams], 8-byte aligned, read in place: the time of every stream's newest frame in microseconds.
 *   memo: int32 [n_streams, max_tracks, LP_SPEED_MEMO_WORDS], 16-byte aligned, lp_speed_state_bytes bytes, all zero = empty (the caller
 *   zeroes it once, zeroes a stream's part together with the tracker's, and all of it when the map changes).  Word 0 = id + 1; 1 = last;
 *   2 = samples pushed (saturating); 3 = ring head (where the next sample goes); 4, 5 = t_first (lo, hi); 6, 7 = X_first, Y_first; 8..10 =
 *   the stored estimate speed (-1: none yet), vx, vy in mm/s; 11 = peak; 12 = over | alerted << 16 (over saturates at 65535); 13 =
 *   span_ms; 14, 15 = 0; 16 + 4 k .. = sample k of a ring of LP_SPEED_RING as t_lo, t_hi, X_mm, Y_mm.  The ring holds n = min(pushed, 8)
 *   samples, the newest at (head - 1) & 7, the oldest at 0 while pushed < 8, else at head.
 * World point of a slot: the anchor ((x1 + x2) * 0.5f, (y1 + y2) * 0.5f) of the stored box in fp32 (the tracker's cx, cy), widened to
 * fp64 as x, y; then one IEEE fp64 operation at a time, rounded on its own, in this order, no fused multiply-add: u = (h0 * x + h1 * y) +
 * h2, v = (h3 * x + h4 * y) + h5, w = (h6 * x + h7 * y) + h8, X = u / w, Y = v / w (correctly rounded divisions), PX = X * 1000.0, PY = Y *
 * 1000.0, X_mm = rint(PX), Y_mm = rint(PY) (ties to even).  Valid iff |ax| <= FLT_MAX and |ay| <= FLT_MAX, w > 0, |PX| <= 2^30 and |PY| <=
 * 2^30 (plain compares, false for NaN).  Everything behind it is integer.
 * Time of a sample: now = the stream's frame counter, last = the slot's last matched frame: t_us = base - int64(int32(now - last)) *
 * period_us, base = clock_us[s] if clock_us is given, else int64(now) * period_us.  The int32 and int64 differences wrap.
 * Every stream s < n_streams is processed, whether or not the tracker call gave it a frame; every slot t < max_tracks, in order:
 *   1. a slot is eligible iff its stream is enabled, hits > 0 and hits >= min_hits;
 *   2. a non-empty memo line whose slot is not eligible or holds another id is gone: if it pushed at least 2 samples, an event of kind 3
 *      (ended) with frame = memo.last, value = peak, aux = the chord speed from the first to the newest sample by the estimator of 5 (0 if
 *      their dt <= 0), the newest sample's position, key 0, hits 0; the line is zeroed;
 *   3. an eligible slot with an empty line starts: id + 1 and last are stored, the stored speed is -1; a valid point is pushed as the
 *      first sample, which is also `first`;
 *   4. an eligible slot holding its id, with slot.last != memo.last: memo.last = slot.last; if the point is valid and (no sample yet, or
 *      t - t_newest >= min_gap_us) it is pushed, overwriting the oldest once the ring holds 8.  A call that pushed is fresh for the slot;
 *   5. only when fresh and n >= 2: o = the oldest, e = the newest sample, dt = t_e - t_o; if dt >= min_span_us: dx, dy int64, d2 = dx * dx +
 *      dy * dy, s = floor(sqrt(d2)) exact, speed = min(s * 10^6 / dt, 2^31 - 1), vx = sign(dx) * min(|dx| * 10^6 / dt, 2^31 - 1), vy
 *      likewise, span_ms = min(dt / 1000, 2^31 - 1), peak = max(peak, speed) (integer divisions of non-negative numbers);
 *   6. only when 5 gave an estimate in this call and limit_mm_s > 0: speed > limit: over += 1, and with over >= confirm and the alerted bit
 *      clear an event of kind 1 (value = speed, aux = limit, frame = last, the voted read as key_lo, key_hi as lp_watch_live packs it,
 *      hits) and the bit is set; speed <= limit: over = 0.  One alert per track;
 *   7. speed_i [n_streams, max_tracks, 8]: (id, speed, vx, vy, X_mm, Y_mm of the newest sample (0, 0 without one), span_ms, n | fresh << 8
 *      | alerted << 9); a slot that is not eligible: (-1, 0, 0, 0, 0, 0, 0, 0);
 *   8. speed_ev [n_streams, max_events, 12]: kind, 0, id, slot, frame, value, X_mm, Y_mm, key_lo, key_hi, hits, aux, in slot order (a slot
 *      yields at most one event per call); speed_count [n_streams]: the number produced, not capped -- lines at or past max_events are
 *      not written, lines from the count to max_events are zero.  All int32, 16-byte aligned; every word of the three is written by every
 *      call.
 * One launch, one workgroup of 128 threads per stream, lane t = slot t: a lane reads its slot's first 16 bytes, its memo header and the
 * newest sample; only a slot with a new detection reads its box, only a push stores a sample and reads the oldest; the votes are read only
 * for a slot that alerts; the events are numbered by a prefix sum over the workgroup and written by their lane.
 * What it does not do: the estimator is the endpoint difference over the ring: no filtering, no acceleration, no lens-distortion model; a
 * plate sits off the calibrated plane by its mounting-height spread; positions are those at the end of the tracker call; now and the
 * clock must not run backwards (dt <= 0: no estimate); zones stay in pixels.
 * Every argument is checked before the launch (LP_ERR_ARG, nothing launched): n_streams < 1, max_tracks outside
 * 1..LP_TRACK_MAX_TRACKS, max_events < 0, the words of the state or of speed_ev at or above 2^31, ncls null or a width outside
 * 1..LP_TRACK_MAX_CLS, min_hits < 1, confirm outside 1..65535, a null pointer (speed_ev only with max_events > 0; clock_us may be null),
 * the state, the map, the memo or an output not 16-byte aligned, a clock not 8-byte aligned, and a written buffer (memo, the three
 * outputs) that overlaps the state, the map, the clock or another one. */
#define LP_SPEED_MAP_WORDS 32
#define LP_SPEED_MEMO_WORDS 48   /* 16 + 4 * LP_SPEED_RING */
#define LP_SPEED_RING 8
size_t lp_speed_state_bytes(int n_streams, int max_tracks);            /* of the memo; 0: bad arguments */
int lp_speed_update(const void* track_state, int n_streams, int max_tracks, const int* ncls /* HOST [8] */,
                    const void* ground_map /* DEVICE, the packed calibration */, const void* clock_us /* DEVICE int64 [n_streams], may be NULL */,
                    int min_hits, int confirm, void* memo, void* speed_i, void* speed_ev, void* speed_count, int max_events,
                    void* stream);

/* lp_tile_gate_luma_batch / lp_tile_gate_update: skip the unchanged tiles of fixed-camera frames in tiled detection.  On a fixed
 * camera nearly every tile of a frame shows the pixels of the frame before, and a tile that has not changed yields the same
 * detections again; these two calls find, per (stream, tile), whether the tile changed against the frame its cached detections were
 * computed on.  The caller runs the network on the flagged tiles only and keeps the rows of the others (runtime.TileGate).  The
 * reference has nothing here; yolov6/utils/tile_gate.py (luma_blocks_np, gate_update_np) restates the rules below on every integer.
 * All frame, grid, table and state pointers are DEVICE pointers; desc, stream_of and n_tiles are HOST arrays.  Nothing is uploaded
 * or read back, nothing is allocated, both calls can be captured in a graph.
 *   Luma: a BGR frame gives L = (29 B + 150 G + 77 R + 128) >> 8; an NV12 frame gives L = Y (the chroma plane is not read: a change
 *   of chroma alone is invisible there).
 *   Block sums (lp_tile_gate_luma_batch): blocks[by][bx] = the sum of L over the pixels y in [4 by, min(4 by + 4, h0)), x in
 *   [4 bx, min(4 bx + 4, w0)): uint16 [ceil(h0 / 4)][ceil(w0 / 4)], at most 4080.  Every frame byte is read once, none past the last
 *   pixel of a row; frames and grids of one call may have any sizes.
 *   Tile region: tile (y0, x0, th, tw) owns the blocks by in [y0 >> 2, (y0 + th - 1) >> 2], bx likewise (every block it overlaps).
 *   Cells: inside a tile's block range, 4 x 4 blocks anchored at the tile's first block, smaller at the end of a range;
 *   npix(cell) = the frame pixels of its blocks, A(cell) = sum |blocks - ref| over its blocks (int32); the cell is changed iff
 *   16 A > thres16 * npix (thres16 = the threshold in sixteenths of a luma level per pixel, 0..4080).
 *   State: tiles int32 [n_streams][max_tiles][LP_TILE_GATE_TILE_WORDS] = (y0, x0, th, tw, ref_off, 0, 0, 0) per tile of a stream's plan,
 *   written once by the caller; ref uint16 [ref_elems], tile (s, t) owning the nby * nbx elements from its ref_off (the regions of
 *   different tiles must not overlap); age int32 [n_streams][max_tiles], -1 = never detected (the caller fills it with -1; writing -1
 *   resets a tile).  n_tiles[s] <= max_tiles <= LP_MERGE_MAX_TILES: the tiles of stream s.
 *   lp_tile_gate_update, per frame b of stream s = stream_of[b] >= 0 (a stream at most once per call; desc[b].blocks, h0, w0 are read,
 *   the planes are not) and tile t < n_tiles[s]: ncell = the number of changed cells, 0 if age < 0 (ref is then not read);
 *   flag = age < 0 || ncell >= min_cells || (refresh > 0 && age + 1 >= refresh).  Flagged: ref <- blocks over the tile's region and
 *   age <- (age < 0 && refresh > 0) ? t % refresh : 0 (the periodic refreshes of a plan are staggered over the period); not flagged:
 *   ref untouched, age += 1.  So ref is always the frame the tile was last flagged on: slow drift accumulates until it crosses
 *   the threshold.  flag uint8 / ncell int32 [n_frames][max_tiles]: every entry is written; t >= n_tiles[s] gives (0, 0); a frame with
 *   stream_of -1 is not gated: (1, 0) for every t, no state read or written.  A table entry that is not inside its frame or whose
 *   region leaves ref gives (1, -1) and touches no state.
 * One luma kernel over two pixel sources (a lane sums 16 pixels x 4 rows with 16-byte loads), one update workgroup per (frame, tile).
 * Every argument is checked before the first launch (LP_ERR_ARG names the frame; nothing is launched): null desc, planes, grids or
 * state pointers, format, h0 or w0 < 1, pitch0 below the row's bytes, misaligned grids or state, max_tiles outside
 * 1..LP_MERGE_MAX_TILES, n_tiles[s] outside 0..max_tiles, stream_of[b] outside -1..n_streams-1, a stream twice in one call, thres16,
 * min_cells < 1, refresh < 0, ref_elems outside 1..2^31-1, and an output (a grid; ref, age, flag, ncell) overlapping an input or
 * another output. */
#define LP_MERGE_MAX_TILES 64   /* tiles per frame: the limit of lp_merge_tiles, which takes what the gate passes on */
#define LP_TILE_GATE_TILE_WORDS 8
typedef struct lp_tile_gate_desc {
    const unsigned char* p0;    /* BGR: the frame, uint8 [h0][w0][3]; NV12: the luma plane.  Any alignment; read only */
    int pitch0;                 /* bytes between rows: >= 3 * w0 (BGR), >= w0 (NV12) */
    int h0, w0;                 /* >= 1 (the luma plane of an NV12 frame alone is read, so odd sizes are fine here) */
    int format;                 /* 0 BGR, 1 NV12 */
    unsigned short* blocks;     /* the frame's block grid, uint16 [ceil(h0 / 4)][ceil(w0 / 4)], 2-byte aligned */
} lp_tile_gate_desc;
int lp_tile_gate_luma_batch(const lp_tile_gate_desc* desc, int n_frames, void* stream);
int lp_tile_gate_update(const lp_tile_gate_desc* desc, int n_frames, const int* stream_of /* HOST [n_frames] */, int n_streams,
                        const int32_t* tiles, const int* n_tiles /* HOST [n_streams] */, int max_tiles,
                        unsigned short* ref, long long ref_elems, int32_t* age, int thres16, int min_cells, int refresh,
                        unsigned char* flag, int32_t* ncell, void* stream);
/* lp_tile_gate_update_gain: lp_tile_gate_update for frames whose exposure or daylight drifts (gate_update_gain_np in
 * yolov6/utils/tile_gate.py, on every integer).  A common factor on every pixel of a tile changes every cell under the rule above;
 * here the reference is scaled by one gain per tile before the cells are compared.  Q12: 4096 is a gain of 1.
 *   Gain of a cell: R_c / C_c = the sum of ref / of blocks over the cell's blocks (<= 65280); R_c == 0: no gain; otherwise
 *   g_c = min((C_c * 4096 + (R_c >> 1)) / R_c, 65535) in unsigned 32-bit arithmetic.
 *   Gain of the tile: m = the cells with a gain; m == 0: G_raw = 4096; otherwise G_raw = the lower median of the g_c, the value of
 *   rank (m - 1) / 2 of the sorted gains.  out_of_range = G_raw < gain_lo || G_raw > gain_hi; G = G_raw clamped to the range.
 *   Changed cell: A_g = sum |blocks * 4096 - ref * G| over its blocks (int32: a term <= 4080 * 16384); changed iff
 *   A_g > thres16 * npix * 256.  With G == 4096 that is lp_tile_gate_update's test.
 *   flag = age < 0 || out_of_range || ncell >= min_cells || (refresh > 0 && age + 1 >= refresh); ref and age move as above.
 *   gain int32 [n_frames][max_tiles] = G_raw.  (flag, ncell, gain) = (1, 0, 0) for a never-detected tile (ref is not read) and for
 *   every t of a frame with stream_of -1, (0, 0, 0) for t >= n_tiles[s], (1, -1, 0) for a bad table entry, which touches no state.
 * The same workgroup per (frame, tile); the median is selected by two radix passes over 256-bin LDS histograms of integer counts.
 * The checks are lp_tile_gate_update's, and: gain non-null, 4-byte aligned and part of the overlap check;
 * 1 <= gain_lo <= 4096 <= gain_hi <= 16384.  Capturable, allocates nothing, no host read. */
int lp_tile_gate_update_gain(const lp_tile_gate_desc* desc, int n_frames, const int* stream_of /* HOST [n_frames] */, int n_streams,
                             const int32_t* tiles, const int* n_tiles /* HOST [n_streams] */, int max_tiles,
                             unsigned short* ref, long long ref_elems, int32_t* age, int thres16, int min_cells, int refresh,
                             int gain_lo, int gain_hi, unsigned char* flag, int32_t* ncell,
                             int32_t* gain /* [n_frames][max_tiles] */, void* stream);

/* lp_eval_counts: the matching loops of Evaler.eval (yolov6/core/evaler.py:153-243, box_iou general.py:93-115) for a
 * batch of images, one workgroup per image.
 *   det [B,max_det,28] fp32 + det_count [B]: detections as lp_nms returns them (xyxy, 8 corner coords, 8 confs, 8 ids)
 *   tgt [B,max_t,20] fp32 + tgt_count [B]:   labels (8 ids, xyxy, 8 corner coords), evaler.py:121-128 layout minus column 0
 *   counts: device int64 [LP_EVAL_NCOUNTS], ACCUMULATED into (zero it before the first batch):
 *           [LP_EVAL_TRUE] labels, [LP_EVAL_PRED] labels matched with IoU >= 0.7, then four groups of ten 0.05-wide IoU
 *           bins from 0.5: matched labels, corners right, classes right, both right; [LP_EVAL_UNBINNED] matched labels
 *           whose IoU fits no bin (IoU >= 1.0f) -- the reference re-uses a stale bin index for those, they are skipped here.
 * The ratios (evaler.py:245-283) are host arithmetic on these integers. */
enum { LP_EVAL_TRUE = 0, LP_EVAL_PRED = 1, LP_EVAL_PRED_BINS = 2, LP_EVAL_COR = 12, LP_EVAL_CLS = 22, LP_EVAL_RIGHT = 32,
       LP_EVAL_UNBINNED = 42, LP_EVAL_NCOUNTS = 43 };
int lp_eval_counts(const float* det, const int32_t* det_count, int max_det, const float* tgt, const int32_t* tgt_count,
                   int max_t, int B, long long* counts, void* stream);

/* Verification hook of the detections-only head (lp_engine_forward_det): it takes the largest sigmoid of a head to be the sigmoid of
 * the head's largest logit, which holds iff the kernels' sigmoid (hardware exp2 and reciprocal) is monotone non-decreasing.  Checks
 * every pair of neighbouring fp32 values (2^32 - 1 pairs, NaNs skipped) on the device and leaves the number of violations in
 * *dev_violations (device memory, 8 bytes).  Expected: 0 (tests/test_hip_kernels.py). */
int lp_check_sigmoid_monotone(unsigned long long* dev_violations, void* stream);

/* Verification hook of the greedy NMS step: the kernels decide torchvision's `inter / union > iou_threshold` with two products and
 * compares where the outcome is certain and with the fp32 division only inside a 2^-19-wide band around the threshold (lp_nms.hip,
 * iou_gt).  Evaluates both forms on n box pairs (device fp32 [n][8]: box i xyxy, box j xyxy); dev_out[k] bit 0 = the product form,
 * bit 1 = the plain division.  Expected: both bits equal for every pair, and equal to the fp32 restatement (tests/test_hip_kernels.py). */
int lp_check_iou_predicate(const float* dev_pairs, long long n, double iou_thres, unsigned char* dev_out, void* stream);

/* Test hook of the LDS-ring kernels: fills all 160 KiB of LDS of every CU with 0xFFFF halves (NaN in fp16 / bf16).  LDS keeps its
 * contents between kernels, so a fragment read that runs ahead of its LDS-DMA would otherwise find the (identical) bytes of the
 * previous launch and go unnoticed; after this call it poisons the output (tests/test_hip_kernels.py). */
int lp_debug_poison_lds(void* stream);

/* Host-side planning of the frame-reading stem kernels (no device needed; used by the CPU tests): the `choice`-th best output tile
 * TH x TW for an Ho x Wo output map of stem_planar_kernel (fused == 0: TW % 4 == 0, TH * TW <= 512, planar halo within its 20 KiB LDS
 * slot) or of stem2_fused_kernel (fused != 0: TW even, TH * TW <= 128, frame window <= 21 KiB, stem tile pitch *hpitch >= 2 TW + 1 with
 * (2 TH + 1) * pitch <= 640 positions).  LP_ERR_UNSUPPORTED: no such tile. */
int lp_plan_stem_tile(int fused, int Ho, int Wo, int choice, int* TH, int* TW, int* hpitch);
/* The same for the block-tiled 3x3 kernels: the `choice`-th best output tile of LP_VARIANT_PIPE16_V0 / _V1 (stride 1) or LP_VARIANT_PIPE16_S2A / _S2B
 * (stride 2) for B images of an Ho x Wo OUTPUT map and nct cout tiles -- TH * TW pixels within the variant's pixel blocks, the halo
 * ((TH - 1) s + 3) x ((TW - 1) s + 3) within its LDS slot, fewest rounds of the persistent grid first; *hpitch = the halo row pitch.
 * LP_ERR_UNSUPPORTED: another variant. */
int lp_plan_block_tile(int variant, int Ho, int Wo, int B, int nct, int choice, int* TH, int* TW, int* hpitch);

#ifdef __cplusplus
}
#endif
#endif /* LP_HIP_H */
