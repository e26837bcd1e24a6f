"""Host side of the HIP engine: turns a ``yolov6.models.yolo.Model`` into the op
graph of libyololp_hip.so (folded weights, NHWC tensors, concat-free sources) and
runs forward / NMS through the C ABI on torch-owned device memory and torch's
current stream.

Replaces, on a GPU, ``Model.forward`` (reference yolov6/models/yolo.py:32-40)
and ``non_max_suppression`` (yolov6/utils/nms.py:31-130).  Weight preparation
follows the reference's order ``float -> fuse_model -> switch_to_deploy``
(inferer.py:25-68): modules that are still un-fused are folded on the fly with
the same formulas, without touching the caller's model.
"""
import copy
import ctypes
import os
import weakref

import numpy as np
import torch
import torch.nn as nn

from yolov6.core.frames import letterbox_placement
from yolov6.core.tiles import hw_pair, plan_frames, tiles_per_frame
from yolov6.hip import abi
from yolov6.layers import common as L
from yolov6.utils.lookback import LookbackHost
from yolov6.utils.nv12 import Nv12Frame, is_nv12_list

DET_CROSSOVER = 0.5   # candidate density (candidates / anchors) above which forward + lp_nms beats the detections-only forward
_DT = {torch.float16: abi.LP_F16, torch.bfloat16: abi.LP_BF16, torch.float32: abi.LP_F32}
_TORCH_DT = {v: k for k, v in _DT.items()}
CLS_HEADS = ('pro', 'alp', 'ad0', 'ad1', 'ad2', 'ad3', 'ad4', 'ad5')
OP_KINDS = ('input', 'conv', 'deconv', 'pool', 'head_cls', 'head_box', 'stem')   # lp_engine_op_info's kind codes


def _dptr(t):
    """Device pointer of a tensor for the C ABI (None stays a null pointer)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _aligned(buf):
    """256-byte aligned base address inside ``buf``: arenas and workspaces are allocated 256 bytes larger than needed."""
    return (buf.data_ptr() + 255) // 256 * 256


def _stream_ptr(device):
    """torch's current stream on ``device`` as the hipStream_t every launch of the library goes to."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _act_of(module):
    if isinstance(module, nn.ReLU):
        return abi.LP_ACT_RELU
    if isinstance(module, (nn.SiLU, L.SiLU)):
        return abi.LP_ACT_SILU
    if isinstance(module, nn.Identity):
        return abi.LP_ACT_NONE
    raise NotImplementedError('activation %s has no HIP epilogue' % type(module).__name__)


def _f32(t):
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t, dtype=np.float32)
    return np.ascontiguousarray(t.detach().float().cpu().numpy())


def _fold_conv_bn(conv, bn):
    """fp32 (weight OIHW, bias) of conv followed by an eval-mode BN, the fuse_conv_and_bn formula
    (torch_utils.py:50-82) evaluated on fp32 copies: the caller's modules are not modified."""
    w = conv.weight.detach().float()
    b = conv.bias.detach().float() if conv.bias is not None else torch.zeros(w.shape[0], device=w.device)
    if bn is not None:
        g, beta = bn.weight.detach().float(), bn.bias.detach().float()
        mu, var = bn.running_mean.float(), bn.running_var.float()
        scale = torch.diag(g.div(torch.sqrt(bn.eps + var)))
        w = torch.mm(scale, w.reshape(w.shape[0], -1)).view(w.shape)
        b = torch.mm(scale, b.reshape(-1, 1)).reshape(-1) + (beta - g.mul(mu).div(torch.sqrt(var + bn.eps)))
    return w, b


def _folded(m):
    """Conv / SimConv / Conv_C3, fused or not."""
    return _fold_conv_bn(m.conv, getattr(m, 'bn', None))


class Engine:
    """One frozen graph + its device buffers for one (model, activation dtype, device)."""

    def __init__(self, dtype, device, mfma16=None):
        """mfma16: None = the library's default (on, unless LP_NO_MFMA16 is set); False = every layer on the 32x32x16 MFMA family;
        True = eligible 3x3 stride-1 layers on v_mfma_f32_16x16x32 (lp_engine_set_mfma16: another fp32 summation order)."""
        self.lib = abi.load()
        self.device = torch.device(device)
        self.dtype = dtype
        self.lp_dtype = _DT[dtype]
        h = ctypes.c_void_p()
        abi.check(self.lib.lp_engine_create(ctypes.byref(h), self.lp_dtype), 'lp_engine_create')
        self.h = h
        if mfma16 is not None:
            abi.check(self.lib.lp_engine_set_mfma16(self.h, 1 if mfma16 else 0), 'lp_engine_set_mfma16')
        self._keep = []            # numpy arrays must outlive the add_* calls
        self.bound = None          # (B, H, W)
        self.arena = None
        self.weights = None
        self.neck_ids = []
        self.tuned = set()         # (B, H, W) shapes whose per-layer kernel variants were autotuned
        self.autotune = os.environ.get('LP_AUTOTUNE', '1') != '0'
        self.max_tuned_shapes = 32   # a directory of oddly sized frames must not pay the tuner for every new shape
        self.graph = False         # hipGraph replay of the forward (set_graph); pred is then a persistent buffer
        self.single_lane = True    # set_single_lane (the library's default; LP_LANES=1: execution lanes on)
        self._last_stream = None   # stream of the last forward: a forward on ANOTHER stream waits for it (one arena)
        self._graph_pred = None
        self._graph_x = None       # graph mode: persistent staging copy of the input (fixed address)
        self.det_crossover = DET_CROSSOVER   # `detect`: candidate density above which forward + lp_nms is the faster form
        self.pass_rate = None      # candidates / anchors of the last batch that went through `detect` (None: not known yet)
        self._pass_probe = None    # (pinned int32 [B], event, N): asynchronous read-back of the candidate counts
        self.det_routes = {'det': 0, 'pred': 0}   # how often `detect` took each form (introspection / tests)
        self.input_id = self.tensor(3, 0)
        abi.check(self.lib.lp_engine_add_input(self.h, self.input_id), 'lp_engine_add_input')
        if os.environ.get('LP_LANES'):
            self.set_single_lane(False)

    @classmethod
    def from_model(cls, model, dtype, device):
        eng = cls(dtype, device)
        with torch.no_grad():
            eng._build(model)
        return eng.finish(model.detect.nl)

    def finish(self, n_levels=3):
        """Freeze the graph, pack the weights and (on a GPU) upload them."""
        abi.check(self.lib.lp_engine_finalize(self.h, n_levels), 'lp_engine_finalize')
        self._keep = []
        self.weight_bytes = self.lib.lp_engine_weight_bytes(self.h)
        if self.device.type == 'cuda':
            with torch.cuda.device(self.device):
                self.weights = torch.empty(self.weight_bytes + 256, dtype=torch.uint8, device=self.device)
                abi.check(self.lib.lp_engine_upload(self.h, _aligned(self.weights), _stream_ptr(self.device)),
                          'lp_engine_upload')
        return self

    def __reduce__(self):
        raise TypeError('an lp Engine owns device memory and a native handle and cannot be pickled or deep-copied; '
                        'it is rebuilt on demand (runtime.engine_for)')

    def __del__(self):
        try:
            if getattr(self, 'h', None):
                self.lib.lp_engine_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # -- helpers -------------------------------------------------------------
    def _ptr(self, arr):
        self._keep.append(arr)
        return arr.ctypes.data_as(ctypes.c_void_p)

    def lane(self, k):
        """Ops added from now on run on execution lane ``k`` (0 = the caller's stream, 1 / 2 = side streams)."""
        abi.check(self.lib.lp_engine_set_lane(self.h, int(k)), 'lp_engine_set_lane')

    def tensor(self, channels, sl):
        return abi.check(self.lib.lp_engine_tensor(self.h, int(channels), int(sl)), 'lp_engine_tensor')

    def conv(self, srcs, weight, bias, k, s, act, sl, res=None, alpha=0.0):
        """act(conv(cat(srcs))+b) [+ alpha*res] -> new tensor id; ``sl`` is the sources' log2 stride."""
        w, b = _f32(weight), _f32(bias)
        dst = self.tensor(w.shape[0], sl + (1 if s == 2 else 0))
        self._add_conv(srcs, w, b, k, s, act, dst, res=res, alpha=alpha)
        return dst

    def _add_conv(self, srcs, w, b, k, s, act, dst, dst2=-1, res=None, alpha=0.0):
        """One conv op (lp_conv_desc) on fp32 numpy weights: ``dst2`` >= 0 makes it a two-destination launch."""
        d = abi.ConvDesc()
        d.n_src = len(srcs)
        for i in range(abi.LP_MAX_SRC):
            d.src[i] = srcs[i] if i < len(srcs) else -1
        d.dst, d.ksize, d.stride, d.act = dst, k, s, act
        d.res = -1 if res is None else res
        d.res_alpha = float(alpha)
        d.weight, d.bias = self._ptr(w), self._ptr(b)
        d.dst2 = dst2
        abi.check(self.lib.lp_engine_add_conv(self.h, ctypes.byref(d)), 'lp_engine_add_conv')

    def conv_pair(self, srcs, wb1, wb2, k, s, act, sl):
        """Two sibling layers on the same input (same kernel size, stride, activation) as ONE launch with two destination
        tensors (lp_conv_desc.dst2): their weight rows stacked.  The sums of every output channel are those of the two
        separate layers (a cout tile never mixes rows), so the results are the same bits.  Returns (dst1, dst2)."""
        (w1, b1), (w2, b2) = [(_f32(w), _f32(b)) for w, b in (wb1, wb2)]
        if w1.shape[0] % 8 != 0:                           # lp_conv_desc.dst2 wants the first layer's channels a multiple of 8
            return (self.conv(srcs, w1, b1, k, s, act, sl), self.conv(srcs, w2, b2, k, s, act, sl))
        w, b = np.ascontiguousarray(np.concatenate([w1, w2], 0)), np.ascontiguousarray(np.concatenate([b1, b2], 0))
        sl_out = sl + (1 if s == 2 else 0)
        dst1, dst2 = self.tensor(w1.shape[0], sl_out), self.tensor(w2.shape[0], sl_out)
        self._add_conv(srcs, w, b, k, s, act, dst1, dst2)
        return dst1, dst2

    def cba_pair(self, m1, m2, srcs, sl):
        """Two Conv / SimConv / Conv_C3 modules reading the same input: one launch when their shapes allow it."""
        c1, c2 = m1.conv, m2.conv
        same = (c1.kernel_size == c2.kernel_size and c1.stride == c2.stride and _act_of(m1.act) == _act_of(m2.act)
                and c1.in_channels == c2.in_channels)
        if not same:
            return self.cba(m1, srcs, sl), self.cba(m2, srcs, sl)
        return self.conv_pair(srcs, _folded(m1), _folded(m2), c1.kernel_size[0], c1.stride[0], _act_of(m1.act), sl)

    # -- module -> ops ---------------------------------------------------------
    def cba(self, m, srcs, sl):
        """Conv / SimConv / Conv_C3 (common.py:21-66, 466-476)."""
        w, b = _folded(m)
        k, s = m.conv.kernel_size[0], m.conv.stride[0]
        return self.conv(srcs, w, b, k, s, _act_of(m.act), sl)

    def basic(self, m, srcs, sl, res=None, alpha=0.0):
        """A 'basic block' of the rep-style stages -> one conv op."""
        if isinstance(m, L.RepVGGBlock):
            if hasattr(m, 'rbr_reparam'):
                w, b, s = m.rbr_reparam.weight, m.rbr_reparam.bias, m.rbr_reparam.stride[0]
            else:
                mf = m if next(m.parameters()).dtype == torch.float32 else copy.deepcopy(m).float()
                w, b = mf.get_equivalent_kernel_bias()
                s = m.rbr_dense.conv.stride[0]
            return self.conv(srcs, w, b, 3, s, abi.LP_ACT_RELU, sl, res, alpha)
        if isinstance(m, (L.ConvWrapper, L.SimConvWrapper)):
            w, b = _folded(m.block)
            c = m.block.conv
            return self.conv(srcs, w, b, c.kernel_size[0], c.stride[0], _act_of(m.block.act), sl, res, alpha)
        if isinstance(m, L.RealVGGBlock):
            w, b = _fold_conv_bn(m.conv, m.bn)
            return self.conv(srcs, w, b, 3, m.conv.stride[0], abi.LP_ACT_RELU, sl, res, alpha)
        raise NotImplementedError('%s has no HIP lowering' % type(m).__name__)

    def stage_block(self, m, srcs, sl):
        """One element of a RepBlock: a basic block or a BottleRep (common.py:437-455)."""
        if isinstance(m, L.BottleRep):
            assert len(srcs) == 1 or not m.shortcut
            y = self.basic(m.conv1, srcs, sl)
            if m.shortcut:
                alpha = float(m.alpha) if not torch.is_tensor(m.alpha) else float(m.alpha.detach().float().item())
                return self.basic(m.conv2, [y], sl, res=srcs[0], alpha=alpha)
            return self.basic(m.conv2, [y], sl)
        return self.basic(m, srcs, sl)

    def rep_block(self, m, srcs, sl):
        """RepBlock (common.py:416-434)."""
        x = self.stage_block(m.conv1, srcs, sl)
        if m.block is not None:
            for blk in m.block:
                x = self.stage_block(blk, [x], sl)
        return x

    def bepc3(self, m, srcs, sl):
        """BepC3 (common.py:479-501): cv3 reads [m(cv1 x), cv2 x] as two sources."""
        if m.concat is True:                              # cv1 and the shortcut cv2 read the same input: one launch
            c1, c2 = self.cba_pair(m.cv1, m.cv2, srcs, sl)
            return self.cba(m.cv3, [self.rep_block(m.m, [c1], sl), c2], sl)
        a = self.rep_block(m.m, [self.cba(m.cv1, srcs, sl)], sl)
        return self.cba(m.cv3, [a], sl)

    def stage(self, m, srcs, sl):
        if isinstance(m, L.RepBlock):
            return self.rep_block(m, srcs, sl)
        if isinstance(m, L.BepC3):
            return self.bepc3(m, srcs, sl)
        raise NotImplementedError('%s has no HIP lowering' % type(m).__name__)

    def pools(self, x, sl, c):
        ids = [self.tensor(c, sl) for _ in range(3)]
        abi.check(self.lib.lp_engine_add_pool5_chain(self.h, x, *ids), 'lp_engine_add_pool5_chain')
        return ids

    def merge_layer(self, m, x, sl):
        """SimCSPSPPF / CSPSPPF (common.py:124-172) or SimSPPF / SPPF (:88-121); concats are multi-source reads."""
        if isinstance(m, L._CSPSPPFBase):
            c1, y0 = self.cba_pair(m.cv1, m.cv2, [x], sl)         # the trunk's first layer and the CSP shortcut read the same input
            x1 = self.cba(m.cv4, [self.cba(m.cv3, [c1], sl)], sl)
            y3 = self.cba(m.cv6, [self.cba(m.cv5, [x1] + self.pools(x1, sl, m.cv4.conv.out_channels), sl)], sl)
            return self.cba(m.cv7, [y0, y3], sl)
        if isinstance(m, L._SPPFBase):
            x1 = self.cba(m.cv1, [x], sl)
            return self.cba(m.cv2, [x1] + self.pools(x1, sl, m.cv1.conv.out_channels), sl)
        raise NotImplementedError('%s has no HIP lowering' % type(m).__name__)

    def bifusion(self, m, x0, sl0, x1, x2):
        """BiFusion (common.py:504-527): x0 at stride sl0 is upsampled 2x; x1 is at sl0-1; x2 at sl0-2."""
        t = m.upsample.upsample_transpose
        up = self.tensor(t.out_channels, sl0 - 1)
        abi.check(self.lib.lp_engine_add_deconv2x2(self.h, x0, up, self._ptr(_f32(t.weight)), self._ptr(_f32(t.bias))),
                  'lp_engine_add_deconv2x2')
        self.lane(1)                                      # the three inputs of cv3 are independent branches
        a = self.cba(m.cv1, [x1], sl0 - 1)
        self.lane(2)
        d = self.cba(m.downsample, [self.cba(m.cv2, [x2], sl0 - 2)], sl0 - 2)
        self.lane(0)
        return self.cba(m.cv3, [up, a, d], sl0 - 1)

    def upsample(self, m, x, sl):
        """Transpose (common.py:174-187): 2x2 stride-2 transposed conv of a map at stride level ``sl``."""
        t = m.upsample_transpose
        up = self.tensor(t.out_channels, sl - 1)
        abi.check(self.lib.lp_engine_add_deconv2x2(self.h, x, up, self._ptr(_f32(t.weight)), self._ptr(_f32(t.bias))),
                  'lp_engine_add_deconv2x2')
        return up

    def _build(self, model):
        bb, nk, det = model.backbone, model.neck, model.detect
        p6 = hasattr(bb, 'ERBlock_6')
        last = 6 if p6 else 5
        x = self.basic(bb.stem, [self.input_id], 0)
        feats = []
        for i in range(2, last + 1):                              # ERBlock_i takes stride 2^(i-1) to 2^i
            st = getattr(bb, 'ERBlock_%d' % i)
            x = self.basic(st[0], [x], i - 1)
            x = self.stage(st[1], [x], i)
            if len(st) > 2:
                x = self.merge_layer(st[2], x, i)
            feats.append(x)
        self.backbone_ops = self.lib.lp_engine_num_ops(self.h)     # ops [0, backbone_ops) are the backbone (bench.py: roofline.backbone_frac)
        # feats[k] is at stride level k + 2; the backbones return P2 only with fuse_P2 (CSPBepBackbone_P6: always)
        bifusion = hasattr(nk, 'Bifusion0')
        has_p2 = bool(getattr(bb, 'fuse_P2', False)) or type(bb).__name__ == 'CSPBepBackbone_P6'
        if bifusion and not has_p2:
            raise NotImplementedError('the BiFusion necks need the P2 output of the backbone (fuse_P2=True)')
        if not bifusion and has_p2:
            raise ValueError('the plain PAN necks take (P3, P4, P5[, P6]): build the backbone with fuse_P2=False')
        nlev = 4 if p6 else 3
        if det.nl != nlev:
            raise ValueError('head with %d levels on a neck with %d outputs' % (det.nl, nlev))
        names_p = ['Rep_p5', 'Rep_p4', 'Rep_p3'] if p6 else ['Rep_p4', 'Rep_p3']
        names_n = ['Rep_n4', 'Rep_n5', 'Rep_n6'] if p6 else ['Rep_n3', 'Rep_n4']
        downs = ['downsample2', 'downsample1', 'downsample0'] if p6 else ['downsample2', 'downsample1']
        x, sl = feats[-1], last                                    # top-down (reppan.py forward passes)
        fpn = []
        for k in range(nlev - 1):
            f = self.cba(getattr(nk, 'reduce_layer%d' % k), [x], sl)
            fpn.append(f)
            if bifusion:
                t = [self.bifusion(getattr(nk, 'Bifusion%d' % k), f, sl, feats[-2 - k], feats[-3 - k])]
            else:                                                  # torch.cat([upsample(f), x_below]) read as two sources
                t = [self.upsample(getattr(nk, 'upsample%d' % k), f, sl), feats[-2 - k]]
            sl -= 1
            x = self.stage(getattr(nk, names_p[k]), t, sl)
        self.neck_ids = [x]
        for k in range(nlev - 1):                                  # bottom-up
            d = self.cba(getattr(nk, downs[k]), [x], sl)
            sl += 1
            x = self.stage(getattr(nk, names_n[k]), [d, fpn[-1 - k]], sl)
            self.neck_ids.append(x)
        # The heads run behind the neck, level i's two towers on lanes i % 3 and (i + 1) % 3.  (Issuing each level's head right
        # behind the neck layer that feeds it, on lanes of its own, was measured: equal with one batch in flight, slower with six --
        # the neck's persistent 3x3 kernels hold every CU's LDS, so the head kernels interleave with them instead of filling gaps;
        # DESIGN 6.3.)
        for i, f in enumerate(self.neck_ids):
            self._head(det, i, f, (i % 3, (i + 1) % 3))
        self.lane(0)

    def _head(self, det, i, f, lanes):
        """Detect's level ``i`` on the neck output ``f`` (effidehead.py:228-245): stem + class tower + the eight class predictors
        on lane ``lanes[0]``, box tower + box / corner predictors on ``lanes[1]``."""
        sl = 3 + i
        self.lane(lanes[0])
        s = self.cba(det.stems[i], [f], sl)
        c, r = self.cba_pair(det.cls_convs[i], det.reg_convs[i], [s], sl)      # the two towers read the stem's output: one launch
        preds = [getattr(det, '%s_preds' % h)[i] for h in CLS_HEADS]
        wc = np.concatenate([_f32(p.weight).reshape(p.out_channels, -1) for p in preds], 0)
        bc = np.concatenate([_f32(p.bias) for p in preds], 0)
        abi.check(self.lib.lp_engine_add_head_cls(self.h, c, i, wc.shape[0], self._ptr(wc), self._ptr(bc)),
                  'lp_engine_add_head_cls')
        self.lane(lanes[1])
        rp, cp = det.reg_preds[i], det.cor_preds[i]
        bins = det.reg_max + 1 if det.use_dfl else 1
        if rp.out_channels != 4 * bins:
            raise NotImplementedError('reg_preds width %d does not match use_dfl/reg_max' % rp.out_channels)
        wb = np.concatenate([_f32(rp.weight).reshape(rp.out_channels, -1), _f32(cp.weight).reshape(8, -1)], 0)
        bbias = np.concatenate([_f32(rp.bias), _f32(cp.bias)], 0)
        proj = self._ptr(_f32(det.proj_conv.weight).reshape(-1)) if bins > 1 else None
        abi.check(self.lib.lp_engine_add_head_box(self.h, r, i, bins, self._ptr(wb), self._ptr(bbias), proj),
                  'lp_engine_add_head_box')
        self.lane(0)

    # -- execution ---------------------------------------------------------------
    def bind(self, B, H, W):
        if self.bound == (B, H, W):
            return
        if H % 32 or W % 32:
            raise ValueError('input height/width must be multiples of 32, got %dx%d' % (H, W))
        need = self.lib.lp_engine_arena_bytes(self.h, B, H, W)
        if need == 0:
            raise ValueError('bad input shape %s: H and W must be positive multiples of the coarsest stride of the model '
                             '(32; 64 with a P6 level), and small enough for the SPPF pool chain, which keeps a whole stride-32 '
                             'map in LDS (up to ~2048x2048 px in f16 / bf16, ~1440x1440 in f32)' % ((B, H, W),))
        if self.arena is None or self.arena.numel() < need + 256:
            self.arena = None
            self.arena = torch.zeros(need + 256, dtype=torch.uint8, device=self.device)
        abi.check(self.lib.lp_engine_bind(self.h, _aligned(self.arena), need, B, H, W), 'lp_engine_bind')
        self.bound = (B, H, W)
        self.n_anchors = self.lib.lp_engine_num_anchors(self.h)

    def set_graph(self, enable=True):
        """Replay the forward as one hipGraph (launch-bound shapes, e.g. the per-image loop of Inferer).  The prediction
        tensor returned by ``forward`` is then a persistent buffer that the next forward overwrites."""
        self.graph = bool(enable)
        abi.check(self.lib.lp_engine_set_graph(self.h, 1 if enable else 0), 'lp_engine_set_graph')

    def _stream_enter(self):
        """The engine has ONE activation arena: a forward issued on another stream than the previous one (the model's
        one-at-a-time callers and an InflightForward slot share engine 0) first waits for what that stream holds.  (No event
        per forward: an event record is a barrier packet with a system-scope fence, ~10 us at the start of the next forward.)"""
        cur = torch.cuda.current_stream(self.device)
        if self._last_stream is not None and self._last_stream.cuda_stream != cur.cuda_stream:
            cur.wait_stream(self._last_stream)
        return cur

    def _stream_leave(self, cur):
        self._last_stream = cur

    def set_single_lane(self, enable=True):
        """Issue every kernel of a forward on the caller's stream (no side lanes): what several forwards in flight on several
        streams want (lp_engine_set_single_lane), and the default; ``False``: independent branches on side streams (worth
        +1.8 % for one yolov6m 1280x1280 batch at a time, -1 ... -4 % elsewhere: profiles/r03_round_ab.txt)."""
        if bool(enable) != self.single_lane:
            self.single_lane = bool(enable)
            abi.check(self.lib.lp_engine_set_single_lane(self.h, 1 if enable else 0), 'lp_engine_set_single_lane')

    def copy_tuning(self, other):
        """Take over the tuned kernel variants (all shapes) of ``other``, an engine of the same model and dtype."""
        abi.check(self.lib.lp_engine_copy_tuning(self.h, other.h), 'lp_engine_copy_tuning')
        self.tuned = set(other.tuned)

    def set_variant(self, op, cfg, nbuf):
        """Force the kernel variant of conv op ``op`` (see lp_engine_set_op_variant); switches the autotuner off."""
        self.autotune = False
        abi.check(self.lib.lp_engine_set_op_variant(self.h, op, cfg, nbuf), 'lp_engine_set_op_variant')

    def set_tile(self, op, choice):
        """Force the output-tile choice of op ``op``'s current variant (see lp_engine_set_op_tile; tests); switches the autotuner off."""
        self.autotune = False
        abi.check(self.lib.lp_engine_set_op_tile(self.h, op, choice), 'lp_engine_set_op_tile')

    def tile(self, op):
        """(choice, TH, TW) of op ``op``'s current variant for the bound shape (lp_engine_op_tile)."""
        c, th, tw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        abi.check(self.lib.lp_engine_op_tile(self.h, op, ctypes.byref(c), ctypes.byref(th), ctypes.byref(tw)), 'lp_engine_op_tile')
        return c.value, th.value, tw.value

    def variant(self, op):
        """(cfg, nbuf) of op ``op``'s current kernel variant (lp_engine_op_variant)."""
        cfg, nb = ctypes.c_int(), ctypes.c_int()
        abi.check(self.lib.lp_engine_op_variant(self.h, op, ctypes.byref(cfg), ctypes.byref(nb)), 'lp_engine_op_variant')
        return cfg.value, nb.value

    def op_io(self, op):
        """(sources, residual or -1, destinations) of op ``op`` as the frozen graph has them, i.e. after the space-to-depth rewrite of
        the stem (lp_engine_op_io): lists of tensor ids."""
        src, dst = (ctypes.c_int * abi.LP_MAX_SRC)(), (ctypes.c_int * 3)()
        n, res = ctypes.c_int(), ctypes.c_int()
        abi.check(self.lib.lp_engine_op_io(self.h, op, src, ctypes.byref(n), ctypes.byref(res), dst), 'lp_engine_op_io')
        return list(src[:n.value]), res.value, [t for t in dst if t >= 0]

    def tensor_view(self, tid):
        """Zero-copy [B,C,h,w] view (channels_last strides) of an arena tensor."""
        off, c, cs, h, w = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        abi.check(self.lib.lp_engine_tensor_info(self.h, tid, ctypes.byref(off), ctypes.byref(c), ctypes.byref(cs),
                                                 ctypes.byref(h), ctypes.byref(w)), 'lp_engine_tensor_info')
        B = self.bound[0]
        esz = torch.empty(0, dtype=self.dtype).element_size()
        base = _aligned(self.arena) - self.arena.data_ptr() + off.value
        n = B * h.value * w.value * cs.value
        flat = self.arena[base:base + n * esz].view(self.dtype)
        return flat.view(B, h.value, w.value, cs.value)[..., :c.value].permute(0, 3, 1, 2)

    def prepare(self, B, H, W, x_dtype=None):
        """Run the one-off kernel-variant tuner for a new shape on a dummy batch, so that callers who time their forwards
        (Evaler / Inferer speed protocol) do not fold the tuner (hundreds of timed launches) into the first timed batch.
        Does nothing for a shape that is already tuned, or that will never be (tuner off, or ``max_tuned_shapes`` reached):
        ``forward`` re-binds such a shape by itself, which is cheap.  No hipGraph is captured here: graphs are keyed on the
        input pointer (lp_engine_forward), so one captured for the dummy tensor could never be replayed; the caller's first
        forward captures its own."""
        if not self._untuned((B, H, W)):
            return
        x = torch.zeros(B, 3, H, W, dtype=x_dtype or self.dtype, device=self.device)
        graph = self.graph
        if graph:
            self.set_graph(False)
        try:
            self.forward(x)
            torch.cuda.current_stream(self.device).synchronize()
        finally:
            if graph:
                self.set_graph(True)

    @staticmethod
    def _check_input(x):
        """The contiguous form of a network input [B,3,H,W] and its (B, H, W)."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError('expected [B,3,H,W], got %s' % (tuple(x.shape),))
        if x.dtype not in _DT:
            raise TypeError('unsupported input dtype %s' % x.dtype)
        return x.contiguous(), (x.shape[0], x.shape[2], x.shape[3])

    def _new_pred(self, B):
        return torch.empty(B, self.n_anchors, abi.LP_PRED_COLS, dtype=torch.float32, device=self.device)

    def _untuned(self, shape):
        """First batch of this (B, H, W) with the tuner on: its kernel variants are still to be timed."""
        return self.autotune and shape not in self.tuned and len(self.tuned) < self.max_tuned_shapes

    def forward(self, x):
        x, shape = self._check_input(x)
        with torch.cuda.device(self.device):
            cur = self._stream_enter()
            self.bind(*shape)
            if self.graph:      # fixed input and output addresses: one captured graph per shape, never re-captured
                if self._graph_pred is None or self._graph_pred.shape != (shape[0], self.n_anchors, abi.LP_PRED_COLS):
                    self._graph_pred = self._new_pred(shape[0])
                pred = self._graph_pred
                x = self._stage_for_graph(x)
            else:
                pred = self._new_pred(shape[0])
            if self._untuned(shape):
                # first batch of this shape: time the kernel variants of every conv layer in place, keep the best
                abi.check(self.lib.lp_engine_autotune(self.h, _dptr(x), _DT[x.dtype], _dptr(pred), _stream_ptr(self.device), 5),
                          'lp_engine_autotune')
                self.tuned.add(shape)
            abi.check(self.lib.lp_engine_forward(self.h, _dptr(x), _DT[x.dtype], _dptr(pred), _stream_ptr(self.device)),
                      'lp_engine_forward')
            self._stream_leave(cur)
        return pred

    def _stage_for_graph(self, x):
        """Graph mode: the captured graph reads a persistent staging buffer (a frame-sized copy on the caller's stream)."""
        gx = self._graph_x
        if gx is None or gx.shape != x.shape or gx.dtype != x.dtype:
            gx = self._graph_x = torch.empty_like(x)
        if gx.data_ptr() != x.data_ptr():
            gx.copy_(x)
        return gx

    def forward_det(self, x, conf_thres, ws=None):
        """Detections-only forward (lp_engine_forward_det) on the current stream: the head writes NMS candidates into the
        workspace instead of the [B,N,290] prediction tensor.  Returns the handle ``nms_candidates`` takes: (workspace tensor,
        B, N).  ``ws``: a workspace to reuse (the caller orders its previous use before this call); by default the
        workspace of the current (device, stream)."""
        x, shape = self._check_input(x)
        if not 0.0 <= conf_thres <= 1.0:
            raise ValueError('conf_thres must be in [0, 1]')
        with torch.cuda.device(self.device):
            if self._untuned(shape):
                self.forward(x)                                 # first batch of this shape: bind + tune through the plain forward
            cur = self._stream_enter()
            self.bind(*shape)
            B, N = shape[0], self.n_anchors
            need = self.lib.lp_nms_workspace_bytes(B, N)
            if ws is None:
                ws = _nms_workspace(self.device, need)
            elif ws.numel() < need + 256:
                raise ValueError('workspace too small: %d bytes needed' % (need + 256))
            if self.graph:
                x = self._stage_for_graph(x)
            abi.check(self.lib.lp_engine_forward_det(self.h, _dptr(x), _DT[x.dtype], float(conf_thres), _aligned(ws), need,
                                                     _stream_ptr(self.device)), 'lp_engine_forward_det')
            self._stream_leave(cur)
        return ws, B, N

    def det_workspace(self, B, H, W):
        """A private workspace for ``forward_det`` on this engine (several batches in flight: one per engine)."""
        with torch.cuda.device(self.device):
            self.bind(B, H, W)
            return torch.empty(self.lib.lp_nms_workspace_bytes(B, self.n_anchors) + 256, dtype=torch.uint8, device=self.device)

    def detect(self, x, conf_thres, iou_thres, max_det, want_keep=False, route=None):
        """``non_max_suppression(Model.forward(x))`` as one call: (det[B,max_det,28], count[B] int32, keep or None).

        Two forms give the same bits (tested): the detections-only forward (lp_engine_forward_det + lp_nms_candidates: the head
        writes NMS candidates, the [B,N,290] prediction tensor is never written) and forward + lp_nms through that tensor.  The
        first wins while few anchors pass the confidence mask (yololps bs=32 at 3.5 %: +5 %; yololpn bs=128 at 17.6 %: +11 %),
        the second when nearly all do (100 %: the 112-byte candidate rows cost more than the tensor they replace, -9 %;
        DESIGN 6.3).  ``route`` None picks by the candidate density of the previous batch (``pass_rate``, read back
        asynchronously: no host sync here) against ``det_crossover``; 'det' / 'pred' force a form."""
        if route is None:
            self._poll_pass_rate()
            route = 'pred' if (self.pass_rate is not None and self.pass_rate > self.det_crossover) else 'det'
        self.det_routes[route] += 1
        if route == 'pred':
            pred = self.forward(x)
            out = nms_padded(pred, conf_thres, iou_thres, max_det, want_keep)
            self._probe_pass_rate(_nms_workspace(self.device, 0), pred.shape[0], pred.shape[1])   # the one nms_padded just filled
            return out
        handle = self.forward_det(x, conf_thres)
        out = nms_candidates(handle, iou_thres, max_det, want_keep)
        self._probe_pass_rate(*handle)
        return out

    def _probe_pass_rate(self, ws, B, N):
        """Queue a copy of the workspace's per-image candidate counts to pinned host memory behind the work just enqueued."""
        with torch.cuda.device(self.device):
            ptr = self.lib.lp_nms_candidate_counts(_aligned(ws), B, N)
            off = ptr - ws.data_ptr()
            pr = self._pass_probe
            if pr is None or pr[0].numel() != B:
                pr = (torch.empty(B, dtype=torch.int32).pin_memory(), torch.cuda.Event(), N)
            pr[0].copy_(ws[off:off + 4 * B].view(torch.int32), non_blocking=True)
            pr[1].record(torch.cuda.current_stream(self.device))
            self._pass_probe = (pr[0], pr[1], N)

    def _poll_pass_rate(self):
        pr = self._pass_probe
        if pr is not None and pr[1].query():
            self.pass_rate = float(pr[0].float().mean()) / max(1, pr[2])

    def op_kinds(self):
        """Kind name of every op of the frozen graph, in op order ('input', 'conv', 'deconv', 'pool', 'head_cls', 'head_box'); needs a
        bound arena (``bind`` / a forward)."""
        return [self._op_info(i)['kind'] for i in range(self.lib.lp_engine_num_ops(self.h))]

    def _op_info(self, i):
        """lp_engine_op_info of op ``i``: its kind name, kernel size, channels and algorithmic FLOPs / bytes."""
        kind, ks, cin, cout = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        fl, by = ctypes.c_double(), ctypes.c_double()
        abi.check(self.lib.lp_engine_op_info(self.h, i, ctypes.byref(kind), ctypes.byref(ks), ctypes.byref(cin),
                                             ctypes.byref(cout), ctypes.byref(fl), ctypes.byref(by)), 'lp_engine_op_info')
        return dict(kind=OP_KINDS[kind.value], ksize=ks.value, cin=cin.value, cout=cout.value, flops=fl.value, bytes=by.value)

    def profile(self, x, reps=3, inner=1):
        """Per-op device milliseconds (hipEvent pairs around ``inner`` back-to-back launches of each op) + op descriptions,
        for bench.py."""
        x = x.contiguous()
        B, _, H, W = x.shape
        with torch.cuda.device(self.device):
            self.bind(B, H, W)
            pred = self._new_pred(B)
            n = self.lib.lp_engine_num_ops(self.h)
            ms = (ctypes.c_float * n)()
            abi.check(self.lib.lp_engine_profile_ops(self.h, _dptr(x), _DT[x.dtype], _dptr(pred), _stream_ptr(self.device), ms, reps,
                                                     inner), 'lp_engine_profile_ops')
        ops = []
        for i in range(n):
            cfg, nb = ctypes.c_int(), ctypes.c_int()
            self.lib.lp_engine_op_variant(self.h, i, ctypes.byref(cfg), ctypes.byref(nb))
            ops.append(dict(self._op_info(i), ms=float(ms[i]),
                            variant='%s%d' % (abi.VARIANT_SHORT.get(cfg.value) or 'ABCDEFGH'[cfg.value], nb.value)))
        # Ops that launch nothing because a fused kernel carries them (the input op and the stem inside stem2_fused_kernel or behind
        # stem_planar_kernel, the 1x1 layer inside pw_s2_fused_kernel) are folded into their carrier's row: their FLOPs and bytes
        # are work of that kernel, and their own row keeps only the note (an empty event pair -- 1.4 us -- is not a 4 000 TFLOP/s launch).
        direct = x.dtype == self.dtype
        for o in ops:
            o['flops_own'], o['bytes_own'] = o['flops'], o['bytes']     # (the layer's own algorithmic figures: what bench.py's roofline sums)
        for j, c in enumerate(ops):
            i = self.lib.lp_engine_op_carrier(self.h, j, 1 if direct else 0)
            if i < 0 or i == j:
                continue
            ops[i]['flops'] += c['flops']
            # the tensor between the layers never reaches memory: the carrier's bytes are its own input-side and output-side ones
            c.update(flops=0.0, bytes=0.0, ms=0.0, carried_by=i, variant=c['variant'] + '>%d' % i)
        return ops


def _weights_version(model):
    return sum(t._version for t in list(model.parameters()) + list(model.buffers()))


# model -> (key, Engine).  Kept OUT of the module's state: an Engine holds a ctypes handle and a CDLL, and nn.Module pickles /
# deep-copies its __dict__ wholesale (the reference's checkpoint format stores whole pickled modules, checkpoint.py:22-32;
# EMA and get_model_info deep-copy the model), which would fail once the model had run on the GPU.
_engines = weakref.WeakKeyDictionary()


def drop_engine(model):
    """Forget the cached engine of ``model`` (its weights were moved, cast or re-fused)."""
    _engines.pop(model, None)


def engine_for(model, dtype=None):
    """Cached engine of a model; rebuilt when the weights were modified in place or the dtype changed."""
    p = next(model.parameters())
    if not p.is_cuda:
        raise RuntimeError('model is not on a GPU')
    dtype = dtype or getattr(model, 'lp_dtype', None) or p.dtype
    if dtype not in _DT:
        raise TypeError('unsupported activation dtype %s' % dtype)
    key = (dtype, p.device, _weights_version(model))
    cached = _engines.get(model)
    if cached is None or cached[0] != key:
        cached = (key, Engine.from_model(model, dtype, p.device))
        _engines[model] = cached
    return cached[1]


def _engine(model):
    """``engine_for(model)`` in the model's graph mode: model.lp_graph = True (set by Inferer) switches the engine to
    hipGraph replay."""
    eng = engine_for(model)
    if bool(getattr(model, 'lp_graph', False)) != eng.graph:
        eng.set_graph(getattr(model, 'lp_graph', False))
    return eng


def prepare_for(model, shape, x_dtype=None):
    """Untimed set-up (the one-off kernel-variant tuner) of ``model``'s engine for input shape [B,3,H,W]."""
    _engine(model).prepare(int(shape[0]), int(shape[2]), int(shape[3]), x_dtype)


def model_forward(model, x):
    """``Model.forward`` on a GPU: [pred[B,N,290] fp32, [f_s8, f_s16, f_s32]].  The feature maps are
    zero-copy channels_last views of the engine's arena (valid until the next forward of this model)."""
    eng = _engine(model)
    pred = eng.forward(x)
    return [pred, [eng.tensor_view(t) for t in eng.neck_ids]]


def _det_buffers(B, max_det, device, index=True):
    """Outputs of an NMS / merge launch: (det [B,max_det,28] fp32, count [B] int32, index [B,max_det] int32 or None)."""
    return (torch.empty(B, max_det, abi.LP_DET_COLS, dtype=torch.float32, device=device),
            torch.empty(B, dtype=torch.int32, device=device),
            torch.empty(B, max_det, dtype=torch.int32, device=device) if index else None)


def nms_candidates(handle, iou_thres, max_det, want_keep=False):
    """Second half of the NMS (lp_nms_candidates: sort, > 30000 cut, greedy suppression, max_det) on the current stream for the
    candidate lists ``Engine.forward_det`` left in its workspace: (det[B,max_det,28], count[B] int32, keep or None)."""
    ws, B, N = handle
    if not 0.0 <= iou_thres <= 1.0:
        raise ValueError('iou_thres must be in [0, 1]')
    lib = abi.load()
    dev = ws.device
    with torch.cuda.device(dev):
        need = lib.lp_nms_workspace_bytes(B, N)
        det, count, keep = _det_buffers(B, max_det, dev, want_keep)
        abi.check(lib.lp_nms_candidates(B, N, float(iou_thres), int(max_det), _dptr(det), _dptr(count), _dptr(keep), _aligned(ws),
                                        need, _stream_ptr(dev)), 'lp_nms_candidates')
    return det, count, keep


def detect_padded(model, x, conf_thres, iou_thres, max_det, want_keep=False, route=None):
    """``Model.forward`` + ``non_max_suppression`` of a GPU model as one call: (det[B,max_det,28], count[B], keep or None);
    see ``Engine.detect`` for the two forms it chooses between.  For callers that only want detections (Inferer, serving)."""
    return _engine(model).detect(x, conf_thres, iou_thres, max_det, want_keep, route)


def _unpad(det, counts, n=None):
    """The reference-shaped list of a padded result: det[b, :counts[b]] of the first ``n`` images (default: all), ``counts``
    being the host copy of the count tensor -- reading it is the caller's one host sync."""
    return [det[b, :counts[b]] for b in range(len(counts) if n is None else n)]


def detect(model, x, conf_thres, iou_thres, max_det, route=None):
    """Reference-shaped result of ``non_max_suppression(model(x)[0], ...)``: list (len B) of [n_i, 28] tensors."""
    det, count, _ = detect_padded(model, x, conf_thres, iou_thres, max_det, route=route)
    return _unpad(det, count.cpu().tolist())


# ---------------------------------------------------------------------------------------------------
_nms_ws, _redact_ws = {}, {}


def _stream_workspace(cache, device, need):
    """``cache``'s workspace of ``device``'s current stream, grown to ``need`` bytes (+ 256 for ``_aligned``), never zeroed."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() < need + 256:
        ws = cache[key] = torch.empty(need + 256, dtype=torch.uint8, device=device)
    return ws


def _nms_workspace(device, need):
    """The NMS workspace of ``device``'s current stream, grown to ``need`` bytes (+ 256 for ``_aligned``)."""
    # one workspace per (device, stream): lp_nms memsets and fills it on the current stream, so two streams must never
    # share one; a regrown buffer is released through the caching allocator, which orders its reuse on this stream
    return _stream_workspace(_nms_ws, device, need)


def nms_padded(prediction, conf_thres, iou_thres, max_det, want_keep=False):
    """Batch NMS through lp_nms without a host sync: (det[B,max_det,28], count[B] int32, keep or None)."""
    if not (prediction.is_cuda and prediction.dtype == torch.float32 and prediction.is_contiguous()):
        raise ValueError('prediction must be a contiguous fp32 CUDA tensor')
    B, N, C = prediction.shape
    if C != abi.LP_PRED_COLS:
        raise ValueError('prediction must have %d columns, got %d' % (abi.LP_PRED_COLS, C))
    lib = abi.load()
    dev = prediction.device
    with torch.cuda.device(dev):
        need = lib.lp_nms_workspace_bytes(B, N)
        ws = _nms_workspace(dev, need)
        det, count, keep = _det_buffers(B, max_det, dev, want_keep)
        abi.check(lib.lp_nms(_dptr(prediction), B, N, float(conf_thres), float(iou_thres), int(max_det), _dptr(det), _dptr(count),
                             _dptr(keep), _aligned(ws), need, _stream_ptr(dev)), 'lp_nms')
    return det, count, keep


def non_max_suppression(prediction, conf_thres, iou_thres, max_det):
    """Reference-shaped result: list (len B) of [n_i, 28] tensors; one host sync for the whole batch."""
    B, N = prediction.shape[0], prediction.shape[1]
    if B == 0 or N == 0:
        return [torch.zeros((0, 28), device=prediction.device)] * B
    src = prediction
    work = prediction
    if work.dtype != torch.float32 or not work.is_contiguous():
        work = work.float().contiguous()
    det, count, _ = nms_padded(work, conf_thres, iou_thres, max_det)
    if work is not src:
        src.copy_(work)          # keep the reference's in-place obj*cls side effect on the caller's tensor
    return _unpad(det, count.cpu().tolist())


# ---------------------------------------------------------------------------------------------------
def _frames_device(frames):
    """The one device of a non-empty list of contiguous uint8 CUDA [h,w,3] frames (ValueError otherwise)."""
    dev = frames[0].device
    for f in frames:
        if not (f.is_cuda and f.device == dev and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous()):
            raise ValueError('frames must be contiguous uint8 CUDA tensors [h, w, 3] on one device')
    return dev


def _nv12_device(frames):
    """The one device of a non-empty list of ``Nv12Frame`` whose planes are CUDA tensors (ValueError otherwise)."""
    dev = frames[0].device
    for f in frames:
        if not (isinstance(f, Nv12Frame) and f.is_cuda and f.device == dev):
            raise ValueError('NV12 frames must be Nv12Frame objects with CUDA planes on one device')
    return dev


def _frames_on(frames, what='frames'):
    """(device, is_nv12) of a non-empty list of frames of ONE kind: contiguous uint8 CUDA [h,w,3] BGR tensors, or ``Nv12Frame``
    objects with CUDA planes (a mixed list is a ValueError)."""
    if is_nv12_list(frames, what):
        return _nv12_device(frames), True
    return _frames_device(frames), False


def _buffer(buf, shape, dtype, device, what='out'):
    """A caller's persistent output buffer, checked; a new tensor of that ``shape`` / ``dtype`` on ``device`` when it is None."""
    if buf is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not (buf.shape == shape and buf.dtype == dtype and buf.device == device and buf.is_contiguous()):
        raise ValueError('%s must be a contiguous %s tensor %s on %s' % (what, dtype, list(shape), device))
    return buf


def _batch_on(frames, n, dtype, batch, what):
    """Argument checks of a batched preprocess of ``n`` images cut from ``frames``: (device, B), where ``batch`` (>= n, >= 1)
    sets B and the slots past n are padding."""
    if dtype not in _DT:
        raise TypeError('unsupported input dtype %s' % dtype)
    if not frames:
        raise ValueError('%s needs at least one frame' % what)
    dev, _ = _frames_on(frames, what)
    B = n if batch is None else int(batch)
    if B < n or B < 1:
        raise ValueError('batch %d < %d images (or < 1)' % (B, n))
    return dev, B


def _check_det_count(det, count, what='det', min_batch=0):
    """det [B >= min_batch, max_det, 28] fp32 and count [B] int32 as ``nms_padded`` returns them: contiguous, on one GPU."""
    if not (det.is_cuda and det.dtype == torch.float32 and det.dim() == 3 and det.shape[2] == abi.LP_DET_COLS
            and det.is_contiguous() and det.shape[0] >= min_batch):
        raise ValueError('%s must be a contiguous CUDA fp32 [B >= %d, max_det, 28] tensor' % (what, min_batch))
    if not (count.is_cuda and count.dtype == torch.int32 and count.is_contiguous() and count.numel() == det.shape[0]
            and count.device == det.device):
        raise ValueError('the count of %s must be a contiguous CUDA int32 [B] tensor on its device' % what)


def nv12_to_bgr(frames, out=None):
    """BGR device frames of a list of ``Nv12Frame`` with CUDA planes on one device (lp_nv12_to_bgr_batch, one launch per 64
    frames, on the current stream): a list of contiguous uint8 [h,w,3] tensors, bit for bit ``nv12_to_bgr_np`` of each frame.
    For the callers that need the frame itself -- plate crops, the best-shot gallery, saving images; detection reads NV12
    directly.  ``out``: a list of persistent [h,w,3] uint8 buffers to write (any alignment); by default the frames are views
    of one new buffer, at 256-byte aligned bases."""
    if not frames:
        return []
    dev = _nv12_device(frames)
    if out is None:
        offs, n = [], 0
        for f in frames:
            offs.append(n)
            n += (f.h * f.w * 3 + 255) // 256 * 256
        buf = torch.empty(n, dtype=torch.uint8, device=dev)
        out = [buf[o:o + f.h * f.w * 3].view(f.h, f.w, 3) for f, o in zip(frames, offs)]
    else:
        out = list(out)
        if len(out) != len(frames):
            raise ValueError('%d output buffers for %d frames' % (len(out), len(frames)))
        out = [_buffer(o, (f.h, f.w, 3), torch.uint8, dev, 'out[%d]' % k) for k, (o, f) in enumerate(zip(out, frames))]
    desc = (abi.Nv12BgrDesc * len(frames))()
    for d, f, o in zip(desc, frames, out):
        d.y, d.uv, d.pitch_y, d.pitch_uv, d.h0, d.w0 = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, f.h, f.w
        d.matrix, d.out = f.matrix_id, o.data_ptr()
    with torch.cuda.device(dev):
        abi.check(abi.load().lp_nv12_to_bgr_batch(desc, len(frames), _stream_ptr(dev)), 'lp_nv12_to_bgr_batch')
    return out


def _bgr_frames(frames):
    """``frames`` as BGR device frames: an NV12 list converted once (``nv12_to_bgr``), a BGR list as it is; None entries stay."""
    live = [f for f in frames if f is not None]
    if not live or not is_nv12_list(live):
        return frames
    it = iter(nv12_to_bgr(live))
    return [None if f is None else next(it) for f in frames]


def _letterbox_regions(frames, plans, geoms, B, H, W, dtype, out, dev):
    """One letterbox call: region ``plans[k]`` = (frame index, y0, x0, th, tw) of ``frames`` with the letterbox geometry ``geoms[k]``
    = (rh, rw, top, left) into slot k of ``out`` [B,3,H,W].  BGR tensors go through lp_preprocess_tiles_batch; ``Nv12Frame``s through
    lp_preprocess_nv12_batch (the same kernel reading the planes: no BGR frame is created)."""
    for k, *_ in plans:
        if not 0 <= k < len(frames):
            raise ValueError('tile of frame %d: %d frames' % (k, len(frames)))
    nv12 = isinstance(frames[0], Nv12Frame)
    desc = ((abi.Nv12Desc if nv12 else abi.TileDesc) * max(len(plans), 1))()
    for d, (k, y0, x0, th, tw), (rh, rw, top, left) in zip(desc, plans, geoms):
        f = frames[k]
        if nv12:
            d.y, d.uv, d.pitch_y, d.pitch_uv, d.matrix = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, f.matrix_id
        else:
            d.img = f.data_ptr()
        d.h0, d.w0, d.y0, d.x0, d.th, d.tw, d.rh, d.rw, d.top, d.left = f.shape[0], f.shape[1], y0, x0, th, tw, rh, rw, top, left
    name = 'lp_preprocess_nv12_batch' if nv12 else 'lp_preprocess_tiles_batch'
    with torch.cuda.device(dev):
        abi.check(getattr(abi.load(), name)(desc, len(plans), B, _dptr(out), _DT[dtype], H, W, _stream_ptr(dev)), name)
    return out


def preprocess_letterbox(frame_bgr_u8, img_size, stride, dtype, auto=True):
    """GPU form of Inferer.precess_image: device uint8 [h,w,3] BGR frame -> [3,H,W] RGB /255 tensor of ``dtype``.
    Geometry (ratio, resized size, padding) is the reference's letterbox arithmetic, done on the host; ``auto=False``
    pads to exactly ``img_size`` instead of the next stride multiple."""
    if not (frame_bgr_u8.is_cuda and frame_bgr_u8.dtype == torch.uint8 and frame_bgr_u8.dim() == 3 and
            frame_bgr_u8.shape[2] == 3 and frame_bgr_u8.is_contiguous()):
        raise ValueError('frame must be a contiguous uint8 CUDA tensor [h, w, 3]')
    h0, w0 = frame_bgr_u8.shape[:2]
    rh, rw, top, left, H, W = letterbox_placement((h0, w0), img_size, stride, auto)
    out = torch.empty(3, H, W, dtype=dtype, device=frame_bgr_u8.device)
    with torch.cuda.device(out.device):
        abi.check(abi.load().lp_preprocess_letterbox(_dptr(frame_bgr_u8), h0, w0, _dptr(out), _DT[dtype], H, W, rh, rw, top, left,
                                                     _stream_ptr(out.device)), 'lp_preprocess_letterbox')
    return out


def preprocess_frames(frames, img_size, stride, dtype, auto=True, batch=None, out=None):
    """Batched ``preprocess_letterbox`` (each frame as the region (0, 0, h, w) of lp_preprocess_tiles_batch, which is
    lp_preprocess_letterbox_batch on whole frames; one launch per 64 frames): a list of contiguous
    uint8 CUDA [h,w,3] BGR frames of any sizes -> (x[B,3,H,W] of ``dtype``, geoms).  ``geoms[i]`` is frame i's
    (rh, rw, top, left) from the host letterbox arithmetic.  With ``auto=True`` every frame must letterbox to the same
    (H, W); ``auto=False`` letterboxes each to exactly ``img_size``.  ``batch`` (>= len(frames)) sets B: slots past the
    frames are padding (114/255).  ``out``: a persistent [B,3,H,W] input buffer to write (graphs are keyed on the
    input pointer).  A list of ``Nv12Frame`` (CUDA planes) is taken instead of BGR tensors: the conversion is fused into the
    letterbox (lp_preprocess_nv12_batch) and x equals, bit for bit, that of the frames ``nv12_to_bgr`` gives."""
    dev, B = _batch_on(frames, len(frames), dtype, batch, 'preprocess_frames')
    places = [letterbox_placement(f.shape, img_size, stride, auto) for f in frames]
    geoms, hws = [p[:4] for p in places], set(p[4:] for p in places)
    if len(hws) != 1:
        raise ValueError('frames letterbox to different shapes %s (source shapes %s): batch them separately or use auto=False'
                         % (sorted(hws), [tuple(f.shape[:2]) for f in frames]))
    H, W = hws.pop()
    out = _buffer(out, (B, 3, H, W), dtype, dev)
    plans = [(k, 0, 0) + tuple(f.shape[:2]) for k, f in enumerate(frames)]      # a whole frame: the region (0, 0, h, w)
    return _letterbox_regions(frames, plans, geoms, B, H, W, dtype, out, dev), geoms


def _rescale_terms(ori_shape, target_shape):
    """Inferer.rescale's (ratio, padx, pady) from the network input (h, w) back to a source image of (h, w[, c])."""
    ratio = min(ori_shape[0] / target_shape[0], ori_shape[1] / target_shape[1])
    return ratio, (ori_shape[1] - target_shape[1] * ratio) / 2, (ori_shape[0] - target_shape[0] * ratio) / 2


def rescale_round(ori_shape, det, target_shape):
    """GPU form of ``Inferer.rescale(ori_shape, det[:, :12], target_shape).round()``, in place on det [n, 28]."""
    if not (det.is_cuda and det.dtype == torch.float32 and det.dim() == 2 and det.shape[1] == abi.LP_DET_COLS and
            det.stride(1) == 1 and det.stride(0) == abi.LP_DET_COLS):
        raise ValueError('det must be a CUDA fp32 [n, 28] tensor with contiguous rows')
    ratio, padx, pady = _rescale_terms(ori_shape, target_shape)
    with torch.cuda.device(det.device):
        abi.check(abi.load().lp_rescale_round(_dptr(det), det.shape[0], float(ratio), float(padx), float(pady),
                                              int(target_shape[1]), int(target_shape[0]), _stream_ptr(det.device)),
                  'lp_rescale_round')
    return det


def rescale_round_batch(det, count, net_hw, src_shapes):
    """Batched ``rescale_round`` (lp_rescale_round_batch), in place on det [B,max_det,28]: rows r < count[b] of image
    b < len(src_shapes) are mapped back to source image b of shape (h, w[, c]) from the network input size ``net_hw``
    (Inferer.rescale's ratio and padding) and rounded.  ``count`` (int32 [B], CUDA) is read on the device: no host sync."""
    _check_det_count(det, count)
    n = len(src_shapes)
    if n > det.shape[0]:
        raise ValueError('%d source shapes for a batch of %d' % (n, det.shape[0]))
    desc = (abi.RescaleDesc * max(n, 1))()
    for d, s in zip(desc, src_shapes):
        d.ratio, d.padx, d.pady = _rescale_terms(net_hw, s)
        d.img_w, d.img_h = int(s[1]), int(s[0])
    with torch.cuda.device(det.device):
        abi.check(abi.load().lp_rescale_round_batch(_dptr(det), _dptr(count), n, det.shape[1], desc, _stream_ptr(det.device)),
                  'lp_rescale_round_batch')
    return det


def detect_frames_padded(model, frames, img_size, conf_thres, iou_thres, max_det, auto=True, batch=None, out=None):
    """The device work of ``detect_frames`` without its host read: (det [B,max_det,28], count [B] int32) on the device, rows
    r < count[b] of frame b < len(frames) in source-image pixels, rounded."""
    dtype = next(model.parameters()).dtype
    x, _ = preprocess_frames(frames, img_size, int(model.stride.max()), dtype, auto=auto, batch=batch, out=out)   # DetectBackend's stride
    det, count, _ = detect_padded(model, x, conf_thres, iou_thres, max_det)
    rescale_round_batch(det, count, x.shape[2:], [tuple(f.shape[:2]) for f in frames])
    return det, count


def detect_frames(model, frames, img_size, conf_thres, iou_thres, max_det, auto=True, batch=None, out=None):
    """Detections of a batch of raw frames (contiguous uint8 CUDA [h,w,3] BGR, any sizes that letterbox to one shape, or any
    sizes with ``auto=False``): ``preprocess_frames`` -> ``detect_padded`` -> ``rescale_round_batch``, then one host read of
    the counts.  Returns a list of [n_i, 28] tensors in source-image pixels, rounded: per frame what Inferer.infer returns,
    bit for bit.  The input dtype is the model's parameter dtype (Inferer's fp16 / fp32 input); ``batch`` / ``out`` as in
    ``preprocess_frames`` (padding slots let a short tail reuse a bound batch size).  ``frames`` may be a list of ``Nv12Frame``
    instead (the conversion is fused into the letterbox; no BGR frame is created): the result is, bit for bit, that of the frames
    ``nv12_to_bgr`` gives."""
    det, count = detect_frames_padded(model, frames, img_size, conf_thres, iou_thres, max_det, auto, batch, out)
    return _unpad(det, count.cpu().tolist(), len(frames))


def _crop_size(crop_hw):
    Hc, Wc = (int(v) for v in crop_hw)
    if not (1 <= Hc <= 1024 and 1 <= Wc <= 1024):
        raise ValueError('crop size %dx%d: need 1..1024 on each side' % (Hc, Wc))
    return Hc, Wc


def _plate_crops_launch(frames, det, count, slots, out, status, crop_hw):
    """lp_plate_crops_batch on frames with ``slots[b]`` = (max_crops, out_slot): out [n_slots,Hc,Wc,3], status [n_slots]."""
    _check_det_count(det, count, min_batch=len(frames))
    if det.device != out.device:
        raise ValueError('det must be on the frames\' device')
    desc = (abi.CropDesc * len(frames))()
    for d, f, (m, o) in zip(desc, frames, slots):
        d.img, d.h0, d.w0, d.max_crops, d.out_slot = f.data_ptr(), f.shape[0], f.shape[1], m, o
    with torch.cuda.device(det.device):
        abi.check(abi.load().lp_plate_crops_batch(desc, len(frames), _dptr(det), _dptr(count), det.shape[1], _dptr(out),
                                                  _dptr(status), status.numel(), crop_hw[0], crop_hw[1], _stream_ptr(det.device)),
                  'lp_plate_crops_batch')


def plate_crops(frames, det, count, crop_hw=(64, 192), max_crops=None, out=None, status=None):
    """Perspective-rectified plate crops (lp_plate_crops_batch, one launch per 64 frames) of the detections of B frames:
    frame b (contiguous uint8 CUDA [h,w,3] BGR) is cut along its rows r < min(count[b], max_det, max_crops) of det
    [B,max_det,28] (fp32, source-frame pixels, as ``rescale_round_batch`` leaves them; count int32 [B] on the device, read by
    the kernel: no host sync).  Returns (crops [B,max_crops,Hc,Wc,3] uint8 BGR, status [B,max_crops] int32): 1 = cut along
    the four corners, 2 = along the box (the corners are not a convex quad of area >= 1), 3 = neither is usable (zeros),
    0 = no such detection (the crop's bytes are left as they were).  ``max_crops`` defaults to 16 (each slot is Hc*Wc*3
    bytes); ``out`` / ``status``: persistent buffers of those shapes.  yolov6.utils.plate_crop.plate_crops_np is the same
    computation on the CPU, bit for bit.  A list of ``Nv12Frame`` is converted with ``nv12_to_bgr`` first."""
    if not frames:
        raise ValueError('plate_crops needs at least one frame')
    frames = _bgr_frames(frames)            # an NV12 list is converted once, on this stream
    dev = _frames_device(frames)
    Hc, Wc = _crop_size(crop_hw)
    n, m = len(frames), 16 if max_crops is None else int(max_crops)
    if m < 0:
        raise ValueError('max_crops must be >= 0')
    out = _buffer(out, (n, m, Hc, Wc, 3), torch.uint8, dev)
    status = _buffer(status, (n, m), torch.int32, dev, 'status')
    _plate_crops_launch(frames, det, count, [(m, b * m) for b in range(n)], out, status, (Hc, Wc))
    return out, status


def crop_sharpness(crops, status, out=None):
    """Laplacian energy of plate crops (lp_crop_sharpness, one workgroup per crop): crops [..., Hc, Wc, 3] uint8 + status [...]
    int32 as ``plate_crops`` returns them -> int64 [...] on the device holding the unsigned 64-bit sums (view the host copy as
    uint64); 0 for status 0 or 3 or a side shorter than 3.  ``out``: a persistent buffer of that shape.
    yolov6.utils.best_shot.crop_sharpness_np is the same computation on the CPU, bit for bit."""
    if not (crops.is_cuda and crops.dtype == torch.uint8 and crops.dim() >= 3 and crops.shape[-1] == 3 and crops.is_contiguous()):
        raise ValueError('crops must be a contiguous uint8 CUDA tensor [..., Hc, Wc, 3]')
    lead = crops.shape[:-3]
    Hc, Wc = _crop_size(crops.shape[-3:-1])
    if not (status.dtype == torch.int32 and status.shape == lead and status.device == crops.device and status.is_contiguous()):
        raise ValueError('status must be a contiguous int32 tensor %s on the crops\' device' % list(lead))
    out = _buffer(out, lead, torch.int64, crops.device, 'sharp')
    with torch.cuda.device(crops.device):
        abi.check(abi.load().lp_crop_sharpness(_dptr(crops), _dptr(status), status.numel(), Hc, Wc, _dptr(out), _stream_ptr(crops.device)),
                  'lp_crop_sharpness')
    return out


def _unpad_with_crops(frames, det, count, crop_hw):
    """(dets, crops, status) of the ``*_with_crops`` entry points from a padded result in frame pixels: the one host read of
    the counts, then the crops packed, frame b's n_b right behind frame b-1's (``crop_hw``: checked by ``_crop_size``)."""
    frames = _bgr_frames(frames)            # an NV12 list is converted once, on this stream, before the host read
    counts = count.cpu().tolist()
    ns = [max(0, min(int(c), det.shape[1])) for c in counts[:len(frames)]]
    offs = np.concatenate([[0], np.cumsum(ns)]).astype(int).tolist()
    crops = torch.empty(offs[-1], *crop_hw, 3, dtype=torch.uint8, device=det.device)
    status = torch.empty(offs[-1], dtype=torch.int32, device=det.device)
    _plate_crops_launch(frames, det, count, list(zip(ns, offs)), crops, status, crop_hw)
    return (_unpad(det, counts, len(frames)), [crops[o:o + k] for o, k in zip(offs, ns)],
            [status[o:o + k] for o, k in zip(offs, ns)])


def detect_frames_with_crops(model, frames, img_size, conf_thres, iou_thres, max_det, crop_hw=(64, 192), auto=True, batch=None,
                             out=None):
    """``detect_frames`` plus the plate crop of every detection: (dets, crops, status).  ``dets`` is bit for bit what
    ``detect_frames`` returns; after its one host read of the counts the crops are packed, frame b's n_b crops right behind
    frame b-1's in one [sum n_b,Hc,Wc,3] uint8 tensor: ``crops[b]`` is an [n_b,Hc,Wc,3] view of it and ``status[b]`` an
    [n_b] int32 view (codes as in ``plate_crops``).  The crops are enqueued here, before the next ``FrameBatcher.put`` may
    reuse the frames' buffer."""
    crop_hw = _crop_size(crop_hw)
    det, count = detect_frames_padded(model, frames, img_size, conf_thres, iou_thres, max_det, auto, batch, out)
    return _unpad_with_crops(frames, det, count, crop_hw)


#: redact_plates(mode='gauss'): the tables of one lp_redact_gauss_batch call stay under this many bytes (a 4K frame takes 33 MB)
GAUSS_WS_CAP = 256 << 20


def _redact_workspace(device, need):
    """The cell table of ``redact_plates`` on ``device``'s current stream, grown to ``need`` bytes (+ 256 for ``_aligned``); one per
    (device, stream), as ``_nms_workspace``.  It needs no zeroing: a call reads only entries it has written itself."""
    return _stream_workspace(_redact_ws, device, need)


def redact_plates(frames, det, count, mode='mosaic', cell=16, margin=0.1, fill=(0, 0, 0), status=None, sigma=None):
    """Make the plates of B device frames unreadable IN PLACE (lp_redact_plates_batch, two launches per 64 frames on the current
    stream, no host read): ``frames`` is a list of contiguous uint8 CUDA [h,w,3] BGR tensors or of ``Nv12Frame`` with CUDA planes
    (one kind; NV12 is redacted in its own planes, no BGR copy exists), ``det`` [>= B,max_det,28] + ``count`` int32 on the device
    as ``detect_frames_padded``, ``detect_tiled_padded`` or ``PlateTracker.update`` (det_out) return them.  EVERY row
    r < min(max(count[b], 0), max_det) of frame b is redacted -- there is no cap -- along its corners, or its box when the
    corners are no convex quad of area >= 1, scaled by ``1 + margin`` about the centre.  ``mode`` 'mosaic': a pixel takes the mean of
    its ``cell`` x ``cell`` cell (even, 2..64; the grid is anchored to the frame, the means are of the frame before the call, so
    overlapping plates and the order of the rows do not matter); 'fill': ``fill`` = (B, G, R), converted with the frame's matrix
    for NV12; 'gauss': a pixel takes the frame as it was before the call under the integer Gaussian of ``sigma`` (0.5..16, None:
    8.0; lp_redact_gauss_batch, whose table takes 4 bytes per frame pixel: the frames go in runs whose tables stay under
    ``GAUSS_WS_CAP``), so the order of the rows and overlaps do not matter either, but a second call blurs again.
    Writes into the caller's tensors and returns status [B,max_det] int32: 1 = corners, 2 = box, 3 = neither usable
    (nothing written), 0 = no such row.  yolov6.utils.redact.redact_plates_np is the same computation on the CPU, bit for bit.

    REDACTION GOES LAST: ``plate_crops``, ``PlateTracker.update_with_shots`` and the best-shot gallery must read the frames
    BEFORE this call on the same stream, or they cut mosaics."""
    from yolov6.utils.redact import check_params, check_sigma, fill_bytes
    if not frames:
        raise ValueError('redact_plates needs at least one frame')
    dev, nv12 = _frames_on(frames, 'redact_plates')
    _check_det_count(det, count, min_batch=len(frames))
    if det.device != dev or det.shape[1] < 1:
        raise ValueError('det must be on the frames\' device with max_det >= 1')
    m, cell, margin = check_params(mode, cell, margin)
    n, max_det = len(frames), det.shape[1]
    status = _buffer(status, (n, max_det), torch.int32, dev, 'status')
    desc = (abi.RedactDesc * n)()
    for d, f in zip(desc, frames):
        if nv12:
            d.p0, d.p1, d.pitch0, d.pitch1, d.format = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, 1
        else:
            d.p0, d.p1, d.pitch0, d.format = f.data_ptr(), None, 3 * f.shape[1], 0
        d.h0, d.w0 = f.shape[0], f.shape[1]
    if m == 2:
        with torch.cuda.device(dev):
            _redact_gauss(desc, [4 * f.shape[0] * f.shape[1] + 16 for f in frames], det, count, status, margin, check_sigma(sigma), dev)
        return status
    # one call per run of frames that share the fill's bytes: a BGR list or a mosaic is one run, an NV12 fill one per matrix
    fills = [fill_bytes(fill, f.matrix if nv12 and m == 1 else None) for f in frames]
    lib, b0 = abi.load(), 0
    with torch.cuda.device(dev):
        while b0 < n:
            b1 = b0 + 1
            while b1 < n and fills[b1] == fills[b0]:
                b1 += 1
            params = abi.RedactParams(m, cell, margin, (ctypes.c_ubyte * 3)(*fills[b0]))
            run = ctypes.cast(ctypes.byref(desc, b0 * ctypes.sizeof(abi.RedactDesc)), ctypes.POINTER(abi.RedactDesc))
            need = lib.lp_redact_workspace_bytes(run, b1 - b0, ctypes.byref(params))
            ws = _redact_workspace(dev, need) if m == 0 else None
            abi.check(lib.lp_redact_plates_batch(run, b1 - b0, _dptr(det[b0:b1]), _dptr(count[b0:b1]), max_det, ctypes.byref(params),
                                                 _dptr(status[b0:b1]), None if ws is None else _aligned(ws), need, _stream_ptr(dev)),
                      'lp_redact_plates_batch')
            b0 = b1
    return status


def _gauss_params(margin, sigma):
    """lp_redact_gauss_params of a public sigma: the taps of sigma for BGR and Y, of sigma / 2 for U and V."""
    from yolov6.utils.redact import gauss_taps
    t, tc = gauss_taps(sigma), gauss_taps(sigma / 2)
    p = abi.RedactGaussParams(margin, len(t) - 1, len(tc) - 1)
    p.taps[:len(t)] = [int(v) for v in t]
    p.taps_c[:len(tc)] = [int(v) for v in tc]
    return p


def _redact_gauss(desc, table_bytes, det, count, status, margin, sigma, dev):
    """lp_redact_gauss_batch over consecutive runs of the frames of ``desc`` whose tables (``table_bytes`` bounds each frame's) stay
    under ``GAUSS_WS_CAP`` together, at least one frame per run: frames are independent, so the split does not show."""
    lib, params, max_det = abi.load(), _gauss_params(margin, sigma), det.shape[1]
    n, b0 = len(table_bytes), 0
    while b0 < n:
        b1, total = b0 + 1, table_bytes[b0]
        while b1 < n and total + table_bytes[b1] <= GAUSS_WS_CAP:
            total += table_bytes[b1]
            b1 += 1
        run = ctypes.cast(ctypes.byref(desc, b0 * ctypes.sizeof(abi.RedactDesc)), ctypes.POINTER(abi.RedactDesc))
        need = lib.lp_redact_gauss_workspace_bytes(run, b1 - b0, ctypes.byref(params))
        ws = _redact_workspace(dev, need)
        abi.check(lib.lp_redact_gauss_batch(run, b1 - b0, _dptr(det[b0:b1]), _dptr(count[b0:b1]), max_det, ctypes.byref(params),
                                            _dptr(status[b0:b1]), _aligned(ws), need, _stream_ptr(dev)), 'lp_redact_gauss_batch')
        b0 = b1


# ---------------------------------------------------------------------------------------------------
# Annotation overlay drawn on the device (yolov6/utils/overlay.py is the specification; lp_overlay_draw_batch)
_overlay_ws = {}
_overlay_params_memo = {}


class OverlayFont:
    """The glyph atlas of ``draw_plates`` on a device, uploaded once: ``atlas`` uint8 [G, gh, gw] coverage and ``glyph_of`` uint16
    [8, 64] as ``yolov6.utils.overlay.build_atlas`` makes them (or any caller's data with the thirteen fixed glyphs)."""

    def __init__(self, atlas, glyph_of, device='cuda'):
        from yolov6.utils.overlay import check_font
        self.atlas_np, self.glyph_of_np = check_font(atlas, glyph_of)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('OverlayFont lives on a GPU; the CPU path takes the arrays themselves (draw_plates_np)')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.atlas = torch.from_numpy(self.atlas_np).to(self.device)
        self.glyph_of = torch.from_numpy(self.glyph_of_np.view(np.int16)).to(self.device)      # the bits of the uint16 table
        self.n_glyphs, self.gh, self.gw = self.atlas_np.shape


def _overlay_params(font, styles, palette, matrix, show_id, label, draw_box):
    """lp_overlay_params of checked styles and palette, the colours in the bytes of a frame of ``matrix`` (None: BGR)."""
    from yolov6.utils.redact import fill_bytes
    key = (font.n_glyphs, font.gh, font.gw, tuple(styles), None if palette is None else palette.tobytes(), matrix, bool(show_id),
           bool(label), bool(draw_box))
    p = _overlay_params_memo.get(key)       # the colour conversion of an NV12 matrix is not free: once per distinct call
    if p is not None:
        return p
    if len(_overlay_params_memo) >= 64:
        _overlay_params_memo.clear()
    p = _overlay_params_memo[key] = abi.OverlayParams()
    p.n_styles = len(styles)
    for d, s in zip(p.styles, styles):
        for name in ('box', 'quad', 'plate', 'text'):
            getattr(d, name)[:] = fill_bytes(getattr(s, name), matrix)
        d.t, d.a_line, d.a_plate, d.a_text, d.pad = s.t, s.a_line, s.a_plate, s.a_text, s.pad
    p.n_palette = 0 if palette is None else len(palette)
    for k in range(p.n_palette):
        p.palette[k][:] = fill_bytes(tuple(int(v) for v in palette[k]), matrix)
    p.n_glyphs, p.gh, p.gw = font.n_glyphs, font.gh, font.gw
    p.show_id, p.label, p.draw_box = int(bool(show_id)), int(bool(label)), int(bool(draw_box))
    return p


def draw_plates(frames, det, count, atlas, glyph_of=None, tid=None, style=None, styles=None, palette=None, show_id=True, label=True,
                draw_box=True, status=None):
    """Draw the detections of B device frames onto them IN PLACE (lp_overlay_draw_batch, two launches per 64 frames on the current
    stream, no host read): box outline, corner-quad outline and a label with the track id and the eight heads' characters.
    ``frames`` is a list of contiguous uint8 CUDA [h,w,3] BGR tensors or of ``Nv12Frame`` with CUDA planes (one kind; NV12 is drawn
    in its own planes, no BGR copy exists); ``det`` [>= B,max_det,28] + ``count`` int32 on the device exactly as
    ``detect_frames_padded``, ``detect_tiled_padded``, ``TileGate.detect_padded``, ``PlateTracker.update`` (det_out) or the
    tracker's ``last_hold`` leave them; ``tid`` int32 [>= B,max_det] as ``PlateTracker.update`` returns it, or None; ``style`` int32
    [>= B,max_det] picks one of ``styles`` (a list of up to 8 ``yolov6.utils.overlay.Style``, colours (B, G, R), converted with
    the frame's matrix for NV12) per row, < 0 skips the row; ``palette`` uint8 [P <= 64, 3] colours the quad and the label plate
    by ``tid % P``.  ``atlas`` is an ``OverlayFont`` (uploaded once, reused), or the two arrays of one.  Writes into the caller's
    tensors and returns status [B,max_det] int32: 1 = corners, 2 = box, 3 = nothing drawable, 0 = no such row or a skipped one.
    ``yolov6.utils.overlay.draw_plates_np`` is the same computation on the CPU, byte for byte.

    THE OVERLAY GOES LAST on a stream: crops and best shots read the frames first, ``redact_plates`` comes next, then this call, so
    outlines sit on top of a mosaic.  Draw on a clone when other consumers need the clean frame."""
    from yolov6.utils.overlay import check_palette, check_styles
    if not frames:
        raise ValueError('draw_plates needs at least one frame')
    dev, nv12 = _frames_on(frames, 'draw_plates')
    _check_det_count(det, count, min_batch=len(frames))
    if det.device != dev or det.shape[1] < 1:
        raise ValueError('det must be on the frames\' device with max_det >= 1')
    font = atlas if isinstance(atlas, OverlayFont) else OverlayFont(atlas, glyph_of, dev)
    if font.device != dev:
        raise ValueError('the OverlayFont is on %s, the frames on %s' % (font.device, dev))
    styles, palette = check_styles(styles), check_palette(palette)
    n, max_det = len(frames), det.shape[1]
    for name, a in (('tid', tid), ('style', style)):
        if a is not None and not (a.is_cuda and a.device == dev and a.dtype == torch.int32 and a.dim() == 2 and a.shape[0] >= n
                                  and a.shape[1] == max_det and a.is_contiguous()):
            raise ValueError('%s must be a contiguous CUDA int32 [>= %d, %d] tensor on the frames\' device' % (name, n, max_det))
    status = _buffer(status, (n, max_det), torch.int32, dev, 'status')
    desc = (abi.RedactDesc * n)()
    for d, f in zip(desc, frames):
        if nv12:
            d.p0, d.p1, d.pitch0, d.pitch1, d.format = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, 1
        else:
            d.p0, d.p1, d.pitch0, d.format = f.data_ptr(), None, 3 * f.shape[1], 0
        d.h0, d.w0 = f.shape[0], f.shape[1]
    # one call per run of frames that share the colours' bytes: a BGR list is one run, an NV12 list one per matrix
    key = [f.matrix if nv12 else None for f in frames]
    lib, b0 = abi.load(), 0
    with torch.cuda.device(dev):
        while b0 < n:
            b1 = b0 + 1
            while b1 < n and key[b1] == key[b0]:
                b1 += 1
            params = _overlay_params(font, styles, palette, key[b0], show_id, label, draw_box)
            run = ctypes.cast(ctypes.byref(desc, b0 * ctypes.sizeof(abi.RedactDesc)), ctypes.POINTER(abi.RedactDesc))
            need = lib.lp_overlay_workspace_bytes(b1 - b0, max_det)
            ws = _stream_workspace(_overlay_ws, dev, need)
            abi.check(lib.lp_overlay_draw_batch(run, b1 - b0, _dptr(det[b0:b1]), _dptr(count[b0:b1]), max_det,
                                                None if tid is None else _dptr(tid[b0:b1]), None if style is None else _dptr(style[b0:b1]),
                                                ctypes.byref(params), _dptr(font.atlas), _dptr(font.glyph_of), _dptr(status[b0:b1]),
                                                _aligned(ws), need, _stream_ptr(dev)), 'lp_overlay_draw_batch')
            b0 = b1
    return status


# ---------------------------------------------------------------------------------------------------
# Baseline JPEG files written on the device (yolov6/utils/jpeg.py is the specification; lp_jpeg_encode_batch)
#: encode_jpeg_padded: the workspace of one lp_jpeg_encode_batch call stays under this many bytes (a 4K frame takes 25 MB)
JPEG_WS_CAP = 256 << 20
#: 'retries': frames ``encode_jpeg`` encoded a second time because their file did not fit the first capacity
jpeg_stats = {'retries': 0}
_jpeg_ws = {}


def _jpeg_sources(frames):
    """The frames of one ``encode_jpeg`` call as (device, flat list of [h,w,3] tensors and 'bt601f' ``Nv12Frame``s): uint8 CUDA BGR
    tensors [h,w,3] of any sizes whose pixels are contiguous (a row pitch above 3 w is fine: views of a larger tensor), [n,h,w,3]
    tensors (n frames each), or ``Nv12Frame``s with CUDA planes; NV12 frames of a matrix other than 'bt601f' are converted to
    BGR frames here (``nv12_to_bgr``)."""
    if torch.is_tensor(frames):
        frames = [frames]
    flat = []
    for f in frames:
        if torch.is_tensor(f) and f.dim() == 4:
            flat.extend(f[k] for k in range(f.shape[0]))
        else:
            flat.append(f)
    if not flat:
        raise ValueError('encode_jpeg needs at least one frame')
    dev = flat[0].device
    other = [k for k, f in enumerate(flat) if isinstance(f, Nv12Frame) and f.matrix != 'bt601f']
    if other:
        for k, bgr in zip(other, nv12_to_bgr([flat[k] for k in other])):
            flat[k] = bgr
    for f in flat:
        if isinstance(f, Nv12Frame):
            if not (f.is_cuda and f.device == dev):
                raise ValueError('NV12 frames must be Nv12Frame objects with CUDA planes on one device')
            continue
        if not (torch.is_tensor(f) and f.is_cuda and f.device == dev and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3
                and f.shape[0] >= 1 and f.shape[1] >= 1 and f.stride(2) == 1 and f.stride(1) == 3 and f.stride(0) >= 3 * f.shape[1]):
            raise ValueError('frames must be uint8 CUDA BGR tensors [h, w, 3] (rows may be pitched) or [n, h, w, 3], on one device')
    for f in flat:
        if not (1 <= f.shape[0] <= 65535 and 1 <= f.shape[1] <= 65535):
            raise ValueError('JPEG sizes are 1..65535, got %d x %d' % (f.shape[0], f.shape[1]))
    return dev, flat


def encode_jpeg_padded(frames, quality=90, restart=16, cap=None):
    """Baseline JPEG files of device frames, left on the device (lp_jpeg_encode_batch, four launches per 32 frames on the current
    stream, no host read): (out uint8 [n, cap], nbytes int32 [n]); ``out[k, :nbytes[k]]`` is the complete file of frame k, byte
    for byte ``yolov6.utils.jpeg.encode_jpeg_np`` of it.  ``frames``: see ``encode_jpeg``.  ``cap``: bytes per file (None:
    ``h * w * 3 // 4 + 4096`` of the largest frame); a file that needs more leaves ``nbytes[k] = -needed`` and nothing written.
    The frames go in runs whose workspace (3 bytes per padded pixel) stays under ``JPEG_WS_CAP``."""
    from yolov6.utils.jpeg import check_params, jpeg_header
    quality, restart = check_params(quality, restart, device=True)
    dev, flat = _jpeg_sources(frames)
    n = len(flat)
    if cap is None:
        cap = max(f.shape[0] * f.shape[1] for f in flat) * 3 // 4 + 4096
    cap = int(cap)
    if not 1 <= cap < 1 << 31:
        raise ValueError('cap must be in 1..2^31-1, got %d' % cap)
    heads = np.stack([np.frombuffer(jpeg_header(f.shape[0], f.shape[1], quality, restart), np.uint8) for f in flat])
    desc = (abi.JpegDesc * n)()
    for d, f in zip(desc, flat):
        if isinstance(f, Nv12Frame):
            d.p0, d.p1, d.pitch0, d.pitch1, d.format, d.matrix = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, 1, f.matrix_id
        else:
            d.p0, d.p1, d.pitch0, d.pitch1, d.format, d.matrix = f.data_ptr(), None, f.stride(0), 0, 0, 0
        d.h0, d.w0 = f.shape[0], f.shape[1]
    lib, params = abi.load(), abi.JpegParams(quality, restart)
    with torch.cuda.device(dev):
        headers = torch.from_numpy(heads).to(dev)
        out = torch.empty((n, cap), dtype=torch.uint8, device=dev)
        nbytes = torch.empty(n, dtype=torch.int32, device=dev)
        ws_of = [(f.shape[0] + 15) // 16 * ((f.shape[1] + 15) // 16) * 776 + 16 for f in flat]     # an upper bound per frame
        b0 = 0
        while b0 < n:
            b1, total = b0 + 1, ws_of[b0]
            while b1 < n and total + ws_of[b1] <= JPEG_WS_CAP:
                total += ws_of[b1]
                b1 += 1
            run = ctypes.cast(ctypes.byref(desc, b0 * ctypes.sizeof(abi.JpegDesc)), ctypes.POINTER(abi.JpegDesc))
            need = lib.lp_jpeg_workspace_bytes(run, b1 - b0, restart)
            ws = _stream_workspace(_jpeg_ws, dev, need)
            abi.check(lib.lp_jpeg_encode_batch(run, b1 - b0, ctypes.byref(params), _dptr(headers[b0:b1]), heads.shape[1], _dptr(out[b0:b1]),
                                               cap, _dptr(nbytes[b0:b1]), _aligned(ws), need, _stream_ptr(dev)), 'lp_jpeg_encode_batch')
            b0 = b1
    return out, nbytes


def encode_jpeg(frames, quality=90, restart=16, cap=None):
    """Baseline JPEG files (a list of ``bytes``) of device frames: 4:2:0, the Annex K tables scaled by ``quality`` 1..100 as
    libjpeg scales them, restart intervals of ``restart`` MCUs (1..32).  ``frames``: a list of uint8 CUDA BGR tensors [h,w,3] of
    any sizes (rows may be pitched: views of a larger tensor), of [n,h,w,3] crop tensors, or of ``Nv12Frame``s with CUDA planes
    ('bt601f' planes feed the transform as they are; the other matrices are converted to a BGR frame first); a single tensor is
    a list of one.  Two host reads: ``nbytes``, then the used bytes.  ``cap`` as ``encode_jpeg_padded``; a frame whose file does
    not fit is encoded again at the capacity it reported, counted in ``jpeg_stats['retries']``."""
    dev, flat = _jpeg_sources(frames)
    out, nbytes = encode_jpeg_padded(flat, quality, restart, cap)
    nb = nbytes.cpu().tolist()
    files = [None] * len(flat)
    again = [k for k, v in enumerate(nb) if v < 0]
    if again:
        jpeg_stats['retries'] += len(again)
        for k, data in zip(again, encode_jpeg([flat[k] for k in again], quality, restart, max(-nb[k] for k in again))):
            files[k] = data
    most = max([v for v in nb if v > 0], default=0)
    if most:
        host = out[:, :most].cpu().numpy()
        for k, v in enumerate(nb):
            if v > 0:
                files[k] = host[k, :v].tobytes()
    return files


# ---------------------------------------------------------------------------------------------------
# Tiled detection of large frames (yolov6/core/tiles.py plans the tiles; lp_preprocess_tiles_batch / lp_merge_tiles)
def preprocess_tiles(frames, plans, img_size, stride, dtype, batch=None, out=None):
    """Letterboxed regions of device frames (lp_preprocess_tiles_batch, one launch per 64 tiles): ``plans`` is a list of
    (frame index, y0, x0, th, tw); tile k is read in place from ``frames[frame]`` (contiguous uint8 CUDA [h,w,3] BGR) and
    letterboxed to exactly ``img_size`` (the reference arithmetic of a (th, tw) image, ``auto=False``) into slot k of
    x [B,3,H,W] of ``dtype``: bit for bit what ``preprocess_frames(auto=False)`` gives for a contiguous copy of the region.
    Returns (x, geoms) with ``geoms[k]`` = (rh, rw, top, left).  ``batch`` (>= len(plans)) sets B, the slots past the tiles
    are padding (114/255); ``out``: a persistent [B,3,H,W] buffer to write."""
    dev, B = _batch_on(frames, len(plans), dtype, batch, 'preprocess_tiles')
    H, W = hw_pair(img_size)
    out = _buffer(out, (B, 3, H, W), dtype, dev)
    geoms = [letterbox_placement((th, tw), [H, W], stride, auto=False)[:4] for _, _, _, th, tw in plans]
    return _letterbox_regions(frames, plans, geoms, B, H, W, dtype, out, dev), geoms


_METRICS = {'iou': 0, 'ios': 1}


def merge_tiles_buffers(F, max_det, device):
    """New (det [F,max_det,28], count [F], src [F,max_det], workspace) of a ``merge_tiles`` of ``F`` frames: what its ``out`` takes."""
    need = abi.load().lp_merge_tiles_workspace_bytes(int(F), int(max_det))
    return _det_buffers(int(F), int(max_det), device) + (torch.empty(need + 16, dtype=torch.uint8, device=device),)


def merge_tiles(det_t, count_t, tiles, frame_shapes, thres, max_det, metric='iou', border=1, out=None):
    """Per-frame merge of per-tile detections on the device (lp_merge_tiles; no host sync): det_t [T',max_det_t,28] fp32 and
    count_t [T'] int32 hold the detections of tiles 0..len(tiles)-1 (T' >= len(tiles)) in tile-local source pixels, rounded;
    ``tiles[t]`` = (frame, y0, x0, th, tw) with a frame's tiles contiguous and frames ascending; ``frame_shapes[f]`` =
    (h, w[, c]).  Returns (det [F,max_det,28], count [F] int32, src [F,max_det] int32) in frame pixels -- the layout
    ``plate_crops`` takes.  Highest-scoring view wins; rows of one tile never suppress each other.
    ``yolov6.utils.tiles.merge_tiles_np`` is the same computation on the CPU, bit for bit, and states the rules.
    ``out``: persistent (det, count, src, workspace) of an earlier call of the same F and max_det to write instead of new tensors
    (``merge_tiles_buffers``), for callers that must not allocate."""
    _check_det_count(det_t, count_t, 'det_t', min_batch=len(tiles))
    if metric not in _METRICS:
        raise ValueError('metric must be one of %s' % sorted(_METRICS))
    dev, F, max_det = det_t.device, len(frame_shapes), int(max_det)
    if max_det < 1:
        raise ValueError('max_det must be >= 1')
    ref = (abi.TileRef * max(len(tiles), 1))()
    for r, (f, y0, x0, th, tw) in zip(ref, tiles):
        r.frame, r.y0, r.x0, r.th, r.tw = f, y0, x0, th, tw
    hw = (ctypes.c_int * max(2 * F, 1))(*[int(v) for s in frame_shapes for v in s[:2]])
    lib = abi.load()
    with torch.cuda.device(dev):
        need = lib.lp_merge_tiles_workspace_bytes(F, max_det)
        if out is None:
            det, count, src, ws = merge_tiles_buffers(F, max_det, dev)
        else:
            det, count, src, ws = out
            _check_det_count(det, count, 'out', min_batch=F)
            if det.shape != (F, max_det, abi.LP_DET_COLS) or det.device != dev or src.shape != (F, max_det) or ws.numel() < need + 16:
                raise ValueError('out must be the merge_tiles_buffers of %d frames and max_det %d on %s' % (F, max_det, dev))
        abi.check(lib.lp_merge_tiles(_dptr(det_t), _dptr(count_t), ref, len(tiles), det_t.shape[1], hw, F, float(thres),
                                     _METRICS[metric], int(border), max_det, _dptr(det), _dptr(count), _dptr(src),
                                     (ws.data_ptr() + 15) // 16 * 16, need, _stream_ptr(dev)), 'lp_merge_tiles')
    return det, count, src


_tile_inputs = {}      # (device, stream, dtype, B, H, W) -> persistent network input of the tile batches (graphs are keyed on the input pointer)


def plan_tiled(frame_shapes, img_size, max_det, tile_hw=None, overlap=0.2, overview=True, tile_max_det=None):
    """(tiles, tile_max_det) of ``detect_tiled`` for frames of ``frame_shapes``: the flat tile table (frame, y0, x0, th, tw)
    and the detections kept per tile, min(max_det, 16384 // most tiles of any frame) by default."""
    tiles = plan_frames(frame_shapes, hw_pair(img_size) if tile_hw is None else tile_hw, overlap, overview)
    most = max(tiles_per_frame(tiles, len(frame_shapes)))
    if most > abi.LP_MERGE_MAX_TILES:
        raise ValueError('%d tiles for one frame (at most %d): use larger tiles or a smaller overlap' % (most, abi.LP_MERGE_MAX_TILES))
    tmd = min(int(max_det), abi.LP_MERGE_MAX_CANDIDATES // most) if tile_max_det is None else int(tile_max_det)
    if tmd < 1:
        raise ValueError('tile_max_det must be >= 1')
    return tiles, tmd


def detect_tiles_padded(model, frames, tiles, img_size, conf_thres, iou_thres, tile_max_det, batch=32):
    """The per-tile half of ``detect_tiled``: the tiles (frame, y0, x0, th, tw) of ``frames`` in chunks of ``batch`` (the tail
    padded, so the engine is bound once) through ``preprocess_tiles`` -> ``detect_padded``, then one ``rescale_round_batch``
    over all tiles with each tile's (th, tw) as its source image.  Returns (det_t [T',tile_max_det,28], count_t [T']) on the
    device, T' = len(tiles) rounded up to a multiple of ``batch``; no host sync."""
    dev, _ = _frames_on(frames, 'detect_tiled')
    dtype = next(model.parameters()).dtype
    H, W = hw_pair(img_size)
    B = int(batch)
    if B < 1:
        raise ValueError('batch must be >= 1')
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, dtype, B, H, W)
    x = _tile_inputs.get(key)
    if x is None:
        x = _tile_inputs[key] = torch.empty(B, 3, H, W, dtype=dtype, device=dev)
    stride = int(model.stride.max())
    dets, counts = [], []
    for c0 in range(0, len(tiles), B):
        preprocess_tiles(frames, tiles[c0:c0 + B], [H, W], stride, dtype, batch=B, out=x)
        det, count, _ = detect_padded(model, x, conf_thres, iou_thres, tile_max_det)
        dets.append(det)
        counts.append(count)
    det_t = dets[0] if len(dets) == 1 else torch.cat(dets)
    count_t = counts[0] if len(counts) == 1 else torch.cat(counts)
    rescale_round_batch(det_t, count_t, (H, W), [(t[3], t[4]) for t in tiles])
    return det_t, count_t


def detect_tiled_padded(model, frames, img_size, conf_thres, iou_thres, max_det, tile_hw=None, overlap=0.2, overview=True,
                        metric='iou', border=1, batch=32, tile_max_det=None):
    """The device work of ``detect_tiled`` without its host read: (det [F,max_det,28], count [F] int32) on the device, in
    frame pixels."""
    if not frames:
        raise ValueError('detect_tiled needs at least one frame')
    shapes = [tuple(f.shape[:2]) for f in frames]
    tiles, tmd = plan_tiled(shapes, img_size, max_det, tile_hw, overlap, overview, tile_max_det)
    det_t, count_t = detect_tiles_padded(model, frames, tiles, img_size, conf_thres, iou_thres, tmd, batch)
    det, count, _ = merge_tiles(det_t, count_t, tiles, shapes, iou_thres, max_det, metric, border)
    return det, count


def detect_tiled(model, frames, img_size, conf_thres, iou_thres, max_det, tile_hw=None, overlap=0.2, overview=True, metric='iou',
                 border=1, batch=32, tile_max_det=None):
    """Detections of large frames (contiguous uint8 CUDA [h,w,3] BGR, any sizes) by tiles: every frame is sliced into
    overlapping ``tile_hw`` tiles (default: the network input size, so a tile maps 1:1 to network pixels) plus, with
    ``overview``, the whole frame (``yolov6.core.tiles.plan_tiles``); the tiles of all frames run through the engine ``batch``
    at a time; the per-tile detections are rescaled to tile pixels, shifted and merged per frame on the device
    (``merge_tiles``: threshold ``iou_thres``, ``metric`` 'iou' or 'ios', cut-plate ``border``), then ONE host read of the
    per-frame counts.  Returns a list of [n_f, 28] tensors in frame pixels.  ``tile_max_det``: detections kept per tile
    (default min(max_det, 16384 // most tiles of any frame)).  With ``tile_hw`` >= the frame this is
    ``detect_frames(auto=False)``, bit for bit.  ``frames`` may be a list of ``Nv12Frame`` instead: the tiles are cut from the planes
    (lp_preprocess_nv12_batch) and the result equals that of the converted frames."""
    det, count = detect_tiled_padded(model, frames, img_size, conf_thres, iou_thres, max_det, tile_hw, overlap, overview, metric,
                                     border, batch, tile_max_det)
    return _unpad(det, count.cpu().tolist())


def detect_tiled_with_crops(model, frames, img_size, conf_thres, iou_thres, max_det, crop_hw=(64, 192), tile_hw=None, overlap=0.2,
                            overview=True, metric='iou', border=1, batch=32, tile_max_det=None):
    """``detect_tiled`` plus the plate crop of every merged detection, cut from the full-resolution frame: (dets, crops, status)
    packed as ``detect_frames_with_crops`` packs them (``plate_crops`` on the merged det / count, which have its layout)."""
    crop_hw = _crop_size(crop_hw)
    det, count = detect_tiled_padded(model, frames, img_size, conf_thres, iou_thres, max_det, tile_hw, overlap, overview, metric,
                                     border, batch, tile_max_det)
    return _unpad_with_crops(frames, det, count, crop_hw)


class TileGate:
    """Tiled detection of fixed-camera streams that runs the network only on the tiles that changed (lp_tile_gate_luma_batch,
    lp_tile_gate_update; ``yolov6.utils.tile_gate`` states the rule and ``TileGateNp`` there is the same class on the CPU).
    ``frame_shapes[s]`` is the fixed (h, w) of camera stream s; the tile plan of every stream is ``plan_tiled``'s, made once; the
    other arguments are ``detect_tiled``'s, plus the rule's ``thres`` (luma levels per pixel a 16 x 16 cell must change by),
    ``min_cells`` (changed cells that flag a tile) and ``refresh`` (calls after which a tile is detected again anyway, 0: never).
    The object owns the device tile table, the per-tile reference block sums and ages, the block grids of the current frames, the
    flags, and a detection cache per stream -- ``cache_det`` [S,Tmax,tile_max_det,28] fp32 and ``cache_count`` [S,Tmax] int32,
    tile-local rounded rows as ``detect_tiles_padded`` returns them.

    ``detect_padded(frames, stream_of=None)`` -> (det [F,max_det,28], count [F] int32) on the device, in frame pixels, with the
    shape and meaning of ``detect_tiled_padded``'s: what ``PlateTracker.update``, ``plate_crops``, ``redact_plates`` and
    ``LookbackRedactor`` take.  ``frames``: BGR device tensors or ``Nv12Frame``s (one kind), frame f of stream ``stream_of[f]``
    (default f); every stream at most once per call, every frame of its stream's shape.  A frame of stream -1 is not gated: it
    goes through ``detect_tiled_padded`` as it is and nothing of it is kept.  Per call: the luma kernel, the update kernel, ONE
    HOST READ of the flags and changed-cell counts (5 bytes per tile slot; the host builds the tile batches, so it must know),
    ``detect_tiles_padded`` on the flagged tiles only (no forward when nothing is flagged), their rows into the cache, the
    call's tiles gathered from the cache, ``merge_tiles`` over the full tile table.  With every tile flagged the result is
    ``detect_tiled_padded``'s bit for bit (with ``tile_max_det`` derived from the streams' plans; the engine computes a tile's rows
    independently of its batch slot).  A steady call allocates nothing on the device; the returned tensors are persistent per
    combination of streams: a later call with the same ``stream_of`` overwrites them.
    ``last_flags`` / ``last_ncell``: per frame of the last call the host lists over its tiles (a frame of stream -1: all 1 / 0);
    ``stats``: calls, tiles_seen, tiles_detected, forwards, summed since construction.
    ``illum='gain'`` (lp_tile_gate_update_gain) tolerates exposure and daylight drift: the cells of a tile are compared after the
    reference is scaled by the tile's gain, the median of its cells' gains, within [1 / ``max_gain``, ``max_gain``]; outside that
    range the tile is detected again.  The one host read then carries 9 bytes per slot; ``last_gain`` holds the Q12 gains of
    the last call (4096 = 1; 0: no estimate -- a never-detected tile, a frame of stream -1, and always with ``illum='none'``), and
    ``stats`` has ``tiles_out_of_range`` as well."""

    def __init__(self, model, frame_shapes, img_size, conf_thres, iou_thres, max_det, tile_hw=None, overlap=0.2, overview=True,
                 metric='iou', border=1, batch=32, tile_max_det=None, thres=2.0, min_cells=1, refresh=50, illum='none', max_gain=1.5):
        from yolov6.utils import tile_gate as tg
        self.thres16, self.min_cells, self.refresh = tg.check_params(thres, min_cells, refresh)
        self.gain_lo, self.gain_hi = tg.check_illum(illum, max_gain)
        self.illum = illum
        if metric not in _METRICS:
            raise ValueError('metric must be one of %s' % sorted(_METRICS))
        self.model, self.img_size = model, img_size
        self.conf_thres, self.iou_thres, self.max_det = conf_thres, iou_thres, int(max_det)
        self.tile_hw, self.overlap, self.overview, self.metric, self.border, self.batch = tile_hw, overlap, overview, metric, border, int(batch)
        self.shapes = [(int(s[0]), int(s[1])) for s in frame_shapes]
        if not self.shapes:
            raise ValueError('TileGate needs at least one stream')
        tiles, self.tile_max_det = plan_tiled(self.shapes, img_size, max_det, tile_hw, overlap, overview, tile_max_det)
        self._arg_tile_max_det = tile_max_det
        S = self.n_streams = len(self.shapes)
        self.plans = [[t[1:] for t in tiles if t[0] == s] for s in range(S)]
        Tmax = self.max_tiles = max(len(p) for p in self.plans)
        dev = next(model.parameters()).device
        if dev.type != 'cuda':
            raise ValueError('TileGate runs on a GPU (TileGateNp is the CPU form)')
        self.device = dev
        W = abi.LP_TILE_GATE_TILE_WORDS
        table = np.zeros((S, Tmax, W), np.int32)
        off = 0
        for s, plan in enumerate(self.plans):
            for t, tile in enumerate(plan):
                by0, by1, bx0, bx1 = tg.tile_blocks(tile)
                table[s, t, :5] = tile + (off,)
                off += (by1 - by0 + 1) * (bx1 - bx0 + 1)
        if off >= 1 << 31:
            raise ValueError('TileGate: the reference block sums of these streams exceed 2^31 entries')
        self._ref_elems = off
        self._n_tiles = (ctypes.c_int * S)(*[len(p) for p in self.plans])
        with torch.cuda.device(dev):
            self._table = torch.from_numpy(table).to(dev)
            self.ref = torch.zeros(off, dtype=torch.int16, device=dev)           # uint16 bit patterns
            self.age = torch.full((S, Tmax), -1, dtype=torch.int32, device=dev)
            cells = [tg.grid_shape(h, w) for h, w in self.shapes]
            starts = np.cumsum([0] + [(a * b + 7) // 8 * 8 for a, b in cells])
            self._grids = torch.zeros(int(starts[-1]), dtype=torch.int16, device=dev)
            self._grid_ptr = [self._grids.data_ptr() + 2 * int(o) for o in starts[:-1]]
            # ncell int32 [S*Tmax], in gain mode gain int32 [S*Tmax], then flag uint8 [S*Tmax]: one read
            self._out_words = 2 if illum == 'gain' else 1
            nb = (4 * self._out_words + 1) * S * Tmax
            self._out = torch.zeros(nb, dtype=torch.uint8, device=dev)
            self._out_host = torch.zeros(nb, dtype=torch.uint8).pin_memory()
            self.cache_det = torch.zeros(S, Tmax, self.tile_max_det, abi.LP_DET_COLS, dtype=torch.float32, device=dev)
            self.cache_count = torch.zeros(S, Tmax, dtype=torch.int32, device=dev)
        self._calls = {}
        self.last_flags, self.last_ncell, self.last_gain = [], [], []
        self.stats = dict(calls=0, tiles_seen=0, tiles_detected=0, forwards=0)
        if illum == 'gain':
            self.stats['tiles_out_of_range'] = 0

    def reset(self, streams=None):
        """Forget ``streams`` (all for None): their tiles count as never detected and their cached rows are cleared."""
        for s in (range(self.n_streams) if streams is None else streams):
            self.age[int(s)].fill_(-1)
            self.cache_det[int(s)].zero_()
            self.cache_count[int(s)].zero_()

    def _call_buffers(self, streams):
        """The persistent buffers of the calls whose gated frames are of ``streams``, in that order."""
        def make():
            idx = [s * self.max_tiles + t for s in streams for t in range(len(self.plans[s]))]
            tiles = [(k,) + tuple(tile) for k, s in enumerate(streams) for tile in self.plans[s]]
            dev = self.device
            return dict(idx=torch.tensor(idx, dtype=torch.int64, device=dev), tiles=tiles, shapes=[self.shapes[s] for s in streams],
                        det_t=torch.empty(len(idx), self.tile_max_det, abi.LP_DET_COLS, dtype=torch.float32, device=dev),
                        count_t=torch.empty(len(idx), dtype=torch.int32, device=dev),
                        merge=merge_tiles_buffers(len(streams), self.max_det, dev))
        return _persistent(self._calls, tuple(streams), make)

    def _describe(self, frames, streams, nv12):
        """The lp_tile_gate_desc array of ``frames`` (of ``streams``, one kind): planes, sizes and each stream's block grid."""
        desc = (abi.TileGateDesc * len(frames))()
        for d, fr, s in zip(desc, frames, streams):
            if nv12:
                d.p0, d.pitch0, d.format = fr.y.data_ptr(), fr.pitch_y, 1
            else:
                d.p0, d.pitch0, d.format = fr.data_ptr(), 3 * fr.shape[1], 0
            d.h0, d.w0, d.blocks = fr.shape[0], fr.shape[1], self._grid_ptr[s]
        return desc

    def _luma(self, desc):
        """lp_tile_gate_luma_batch on the current stream: the block sums of the described frames into their streams' grids."""
        abi.check(abi.load().lp_tile_gate_luma_batch(desc, len(desc), _stream_ptr(self.device)), 'lp_tile_gate_luma_batch')

    def _update(self, desc, streams):
        """lp_tile_gate_update on the current stream: flags and changed-cell counts of the call into ``_out``, ref and age moved on."""
        S, Tmax, n = self.n_streams, self.max_tiles, len(streams)
        head = (desc, n, (ctypes.c_int * n)(*streams), S, _dptr(self._table), self._n_tiles, Tmax, _dptr(self.ref), self._ref_elems,
                _dptr(self.age), self.thres16, self.min_cells, self.refresh)
        flag = ctypes.c_void_p(self._out.data_ptr() + 4 * self._out_words * S * Tmax)
        if self.illum == 'gain':
            gain = ctypes.c_void_p(self._out.data_ptr() + 4 * S * Tmax)
            abi.check(abi.load().lp_tile_gate_update_gain(*head, self.gain_lo, self.gain_hi, flag, _dptr(self._out), gain,
                                                          _stream_ptr(self.device)), 'lp_tile_gate_update_gain')
        else:
            abi.check(abi.load().lp_tile_gate_update(*head, flag, _dptr(self._out), _stream_ptr(self.device)), 'lp_tile_gate_update')

    def detect_padded(self, frames, stream_of=None):
        from yolov6.utils import tile_gate as tg
        if not frames:
            raise ValueError('TileGate.detect_padded needs at least one frame')
        frames = list(frames)
        dev, nv12 = _frames_on(frames, 'TileGate')
        if dev != self.device:
            raise ValueError('TileGate: the frames must be on the model\'s device %s' % self.device)
        so = tg.check_streams(stream_of, len(frames), self.n_streams)
        gated = [f for f, s in enumerate(so) if s >= 0]
        for f in gated:
            if tuple(frames[f].shape[:2]) != self.shapes[so[f]]:
                raise ValueError('TileGate: a frame of %s on stream %d, whose frames are %s: a stream has one fixed frame size'
                                 % (tuple(frames[f].shape[:2]), so[f], self.shapes[so[f]]))
        S, Tmax, n = self.n_streams, self.max_tiles, len(gated)
        flags, ncell, gains = [None] * len(frames), [None] * len(frames), [None] * len(frames)
        det_g = count_g = None
        todo = []
        with torch.cuda.device(dev):
            if gated:
                streams = [so[f] for f in gated]
                desc = self._describe([frames[f] for f in gated], streams, nv12)
                self._luma(desc)
                self._update(desc, streams)
                self._out_host.copy_(self._out, non_blocking=True)
                torch.cuda.current_stream(dev).synchronize()          # the one host read of a call: the host builds the tile batches
                host = self._out_host.numpy()
                words = host[:4 * self._out_words * S * Tmax].view(np.int32).reshape(self._out_words, S, Tmax)
                nc_all, fl_all = words[0], host[4 * self._out_words * S * Tmax:].reshape(S, Tmax)
                for k, f in enumerate(gated):
                    nt = len(self.plans[so[f]])
                    flags[f], ncell[f] = fl_all[k, :nt].tolist(), nc_all[k, :nt].tolist()
                    gains[f] = words[1][k, :nt].tolist() if self.illum == 'gain' else [0] * nt
                    if min(ncell[f]) < 0:
                        raise RuntimeError('TileGate: the device tile table of stream %d is damaged' % so[f])
                    todo += [(f, t) for t in range(nt) if flags[f][t]]
                if todo:
                    tiles = [(f,) + tuple(self.plans[so[f]][t]) for f, t in todo]
                    det_t, count_t = detect_tiles_padded(self.model, frames, tiles, self.img_size, self.conf_thres, self.iou_thres,
                                                         self.tile_max_det, self.batch)
                    dst = torch.tensor([so[f] * Tmax + t for f, t in todo], dtype=torch.int64, device=dev)
                    self.cache_det.view(S * Tmax, self.tile_max_det, abi.LP_DET_COLS).index_copy_(0, dst, det_t[:len(todo)])
                    self.cache_count.view(-1).index_copy_(0, dst, count_t[:len(todo)])
                buf = self._call_buffers(streams)
                torch.index_select(self.cache_det.view(S * Tmax, self.tile_max_det, abi.LP_DET_COLS), 0, buf['idx'], out=buf['det_t'])
                torch.index_select(self.cache_count.view(-1), 0, buf['idx'], out=buf['count_t'])
                det_g, count_g, _ = merge_tiles(buf['det_t'], buf['count_t'], buf['tiles'], buf['shapes'], self.iou_thres, self.max_det,
                                                self.metric, self.border, out=buf['merge'])
            self.stats['calls'] += 1
            self.stats['tiles_seen'] += sum(len(self.plans[so[f]]) for f in gated)
            self.stats['tiles_detected'] += len(todo)
            self.stats['forwards'] += -(-len(todo) // self.batch)
            if self.illum == 'gain':
                self.stats['tiles_out_of_range'] += tg.count_out_of_range([gains[f] for f in gated], self.gain_lo, self.gain_hi)
            if n == len(frames):
                self.last_flags, self.last_ncell, self.last_gain = flags, ncell, gains
                return det_g, count_g
            # frames of stream -1: not gated, nothing kept
            loose = [f for f, s in enumerate(so) if s < 0]
            lf = [frames[f] for f in loose]
            det_u, count_u = detect_tiled_padded(self.model, lf, self.img_size, self.conf_thres, self.iou_thres, self.max_det, self.tile_hw,
                                                 self.overlap, self.overview, self.metric, self.border, self.batch, self._arg_tile_max_det)
            for f, fr in zip(loose, lf):
                nt = len(plan_tiled([tuple(fr.shape[:2])], self.img_size, self.max_det, self.tile_hw, self.overlap, self.overview)[0])
                flags[f], ncell[f], gains[f] = [1] * nt, [0] * nt, [0] * nt
                self.stats['tiles_seen'] += nt
                self.stats['tiles_detected'] += nt
                self.stats['forwards'] += -(-nt // self.batch)
            det = torch.zeros(len(frames), self.max_det, abi.LP_DET_COLS, dtype=torch.float32, device=dev)
            count = torch.zeros(len(frames), dtype=torch.int32, device=dev)
            if gated:
                g = torch.tensor(gated, dtype=torch.int64, device=dev)
                det[g], count[g] = det_g, count_g
            u = torch.tensor(loose, dtype=torch.int64, device=dev)
            det[u], count[u] = det_u, count_u
        self.last_flags, self.last_ncell, self.last_gain = flags, ncell, gains
        return det, count

    def detect(self, frames, stream_of=None):
        """``detect_padded`` unpadded: a list of [n_f, 28] tensors (copies), with one more host read, of the counts, as
        ``detect_tiled`` has."""
        det, count = self.detect_padded(frames, stream_of)
        return [d.clone() for d in _unpad(det, count.cpu().tolist())]


# ---------------------------------------------------------------------------------------------------
# Plate tracking across video frames (lp_track_update; yolov6/utils/track.py states the rules)
def _host_lists(stream_of, B, flush=None):
    """The host lists of a per-stream call as the C ABI takes them: (stream_of as int [max(B, 1)], flush as a pointer to one byte
    per stream, or None)."""
    so = (ctypes.c_int * max(B, 1))(*stream_of)
    return so, None if flush is None else ctypes.cast((ctypes.c_ubyte * len(flush))(*flush), ctypes.c_void_p)


def _zero_streams(state, n_streams, streams):
    """Zero the part of ``streams`` (all for None) in a state tensor of ``n_streams`` equal parts."""
    st = state.view(n_streams, -1)
    if streams is None:
        st.zero_()
    else:
        for s in streams:
            st[int(s)].zero_()


def _persistent(cache, key, make):
    """``cache[key]``, from ``make()`` at the first use of the key: the persistent buffers of one call shape."""
    buf = cache.get(key)
    if buf is None:
        buf = cache[key] = make()
    return buf


class Watchlist:
    """A watchlist on the device (lp_watch_match; ``yolov6.utils.watch`` states the rule and ``watch_match_np`` there is the
    same computation on the CPU, on every int32): ``entries`` [N,8] ids (0..63, 255 = wildcard; ``watch.parse_watchlist`` reads
    a file), ``confuse`` [3,64,64] sixteenths or None (``watch.confuse_table``).  Validated and uploaded once; a changed list is
    a new object.  ``n``: its length; ``entries_np`` / ``confuse_np``: the checked host copies."""

    def __init__(self, entries, confuse=None, device='cuda'):
        from yolov6.utils import watch
        self.entries_np = watch.check_entries(entries)
        self.confuse_np = None if confuse is None else watch.check_confuse(confuse)
        self.n = len(self.entries_np)
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise ValueError('Watchlist lives on a GPU (watch_match_np is the CPU form)')
        self.device = torch.device('cuda', torch.cuda.current_device() if dev.index is None else dev.index)
        self.entries = torch.from_numpy(self.entries_np).to(self.device)
        self.confuse = None if self.confuse_np is None else torch.from_numpy(self.confuse_np).to(self.device)
        self._out = {}

    def buffers(self, S, max_ended):
        """The persistent (match_i [S,max_ended,4] int32, workspace) of a ``match`` of that shape."""
        key = (int(S), int(max_ended))
        need = abi.load().lp_watch_workspace_bytes(*key)
        return _persistent(self._out, key, lambda: (torch.empty(key[0], key[1], 4, dtype=torch.int32, device=self.device),
                                                    torch.empty(need + 256, dtype=torch.uint8, device=self.device)))

    def match(self, ended_i, ended_f, ended_count, max_mismatch=1, max_cost=None):
        """match_i [S,max_ended,4] int32 = (entry, mismatches, cost, n_hits) per line of the ended records of a
        ``PlateTracker.update`` (device tensors), enqueued on the current stream with no host read: the accepted entry of the
        smallest (cost, index), -1 for none, and how many were accepted.  ``max_mismatch`` 0..8; ``max_cost``: a float in fully
        confident mismatches (``watch.cost_units`` makes it the integer of the rule; None: no limit).  Persistent buffers per
        (S, max_ended): a later call of the same shape overwrites what the earlier one returned."""
        from yolov6.utils import watch
        return self._match(ended_i, ended_f, ended_count, *watch.check_params(max_mismatch, watch.cost_units(max_cost)))

    def _match(self, ended_i, ended_f, ended_count, mm, mc):
        """``match`` with the two limits as the checked integers of the rule."""
        if ended_i.dim() != 3 or ended_i.shape[2] != 12 or ended_i.dtype != torch.int32 or ended_f.shape != ended_i.shape \
                or ended_f.dtype != torch.float32 or ended_count.dtype != torch.int32 or ended_count.shape != ended_i.shape[:1]:
            raise ValueError('ended_i int32 / ended_f fp32 must be [S,max_ended,12] and ended_count int32 [S]')
        for t in (ended_i, ended_f, ended_count):
            if t.device != self.device or not t.is_contiguous():
                raise ValueError('the ended records must be contiguous tensors on the watchlist\'s device %s' % self.device)
        S, max_ended = ended_i.shape[:2]
        match_i, ws = self.buffers(S, max_ended)
        base = _aligned(ws)
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_watch_match(_dptr(self.entries), self.n, _dptr(self.confuse), _dptr(ended_i), _dptr(ended_f),
                                                _dptr(ended_count), S, max_ended, mm, mc, _dptr(match_i), ctypes.c_void_p(base),
                                                ws.numel() - (base - ws.data_ptr()), _stream_ptr(self.device)), 'lp_watch_match')
        return match_i


class SightLog:
    """A log of sightings on the device (lp_sight_update; ``yolov6.utils.sight`` states the rule and ``sight_update_np`` there is
    the same computation on the CPU, on every int32): a ring of ``capacity`` reads of ``n_streams`` streams that one call scans
    for the earlier sightings of the reads that end and then appends them to.  ``confuse`` [3,64,64] sixteenths or None
    (``watch.confuse_table``); ``pair`` uint8 [S,S] or None: pair[s_read][s_entry] != 0 lets entries of stream s_entry match reads
    of stream s_read.  The object owns the zeroed state (int32 [1 + capacity, 8]) and persistent output buffers per
    (S, max_ended)."""

    def __init__(self, capacity, n_streams, confuse=None, pair=None, device='cuda'):
        from yolov6.utils import sight, watch
        self.capacity, self.n_streams = sight.check_log(capacity, n_streams)
        self.confuse_np = None if confuse is None else watch.check_confuse(confuse)
        self.pair_np = sight.check_pair(pair, self.n_streams)
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise ValueError('SightLog lives on a GPU (SightLogNp is the CPU form)')
        self.device = torch.device('cuda', torch.cuda.current_device() if dev.index is None else dev.index)
        self.confuse = None if self.confuse_np is None else torch.from_numpy(self.confuse_np).to(self.device)
        self.pair = None if self.pair_np is None else torch.from_numpy(self.pair_np).to(self.device)
        nbytes = abi.load().lp_sight_state_bytes(self.capacity)
        #: int32 [1 + capacity, 8] on the device: the header row and one row per slot
        self.state = torch.zeros(nbytes // 4, dtype=torch.int32, device=self.device).view(1 + self.capacity, 8)
        self._now = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._bound = 0          # no fewer than the appends since the last clear: every call adds its lines
        self._out = {}

    @property
    def total(self):
        """The reads appended since the last ``clear`` (a host read, outside the hot path)."""
        return int(self.state[0, 0].item())

    def clear(self):
        """Empty the log."""
        self.state.zero_()
        self._bound = 0

    def buffers(self, S, max_ended):
        """The persistent (sight_i [S,max_ended,8] int32, workspace) of an ``update`` of that shape."""
        key = (int(S), int(max_ended))
        need = abi.load().lp_sight_workspace_bytes(*key)
        return _persistent(self._out, key, lambda: (torch.empty(key[0], key[1], 8, dtype=torch.int32, device=self.device),
                                                    torch.empty(need + 256, dtype=torch.uint8, device=self.device)))

    def update(self, ended_i, ended_f, ended_count, now, window, min_hits=1, max_mismatch=1, max_cost=None):
        """sight_i [S,max_ended,8] int32 = (slot, mismatches, cost, n_hits, prev_stream, prev_id, prev_stamp, prev_seq) per line of
        the ended records of a ``PlateTracker.update`` (device tensors): the best earlier sighting within ``window`` of ``now`` of
        every read of at least ``min_hits`` hits, (-1, 0, 0, 0, -1, -1, 0, 0) for none; then the reads are appended.  Enqueued on the
        current stream with no host read.  ``now``: an int (copied into a buffer of the log's with one enqueued copy) or a device
        int32 [1] that the call reads in place; ``max_cost``: a float in fully confident mismatches (None: no limit).  Persistent
        buffers per (S, max_ended): a later call of the same shape overwrites what the earlier one returned."""
        from yolov6.utils import sight, watch
        mm, mc = watch.check_params(max_mismatch, watch.cost_units(max_cost))
        if torch.is_tensor(now):
            _, window, min_hits = sight.check_call(0, window, min_hits)
        else:
            now, window, min_hits = sight.check_call(now, window, min_hits)
            self._now.fill_(now)
            now = self._now
        return self._update(ended_i, ended_f, ended_count, now, window, min_hits, mm, mc)

    def _update(self, ended_i, ended_f, ended_count, now, window, min_hits, mm, mc):
        """``update`` with ``now`` on the device and the parameters as the checked integers of the rule."""
        if ended_i.dim() != 3 or ended_i.shape[2] != 12 or ended_i.dtype != torch.int32 or ended_f.shape != ended_i.shape \
                or ended_f.dtype != torch.float32 or ended_count.dtype != torch.int32 or ended_count.shape != ended_i.shape[:1]:
            raise ValueError('ended_i int32 / ended_f fp32 must be [S,max_ended,12] and ended_count int32 [S]')
        if now.dtype != torch.int32 or now.numel() != 1:
            raise ValueError('now must be an int or a device int32 [1]')
        for t in (ended_i, ended_f, ended_count, now):
            if t.device != self.device or not t.is_contiguous():
                raise ValueError('the ended records and now must be contiguous tensors on the log\'s device %s' % self.device)
        S, max_ended = ended_i.shape[:2]
        if S != self.n_streams:
            raise ValueError('the ended records must have the log\'s %d streams' % self.n_streams)
        from yolov6.utils.sight import MAX_APPENDS
        if self._bound + S * max_ended > MAX_APPENDS:
            raise RuntimeError('the log takes fewer than 2^31 appends between clears: clear() it')
        self._bound += S * max_ended
        sight_i, ws = self.buffers(S, max_ended)
        base = _aligned(ws)
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_sight_update(_dptr(self.state), self.capacity, _dptr(self.confuse), _dptr(self.pair), _dptr(ended_i),
                                                 _dptr(ended_f), _dptr(ended_count), S, max_ended, _dptr(now), window, min_hits, mm, mc,
                                                 _dptr(sight_i), ctypes.c_void_p(base), ws.numel() - (base - ws.data_ptr()),
                                                 _stream_ptr(self.device)), 'lp_sight_update')
        return sight_i


class PlateTracker:
    """``n_streams`` independent device-resident plate trackers of ``max_tracks`` slots each (lp_track_update, one workgroup per
    stream): detections of consecutive frames are associated by the IoU of expanded, velocity-predicted boxes
    (``match_thres``, ``expand``), a row that matches nothing and scores at least ``new_thres`` starts a track, a track unseen
    for more than ``max_age`` frames ends, and every track votes its eight character heads over its frames, weighted by
    confidence.  ``ncls``: the eight head widths, a model, or None for the shipped configs' (31, 24, 37 x 6).  The object owns
    the zeroed state tensor and persistent output buffers (one set per (B, max_det, max_ended): a later ``update`` of the same
    shape overwrites what the earlier one returned).  ``yolov6.utils.track.PlateTrackerNp`` is the same computation on the
    CPU, bit for bit."""

    def __init__(self, n_streams, max_tracks=64, match_thres=0.3, new_thres=0.0, expand=0.5, max_age=5, ncls=None, device=None):
        from yolov6.utils import track
        track.check_params(n_streams, max_tracks, match_thres, new_thres, expand, max_age)
        self.n_streams, self.max_tracks, self.max_age = int(n_streams), int(max_tracks), int(max_age)
        self.ncls = track.ncls_of(ncls)
        dev = torch.device('cuda' if device is None else device)
        if dev.type != 'cuda':
            raise ValueError('PlateTracker runs on a GPU (PlateTrackerNp is the CPU form)')
        self.device = torch.device('cuda', torch.cuda.current_device() if dev.index is None else dev.index)
        self._params = abi.TrackParams(float(match_thres), float(new_thres), float(expand), self.max_age, (ctypes.c_int * 8)(*self.ncls))
        lib = abi.load()
        self._words = lib.lp_track_state_bytes(1, self.max_tracks) // 4
        self.state = torch.zeros(self.n_streams * self._words, dtype=torch.int32, device=self.device)
        self._drop_word = lib.lp_track_dropped_offset(self.max_tracks, 0) // 4
        self._out = {}
        self._slot = {}
        self._shots = None
        self._stack = None
        #: (stack_crops [S,max_ended,Hc,Wc,3] uint8, stack_i [S,max_ended,4] int32) of the last ``update_with_shots`` after
        #: ``enable_stack``, line-parallel to its ended_i, else None
        self.last_stack = None
        self._hold = None
        #: (det_hold, count_hold, tid_hold) of the last ``update`` after ``enable_hold``, else None
        self.last_hold = None
        #: the tid buffer [B,max_det] the last ``update`` filled (what ``LookbackRedactor.push`` reads), else None
        self.last_tid = None
        self._watch = None
        #: match_i [S,max_ended,4] int32 of the last ``update`` after ``enable_watch``, line-parallel to its ended_i, else None
        self.last_watch = None
        self._live = None
        #: live_i [S,max_tracks,8] int32 of the last ``update`` after ``enable_live_watch``, else None
        self.last_live = None
        #: (q_i, q_f, q_slot, q_count) of that lookup: the fresh reads in the ended-record layout, else None
        self.last_live_reads = None
        self._sight = None
        #: sight_i [S,max_ended,8] int32 of the last ``update`` after ``enable_sightings``, line-parallel to its ended_i, else None
        self.last_sight = None
        #: int32 [1] on the device: the clock of ``enable_sightings``, incremented by one per call; the caller may set it
        self.sight_now = torch.zeros(1, dtype=torch.int32, device=self.device)

    def reset(self, streams=None):
        """Zero the state of ``streams`` (all for None): no tracks, frame counter, next id and ``dropped`` at 0; their best-shot
        galleries (``enable_best_shot``) and stacks (``enable_stack``) are emptied with them, and their memo of
        ``enable_live_watch``.  The log of ``enable_sightings`` and ``sight_now`` stay as they are."""
        _zero_streams(self.state, self.n_streams, streams)
        if self._stack is not None:
            _zero_streams(self._stack['state'], self.n_streams, streams)
        if self._live is not None:
            _zero_streams(self._live['memo'], self.n_streams, streams)
        if self._shots is not None:
            _zero_streams(self._shots['state'], self.n_streams, streams)

    @property
    def dropped(self):
        """int32 [n_streams] view of the state: rows that found no free slot since the last reset (on the device)."""
        return self.state.view(self.n_streams, self._words)[:, self._drop_word]

    def update(self, det, count, stream_of=None, flush=None, max_ended=None):
        """``B`` frames: det [B,max_det,28] fp32 + count [B] int32 on the device (``detect_frames_padded`` /
        ``detect_tiled_padded`` / ``nms_padded`` layout); ``stream_of[b]`` (host ints, default ``range(B)``: one frame from
        each of B cameras) names the stream of frame b or is -1 for a frame that is not tracked; ``flush[s]`` ends the live
        tracks of stream s after its frames.  Returns (det_out [B,max_det,28], tid [B,max_det] int32, ended_i
        [S,max_ended,12] int32, ended_f [S,max_ended,12] fp32, ended_count [S] int32), all on the device, no host read: det_out
        is det with the class columns of every tracked row replaced by its track's voted read (columns 12..19 the vote
        shares, 20..27 the voted ids), tid the track id per row (-1: untracked), ended_* the tracks that ended in this call
        (id, first, last, hits, ids | shares, last box), ``max_ended`` per stream (default ``max_tracks``)."""
        from yolov6.utils import track
        _check_det_count(det, count)
        if det.device != self.device:
            raise ValueError('det must be on the tracker\'s device %s' % self.device)
        B, max_det, S = det.shape[0], det.shape[1], self.n_streams
        stream_of, flush, max_ended = track.check_call(S, B, stream_of, flush, self.max_tracks if max_ended is None else max_ended)
        out = self.buffers(B, max_det, max_ended)
        det_out, tid, ended_i, ended_f, ended_count = out
        self.last_tid = tid
        so, fl = _host_lists(stream_of, B, flush)
        hp, hold = None, (None, None, None)
        if self._hold is not None:
            hp, hold = ctypes.byref(self._hold['params']), self.hold_buffers(B, max_det)
            self.last_hold = hold
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_track_update_hold(_dptr(self.state), S, self.max_tracks, ctypes.byref(self._params), _dptr(det),
                                                      _dptr(count), B, max_det, so, fl, _dptr(det_out),
                                                      _dptr(tid), _dptr(self.slot_buffer(B, max_det)), _dptr(ended_i), _dptr(ended_f),
                                                      _dptr(ended_count), max_ended, hp, _dptr(hold[0]), _dptr(hold[1]), _dptr(hold[2]),
                                                      _stream_ptr(self.device)), 'lp_track_update_hold')
        if self._watch is not None:
            wl, mm, mc = self._watch
            self.last_watch = wl._match(ended_i, ended_f, ended_count, mm, mc)
        if self._live is not None:
            self._live_watch()
        if self._sight is not None:
            log, params = self._sight
            self.last_sight = log._update(ended_i, ended_f, ended_count, self.sight_now, *params)
            self.sight_now.add_(1)
        return out

    # ---- the ended reads matched against the earlier reads of all streams (lp_sight_update; yolov6/utils/sight.py states the rule) ----
    def enable_sightings(self, log, window=0, min_hits=1, max_mismatch=1, max_cost=None):
        """From now on every ``update`` / ``update_with_shots`` / ``flush_all*`` also enqueues, at its end on the same stream (behind
        the lookups of ``enable_watch`` and ``enable_live_watch``), lp_sight_update of the records it ended on ``log`` (a ``SightLog``
        of this device and of the tracker's ``n_streams``), and leaves sight_i [S,max_ended,8] int32 = (slot, mismatches, cost, n_hits,
        prev_stream, prev_id, prev_stamp, prev_seq), line-parallel to ended_i, in ``last_sight``.  The clock is ``sight_now``, a device
        int32 [1]: the call reads it in place and then increments it by one on the device, so that left alone it counts the
        tracker's calls; a caller with a clock of its own sets the tensor before every call (``sight_now.fill_(t)`` or a copy).
        ``window`` is in the clock's units.  No host read, no allocation per call; a caller
        that replays a captured update counts those appends itself (fewer than 2^31 between two ``log.clear()``).  Returns, state
        and every other buffer are what they are without it.  ``enable_sightings(None)`` turns it off."""
        from yolov6.utils import sight, watch
        self.last_sight = None
        if log is None:
            self._sight = None
            return
        if not isinstance(log, SightLog) or log.device != self.device or log.n_streams != self.n_streams:
            raise ValueError('enable_sightings needs a SightLog of %d streams on the tracker\'s device %s' % (self.n_streams, self.device))
        _, window, min_hits = sight.check_call(0, window, min_hits)
        self._sight = (log, (window, min_hits) + watch.check_params(max_mismatch, watch.cost_units(max_cost)))

    # ---- the live tracks looked up in a watchlist (lp_watch_live; yolov6/utils/watch_live.py states the rule) -----------------
    def enable_live_watch(self, watchlist, min_hits=3, max_mismatch=1, max_cost=None):
        """From now on every ``update`` / ``update_with_shots`` / ``flush_all*`` also enqueues, at its end on the same stream
        (behind the lookup of ``enable_watch`` if that is on), the lookup of the LIVE tracks of at least ``min_hits`` hits in
        ``watchlist`` (a ``Watchlist`` on this device): once per track when it gets there, and again only when its voted read
        changes; a memo per slot, owned by the tracker, holds the answers.  ``last_live`` = live_i [S,max_tracks,8] int32, one
        row per slot: (id, entry, mismatches, cost, n_hits, fresh, hits, last_at_lookup), or (-1, -1, 0, 0, 0, 0, 0, 0) for a
        slot without a looked-up track; a row with fresh == 1 and entry >= 0 is an alert.  ``last_live_reads`` = (q_i, q_f,
        q_slot, q_count): the reads looked up in this call.  Persistent buffers, no host read, no allocation per call.  Returns,
        state and every other buffer are what they are without it.  Calling it again zeroes the memo;
        ``enable_live_watch(None)`` turns it off.  ``PlateTrackerNp.enable_live_watch`` is the same on the CPU, on every int32."""
        from yolov6.utils import watch, watch_live
        self.last_live = self.last_live_reads = None
        if watchlist is None:
            self._live = None
            return
        if not isinstance(watchlist, Watchlist) or watchlist.device != self.device:
            raise ValueError('enable_live_watch needs a Watchlist on the tracker\'s device %s' % self.device)
        min_hits = watch_live.check_min_hits(min_hits)
        mm, mc = watch.check_params(max_mismatch, watch.cost_units(max_cost))
        S, T, dev, lib = self.n_streams, self.max_tracks, self.device, abi.load()
        i32 = dict(dtype=torch.int32, device=dev)
        self._live = dict(
            watchlist=watchlist, min_hits=min_hits, limits=(mm, mc), ncls=(ctypes.c_int * 8)(*self.ncls),
            memo=torch.zeros(lib.lp_watch_live_state_bytes(S, T) // 4, **i32).view(S, T, 8),
            live_i=torch.empty(S, T, 8, **i32), q_i=torch.empty(S, T, 12, **i32),
            q_f=torch.empty(S, T, 12, dtype=torch.float32, device=dev), q_slot=torch.empty(S, T, **i32), q_count=torch.empty(S, **i32),
            ws=torch.empty(lib.lp_watch_live_workspace_bytes(S, T) + 256, dtype=torch.uint8, device=dev))

    @property
    def live_memo(self):
        """The memo of ``enable_live_watch``: int32 [S,max_tracks,8] on the device (id + 1, key_lo, key_hi, entry, mismatches,
        cost, n_hits, last_at_lookup), else None."""
        return None if self._live is None else self._live['memo']

    def _live_watch(self):
        """Enqueue lp_watch_live on the state as it stands."""
        lw = self._live
        wl, ws = lw['watchlist'], lw['ws']
        base = _aligned(ws)
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_watch_live(_dptr(self.state), self.n_streams, self.max_tracks, lw['ncls'], lw['min_hits'], _dptr(lw['memo']),
                                               _dptr(wl.entries), wl.n, _dptr(wl.confuse), lw['limits'][0], lw['limits'][1], _dptr(lw['q_i']),
                                               _dptr(lw['q_f']), _dptr(lw['q_slot']), _dptr(lw['q_count']), _dptr(lw['live_i']),
                                               ctypes.c_void_p(base), ws.numel() - (base - ws.data_ptr()), _stream_ptr(self.device)),
                      'lp_watch_live')
        self.last_live = lw['live_i']
        self.last_live_reads = (lw['q_i'], lw['q_f'], lw['q_slot'], lw['q_count'])

    # ---- the ended reads looked up in a watchlist (lp_watch_match; yolov6/utils/watch.py states the rule) ----------------------
    def enable_watch(self, watchlist, max_mismatch=1, max_cost=None):
        """From now on every ``update`` / ``update_with_shots`` / ``flush_all*`` also enqueues, behind the tracker on the same
        stream, the lookup of the records it ended in ``watchlist`` (a ``Watchlist`` on this device) and leaves match_i
        [S,max_ended,4] int32 = (entry, mismatches, cost, n_hits), line-parallel to ended_i, in ``last_watch``.  ``max_cost``: a float
        in fully confident mismatches (``watch.cost_units``; None: no limit).  Returns, state and every other buffer are what
        they are without it.  ``enable_watch(None)`` turns it off."""
        from yolov6.utils import watch
        self.last_watch = None
        if watchlist is None:
            self._watch = None
            return
        if not isinstance(watchlist, Watchlist) or watchlist.device != self.device:
            raise ValueError('enable_watch needs a Watchlist on the tracker\'s device %s' % self.device)
        self._watch = (watchlist,) + watch.check_params(max_mismatch, watch.cost_units(max_cost))

    # ---- redaction held over missed frames (lp_track_update_hold; rule 11 of yolov6/utils/track.py) -----------------------------
    def enable_hold(self, min_hits=1, max_misses=None):
        """From now on every ``update`` / ``update_with_shots`` also fills ``hold_buffers`` (``last_hold``): the frame's rows
        followed by a predicted row for every track of at least ``min_hits`` hits that the frame missed, for at most
        ``max_misses`` frames in a row (None, or anything above ``max_age``: ``max_age``, where the track ends).  That is the
        (det, count) to hand ``redact_plates``, so that a plate the detector loses for a frame is still covered.  Returns,
        state and every other buffer are what they are without it."""
        min_hits, max_misses = int(min_hits), self.max_age if max_misses is None else int(max_misses)
        if min_hits < 1 or max_misses < 0:
            raise ValueError('hold needs min_hits >= 1 and max_misses >= 0')
        self._hold = dict(params=abi.TrackHoldParams(min_hits, max_misses), out={})

    def hold_buffers(self, B, max_det):
        """The persistent (det_hold [B,max_det+max_tracks,28] fp32, count_hold [B] int32, tid_hold [B,max_det+max_tracks] int32)
        an ``update`` of that shape fills after ``enable_hold`` (``PlateTrackerNp.hold_buffers``)."""
        if self._hold is None:
            raise RuntimeError('call enable_hold() first')
        B, rows, dev = int(B), int(max_det) + self.max_tracks, self.device
        return _persistent(self._hold['out'], (B, int(max_det)), lambda: (
            torch.empty(B, rows, abi.LP_DET_COLS, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
            torch.empty(B, rows, dtype=torch.int32, device=dev)))

    def slot_buffer(self, B, max_det):
        """The persistent int32 [B,max_det] tensor an ``update`` of that shape fills beside its returns: the tracker slot of each
        matched or new row's track, -1 wherever tid is -1 (``PlateTrackerNp.last_slot``)."""
        key = (int(B), int(max_det))
        return _persistent(self._slot, key, lambda: torch.empty(key, dtype=torch.int32, device=self.device))

    def buffers(self, B, max_det, max_ended=None):
        """The persistent outputs of an ``update`` of B frames of max_det rows: (det_out, tid, ended_i, ended_f, ended_count)."""
        S, dev = self.n_streams, self.device
        key = (int(B), int(max_det), self.max_tracks if max_ended is None else int(max_ended))
        return _persistent(self._out, key, lambda: (
            torch.empty(key[0], key[1], abi.LP_DET_COLS, dtype=torch.float32, device=dev),
            torch.empty(key[0], key[1], dtype=torch.int32, device=dev), torch.empty(S, key[2], 12, dtype=torch.int32, device=dev),
            torch.empty(S, key[2], 12, dtype=torch.float32, device=dev), torch.empty(S, dtype=torch.int32, device=dev)))

    def flush_all(self, max_det=1, max_ended=None):
        """End every live track of every stream: ``update`` of zero frames with every flush flag set."""
        det = torch.empty(0, int(max_det), abi.LP_DET_COLS, dtype=torch.float32, device=self.device)
        count = torch.empty(0, dtype=torch.int32, device=self.device)
        return self.update(det, count, stream_of=[], flush=[1] * self.n_streams, max_ended=max_ended)

    # ---- the best shot of every track (lp_crop_sharpness, lp_best_shot_update; yolov6/utils/best_shot.py states the rules) ----
    def enable_best_shot(self, crop_hw=(64, 192), max_crops=16, min_score=0.0):
        """Allocate the zeroed gallery: per slot the sharpest ``crop_hw`` crop its track has shown (``update_with_shots``).  The
        first ``max_crops`` rows of a frame compete; a row needs a mean confidence of at least ``min_score``."""
        Hc, Wc = _crop_size(crop_hw)
        if int(max_crops) < 1:
            raise ValueError('max_crops must be >= 1')
        if not abs(float(min_score)) <= 3.0e38:
            raise ValueError('min_score must be finite (|min_score| <= 3e38)')
        nbytes = abi.load().lp_best_shot_state_bytes(self.n_streams, self.max_tracks, Hc, Wc)
        self._stack = self.last_stack = None        # (a stack is made for the gallery's crop size: enable_stack again)
        self._shots = dict(crop_hw=(Hc, Wc), max_crops=int(max_crops), min_score=float(min_score), out={},
                           state=torch.zeros(nbytes, dtype=torch.uint8, device=self.device),
                           blank=torch.zeros(1, 1, 3, dtype=torch.uint8, device=self.device))

    def shot_buffers(self, B, max_ended=None):
        """The persistent buffers of an ``update_with_shots`` of B frames: (crops [B,max_crops,Hc,Wc,3] uint8, status
        [B,max_crops] int32, sharp [B,max_crops] int64, shot_crops [S,max_ended,Hc,Wc,3] uint8, shot_i [S,max_ended,4] int32,
        shot_q [S,max_ended] int64, shot_det [S,max_ended,28] fp32)."""
        if self._shots is None:
            raise RuntimeError('call enable_best_shot() first')
        sh, S, dev = self._shots, self.n_streams, self.device
        (Hc, Wc), m = sh['crop_hw'], sh['max_crops']
        key = (int(B), self.max_tracks if max_ended is None else int(max_ended))
        return _persistent(sh['out'], key, lambda: (
            torch.zeros(key[0], m, Hc, Wc, 3, dtype=torch.uint8, device=dev), torch.zeros(key[0], m, dtype=torch.int32, device=dev),
            torch.zeros(key[0], m, dtype=torch.int64, device=dev), torch.zeros(S, key[1], Hc, Wc, 3, dtype=torch.uint8, device=dev),
            torch.empty(S, key[1], 4, dtype=torch.int32, device=dev), torch.empty(S, key[1], dtype=torch.int64, device=dev),
            torch.empty(S, key[1], abi.LP_DET_COLS, dtype=torch.float32, device=dev)))

    def update_with_shots(self, frames, det, count, stream_of=None, flush=None, max_ended=None):
        """``update`` plus the best shot of every track that ends in it, enqueued back to back with no host read: the tracker,
        ``plate_crops`` of ``frames`` (contiguous uint8 CUDA [h,w,3] BGR, frame b of ``det``; shorter than B or None where
        ``stream_of`` is -1) along the rows of ``det`` as given, ``crop_sharpness``, then lp_best_shot_update.  Returns the five
        tensors of ``update`` followed by (shot_crops [S,max_ended,Hc,Wc,3] uint8, shot_i [S,max_ended,4] int32 = frame, row,
        status, valid; shot_q [S,max_ended] int64 holding the unsigned sharpness; shot_det [S,max_ended,28] fp32 = the shot's
        row with its per-frame confidences), line-parallel to ended_i / ended_f; persistent buffers per shape.  The crop of a
        record without a shot (valid 0) is left as it was.  yolov6.utils.best_shot.BestShotNp is the same computation on the
        CPU, bit for bit.  ``frames`` may be ``Nv12Frame``s instead: they are converted once (``nv12_to_bgr``) on this stream."""
        from yolov6.utils import track
        if self._shots is None:
            raise RuntimeError('call enable_best_shot() first')
        S, B = self.n_streams, det.shape[0]
        stream_of, _, max_ended = track.check_call(S, B, stream_of, flush, self.max_tracks if max_ended is None else max_ended)
        frames = list(frames) + [None] * (B - len(frames))
        if len(frames) != B:
            raise ValueError('%d frames for a batch of %d' % (len(frames), B))
        for b, f in enumerate(frames):
            if f is None and stream_of[b] >= 0:
                raise ValueError('frame %d of stream %d is missing' % (b, stream_of[b]))
        live = [f for f in frames if f is not None]
        if live and _frames_on(live, 'update_with_shots')[0] != self.device:
            raise ValueError('frames must be on the tracker\'s device %s' % self.device)
        frames = _bgr_frames(frames)        # an NV12 list is converted once, on this stream
        out = self.update(det, count, stream_of, flush, max_ended)
        crops, status, sharp = self._shot_crops(frames, det, count, stream_of, max_ended)
        if B:
            crop_sharpness(crops, status, out=sharp)
        shots = self._shot_gallery(det, count, stream_of, max_ended)
        if self._stack is not None:
            self.last_stack = self._stack_update(det, count, stream_of, max_ended)
        return out + shots

    def _shot_crops(self, frames, det, count, stream_of, max_ended):
        """The crop stage of ``update_with_shots``: (crops, status, sharp) of ``shot_buffers``, the first two written."""
        sh, B = self._shots, det.shape[0]
        crops, status, sharp = self.shot_buffers(B, max_ended)[:3]
        m = sh['max_crops']
        if B:
            # a frame that is not tracked takes no slots: its status keeps what an earlier call left, and nothing reads it
            off = [f is None or stream_of[b] < 0 for b, f in enumerate(frames)]
            _plate_crops_launch([sh['blank'] if o else f for o, f in zip(off, frames)], det, count,
                                [(0 if o else m, b * m) for b, o in enumerate(off)], crops, status, sh['crop_hw'])
        return crops, status, sharp

    def _shot_gallery(self, det, count, stream_of, max_ended):
        """The gallery stage of ``update_with_shots`` behind ``update`` of the same arguments: (shot_crops, shot_i, shot_q,
        shot_det)."""
        sh, S, (B, max_det) = self._shots, self.n_streams, det.shape[:2]
        crops, status, sharp, shot_crops, shot_i, shot_q, shot_det = self.shot_buffers(B, max_ended)
        _, tid, ended_i, _, ended_count = self.buffers(B, max_det, max_ended)
        so, _ = _host_lists(stream_of, B)
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_best_shot_update(_dptr(sh['state']), S, self.max_tracks, sh['crop_hw'][0], sh['crop_hw'][1], _dptr(det),
                                                     _dptr(count), B, max_det, _dptr(tid), _dptr(self.slot_buffer(B, max_det)), _dptr(crops),
                                                     _dptr(status), _dptr(sharp), sh['max_crops'], so, _dptr(ended_i), _dptr(ended_count),
                                                     max_ended, sh['min_score'], _dptr(shot_crops), _dptr(shot_i), _dptr(shot_q),
                                                     _dptr(shot_det), _stream_ptr(self.device)), 'lp_best_shot_update')
        return shot_crops, shot_i, shot_q, shot_det

    # ---- one denoised picture per track (lp_stack_update; yolov6/utils/stack.py states the rule and its limits) ------------------
    def enable_stack(self, search=2, max_frames=64, min_width=0.0, min_sharp=0):
        """From now on every ``update_with_shots`` / ``flush_all_with_shots`` also enqueues, behind the gallery on the same
        stream, lp_stack_update on the same crops: the rectified (status 1) crops of every track, at most ``max_frames`` (1..255)
        of them, each from a plate at least ``min_width`` frame pixels wide and of a sharpness of at least ``min_sharp``, are
        aligned by an integer shift of at most ``search`` (0..4) pixels and summed, and the rounded mean of a track that ends is
        left in ``last_stack`` = (stack_crops [S,max_ended,Hc,Wc,3] uint8, stack_i [S,max_ended,4] int32 = n, first_frame,
        last_frame, valid), line-parallel to ended_i; persistent buffers per shape, the crop of a record without a stack (valid 0)
        is left as it was.  It needs ``enable_best_shot`` first and shares its ``crop_hw``, ``max_crops`` and ``min_score``.  The
        nine returns, the tracker's and the gallery's state are what they are without it.  Calling it again starts from empty
        stacks; ``enable_stack(None)`` turns it off.  ``PlateTrackerNp.enable_stack`` with ``yolov6.utils.stack.StackNp`` is the
        same computation on the CPU, bit for bit."""
        from yolov6.utils import stack
        self.last_stack = None
        if search is None:
            self._stack = None
            return
        if self._shots is None:
            raise RuntimeError('call enable_best_shot() first')
        sh = self._shots
        search, max_frames, min_width, min_sharp, min_score = stack.check_params(search, max_frames, min_width, min_sharp, sh['min_score'])
        nbytes = abi.load().lp_stack_state_bytes(self.n_streams, self.max_tracks, *sh['crop_hw'])
        self._stack = dict(params=abi.StackParams(min_score, min_width, min_sharp, search, max_frames), out={},
                           state=torch.zeros(nbytes, dtype=torch.uint8, device=self.device))

    def stack_buffers(self, max_ended=None):
        """The persistent (stack_crops [S,max_ended,Hc,Wc,3] uint8, stack_i [S,max_ended,4] int32) of an ``update_with_shots``
        with that ``max_ended`` after ``enable_stack``."""
        if self._stack is None:
            raise RuntimeError('call enable_stack() first')
        S, dev, (Hc, Wc) = self.n_streams, self.device, self._shots['crop_hw']
        key = self.max_tracks if max_ended is None else int(max_ended)
        return _persistent(self._stack['out'], key, lambda: (torch.zeros(S, key, Hc, Wc, 3, dtype=torch.uint8, device=dev),
                                                             torch.empty(S, key, 4, dtype=torch.int32, device=dev)))

    def _stack_update(self, det, count, stream_of, max_ended):
        """The stack stage of ``update_with_shots`` behind the gallery stage of the same arguments: (stack_crops, stack_i)."""
        sh, sk, S, (B, max_det) = self._shots, self._stack, self.n_streams, det.shape[:2]
        crops, status, sharp = self.shot_buffers(B, max_ended)[:3]
        _, tid, ended_i, _, ended_count = self.buffers(B, max_det, max_ended)
        stack_crops, stack_i = self.stack_buffers(max_ended)
        so, _ = _host_lists(stream_of, B)
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_stack_update(_dptr(sk['state']), S, self.max_tracks, sh['crop_hw'][0], sh['crop_hw'][1], _dptr(det),
                                                 _dptr(count), B, max_det, _dptr(tid), _dptr(self.slot_buffer(B, max_det)), _dptr(crops),
                                                 _dptr(status), _dptr(sharp), sh['max_crops'], so, _dptr(ended_i), _dptr(ended_count),
                                                 max_ended, ctypes.byref(sk['params']), _dptr(stack_crops), _dptr(stack_i),
                                                 _stream_ptr(self.device)), 'lp_stack_update')
        return stack_crops, stack_i

    def flush_all_with_shots(self, max_det=1, max_ended=None):
        """``flush_all`` with the best shots of the tracks it ends: ``update_with_shots`` of zero frames."""
        det = torch.empty(0, int(max_det), abi.LP_DET_COLS, dtype=torch.float32, device=self.device)
        count = torch.empty(0, dtype=torch.int32, device=self.device)
        return self.update_with_shots([], det, count, stream_of=[], flush=[1] * self.n_streams, max_ended=max_ended)


class LookbackRedactor(LookbackHost):
    """Redaction delayed by ``depth`` frames, so that the frames BEFORE a plate's first detection are covered too
    (lp_lookback_update; ``yolov6.utils.lookback`` states the rule, and ``LookbackNp`` there is the same object on numpy).  It
    needs a ``PlateTracker`` with ``enable_hold`` called (RuntimeError otherwise).  ``max_back``: frames before the first detection
    that are covered (default ``depth``); ``back_cap``: back rows a stored frame can take (default ``max_tracks``); ``mode``,
    ``cell``, ``margin``, ``fill``, ``sigma``: as ``redact_plates``.

    ``push(frames, stream_of, flush)`` right after ``tracker.update(...)`` / ``update_with_shots(...)`` of the same frames
    enqueues lp_lookback_update on ``tracker.last_hold``, ``last_tid`` and ``slot_buffer`` and keeps REFERENCES to the frames per
    stream (BGR device tensors or ``Nv12Frame``s; no copy: the caller hands them over and must not write them until they come
    back), then redacts every frame that leaves the delay in this call with the rows released for it, one ``redact_plates`` call
    per push (plus one per flushed stream), and returns them as [(stream, frame_number, frame), ...] in release order; an
    untracked frame comes back at once as (-1, -2, frame).  Which frame leaves at which b follows from the host's own
    per-stream counters: no host read, and no allocation in the steady state (persistent buffers per update shape).
    ``flush`` / ``flush_all()`` hand the tail frames back the same way.

    Crops and best shots read the frames at update time, before any redaction of them is enqueued, so the order rule
    "redaction goes last" holds by construction."""

    def __init__(self, tracker, depth, max_back=None, back_cap=None, mode='mosaic', cell=16, margin=0.1, fill=(0, 0, 0), sigma=None):
        if not isinstance(tracker, PlateTracker):
            raise TypeError('LookbackRedactor needs a PlateTracker (LookbackNp is the CPU form)')
        self._init_host(tracker, depth, max_back, back_cap, mode, cell, margin, fill, sigma)
        self.device = tracker.device
        self.state = None          # allocated by the first push: the entries' rows follow max_det
        self._rows = None
        self._out, self._status, self._blank = {}, {}, {}

    def _slots(self):
        B, hold_rows = self.tracker.last_hold[0].shape[:2]
        return self.tracker.slot_buffer(B, hold_rows - self.max_tracks)

    def _allocated(self):
        return self.state is not None

    @property
    def entry_rows(self):
        """Rows of a stored entry (max_det + max_tracks + back_cap); None before the first push with frames."""
        return self._rows

    def _state_for(self, rows):
        if self.state is None:
            nbytes = abi.load().lp_lookback_state_bytes(self.n_streams, self.max_tracks, self.depth, rows)
            if nbytes == 0:
                raise ValueError('lookback: entries of %d rows do not fit (rows * 28 must stay below 2^31)' % rows)
            self._rows = rows
            self.state = torch.zeros(nbytes // 4, dtype=torch.int32, device=self.device)
        elif rows != self._rows:
            raise ValueError('this delay line holds entries of %d rows, the update has %d' % (self._rows, rows))
        return self.state

    def buffers(self, B, rows):
        """The persistent outputs of a push behind an update of B frames: (rel_det [B,rows,28], rel_count [B], rel_frame [B],
        tail_det [S,D,rows,28], tail_count [S,D], tail_frame [S,D])."""
        key, S, D, dev = (int(B), int(rows)), self.n_streams, self.depth, self.device

        def make():                             # the tails do not depend on B: every shape shares the first one's
            tails = next(iter(self._out.values()))[3:] if self._out else (
                torch.empty(S, D, key[1], abi.LP_DET_COLS, dtype=torch.float32, device=dev),
                torch.empty(S, D, dtype=torch.int32, device=dev), torch.empty(S, D, dtype=torch.int32, device=dev))
            return (torch.empty(key[0], key[1], abi.LP_DET_COLS, dtype=torch.float32, device=dev),
                    torch.empty(key[0], dtype=torch.int32, device=dev), torch.empty(key[0], dtype=torch.int32, device=dev)) + tuple(tails)
        return _persistent(self._out, key, make)

    def reset(self, streams=None):
        """Zero the state of ``streams`` (all for None) and forget their frames; use it together with ``PlateTracker.reset``."""
        if self.state is not None:
            _zero_streams(self.state, self.n_streams, streams)
        self._reset_host(streams)

    @property
    def dropped(self):
        """int32 [n_streams] on the host: the back rows that found no room since the last reset (a host read, outside the hot
        path)."""
        if self.state is None:
            return np.zeros(self.n_streams, np.int32)
        return self.state.view(self.n_streams, -1)[:, 2].cpu().numpy()

    def _update(self, det_hold, count_hold, tid, slot, stream_of, flush):
        B, hold_rows, max_det, S = det_hold.shape[0], det_hold.shape[1], tid.shape[1], self.n_streams
        if B == 0 and self.state is not None:
            hold_rows, max_det = self._rows - self.back_cap, 1      # a call without frames (a flush) takes the entries as they are
        rows = hold_rows + self.back_cap
        state = self._state_for(rows)
        out = self.buffers(B, rows)
        so, fl = _host_lists(stream_of, B, flush)
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_lookback_update(_dptr(state), S, self.max_tracks, self.depth, self.max_back, self.back_cap,
                                                    _dptr(det_hold), _dptr(count_hold), _dptr(tid), _dptr(slot), B, max_det, hold_rows,
                                                    so, fl, _dptr(out[0]), _dptr(out[1]), _dptr(out[2]),
                                                    _dptr(out[3]), _dptr(out[4]), _dptr(out[5]), _stream_ptr(self.device)),
                      'lp_lookback_update')
        return out

    def _blank_like(self, frame):
        """A scratch frame of the kind of ``frame`` for a slot of the redact call that has no frame (its count is 0)."""
        key = frame.matrix if isinstance(frame, Nv12Frame) else None
        blank = self._blank.get(key)
        if blank is None:
            if key is None:
                blank = torch.zeros(1, 1, 3, dtype=torch.uint8, device=self.device)
            else:
                blank = Nv12Frame.from_packed(torch.zeros(6, dtype=torch.uint8, device=self.device), 2, 2, key)
            self._blank[key] = blank
        return blank

    def _status_for(self, n, rows):
        return _persistent(self._status, (n, rows), lambda: torch.empty(n, rows, dtype=torch.int32, device=self.device))

    def _redact(self, frames, rel, tails, out):
        kw = dict(mode=self.mode, cell=self.cell, margin=self.margin, fill=self.fill, sigma=self.sigma)
        rel_det, rel_count, _, tail_det, tail_count, _ = out
        B, rows = rel_det.shape[:2]
        if rel:
            # one call over all B slots: slot b takes the frame that leaves at b; a slot that releases nothing has rel_count 0
            # and takes frame b itself (no byte changes), or a scratch frame where there is none
            # (a frame that enters and leaves within this push is in the list twice, at its own b with count 0 and at the b
            # that releases it: redact_plates reads and writes a frame only along its rows, so the count-0 entry touches nothing)
            leaving = {b: fr for b, _, _, fr in rel}
            lst = [leaving.get(b, frames[b]) for b in range(B)]
            lst = [self._blank_like(rel[0][3]) if fr is None else fr for fr in lst]
            redact_plates(lst, rel_det, rel_count, status=self._status_for(B, rows), **kw)
        done = [(s, g, fr) for _, s, g, fr in rel]
        for s, items in tails:
            if items:
                redact_plates([fr for _, fr in items], tail_det[s], tail_count[s], status=self._status_for(len(items), rows), **kw)
                done += [(s, g, fr) for g, fr in items]
        return done


def eval_counts(det, det_count, tgt, tgt_count, counts=None):
    """Counters of the LP accuracy metric for one batch (``lp_eval_counts``): det [B,max_det,28] fp32 + det_count [B]
    int32 as ``nms_padded`` returns them, tgt [B,max_t,20] fp32 + tgt_count [B] int32; ``counts`` (int64 [43], CUDA) is
    accumulated into and returned (allocated zeroed when None)."""
    dev = det.device
    _check_det_count(det, det_count)
    if not (tgt.dtype == torch.float32 and tgt.dim() == 3 and tgt.shape[2] == 20 and tgt.is_contiguous() and tgt.device == dev
            and tgt_count.dtype == torch.int32 and tgt_count.is_contiguous() and tgt_count.device == dev
            and det.shape[0] == tgt.shape[0] == tgt_count.numel()):
        raise ValueError('eval_counts: expected contiguous CUDA tgt [B,T,20] fp32 and int32 tgt_count [B] on det\'s device')
    if counts is None:
        counts = torch.zeros(abi.LP_EVAL_NCOUNTS, dtype=torch.int64, device=dev)
    elif not (counts.dtype == torch.int64 and counts.numel() == abi.LP_EVAL_NCOUNTS and counts.device == dev and counts.is_contiguous()):
        raise ValueError('eval_counts: counts must be a contiguous CUDA int64 [%d] tensor' % abi.LP_EVAL_NCOUNTS)
    with torch.cuda.device(dev):
        abi.check(abi.load().lp_eval_counts(_dptr(det), _dptr(det_count), det.shape[1], _dptr(tgt), _dptr(tgt_count), tgt.shape[1],
                                            det.shape[0], _dptr(counts), _stream_ptr(dev)), 'lp_eval_counts')
    return counts
