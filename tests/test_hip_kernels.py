"""GPU parity tests of the individual HIP kernels, called through the C ABI
(via yolov6.hip.runtime.Engine, the ctypes host).  The checker is the CPU
oracle: plain torch fp32 ops for the float kernels."""
import pytest
import torch
import torch.nn.functional as F

from lp_testing import assert_elementwise, conv_ref64, ref_images, rel_err

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# stated tolerances (relative to the largest reference magnitude): fp32 engine = exact-fp32 MFMA with a
# different summation order; fp16 / bf16 = inputs, weights and outputs rounded to 11 / 8 significant bits
TOL = {torch.float32: 2e-5, torch.float16: 4e-3, torch.bfloat16: 3e-2}


def _engine(dtype, mfma16=False):
    """Kernel tests compare variants bit for bit with the default one: the default stays on the 32x32x16 family here; the
    16x16x32 family (another fp32 summation order) is selected explicitly where it is the subject (LP_VARIANT_PIPE16_*)."""
    from yolov6.hip.runtime import Engine
    return Engine(dtype, 'cuda:0', mfma16=mfma16)


def _fill(eng, tid, ref_nchw):
    """Write an NCHW fp32 reference tensor into arena tensor ``tid`` (all stored channels, padding = 0)."""
    v = eng.tensor_view(tid)                                     # [B,C,h,w] view, logical channels
    v.copy_(ref_nchw.to(v.device, v.dtype))


def _run(eng, B, H, W):
    x = torch.zeros(B, 3, H, W, device='cuda:0')
    return eng.forward(x)


def _poison_lds():
    import ctypes
    from yolov6.hip import abi
    abi.check(abi.load().lp_debug_poison_lds(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'lp_debug_poison_lds')


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


CONV_CASES = [
    # (cin list, cout, k, s, act, residual, H, W at the source resolution, B)
    ([64], 64, 3, 1, 'relu', False, 40, 40, 2),        # CFG_B, exact tiles
    ([128], 128, 3, 1, 'relu', False, 20, 20, 3),      # CFG_A, ragged 20x20 map
    ([32], 64, 3, 2, 'relu', False, 64, 48, 2),        # stride 2
    ([3], 32, 3, 2, 'relu', False, 64, 64, 2),         # stem-like: 3 real channels of 8 stored
    ([64, 64], 128, 3, 1, 'relu', False, 24, 16, 2),   # two sources (concat-free PAN input)
    ([256], 128, 1, 1, 'relu', False, 20, 20, 2),      # 1x1 reduce
    ([64, 64, 64, 64], 64, 1, 1, 'relu', False, 12, 20, 2),   # SPPF cv5: four sources
    ([128, 64, 64], 64, 1, 1, 'silu', False, 16, 16, 1),
    ([96], 96, 3, 1, 'relu', True, 16, 24, 2),         # BottleRep residual, cout not a tile multiple
    ([40], 24, 3, 1, 'none', False, 8, 8, 1),  # small odd channel counts (8-multiples)
    ([5], 5, 3, 1, 'relu', True, 8, 8, 1),             # logical channels not a multiple of 8 (padded storage)
    ([16], 8, 1, 1, 'silu', False, 8, 8, 1),           # CFG_C
    ([512], 512, 3, 1, 'relu', False, 20, 20, 1),      # deep K (4608)
]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: '%s-%d-k%ds%d-%s%s' % ('+'.join(map(str, c[0])), c[1], c[2], c[3], c[4], '-res' if c[5] else ''))
def test_conv(case, dtype):
    from yolov6.hip import abi
    cins, cout, k, s, act, use_res, h, w, B = case
    sl = 5          # source tensors at 1/32 resolution: any h, w gives an input size the engine accepts
    eng = _engine(dtype)
    srcs = [eng.tensor(c, sl) for c in cins]
    cin = sum(cins)
    wt = _rand((cout, cin, k, k), 1, (2.0 / (cin * k * k)) ** 0.5)
    bias = _rand((cout,), 2, 0.5)
    res_id = eng.tensor(cout, sl) if use_res else None
    act_id = {'none': abi.LP_ACT_NONE, 'relu': abi.LP_ACT_RELU, 'silu': abi.LP_ACT_SILU}[act]
    dst = eng.conv(srcs, wt, bias, k, s, act_id, sl, res=res_id, alpha=0.75)
    eng.finish()
    H, W = h << sl, w << sl
    eng.bind(B, H, W)
    xs = [_rand((B, c, h, w), 10 + i) for i, c in enumerate(cins)]
    q = lambda t: t.to(dtype).float()                     # what the engine actually stores
    for t, x in zip(srcs, xs):
        _fill(eng, t, x)
    res = _rand((B, cout, h // s, w // s), 20) if use_res else None
    if use_res:
        _fill(eng, res_id, res)
    _run(eng, B, H, W)
    got = eng.tensor_view(dst).float().cpu()
    ref = F.conv2d(torch.cat([q(x) for x in xs], 1), q(wt), bias, stride=s, padding=k // 2)
    ref = {'none': lambda t: t, 'relu': F.relu, 'silu': F.silu}[act](ref)
    if use_res:
        ref = q(ref) + 0.75 * q(res) if dtype != torch.float32 else ref + 0.75 * res
    assert got.shape == ref.shape
    assert rel_err(got, ref) <= TOL[dtype], rel_err(got, ref)
    assert torch.isfinite(got).all()
    # on top of the max-norm: every element within one ulp of the storage type + the fp32 accumulation bound of the float64 reference
    ref64, mag64, K, slack = conv_ref64(xs, wt, bias, dtype, s, k // 2, act, res, 0.75)
    assert_elementwise(got, ref64, mag64, K, dtype, transcendental=act == 'silu', slack64=slack)


STREAM_CASES = [
    # (cin list, cout, act, residual, h, w, B)
    ([64], 64, 'relu', False, 40, 40, 2),                 # one K-chunk, exact tiles
    ([256], 128, 'relu', False, 20, 20, 2),               # 128-row weight packing, four chunks
    ([64, 64, 64, 64], 64, 'relu', False, 12, 20, 2),     # SPPF cv5: four sources
    ([128, 64, 64], 64, 'silu', False, 16, 16, 1),        # BiFusion concat
    ([96], 192, 'relu', True, 13, 7, 3),                  # 96 channels: a partial second K-chunk in f16 / bf16; residual, ragged pixel count
    ([64, 96, 32], 64, 'relu', False, 11, 9, 2),          # partial chunks in the middle and at the end of a concat
    ([64], 128, 'relu', True, 13, 7, 3),                  # residual with 128 couts per wave
    ([128], 128, 'none', False, 9, 5, 1),                 # fewer pixels than one workgroup's tiles
]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', [(16, 2), (17, 2)], ids=lambda v: 'wc%d' % (2 if v[0] == 16 else 4))    # LP_VARIANT_STREAM64 / 128
@pytest.mark.parametrize('case', STREAM_CASES, ids=lambda c: '%s-%d-%s%s' % ('+'.join(map(str, c[0])), c[1], c[2], '-res' if c[3] else ''))
def test_conv1x1_stream(case, variant, dtype):
    """The streaming 1x1 kernel against the oracle, and bit-for-bit against the implicit-GEMM kernel on the same packing."""
    from yolov6.hip import abi
    cins, cout, act, use_res, h, w, B = case
    sl = 5
    eng = _engine(dtype)
    srcs = [eng.tensor(c, sl) for c in cins]
    cin = sum(cins)
    wt = _rand((cout, cin, 1, 1), 1, (2.0 / cin) ** 0.5)
    bias = _rand((cout,), 2, 0.5)
    res_id = eng.tensor(cout, sl) if use_res else None
    act_id = {'none': abi.LP_ACT_NONE, 'relu': abi.LP_ACT_RELU, 'silu': abi.LP_ACT_SILU}[act]
    dst = eng.conv(srcs, wt, bias, 1, 1, act_id, sl, res=res_id, alpha=0.75)
    eng.finish()
    H, W = h << sl, w << sl
    eng.bind(B, H, W)
    eng.autotune = False
    xs = [_rand((B, c, h, w), 10 + i) for i, c in enumerate(cins)]
    q = lambda t: t.to(dtype).float()
    for t, x in zip(srcs, xs):
        _fill(eng, t, x)
    res = _rand((B, cout, h, w), 20) if use_res else None
    if use_res:
        _fill(eng, res_id, res)
    conv_op = eng.lib.lp_engine_num_ops(eng.h) - 1
    _run(eng, B, H, W)                                     # default implicit-GEMM variant
    base = eng.tensor_view(dst).clone()
    eng.tensor_view(dst).zero_()
    # the kernel takes an op only if its weight packing has whole cout tiles of the wave (the engine packs by least
    # padding: 128-row tiles only for multiples of 128), every source is made of whole 32-byte K-steps (a last K-chunk may
    # be partial: 96 channels), and the
    # resident weights + bias + staging fit the 160 KiB of LDS
    sz = torch.empty(0, dtype=dtype).element_size()
    wc = 2 if variant[0] == 16 else 4
    kc = 128 // sz
    stored = [(c + 7) // 8 * 8 for c in cins]
    nchunks = sum(-(-c // kc) for c in stored)
    lds = nchunks * 32 * wc * 128 + 32 * wc * 4 + 4 * (128 // wc) * (32 * wc * sz + 16)
    fits = (wc == 2 or cout % 128 == 0) and all(c % (kc // 4) == 0 for c in stored) and lds <= 160 * 1024 and nchunks <= 8
    if not fits:
        with pytest.raises(RuntimeError):
            eng.set_variant(conv_op, *variant)
        return
    eng.set_variant(conv_op, *variant)
    _run(eng, B, H, W)
    got = eng.tensor_view(dst)
    assert torch.equal(got, base)
    ref = F.conv2d(torch.cat([q(x) for x in xs], 1), q(wt), bias)
    ref = {'none': lambda t: t, 'relu': F.relu, 'silu': F.silu}[act](ref)
    if use_res:
        ref = q(ref) + 0.75 * q(res) if dtype != torch.float32 else ref + 0.75 * res
    assert rel_err(got.float().cpu(), ref) <= TOL[dtype]


def test_conv1x1_stream_rejects_unfit_ops():
    from yolov6.hip import abi
    eng = _engine(torch.float16)
    src = eng.tensor(16, 5)
    eng.conv([src], _rand((8, 16, 1, 1), 1), _rand((8,), 2), 1, 1, abi.LP_ACT_RELU, 5)       # 32-row packing
    src3 = eng.tensor(64, 5)
    eng.conv([src3], _rand((64, 64, 3, 3), 1), _rand((64,), 2), 3, 1, abi.LP_ACT_RELU, 5)   # 3x3
    eng.finish()
    eng.bind(1, 64, 64)
    n = eng.lib.lp_engine_num_ops(eng.h)
    for op in (n - 2, n - 1):
        with pytest.raises(RuntimeError):
            eng.set_variant(op, 16, 2)
    with pytest.raises(RuntimeError):
        eng.set_variant(0, 0, 1)                          # the input op has no variants


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cin,cout,h,w', [(128, 128, 20, 20), (64, 64, 10, 14), (16, 24, 6, 6)])
def test_deconv2x2(cin, cout, h, w, dtype):
    import ctypes
    from yolov6.hip import abi
    from yolov6.hip.runtime import _f32
    eng = _engine(dtype)
    src, dst = eng.tensor(cin, 5), eng.tensor(cout, 4)
    wt = _rand((cin, cout, 2, 2), 3, (1.0 / cin) ** 0.5)
    bias = _rand((cout,), 4, 0.5)
    abi.check(eng.lib.lp_engine_add_deconv2x2(eng.h, src, dst, eng._ptr(_f32(wt)), eng._ptr(_f32(bias))))
    eng.finish()
    B = 2
    eng.bind(B, h * 32, w * 32)
    x = _rand((B, cin, h, w), 5)
    _fill(eng, src, x)
    _run(eng, B, h * 32, w * 32)
    got = eng.tensor_view(dst).float().cpu()
    q = lambda t: t.to(dtype).float()
    ref = F.conv_transpose2d(q(x), q(wt), bias, stride=2)
    assert rel_err(got, ref) <= TOL[dtype]
    ref64, mag64, K, _ = conv_ref64([x], wt, bias, dtype, 2, transposed=True)
    assert_elementwise(got, ref64, mag64, K, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c,h,w', [(256, 20, 20), (64, 13, 7), (8, 4, 3), (40, 40, 40), (32, 2, 1), (16, 1, 5)])
def test_pool_chain(c, h, w, dtype):
    from yolov6.hip import abi
    eng = _engine(dtype)
    ids = [eng.tensor(c, 5) for _ in range(4)]
    abi.check(eng.lib.lp_engine_add_pool5_chain(eng.h, *ids))
    eng.finish()
    B = 2
    eng.bind(B, h * 32, w * 32)
    x = _rand((B, c, h, w), 6).to(dtype).float()
    _fill(eng, ids[0], x)
    _run(eng, B, h * 32, w * 32)
    y = x
    for t in ids[1:]:
        y = F.max_pool2d(y, 5, 1, 2)
        assert torch.equal(eng.tensor_view(t).float().cpu(), y)      # max is exact in every dtype


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('xdtype', [torch.float32, torch.float16])
def test_input_layout(dtype, xdtype):
    eng = _engine(dtype)
    eng.finish()
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(7)).to(xdtype)
    eng.forward(x.cuda())
    got = eng.tensor_view(eng.input_id).float().cpu()
    assert torch.equal(got, x.float().to(dtype).float())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('bins', [1, 17])
def test_head(dtype, bins):
    """head_cls (8 predictors + sigmoid) and head_box (+DFL) + decode against the oracle's decode."""
    from yolov6.hip import abi
    from yolov6.hip.runtime import _f32
    from oracle import lp_oracle
    C, B, H, W = 64, 2, 128, 96
    eng = _engine(dtype)
    feats = [eng.tensor(C, 3 + i) for i in range(3)]
    ws = []
    for i, f in enumerate(feats):
        wc, bc = _rand((277, C), 30 + i, 0.3), _rand((277,), 40 + i, 1.0)
        wb, bb = _rand((4 * bins + 8, C), 50 + i, 0.2), _rand((4 * bins + 8,), 60 + i, 1.0)
        proj = torch.linspace(0, bins - 1, bins)
        abi.check(eng.lib.lp_engine_add_head_cls(eng.h, f, i, 277, eng._ptr(_f32(wc)), eng._ptr(_f32(bc))))
        abi.check(eng.lib.lp_engine_add_head_box(eng.h, f, i, bins, eng._ptr(_f32(wb)), eng._ptr(_f32(bb)),
                                                 eng._ptr(_f32(proj)) if bins > 1 else None))
        ws.append((wc, bc, wb, bb, proj))
    eng.finish()
    eng.bind(B, H, W)
    xs = [_rand((B, C, H >> (3 + i), W >> (3 + i)), 70 + i) for i in range(3)]
    for f, x in zip(feats, xs):
        _fill(eng, f, x)
    pred = _run(eng, B, H, W).cpu()
    q = lambda t: t.to(dtype).float()
    cls_all, reg_all, cor_all = [], [], []
    for (wc, bc, wb, bb, proj), x in zip(ws, xs):
        l = x.shape[2] * x.shape[3]
        cls_all.append(torch.sigmoid(F.conv2d(q(x), q(wc)[..., None, None], bc)).reshape(B, 277, l))
        o = F.conv2d(q(x), q(wb)[..., None, None], bb)
        reg = o[:, :4 * bins]
        if bins > 1:
            reg = F.conv2d(F.softmax(reg.reshape(B, 4, bins, l).permute(0, 2, 1, 3), dim=1), proj.reshape(1, bins, 1, 1))
        reg_all.append(reg.reshape(B, 4, l))
        cor_all.append(o[:, 4 * bins:].reshape(B, 8, l))
    cat = lambda p: torch.cat(p, -1).permute(0, 2, 1)
    pts, st = lp_oracle.anchors([x.shape[2:] for x in xs])
    box, corners = lp_oracle.decode(cat(reg_all), cat(cor_all), pts, st)
    ref = torch.cat([box, torch.ones(B, box.shape[1], 1), corners, cat(cls_all)], -1)
    assert pred.shape == ref.shape
    assert torch.equal(pred[..., 4], torch.ones_like(pred[..., 4]))
    tol = TOL[dtype]
    assert float((pred[..., 13:] - ref[..., 13:]).abs().max()) <= tol * 2            # probabilities
    # ... and elementwise: fp32 outputs of v_exp_f32 + v_rcp_f32 on an fp32 sum of C + 1 terms
    cls64 = [conv_ref64([x], wc[..., None, None], bc, dtype, act='sigmoid') for (wc, bc, _, _, _), x in zip(ws, xs)]
    cat64 = lambda k: torch.cat([c[k].reshape(B, 277, -1) for c in cls64], -1).permute(0, 2, 1)
    assert_elementwise(pred[..., 13:], cat64(0), cat64(1), cls64[0][2], torch.float32, transcendental=True)
    scale = float(ref[..., :13].abs().max())
    assert float((pred[..., :13] - ref[..., :13]).abs().max()) <= tol * scale * (4 if bins > 1 else 2)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('xdtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('cout,H,W', [(32, 64, 96), (16, 128, 64), (48, 32, 32)])
def test_fused_stem(dtype, xdtype, cout, H, W):
    """3x3 s2 conv reading the caller's NCHW image directly (stem_kernel)."""
    from yolov6.hip import abi
    eng = _engine(dtype)
    wt = _rand((cout, 3, 3, 3), 1, (2.0 / 27) ** 0.5)
    bias = _rand((cout,), 2, 0.5)
    dst = eng.conv([eng.input_id], wt, bias, 3, 2, abi.LP_ACT_RELU, 0)
    eng.finish()
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(3)).to(xdtype)
    eng.forward(x.cuda())
    got = eng.tensor_view(dst).float().cpu()
    q = lambda t: t.float().to(dtype).float()
    ref = F.relu(F.conv2d(q(x), q(wt), bias, stride=2, padding=1))
    assert got.shape == ref.shape
    assert rel_err(got, ref) <= TOL[dtype]
    ref64, mag64, K, _ = conv_ref64([x.float()], wt, bias, dtype, 2, 1, 'relu')
    assert_elementwise(got, ref64, mag64, K, dtype)


# ---- LP accuracy metric (lp_eval_counts) -----------------------------------------------------------------------
def _metric_oracle():
    import os
    import sys
    from conftest import REPO
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    from oracle import lp_metric
    return lp_metric


@pytest.mark.parametrize('case', ['metric_synth_a', 'metric_synth_b', 'metric_crafted'])
def test_eval_counts_golden(case):
    """The kernel (through yolov6.utils.lp_metric / Evaler.eval on CUDA tensors) on the inputs of the reference goldens:
    counters identical to the oracle's, results identical to the reference's Evaler.eval."""
    from conftest import load_golden
    from lp_testing import unpack_lists
    from yolov6.utils import lp_metric
    from yolov6.core.evaler import Evaler
    z = load_golden(case)
    preds, targets = unpack_lists(z, 'pred', 28), unpack_lists(z, 'tgt', 20)
    ref_c = _metric_oracle().counts([[p.numpy() for p in b] for b in preds], [[t.numpy() for t in b] for b in targets], strict=False)
    dp = [[p.cuda() for p in b] for b in preds]
    dt = [[t.cuda() for t in b] for b in targets]
    assert lp_metric.counts(dp, dt).tolist() == ref_c.tolist()
    out = Evaler(None, device=torch.device('cuda:0'), half=False).eval(dp, dt, None, 'val')
    assert out[:5] == z['scalars'].tolist() and out[5] == z['mAP_list'].tolist() and out[6] == z['recall_list'].tolist()


@pytest.mark.parametrize('B,max_pred,max_tgt', [(32, 300, 6), (5, 1000, 12), (3, 2, 1)])
def test_eval_counts_random(B, max_pred, max_tgt):
    """Bigger seeded batches (more detections than threads of a workgroup) against the oracle; two batches accumulate."""
    from lp_testing import synth_metric_batch
    from yolov6.utils import lp_metric
    M = _metric_oracle()
    batches = [synth_metric_batch(100 + k, B, max_pred, max_tgt) for k in range(2)]
    preds, targets = [b[0] for b in batches], [b[1] for b in batches]
    ref_c = M.counts([[p.numpy() for p in b] for b in preds], [[t.numpy() for t in b] for b in targets], strict=False)
    got = lp_metric.counts([[p.cuda() for p in b] for b in preds], [[t.cuda() for t in b] for b in targets])
    assert got.tolist() == ref_c.tolist()
    assert int(ref_c[M.I_PRED_BINS:M.I_PRED_BINS + 10].sum()) > 0          # the case exercises the bins


def test_eval_counts_edges():
    """Identical boxes (IoU 1: no bin), duplicate detections (first index wins), empty images, argument checks."""
    from yolov6.hip import runtime
    from yolov6.utils import lp_metric
    M = _metric_oracle()
    pred = torch.zeros(3, 28)
    pred[:, :4] = torch.tensor([[10., 10., 50., 30.], [10., 10., 50., 30.], [100., 100., 140., 120.]])
    pred[0, 20:] = 1.0                       # detection 0 has the right classes, its duplicate 1 does not
    tgt = torch.zeros(2, 20)
    tgt[:, :8] = 1.0
    tgt[0, 8:12] = torch.tensor([10., 10., 50., 29.])      # IoU 0.95 with detections 0 and 1
    tgt[0, 12:] = pred[0, 4:12]
    tgt[1, 8:12] = pred[2, :4]                              # IoU 1.0: unbinned
    preds = [[pred, torch.zeros(0, 28)], [torch.zeros(0, 28)]]
    targets = [[tgt, tgt[:1]], [torch.zeros(0, 20)]]
    ref_c = M.counts([[p.numpy() for p in b] for b in preds], [[t.numpy() for t in b] for b in targets], strict=False)
    got = lp_metric.counts([[p.cuda() for p in b] for b in preds], [[t.cuda() for t in b] for b in targets])
    assert got.tolist() == ref_c.tolist()
    assert int(got[lp_metric.UNBINNED]) == 1 and int(got[lp_metric.RIGHT + 9]) == 1 and int(got[lp_metric.TRUE]) == 3
    with pytest.raises(ValueError):
        runtime.eval_counts(torch.zeros(2, 4, 28, device='cuda'), torch.zeros(2, dtype=torch.int32, device='cuda'),
                            torch.zeros(3, 1, 20, device='cuda'), torch.zeros(3, dtype=torch.int32, device='cuda'))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,H,W,B', [(64, 128, 96, 2), (128, 96, 32, 3), (192, 64, 64, 1)])
def test_head_cls_rows_variant(C, H, W, B, dtype):
    """The row-writer form of the class predictors (LP_VARIANT_ROWS) against the tiled generic kernel: bit-identical columns
    13..289, also when 32-anchor tiles straddle images (12x4 = 48 anchors per image) and at the ragged tail."""
    from yolov6.hip import abi
    from yolov6.hip.runtime import _f32
    eng = _engine(dtype)
    feats = [eng.tensor(C, 3 + i) for i in range(3)]
    for i, f in enumerate(feats):
        wc, bc = _rand((277, C), 30 + i, 0.3), _rand((277,), 40 + i, 1.0)
        abi.check(eng.lib.lp_engine_add_head_cls(eng.h, f, i, 277, eng._ptr(_f32(wc)), eng._ptr(_f32(bc))))
    eng.finish()
    eng.bind(B, H, W)
    eng.autotune = False
    for i, f in enumerate(feats):
        _fill(eng, f, _rand((B, C, H >> (3 + i), W >> (3 + i)), 70 + i))
    base = _run(eng, B, H, W)[..., 13:].clone()
    sz = torch.empty(0, dtype=dtype).element_size()
    fits = C % (128 // sz) == 0 and C // (128 // sz) <= 3
    for op in (1, 2, 3):
        if fits:
            eng.set_variant(op, 18, 1)
        else:
            with pytest.raises(RuntimeError):
                eng.set_variant(op, 18, 1)
    if not fits:
        return
    got = _run(eng, B, H, W)[..., 13:]
    assert torch.equal(got, base)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    for op in (1, 2, 3):                      # and back to the tiled kernel
        eng.set_variant(op, 2, 1)
    assert torch.equal(_run(eng, B, H, W)[..., 13:], base)


VARIANT_SHAPES = [
    # (cin list, cout, k, s, map size): every packing class, both strides, single / multi source, a small-M case
    ([64], 64, 3, 1, 80), ([64], 128, 3, 2, 80), ([128], 128, 3, 1, 40), ([128], 256, 3, 2, 40), ([256], 256, 3, 1, 20),
    ([64], 64, 1, 1, 80), ([128, 64], 64, 1, 1, 80), ([256], 128, 1, 1, 40), ([128, 128, 128], 128, 1, 1, 40),
    ([64], 64, 3, 1, 40, 'res'), ([128], 128, 3, 1, 20, 'res'), ([128], 128, 1, 1, 40, 'res'),      # BottleRep residual epilogue
]


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('act', ['relu', 'silu'])
@pytest.mark.parametrize('shape', VARIANT_SHAPES, ids=lambda c: '%s-%d-k%ds%d-%d' % ('+'.join(map(str, c[0])), c[1], c[2], c[3], c[4]))
def test_every_kernel_variant_gives_the_same_bits(shape, act, dtype):
    """The autotuner may pick any variant (workgroup tile, ring depth, streaming kernel) per layer and per input shape, so
    all of them must agree bit for bit -- otherwise results would depend on timing noise and on the batch size.  (SiLU once
    differed by one fp16 ulp between instantiations: the compiler folded its multiply into the f32 -> f16 conversion in
    some of them.)"""
    from yolov6.hip import abi
    cins, cout, k, s, hw = shape[:5]
    use_res = len(shape) > 5
    B, sl = 2, 5
    eng = _engine(dtype)
    eng.autotune = False
    srcs = [eng.tensor(c, sl) for c in cins]
    cin = sum(cins)
    wt = _rand((cout, cin, k, k), 1, (2.0 / (cin * k * k)) ** 0.5)
    act_id = {'relu': abi.LP_ACT_RELU, 'silu': abi.LP_ACT_SILU}[act]
    res_id = eng.tensor(cout, sl) if use_res else None
    dst = eng.conv(srcs, wt, _rand((cout,), 2, 0.3), k, s, act_id, sl, res=res_id, alpha=0.7)
    eng.finish()
    eng.bind(B, hw << sl, hw << sl)
    for i, (t, c) in enumerate(zip(srcs, cins)):
        _fill(eng, t, _rand((B, c, hw, hw), 10 + i))
    if use_res:
        _fill(eng, res_id, _rand((B, cout, hw, hw), 20))
    op = eng.lib.lp_engine_num_ops(eng.h) - 1
    # two families, each bit-identical inside: 32x32x16 (tiles A..F, streaming 1x1, LP_VARIANT_PIPE_*) and 16x16x32
    # (LP_VARIANT_PIPE16_*: fixed tiles 39 / 41, tiles of any number of 16-pixel blocks 42 / 43).  Which family runs a layer is a
    # function of the layer alone (lp_engine_set_mfma16), so the autotuner's freedom stays inside one family.
    fam32 = [(c, n) for c in list(range(8)) + [16, 17] for n in (1, 2)] + [(32, 3), (33, 3), (34, 3), (35, 3)]
    fam16 = [(c, 3) for c in (39, 41, 42, 43)]
    bases = []
    for fam in (fam32, fam16):
        base, tried = None, 0
        for cfg, nb in fam:
            try:
                eng.set_variant(op, cfg, nb)
            except RuntimeError:
                continue
            eng.tensor_view(dst).zero_()
            _run(eng, B, hw << sl, hw << sl)
            out = eng.tensor_view(dst).clone()
            tried += 1
            if base is None:
                base = out
            else:
                assert torch.equal(out, base), (cfg, nb)
        assert tried >= 2 or fam is fam16
        bases.append(base)
    if bases[1] is not None:                                  # the families agree to rounding
        d = (bases[0].float() - bases[1].float()).abs()
        assert float(d.max()) <= TOL[dtype] * float(bases[0].float().abs().max())
        assert k == 3 and s == 1 and cin % 64 == 0 and cout > 64


PIPE_CASES = [
    # (cin list, cout, act, residual, h, w, B): the pipelined 3x3 stride-1 kernel (LP_VARIANT_PIPE_*) on shapes where a
    # persistent workgroup walks several tiles (more tiles than CUs), single-chunk layers (the ring outruns a tile), ragged
    # maps, concat sources, partial cout tiles and the residual epilogue
    ([64], 64, 'relu', False, 160, 160, 6),
    ([128], 128, 'relu', False, 40, 40, 40),
    ([256], 256, 'silu', False, 20, 20, 70),
    ([64, 64], 128, 'relu', False, 40, 40, 40),
    ([16], 64, 'relu', False, 40, 40, 3),
    ([8], 128, 'none', False, 24, 40, 2),
    ([96], 192, 'relu', True, 13, 27, 5),
    ([64], 64, 'relu', True, 33, 17, 3),
    ([512], 512, 'relu', False, 20, 20, 2),
    ([12], 32, 'relu', False, 96, 160, 3),           # the stem in its space-to-depth form: 32-cout packing, one K-chunk
    ([16], 24, 'silu', False, 33, 47, 2),
]


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('case', PIPE_CASES, ids=lambda c: '%s-%d-%s%s-%dx%dx%d' % ('+'.join(map(str, c[0])), c[1], c[2], '-res' if c[3] else '', c[6], c[4], c[5]))
def test_conv3x3_pipe(case, dtype):
    """Pipelined 3x3 kernel: bit-identical to the generic implicit-GEMM kernel (same K order, same epilogue arithmetic) and
    within the stated tolerance of F.conv2d in fp32."""
    from yolov6.hip import abi
    cins, cout, act, use_res, h, w, B = case
    sl = 5
    eng = _engine(dtype)
    eng.autotune = False
    srcs = [eng.tensor(c, sl) for c in cins]
    cin = sum(cins)
    wt = _rand((cout, cin, 3, 3), 1, (2.0 / (cin * 9)) ** 0.5)
    bias = _rand((cout,), 2, 0.5)
    res_id = eng.tensor(cout, sl) if use_res else None
    act_id = {'none': abi.LP_ACT_NONE, 'relu': abi.LP_ACT_RELU, 'silu': abi.LP_ACT_SILU}[act]
    dst = eng.conv(srcs, wt, bias, 3, 1, act_id, sl, res=res_id, alpha=0.75)
    eng.finish()
    H, W = h << sl, w << sl
    eng.bind(B, H, W)
    xs = [_rand((B, c, h, w), 10 + i) for i, c in enumerate(cins)]
    q = lambda t: t.to(dtype).float()
    for t, x in zip(srcs, xs):
        _fill(eng, t, x)
    res = _rand((B, cout, h, w), 20) if use_res else None
    if use_res:
        _fill(eng, res_id, res)
    op = eng.lib.lp_engine_num_ops(eng.h) - 1
    _run(eng, B, H, W)
    base = eng.tensor_view(dst).clone()
    ref = F.conv2d(torch.cat([q(x) for x in xs], 1), q(wt), bias, padding=1)
    ref = {'none': lambda t: t, 'relu': F.relu, 'silu': F.silu}[act](ref)
    if use_res:
        ref = q(ref) + 0.75 * q(res)
    assert rel_err(base.float().cpu(), ref) <= TOL[dtype]
    tried = 0
    for cfg in (32, 33, 34, 35):                       # the pipelined variants
        try:
            eng.set_variant(op, cfg, 3)
        except RuntimeError:
            continue
        tried += 1
        for rep in range(2):
            # LDS keeps its bytes between kernels: without the poison a fragment read that ran ahead of its LDS-DMA would find
            # the identical bytes of the launch before and pass
            _poison_lds()
            eng.tensor_view(dst).fill_(float('nan'))
            _run(eng, B, H, W)
            out = eng.tensor_view(dst)
            assert torch.equal(out, base), (cfg, rep, float((out.float() - base.float()).abs().max()))
    assert tried >= 1


PIPE16_CASES = [
    # (cin list, cout, act, residual, h, w, B): layers whose K-chunks are a multiple of four (input channels a multiple of 64) with the 128-row weight packing
    ([64], 128, 'relu', False, 160, 160, 3),
    ([128], 128, 'relu', False, 40, 40, 40),
    ([256], 256, 'silu', False, 20, 20, 70),
    ([64, 64], 128, 'relu', False, 40, 40, 20),
    ([64], 96, 'relu', True, 33, 17, 3),              # residual, partial cout tile
    ([128], 72, 'none', False, 13, 27, 5),            # partial cout tile
    ([512], 512, 'relu', False, 20, 20, 2),
    ([64], 128, 'relu', False, 124, 252, 2),          # many tiles per workgroup, ragged
]


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('case', PIPE16_CASES, ids=lambda c: '%s-%d-%s%s-%dx%dx%d' % ('+'.join(map(str, c[0])), c[1], c[2], '-res' if c[3] else '', c[6], c[4], c[5]))
def test_conv3x3_pipe16(case, dtype):
    """The pipelined 3x3 kernel on v_mfma_f32_16x16x32 (LP_VARIANT_PIPE16_*): within the stated tolerance of F.conv2d in fp32 and of
    the 32x32x16 family (another fp32 summation order, so not bit for bit), its tilings bit-identical among themselves, every
    launch reproducible with a poisoned LDS ring in front of it."""
    from yolov6.hip import abi
    cins, cout, act, use_res, h, w, B = case
    sl = 5 if h <= 64 else 3
    eng = _engine(dtype)
    eng.autotune = False
    srcs = [eng.tensor(c, sl) for c in cins]
    cin = sum(cins)
    wt = _rand((cout, cin, 3, 3), 1, (2.0 / (cin * 9)) ** 0.5)
    bias = _rand((cout,), 2, 0.5)
    res_id = eng.tensor(cout, sl) if use_res else None
    act_id = {'none': abi.LP_ACT_NONE, 'relu': abi.LP_ACT_RELU, 'silu': abi.LP_ACT_SILU}[act]
    dst = eng.conv(srcs, wt, bias, 3, 1, act_id, sl, res=res_id, alpha=0.75)
    eng.finish()
    H, W = h << sl, w << sl
    eng.bind(B, H, W)
    xs = [_rand((B, c, h, w), 10 + i) for i, c in enumerate(cins)]
    q = lambda t: t.to(dtype).float()
    for t, x in zip(srcs, xs):
        _fill(eng, t, x)
    res = _rand((B, cout, h, w), 20) if use_res else None
    if use_res:
        _fill(eng, res_id, res)
    op = eng.lib.lp_engine_num_ops(eng.h) - 1
    _run(eng, B, H, W)
    base32 = eng.tensor_view(dst).clone()                  # the default variant: 32x32x16 family
    ref = F.conv2d(torch.cat([q(x) for x in xs], 1), q(wt), bias, padding=1)
    ref = {'none': lambda t: t, 'relu': F.relu, 'silu': F.silu}[act](ref)
    if use_res:
        ref = q(ref) + 0.75 * q(res)
    base16 = None
    for cfg in (39, 41, 42, 43):               # fixed tiles, then tiles of any number of 16-pixel blocks: the same sums
        try:
            eng.set_variant(op, cfg, 3)
        except RuntimeError:
            continue
        for rep in range(2):
            _poison_lds()
            eng.tensor_view(dst).fill_(float('nan'))
            _run(eng, B, H, W)
            out = eng.tensor_view(dst)
            if base16 is None:
                base16 = out.clone()
                assert rel_err(base16.float().cpu(), ref) <= TOL[dtype], (cfg, rel_err(base16.float().cpu(), ref))
                # the two families differ by fp32 summation order only: a rounding flip here and there in the 16-bit result
                d = (base16.float() - base32.float()).abs()
                assert float(d.max()) <= TOL[dtype] * float(ref.abs().max()) and float((d > 0).float().mean()) < 0.25
            assert torch.equal(out, base16), (cfg, rep, int((out != base16).sum()), int(torch.isnan(out.float()).sum()))
    assert base16 is not None
    # both families elementwise against the float64 reference (of up to three images of the batch)
    im = ref_images(B)
    ref64, mag64, K, slack = conv_ref64([x[im] for x in xs], wt, bias, dtype, 1, 1, act, res[im] if use_res else None, 0.75)
    for fam in (base32, base16):
        assert_elementwise(fam[im], ref64, mag64, K, dtype, transcendental=act == 'silu', slack64=slack)


S2P16_CASES = [
    # (cin list, cout, act, h, w of the INPUT map, B): 3x3 stride-2 layers with the 128-row weight packing (more than 64 stored couts)
    ([64], 128, 'relu', 160, 160, 3),               # yololps' ERBlock_3[0]: 5 x 40 tiles, several per workgroup
    ([128], 256, 'relu', 80, 80, 8),                # ERBlock_4[0]: two cout tiles
    ([256], 512, 'silu', 40, 40, 6),                # ERBlock_5[0]: sixteen chunks, four cout tiles, 10 x 20 tiles
    ([48], 96, 'relu', 64, 96, 2),                  # yolov6m's ERBlock_2[0]: three chunks (odd: tiles alternate ring phases), partial cout tile
    ([96], 200, 'none', 34, 22, 3),                 # ragged 17 x 11 output, partial second cout tile (192 couts would take the 64-row packing)
    ([16], 128, 'relu', 252, 124, 7),               # ONE chunk per tile, >= 3 tiles per workgroup: the ring crosses a tile at every chunk
    ([64, 64], 128, 'relu', 40, 40, 5),             # two sources
    ([128], 72, 'relu', 26, 54, 5),                 # partial cout tile
]


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('case', S2P16_CASES, ids=lambda c: '%s-%d-%s-%dx%dx%d' % ('+'.join(map(str, c[0])), c[1], c[2], c[5], c[3], c[4]))
def test_conv3x3_s2p16(case, dtype):
    """The 3x3 stride-2 kernel on v_mfma_f32_16x16x32 (LP_VARIANT_PIPE16_S2A / _S2B, lp_conv3x3_s2p16.inc): within the stated
    tolerance of F.conv2d in fp32 and of conv_mfma_kernel<KS=3,S=2> (another fp32 summation order, so not bit for bit), its two wave
    grids bit-identical to each other, every launch reproducible with a poisoned LDS in front of it (three halo + two weight slots, counted vmcnt; tiles with one,
    three and sixteen chunks)."""
    from yolov6.hip import abi
    cins, cout, act, h, w, B = case
    sl = 5 if h <= 64 else 3
    eng = _engine(dtype)
    eng.autotune = False
    srcs = [eng.tensor(c, sl) for c in cins]
    cin = sum(cins)
    wt = _rand((cout, cin, 3, 3), 1, (2.0 / (cin * 9)) ** 0.5)
    bias = _rand((cout,), 2, 0.5)
    act_id = {'none': abi.LP_ACT_NONE, 'relu': abi.LP_ACT_RELU, 'silu': abi.LP_ACT_SILU}[act]
    dst = eng.conv(srcs, wt, bias, 3, 2, act_id, sl)
    eng.finish()
    H, W = h << sl, w << sl
    eng.bind(B, H, W)
    xs = [_rand((B, c, h, w), 10 + i) for i, c in enumerate(cins)]
    q = lambda t: t.to(dtype).float()
    for t, x in zip(srcs, xs):
        _fill(eng, t, x)
    op = eng.lib.lp_engine_num_ops(eng.h) - 1
    _run(eng, B, H, W)
    base32 = eng.tensor_view(dst).clone()                  # the default variant: conv_mfma_kernel<KS=3,S=2>
    ref = F.conv2d(torch.cat([q(x) for x in xs], 1), q(wt), bias, stride=2, padding=1)
    ref = {'none': lambda t: t, 'relu': F.relu, 'silu': F.silu}[act](ref)
    assert rel_err(base32.float().cpu(), ref) <= TOL[dtype]
    base16 = None
    for cfg in (abi.LP_VARIANT_PIPE16_S2A, abi.LP_VARIANT_PIPE16_S2B):
        eng.set_variant(op, cfg, 3)
        for rep in range(2):
            _poison_lds()
            eng.tensor_view(dst).fill_(float('nan'))
            _run(eng, B, H, W)
            out = eng.tensor_view(dst)
            if base16 is None:
                base16 = out.clone()
                assert rel_err(base16.float().cpu(), ref) <= TOL[dtype], (cfg, rel_err(base16.float().cpu(), ref))
                d = (base16.float() - base32.float()).abs()
                assert float(d.max()) <= TOL[dtype] * float(ref.abs().max()) and float((d > 0).float().mean()) < 0.25
            assert torch.equal(out, base16), (cfg, rep, int((out != base16).sum()), int(torch.isnan(out.float()).sum()))
    im = ref_images(B)
    ref64, mag64, K, _ = conv_ref64([x[im] for x in xs], wt, bias, dtype, 2, 1, act)
    for fam in (base32, base16):
        assert_elementwise(fam[im], ref64, mag64, K, dtype, transcendental=act == 'silu')


RING_CASES = [
    # (cin, cout, h, w, B): ONE K-chunk per tile (every chunk of the stream crosses a tile boundary: the DMA tile iterator and the
    # per-tile halo map advance once per chunk) and at least three tiles per persistent workgroup, ragged maps included
    (12, 32, 252, 252, 7),        # PIPE_C: 512-pixel tiles
    (16, 64, 252, 252, 7),        # PIPE_B (64-cout packing)
    (16, 128, 124, 252, 7),       # PIPE_D / PIPE_F (128-cout packing)
    (32, 128, 96, 100, 9),        # two chunks per tile: tiles alternate between ring phases
]


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('case', RING_CASES, ids=lambda c: '%d-%d-%dx%dx%d' % c)
def test_conv3x3_pipe_ring_with_poisoned_lds(case, dtype):
    """the hazard of the one-chunk-per-tile configuration made deterministic.  Every CU's LDS is filled with
    NaN patterns before each launch, tiles have one (or two) K-chunks so that the ring protocol crosses a tile boundary at every
    chunk, every workgroup walks >= 3 tiles; three launches per variant must reproduce the generic kernel's bits."""
    from yolov6.hip import abi
    cin, cout, h, w, B = case
    sl = 3
    eng = _engine(dtype)
    eng.autotune = False
    src = eng.tensor(cin, sl)
    wt = _rand((cout, cin, 3, 3), 1, (2.0 / (cin * 9)) ** 0.5)
    bias = _rand((cout,), 2, 0.5)
    dst = eng.conv([src], wt, bias, 3, 1, abi.LP_ACT_RELU, sl)
    eng.finish()
    H, W = h << sl, w << sl
    eng.bind(B, H, W)
    x = _rand((B, cin, h, w), 10)
    _fill(eng, src, x)
    op = eng.lib.lp_engine_num_ops(eng.h) - 1
    _run(eng, B, H, W)
    base = eng.tensor_view(dst).clone()
    q = lambda t: t.to(dtype).float()
    ref = F.relu(F.conv2d(q(x), q(wt), bias, padding=1))
    assert rel_err(base.float().cpu(), ref) <= TOL[dtype]
    tried = 0
    for cfg in (32, 33, 34, 35):
        try:
            eng.set_variant(op, cfg, 3)
        except RuntimeError:
            continue
        tried += 1
        for rep in range(3):
            _poison_lds()
            eng.tensor_view(dst).fill_(float('nan'))
            _run(eng, B, H, W)
            out = eng.tensor_view(dst)
            assert torch.equal(out, base), (cfg, rep, int((out != base).sum()), int(torch.isnan(out.float()).sum()))
    assert tried >= 1


def test_sigmoid_of_the_kernels_is_monotone_over_all_of_fp32():
    """The detections-only head computes max-of-sigmoids as sigmoid-of-max (lp_head_rows.inc): exact iff the kernels' sigmoid
    (v_exp_f32 + v_rcp_f32) never decreases.  Checked for every pair of neighbouring fp32 values on the device."""
    import ctypes
    from yolov6.hip import abi
    lib = abi.load()
    bad = torch.full((1,), -1, dtype=torch.int64, device='cuda')
    abi.check(lib.lp_check_sigmoid_monotone(ctypes.c_void_p(bad.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
              'lp_check_sigmoid_monotone')
    torch.cuda.synchronize()
    assert int(bad[0]) == 0


@pytest.mark.parametrize('iou_thres', [0.45, 0.65, 0.5, 0.1, 0.999, 0.0, 1.0])
def test_iou_predicate_product_form_equals_the_division(iou_thres):
    """greedy NMS (lp_nms.hip, iou_gt): `inter / union > iou_threshold` is decided by two products and compares where the outcome
    is certain and by the fp32 division only inside a 2^-19-wide band around the threshold.  Both forms, side by side on the
    device, against the fp32 op-by-op restatement (numpy) of torchvision's expression: random pairs, pairs whose IoU sits within
    a few ulps of the threshold on either side (including exactly on it), degenerate and disjoint boxes."""
    import ctypes
    import numpy as np
    from yolov6.hip import abi
    rng = np.random.default_rng(int(iou_thres * 1000))
    f32 = np.float32
    thr_f = f32(iou_thres)
    if float(thr_f) > iou_thres:
        thr_f = np.nextafter(thr_f, f32(-np.inf))
    pairs = []
    # random overlapping / disjoint boxes in pixel ranges
    n = 200000
    xy = rng.uniform(0, 640, (n, 2, 2)).astype(f32)
    wh = rng.uniform(0.5, 300, (n, 2, 2)).astype(f32)
    pairs.append(np.concatenate([xy[:, 0], xy[:, 0] + wh[:, 0], xy[:, 1], xy[:, 1] + wh[:, 1]], 1))
    # nested boxes [0,0,a,1] and [0,0,b,1]: IoU = b / a, with b stepped through the fp32 neighbours of t * a
    a = rng.uniform(1, 1000, 4000).astype(f32)
    for k in range(-40, 41):
        b = (thr_f * a).astype(f32)
        for _ in range(abs(k)):
            b = np.nextafter(b, f32(np.inf) if k > 0 else f32(-np.inf))
        z = np.zeros_like(a)
        pairs.append(np.stack([z, z, a, z + 1, z, z, b, z + 1], 1))
    # shifted equal squares: IoU = (s - d) / (s + d) crossing the threshold
    s = rng.uniform(10, 500, 100000).astype(f32)
    t_ = float(thr_f)
    d = (s * f32((1 - t_) / (1 + t_))).astype(f32) * rng.uniform(0.99999, 1.00001, s.shape).astype(f32)
    z = np.zeros_like(s)
    pairs.append(np.stack([z, z, s, s, d, z, d + s, s], 1))
    # degenerate: zero-area, inverted and touching boxes, huge and tiny sides
    pairs.append(np.array([[0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 10, 10, 10, 0, 20, 10], [5, 5, 1, 1, 0, 0, 10, 10],
                           [0, 0, 1e20, 1e20, 0, 0, 1e20, 1e20], [0, 0, 3e38, 3e38, 0, 0, 3e38, 3e38], [0, 0, 1e-30, 1e-30, 0, 0, 1e-30, 1e-30],
                           [0, 0, 10, 10, 0, 0, 10, 10], [0, 0, 10, 10, 2, 2, 8, 8]], dtype=f32))
    # NaN and infinite coordinates (tests/test_nonfinite_gpu.py: what a diverged box head hands the NMS): a NaN anywhere makes the IoU
    # NaN, an infinite side makes it 0 or, inf - inf or inf / inf, NaN -- `> threshold` is false for all of them, in both forms
    nan, inf = np.nan, np.inf
    nonfinite = np.array([[nan, 0, 10, 10, 0, 0, 10, 10], [0, 0, 10, 10, 0, nan, 10, 10], [0, 0, 10, nan, 0, 0, 10, nan], [nan] * 8,
                          [0, 0, inf, 10, 0, 0, 10, 10], [-inf, 0, inf, 10, 0, 0, 10, 10], [0, 0, inf, inf, 0, 0, inf, inf],
                          [-inf, -inf, inf, inf, -inf, -inf, inf, inf], [inf, inf, inf, inf, 0, 0, 10, 10], [0, 0, 10, 10, -inf, 0, -inf, 10],
                          [0, 0, 10, 10, 2, 2, inf, 8], [nan, 0, 10, 10, 0, 0, inf, inf], [0, 0, 10, 10, 0, 0, 10, 10]], dtype=f32)
    pairs.append(nonfinite)
    q = np.ascontiguousarray(np.concatenate(pairs, 0).astype(f32))
    with np.errstate(all='ignore'):
        ia = (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1])
        ja = (q[:, 6] - q[:, 4]) * (q[:, 7] - q[:, 5])
        w = np.minimum(q[:, 2], q[:, 6]) - np.maximum(q[:, 0], q[:, 4])
        h = np.minimum(q[:, 3], q[:, 7]) - np.maximum(q[:, 1], q[:, 5])
        w = np.where(w > 0, w, f32(0))
        h = np.where(h > 0, h, f32(0))
        inter = (w * h).astype(f32)
        ovr = inter / ((ia + ja).astype(f32) - inter).astype(f32)
        want = ovr.astype(np.float64) > iou_thres            # torchvision compares in double against the python float
    assert not want[-len(nonfinite):-1].any() and np.isnan(ovr[-len(nonfinite):-1]).sum() >= 6      # (the last row: a finite sentinel)
    dq = torch.from_numpy(q).cuda()
    out = torch.zeros(len(q), dtype=torch.uint8, device='cuda')
    abi.check(abi.load().lp_check_iou_predicate(ctypes.c_void_p(dq.data_ptr()), len(q), float(iou_thres), ctypes.c_void_p(out.data_ptr()),
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'lp_check_iou_predicate')
    got = out.cpu().numpy()
    assert np.array_equal((got & 2) != 0, want)              # the division form == the restatement
    assert np.array_equal((got & 1) != 0, want)              # the product form == the same
    if 0.0 < iou_thres < 1.0:
        assert want.any() and not want.all()


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('h,w,B', [(20, 20, 3), (6, 14, 2), (40, 40, 8)])
def test_bifusion_fused_equals_its_three_ops(h, w, B, dtype):
    """LP_VARIANT_FUSED_BIFUSION: BiFusion's cv3(cat[upsample(x0), cv1(x1), d]) (common.py:504-527) as one kernel gives the bits of the
    transposed conv, cv1 and cv3 run as three launches, and matches torch within the stated tolerance.  h x w = the COARSE map."""
    from yolov6.hip import abi
    import ctypes
    from yolov6.hip.runtime import _f32
    C0, C1, C = 64, 128, 64
    eng = _engine(dtype)
    eng.autotune = False
    sl = 4                                      # coarse level; the fine level is sl - 1
    x0, x1, d = eng.tensor(C0, sl), eng.tensor(C1, sl - 1), eng.tensor(C, sl - 1)
    u = eng.tensor(C, sl - 1)
    wd, bd = _rand((C0, C, 2, 2), 1, (1.0 / C0) ** 0.5), _rand((C,), 2, 0.3)
    abi.check(eng.lib.lp_engine_add_deconv2x2(eng.h, x0, u, eng._ptr(_f32(wd)), eng._ptr(_f32(bd))))
    w1, b1 = _rand((C, C1, 1, 1), 3, (2.0 / C1) ** 0.5), _rand((C,), 4, 0.3)
    a = eng.conv([x1], w1, b1, 1, 1, abi.LP_ACT_RELU, sl - 1)
    w3, b3 = _rand((C, 3 * C, 1, 1), 5, (2.0 / (3 * C)) ** 0.5), _rand((C,), 6, 0.3)
    out = eng.conv([u, a, d], w3, b3, 1, 1, abi.LP_ACT_RELU, sl - 1)
    eng.finish()
    H, W = h << sl, w << sl
    eng.bind(B, H, W)
    X0, X1, D = _rand((B, C0, h, w), 10), _rand((B, C1, 2 * h, 2 * w), 11), _rand((B, C, 2 * h, 2 * w), 12)
    for t, x in ((x0, X0), (x1, X1), (d, D)):
        _fill(eng, t, x)
    op = eng.lib.lp_engine_num_ops(eng.h) - 1
    _run(eng, B, H, W)
    want = eng.tensor_view(out).clone()
    q = lambda t: t.to(dtype).float()
    ru = q(F.conv_transpose2d(q(X0), q(wd), bd, stride=2))
    ra = q(F.relu(F.conv2d(q(X1), q(w1), b1)))
    ref = F.relu(F.conv2d(torch.cat([ru, ra, q(D)], 1), q(w3), b3))
    assert rel_err(want.float().cpu(), ref) <= TOL[dtype]
    eng.set_variant(op, abi.LP_VARIANT_FUSED_BIFUSION, 3)
    assert eng.lib.lp_engine_op_carrier(eng.h, 1, 0) == op and eng.lib.lp_engine_op_carrier(eng.h, 2, 0) == op      # deconv, cv1 ride along
    for rep in range(2):
        for t in (u, a, out):
            eng.tensor_view(t).fill_(float('nan'))
        _run(eng, B, H, W)
        got = eng.tensor_view(out)
        assert torch.equal(got, want), (rep, int((got != want).sum()), int(torch.isnan(got.float()).sum()))
        assert torch.isnan(eng.tensor_view(u).float()).all() and torch.isnan(eng.tensor_view(a).float()).all()      # never written: they stay on chip
    eng.set_variant(op, 1, 1)                   # back to the three launches
    assert eng.lib.lp_engine_op_carrier(eng.h, 1, 0) == -1
    _run(eng, B, H, W)
    assert torch.equal(eng.tensor_view(out), want) and not torch.isnan(eng.tensor_view(u).float()).any()


PAIR_CASES = [
    # (cin list, cout1, cout2, k, act, h, w, B): two sibling layers on one input as ONE launch with two destinations
    ([64], 64, 64, 1, 'relu', 40, 24, 2),
    ([96], 64, 64, 1, 'relu', 17, 9, 3),                  # BepC3 cv1 / cv2 of yolov6m: a partial last K-chunk too
    ([128, 64], 128, 128, 1, 'relu', 20, 20, 2),
    ([512], 256, 256, 1, 'relu', 20, 20, 2),              # SimCSPSPPF cv1 / cv2
    ([64], 64, 64, 3, 'silu', 40, 40, 2),                 # the class / box towers of a head level
    ([128], 128, 128, 3, 'silu', 20, 20, 3),
    ([16], 8, 24, 3, 'relu', 12, 20, 2),                  # narrow tensors: 8 + 24 channels in one 32-row cout tile
]


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32], ids=['f16', 'bf16', 'f32'])
@pytest.mark.parametrize('case', PAIR_CASES, ids=lambda c: '%s-%d+%d-k%d' % ('+'.join(map(str, c[0])), c[1], c[2], c[3]))
def test_two_destination_conv_equals_two_convs(case, dtype):
    """lp_conv_desc.dst2 (runtime.Engine.conv_pair): the rows of two sibling layers stacked in one launch give, in each of the two
    destination tensors, the bits the layer gives alone -- in the default variant and in every variant that takes the op."""
    from yolov6.hip import abi
    cins, c1, c2, k, act, h, w, B = case
    sl = 5
    eng = _engine(dtype)
    eng.autotune = False
    srcs = [eng.tensor(c, sl) for c in cins]
    cin = sum(cins)
    w1, b1 = _rand((c1, cin, k, k), 1, (2.0 / (cin * k * k)) ** 0.5), _rand((c1,), 2, 0.5)
    w2, b2 = _rand((c2, cin, k, k), 3, (2.0 / (cin * k * k)) ** 0.5), _rand((c2,), 4, 0.5)
    act_id = {'none': abi.LP_ACT_NONE, 'relu': abi.LP_ACT_RELU, 'silu': abi.LP_ACT_SILU}[act]
    ra = eng.conv(srcs, w1, b1, k, 1, act_id, sl)
    rb = eng.conv(srcs, w2, b2, k, 1, act_id, sl)
    pa, pb = eng.conv_pair(srcs, (w1, b1), (w2, b2), k, 1, act_id, sl)
    eng.finish()
    H, W = h << sl, w << sl
    eng.bind(B, H, W)
    for i, (t, c) in enumerate(zip(srcs, cins)):
        _fill(eng, t, _rand((B, c, h, w), 10 + i))
    op = eng.lib.lp_engine_num_ops(eng.h) - 1
    assert op == 3                                        # input + two single convs + ONE pair op
    _run(eng, B, H, W)
    want_a, want_b = eng.tensor_view(ra).clone(), eng.tensor_view(rb).clone()
    assert torch.equal(eng.tensor_view(pa), want_a) and torch.equal(eng.tensor_view(pb), want_b)
    tried = 0
    variants = [(c, n) for c in range(6) for n in (1, 2)] + ([(16, 2), (17, 2)] if k == 1 else [(32, 3), (33, 3), (34, 3), (35, 3)])
    for cfg, nb in variants:
        try:
            eng.set_variant(op, cfg, nb)
        except RuntimeError:
            continue
        tried += 1
        eng.tensor_view(pa).fill_(float('nan'))
        eng.tensor_view(pb).fill_(float('nan'))
        _run(eng, B, H, W)
        assert torch.equal(eng.tensor_view(pa), want_a) and torch.equal(eng.tensor_view(pb), want_b), (cfg, nb)
    assert tried >= 1
    # the 16x16x32 family sums in another order: the pair equals the two single layers run in the SAME family, bit for bit
    for cfg in (39, 41, 42, 43):
        try:
            for o in (1, 2, 3):
                eng.set_variant(o, cfg, 3)
        except RuntimeError:
            continue
        for t in (ra, rb, pa, pb):
            eng.tensor_view(t).fill_(float('nan'))
        _run(eng, B, H, W)
        assert torch.equal(eng.tensor_view(pa), eng.tensor_view(ra)) and torch.equal(eng.tensor_view(pb), eng.tensor_view(rb)), cfg
        assert rel_err(eng.tensor_view(ra).float().cpu(), want_a.float().cpu()) <= TOL[dtype]
