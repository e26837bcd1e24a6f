"""Exact-arithmetic GPU tests of the convolution kernels (single-op engines through the C ABI, as in test_hip_kernels.py).

Grid data (lp_testing.grid_rand: multiples of 1/4, bias multiples of 1/16) makes every product and every partial sum exact in
fp32 whatever the summation order, so the bits of the result are known in advance: the float64 convolution, converted to fp32
without rounding and rounded ONCE, to nearest-even, to the storage type; the residual epilogue adds alpha * res to the ROUNDED
activation and rounds once more.  Every kernel variant and every output tile the autotuner can pick (lp_engine_set_op_tile) must
give exactly those bits -- the 16x16x32 family too, whose other summation order makes no difference on this data.  Conditions on
the data (exactness bound, share of outputs that need rounding, share of ties) are asserted on the CPU in test_exact_cpu.py and,
for the shapes run here, again below.  Every (variant, B, choice, TH, TW) that ran is appended to exact_tiles.log in the folder of the test logs
(lp_testing.log_dir, next to the parity log)."""
import os

import pytest
import torch
import torch.nn.functional as F

import lp_testing as X
import test_hip_kernels as T
from test_hip_kernels import _engine, _fill, _poison_lds

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT_ID = {F16: 'f16', BF16: 'bf16', F32: 'f32'}
LOG_NAME = 'exact_tiles.log'
SEEN = {}            # kernel family -> {(TH, TW)} over the whole session (asserted by the last test of this file)
NAN = float('nan')

GENERIC = [(c, n) for c in range(6) for n in (1, 2)]                  # implicit-GEMM tiles A..F x ring depth
STREAM = [(16, 2), (17, 2)]
PIPE = [(c, 3) for c in (32, 33, 34, 35)]
PIPE16 = [(c, 3) for c in (39, 41)]
PIPE16_V = [(c, 3) for c in (42, 43)]
S2P16 = [(c, 3) for c in (48, 49)]
ALL_VARIANTS = GENERIC + STREAM + PIPE + PIPE16 + PIPE16_V + S2P16


def _family(cfg):
    return ('generic' if cfg < 16 else 'stream' if cfg < 32 else 'PIPE' if cfg < 36 else 'planar' if cfg == 36 else 'fused_stem' if cfg == 37
            else 'fused_pw' if cfg == 38 else 'PIPE16' if cfg < 42 else 'PIPE16_V' if cfg < 48 else 'S2P16')


def _log(line):
    with open(os.path.join(X.log_dir(), LOG_NAME), 'a') as f:
        f.write(line + '\n')


def _frame(B, H, W):
    return torch.zeros(B, 3, H, W, device='cuda:0')


def _check(eng, dsts, wants, what):
    """All destinations against their expected bits with ONE device synchronisation; details only on a mismatch."""
    bad = sum(X.bit_mismatch_count(eng.tensor_view(d), w) for d, w in zip(dsts, wants))
    if int(bad):
        for i, (d, w) in enumerate(zip(dsts, wants)):
            X.assert_bits(eng.tensor_view(d), w, '%s, output %d' % (what, i))


def _walk(eng, ops, dsts, wants, variants, x, tag, B, fused_nan=(), check=None, choices=4):
    """Every variant of ``variants`` that takes the ops, and for each the tile choices 0..3 (a choice that repeats the tile before
    it is skipped): poisoned LDS in front of the pipelined kernels, NaN-filled destinations, the exact bits out.  Returns
    {family: {(TH, TW)}} of what ran.  ``check``: the comparison in place of _check (tests/test_nonfinite_gpu.py: expected tensors
    that hold NaN); ``choices``: tile choices 0 .. choices - 1 only."""
    check = check or _check
    ran = {}
    for cfg, nb in variants:
        try:
            for op in ops:
                eng.set_variant(op, cfg, nb)
        except RuntimeError:
            continue                                        # the variant does not fit the layer (or the dtype)
        prev = None
        for choice in range(choices):
            try:
                for op in ops:
                    eng.set_tile(op, choice)
                th, tw = eng.tile(ops[0])[1:]
            except RuntimeError:
                if choice > 0:
                    break                                   # streaming kernel: no tiles; stem / fused forms: no further candidate
                th = tw = 0
            if (th, tw) == prev:
                continue
            prev = (th, tw)
            if cfg >= 32:
                _poison_lds()
            for d in list(dsts) + list(fused_nan):
                eng.tensor_view(d).fill_(NAN)
            eng.forward(x)
            check(eng, dsts, wants, '%s variant %d/%d choice %d tile %dx%d' % (tag, cfg, nb, choice, th, tw))
            if th:
                ran.setdefault(_family(cfg), set()).add((th, tw))
                SEEN.setdefault(_family(cfg), set()).add((th, tw))
            _log('%s B=%d choice=%d TH=%d TW=%d %s' % (_family(cfg) + ':%d/%d' % (cfg, nb), B, choice, th, tw, tag))
    return ran


def _assert_rounding_exercised(pre, dtype, what):
    if dtype != F32:
        for act in ('none', 'relu'):
            inexact, ties = X.rounding_stats(pre, act, dtype)
            assert inexact >= 0.25 and ties >= 0.01, (what, act, inexact, ties)


EPILOGUES = [('none', False), ('relu', False), ('none', True), ('relu', True)]


def _four_epilogue_engine(dtype, cins, cout, k, s, sl, xs, wt, bias, res, B, H, W, epilogues=EPILOGUES, mfma16=False):
    """One engine with the layer once per epilogue (none / ReLU, without / with the residual): four ops over the same sources and
    weights, so that one forward and one float64 convolution serve all four."""
    from yolov6.hip import abi
    eng = _engine(dtype, mfma16)
    eng.autotune = False
    srcs = [eng.tensor(c, sl) for c in cins]
    res_id = eng.tensor(cout, sl + (1 if s == 2 else 0)) if any(r for _, r in epilogues) else None
    act_id = {'none': abi.LP_ACT_NONE, 'relu': abi.LP_ACT_RELU}
    dsts = [eng.conv(srcs, wt, bias, k, s, act_id[a], sl, res=res_id if r else None, alpha=X.RES_ALPHA if r else 0.0) for a, r in epilogues]
    eng.finish()
    eng.bind(B, H, W)
    for t, x in zip(srcs, xs):
        _fill(eng, t, x)
    if res_id is not None:
        _fill(eng, res_id, res)
    return eng, list(range(1, 1 + len(dsts))), dsts


_CONV_CACHE = {}


def _conv64(key, xs, wt, k, s):
    """float64 convolution on the CPU without the bias (x and w are the same data for every dtype): computed once per case and
    kept on the device."""
    if _CONV_CACHE.get('key') != key:
        _CONV_CACHE.clear()
        _CONV_CACHE.update(key=key, conv=F.conv2d(torch.cat(xs, 1), wt, None, stride=s, padding=k // 2).cuda())
    return _CONV_CACHE['conv']


CASES = X.exact_conv_cases()


def test_device_conversions_round_like_the_cpu():
    """The expected bits are torch's float64 -> float32 -> storage type conversions; the big tensors are converted on the device:
    the same round-to-nearest-even there (ties, the overflow threshold and fp16 subnormals included)."""
    v = torch.cat([X.grid_rand((1 << 16,), 7, -4096.0, 4096.0, 1.0 / 16), X.grid_rand((1 << 12,), 8, -70000.0, 70000.0, 4.0),
                   X.grid_rand((1 << 12,), 9, -2.0 ** -12, 2.0 ** -12, 2.0 ** -26)])
    for dtype in (F16, BF16):
        assert X.bit_mismatches(v.cuda().float().to(dtype).cpu(), v.float().to(dtype)) == 0
        pre, res = v[:1 << 16], v[:1 << 16].flip(0).float().to(dtype).double()         # a residual the storage type holds
        assert X.bit_mismatches(X.exact_epilogue(pre.cuda(), 'relu', dtype, res.cuda()).cpu(), X.exact_epilogue(pre, 'relu', dtype, res)) == 0


@pytest.mark.parametrize('dtype', [F16, BF16, F32], ids=['f16', 'bf16', 'f32'])        # (the top decorator varies fastest: one float64
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])                       # convolution per case serves the three dtypes)
def test_conv_bits_every_variant_every_tile(case, dtype):
    """The shapes of the parity tests (batch trimmed for the float64 CPU reference), none / ReLU x without / with residual:
    generic A..F x ring depth 1 / 2, streaming 1x1, PIPE, PIPE16, PIPE16_V, S2P16 -- whatever takes the layer -- on every tile
    choice 0..3, bit for bit the exact reference."""
    name, cins, cout, k, s, h, w, B = case
    sl = 5 if h <= 64 else 3
    H, W = h << sl, w << sl
    xs, wt, bias, res = X.grid_inputs(cins, cout, k, B, h, w, dtype, res_hw=(h // s, w // s))
    X.assert_grid_exact(xs, wt, bias, dtype)
    pre = _conv64(case, xs, wt, k, s) + bias.cuda().view(1, -1, 1, 1)      # (the epilogue: torch's conversions on the device)
    _assert_rounding_exercised(pre, dtype, name)
    wants = [X.exact_epilogue(pre, a, dtype, res.cuda() if r else None) for a, r in EPILOGUES]
    eng, ops, dsts = _four_epilogue_engine(dtype, cins, cout, k, s, sl, xs, wt, bias, res, B, H, W)
    x = _frame(B, H, W)
    eng.forward(x)                                                   # the default variant as planned
    _check(eng, dsts, wants, name + ' default')
    ran = _walk(eng, ops, dsts, wants, ALL_VARIANTS, x, '%s-%s' % (name, DT_ID[dtype]), B)
    assert 'generic' in ran


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('stride', [1, 2])
def test_block_tiled_kernels_over_batch_sizes(stride, dtype):
    """conv_pick_tile16v plans by B and the CU count: the block-tiled stride-1 kernel (PIPE16_V0 / _V1) and the stride-2 kernel
    (S2P16 A / B) on one small map for B = 1, 2, 3, 5, 8, 16, 32 x choices 0..3; at least two distinct tiles each."""
    cins, cout, k = [64], 128, 3
    h = w = 20 * stride                                             # a 20 x 20 output map
    sl, Bmax = 3, 32
    xs, wt, bias, res = X.grid_inputs(cins, cout, k, Bmax, h, w, dtype, res_hw=(20, 20))
    X.assert_grid_exact(xs, wt, bias, dtype)
    pre = _conv64(('bsweep', stride), xs, wt, k, stride) + bias.cuda().view(1, -1, 1, 1)
    _assert_rounding_exercised(pre, dtype, 'bsweep')
    res_d = res.cuda()
    family = 'PIPE16_V' if stride == 1 else 'S2P16'
    tiles = set()
    for B in (1, 2, 3, 5, 8, 16, 32):
        wants = [X.exact_epilogue(pre[:B], a, dtype, res_d[:B] if r else None) for a, r in EPILOGUES]
        eng, ops, dsts = _four_epilogue_engine(dtype, cins, cout, k, stride, sl, [t[:B] for t in xs], wt, bias, res[:B], B, h << sl, w << sl)
        ran = _walk(eng, ops, dsts, wants, PIPE16_V if stride == 1 else S2P16, _frame(B, h << sl, w << sl), 'bsweep-s%d-%s' % (stride, DT_ID[dtype]), B)
        assert family in ran, (B, ran)
        tiles |= ran[family]
    assert len(tiles) >= 2, tiles


PAIRS = [(c[0], c[1], c[2], c[3], c[5], c[6], min(c[7], 2)) for c in T.PAIR_CASES]


def pair_data(case, dtype):
    cins, c1, c2, k, h, w, B = case
    xs, wt, bias, _ = X.grid_inputs(cins, c1 + c2, k, B, h, w, dtype)
    X.assert_grid_exact(xs, wt, bias, dtype)
    return xs, wt, bias, F.conv2d(torch.cat(xs, 1), wt, bias, padding=k // 2)


@pytest.mark.parametrize('dtype', [F16, BF16, F32], ids=['f16', 'bf16', 'f32'])
@pytest.mark.parametrize('case', PAIRS, ids=lambda c: '%s-%d+%d-k%d' % ('+'.join(map(str, c[0])), c[1], c[2], c[3]))
def test_two_destination_conv_bits(case, dtype):
    """lp_conv_desc.dst2: two sibling layers as one launch, none and ReLU: both destinations carry the exact bits on every
    variant and tile."""
    from yolov6.hip import abi
    cins, c1, c2, k, h, w, B = case
    sl = 5
    xs, wt, bias, pre = pair_data(case, dtype)
    _assert_rounding_exercised(pre, dtype, 'pair')
    eng = _engine(dtype)
    eng.autotune = False
    srcs = [eng.tensor(c, sl) for c in cins]
    dsts, wants = [], []
    for act, act_id in (('none', abi.LP_ACT_NONE), ('relu', abi.LP_ACT_RELU)):
        dsts += eng.conv_pair(srcs, (wt[:c1], bias[:c1]), (wt[c1:], bias[c1:]), k, 1, act_id, sl)
        y = X.exact_epilogue(pre, act, dtype)
        wants += [y[:, :c1].cuda(), y[:, c1:].cuda()]
    eng.finish()
    assert eng.lib.lp_engine_num_ops(eng.h) == 3                     # input + two pair ops
    eng.bind(B, h << sl, w << sl)
    for t, x in zip(srcs, xs):
        _fill(eng, t, x)
    x = _frame(B, h << sl, w << sl)
    eng.forward(x)
    _check(eng, dsts, wants, 'pair default')
    ran = _walk(eng, [1, 2], dsts, wants, ALL_VARIANTS, x, 'pair-%s-%d+%d-k%d-%s' % ('+'.join(map(str, cins)), c1, c2, k, DT_ID[dtype]), B)
    assert 'generic' in ran


DECONV_SHAPES = [(128, 128, 20, 20), (64, 64, 10, 14), (16, 24, 6, 6)]        # test_deconv2x2's


def deconv_data(cin, cout, h, w, dtype, B=2):
    xs, wt, bias, _ = X.grid_inputs([cin], cout, 2, B, h, w, dtype, wshape=(cin, cout, 2, 2))
    X.assert_grid_exact(xs, wt, bias, dtype, fan_in=cin)
    return xs[0], wt, bias, F.conv_transpose2d(xs[0], wt, bias, stride=2)


@pytest.mark.parametrize('dtype', [F16, BF16, F32], ids=['f16', 'bf16', 'f32'])
@pytest.mark.parametrize('cin,cout,h,w', DECONV_SHAPES)
def test_deconv2x2_bits(cin, cout, h, w, dtype):
    """The 2x2 stride-2 transposed convolution (four weight phases through the implicit-GEMM kernel) on every tile."""
    import ctypes
    from yolov6.hip import abi
    from yolov6.hip.runtime import _f32
    B = 2
    x0, wt, bias, pre = deconv_data(cin, cout, h, w, dtype, B)
    _assert_rounding_exercised(pre, dtype, 'deconv')
    want = X.exact_epilogue(pre, 'none', dtype).cuda()
    eng = _engine(dtype)
    eng.autotune = False
    src, dst = eng.tensor(cin, 5), eng.tensor(cout, 4)
    abi.check(eng.lib.lp_engine_add_deconv2x2(eng.h, src, dst, eng._ptr(_f32(wt)), eng._ptr(_f32(bias))))
    eng.finish()
    eng.bind(B, h * 32, w * 32)
    _fill(eng, src, x0)
    x = _frame(B, h * 32, w * 32)
    eng.forward(x)
    _check(eng, [dst], [want], 'deconv default')
    ran = _walk(eng, [1], [dst], [want], GENERIC, x, 'deconv-%d-%d-%dx%d-%s' % (cin, cout, h, w, DT_ID[dtype]), B)
    assert 'generic' in ran


# ---- the stem forms: the caller's NCHW frame is the data ----------------------------------------------------------------------
STEM_SHAPES = [(32, 64, 96), (16, 128, 64), (48, 32, 32), (32, 256, 320)]        # test_fused_stem's and a frame of several tiles


def stem_data(cout, H, W, dtype, B=2):
    frame = X.grid_rand((B, 3, H, W), 3, -4.0, 4.0)
    _, wt, bias, _ = X.grid_inputs([3], cout, 3, 1, 1, 1, dtype)
    X.assert_grid_exact([frame], wt, bias, dtype)
    return frame, wt, bias, F.conv2d(frame, wt, bias, stride=2, padding=1)


@pytest.mark.parametrize('dtype', [F16, BF16, F32], ids=['f16', 'bf16', 'f32'])
@pytest.mark.parametrize('act', ['none', 'relu'])
@pytest.mark.parametrize('cout,H,W', STEM_SHAPES)
def test_stem_bits(cout, H, W, act, dtype):
    """The 3x3 stride-2 stem on a grid-valued NCHW frame: the input op + the stem's kernels (generic and pipelined, every tile)
    for a frame of the engine's dtype and an fp32 frame, and the planar stem (PIPE_P: reads the frame itself) on every tile."""
    import ctypes
    from yolov6.hip import abi
    B = 2
    frame, wt, bias, pre = stem_data(cout, H, W, dtype, B)
    _assert_rounding_exercised(pre, dtype, 'stem')
    want = X.exact_epilogue(pre, act, dtype).cuda()
    eng = _engine(dtype)
    eng.autotune = False
    dst = eng.conv([eng.input_id], wt, bias, 3, 2, {'none': abi.LP_ACT_NONE, 'relu': abi.LP_ACT_RELU}[act], 0)
    eng.finish()
    tag = 'stem-%d-%dx%d-%s-%s' % (cout, H, W, act, DT_ID[dtype])
    for xdt in dict.fromkeys((dtype, F32)):
        x = frame.to(xdt).cuda()
        eng.forward(x)
        _check(eng, [dst], [want], tag + ' default')
        ran = _walk(eng, [1], [dst], [want], GENERIC + PIPE, x, tag, B)
        assert 'generic' in ran
    if dtype != F32:
        x = frame.to(dtype).cuda()
        assert x.data_ptr() % 16 == 0
        ran = _walk(eng, [1], [dst], [want], [(abi.LP_VARIANT_PIPE_P, 3)], x, tag, B)
        assert ran.get('planar'), 'the planar stem did not take the op'
        cfg = ctypes.c_int()
        abi.check(eng.lib.lp_engine_op_variant(eng.h, 1, ctypes.byref(cfg), None), 'lp_engine_op_variant')
        assert cfg.value == abi.LP_VARIANT_PIPE_P


def _two_stage(dtype, pre1, w2, b2, k2, s2):
    """Second layer on the ROUNDED output of a first ReLU layer (what a fused kernel keeps in LDS): exactness of the second sum
    is asserted with the actual magnitudes, in units of 1/64 (y1: multiples of 1/16, w2: of 1/4)."""
    y1 = X.exact_epilogue(pre1, 'relu', dtype).double()
    bound = w2[0].numel() * float(y1.abs().max()) * float(w2.abs().max()) + float(b2.abs().max())
    assert bound < 2 ** 24 / 64, bound
    return y1, F.conv2d(y1, w2, b2, stride=s2, padding=k2 // 2)


FUSED_STEM_SHAPES = [(32, 64, 160, 224), (16, 32, 96, 128), (16, 32, 64, 64), (32, 64, 320, 320)]
FUSED_PW_SHAPES = [(64, 64, 40, 56), (32, 32, 24, 32), (64, 32, 80, 80), (32, 64, 16, 16)]


def fused_data(kind, c1, c2, H, W, dtype, B=2):
    """Two layers, ReLU both: stem 3x3 s2 (3 -> c1) + 3x3 s2 (c1 -> c2) on an H x W frame, or 1x1 (64 -> c1) + 3x3 s2 (c1 -> c2) on an
    H x W map.  Smaller ranges than GRID_RANGE in the first layer, so that the second sum stays exact (_two_stage)."""
    stem = kind == 'stem'
    x0 = X.grid_rand((B, 3 if stem else 64, H, W), 3 if stem else 10, -2.0, 2.0)
    w1 = X.grid_rand((c1, 3, 3, 3) if stem else (c1, 64, 1, 1), 1, -2.0, 2.0)
    b1 = X.grid_rand((c1,), 2, -8.0, 32.0, 1.0 / 16)
    w2 = X.grid_rand((c2, c1, 3, 3), 4, -2.0, 2.0) if stem else X.grid_rand((c2, c1, 3, 3), 4, -1.0, 1.0)
    b2 = X.grid_rand((c2,), 5, -X.GRID_RANGE[dtype][1] / 4, X.GRID_RANGE[dtype][1], 1.0 / 16)
    X.assert_grid_exact([x0], w1, b1, dtype)
    pre1 = F.conv2d(x0, w1, b1, stride=2, padding=1) if stem else F.conv2d(x0, w1, b1)
    y1, pre2 = _two_stage(dtype, pre1, w2, b2, 3, 2)
    inexact, ties = X.rounding_stats(pre2, 'relu', dtype)
    assert inexact >= 0.25 and ties >= 0.01, (inexact, ties)
    return x0, w1, b1, w2, b2, y1, pre2


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('c1,c2,H,W', FUSED_STEM_SHAPES)
def test_fused_stem_bits(c1, c2, H, W, dtype):
    """LP_VARIANT_FUSED_STEM2: input op + stem + the 3x3 stride-2 layer behind it as one kernel, on every tile the form has: the
    exact bits of the two layers (the stem's output rounded to the storage type in between).  The three separate ops first."""
    from yolov6.hip import abi
    B = 2
    frame, w1, b1, w2, b2, y1, pre2 = fused_data('stem', c1, c2, H, W, dtype, B)
    want1, want2 = y1.float().to(dtype).cuda(), X.exact_epilogue(pre2, 'relu', dtype).cuda()
    eng = _engine(dtype)
    eng.autotune = False
    a = eng.conv([eng.input_id], w1, b1, 3, 2, abi.LP_ACT_RELU, 0)
    d = eng.conv([a], w2, b2, 3, 2, abi.LP_ACT_RELU, 1)
    eng.finish()
    x = frame.to(dtype).cuda()
    eng.forward(x)
    _check(eng, [a, d], [want1, want2], 'fused stem: separate ops')
    tag = 'fused_stem-%d-%d-%dx%d-%s' % (c1, c2, H, W, DT_ID[dtype])
    ran = _walk(eng, [2], [d], [want2], [(abi.LP_VARIANT_FUSED_STEM2, 3)], x, tag, B, fused_nan=[a])
    assert ran.get('fused_stem'), 'the fused stem did not take the op'
    assert torch.isnan(eng.tensor_view(a).float()).all()             # the stem's output stayed on chip: the fused kernel ran


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('c1,c2,h,w', FUSED_PW_SHAPES)
def test_fused_1x1_stride2_bits(c1, c2, h, w, dtype):
    """LP_VARIANT_FUSED_PW_S2: a 1x1 layer (64 -> c1) and the 3x3 stride-2 layer behind it (c1 -> c2) as one kernel, every tile."""
    from yolov6.hip import abi
    B, sl = 2, 3
    x0, w1, b1, w2, b2, y1, pre2 = fused_data('pw', c1, c2, h, w, dtype, B)
    want1, want2 = y1.float().to(dtype).cuda(), X.exact_epilogue(pre2, 'relu', dtype).cuda()
    eng = _engine(dtype)
    eng.autotune = False
    src = eng.tensor(64, sl)
    a = eng.conv([src], w1, b1, 1, 1, abi.LP_ACT_RELU, sl)
    d = eng.conv([a], w2, b2, 3, 2, abi.LP_ACT_RELU, sl)
    eng.finish()
    eng.bind(B, h << sl, w << sl)
    _fill(eng, src, x0)
    x = _frame(B, h << sl, w << sl)
    eng.forward(x)
    _check(eng, [a, d], [want1, want2], 'fused 1x1 + s2: separate ops')
    tag = 'fused_pw-%d-%d-%dx%d-%s' % (c1, c2, h, w, DT_ID[dtype])
    ran = _walk(eng, [2], [d], [want2], [(abi.LP_VARIANT_FUSED_PW_S2, 3)], x, tag, B, fused_nan=[a])
    if c1 == c2:                  # the pairs of the models (64 -> 64 -> 64, 64 -> 32 -> 32) must take the form; mixed widths run it if it fits
        assert ran.get('fused_pw'), 'the fused form did not take the op'
    if ran.get('fused_pw'):
        assert torch.isnan(eng.tensor_view(a).float()).all()


# ---- the layers of the benchmark's models -------------------------------------------------------------------------------------
BENCH_BATCH = {'yololpn': 128, 'yololps': 32, 'yolov6m': 8}         # batch sizes of the benchmark runs kept under profiles/


def _device_conv64(x, wt, k, s):
    """float64 convolution on the device, image by image.  Tied to the plain CPU arithmetic by _spot_check."""
    xd, wd = x.cuda(), wt.cuda()
    return torch.cat([F.conv2d(xd[b:b + 1], wd, None, stride=s, padding=k // 2) for b in range(x.shape[0])], 0)


def _spot_check(conv_dev, x, wt, k, s, n=96, seed=0):
    """n output elements (the four map corners first) recomputed on the CPU as plain float64 dot products."""
    p = k // 2
    xp, wt = F.pad(x, (p, p, p, p)), wt.cpu()
    B, co, ho, wo = conv_dev.shape
    g = torch.Generator().manual_seed(seed)
    idx = [(B - 1, co - 1, oy, ox) for oy in (0, ho - 1) for ox in (0, wo - 1)]
    idx += [tuple(int(torch.randint(0, m, (1,), generator=g)) for m in (B, co, ho, wo)) for _ in range(n - 4)]
    ib, ic, iy, ix = [torch.tensor(v) for v in zip(*idx)]
    got = conv_dev[ib.cuda(), ic.cuda(), iy.cuda(), ix.cuda()].cpu()
    patches = torch.stack([xp[b, :, oy * s:oy * s + k, ox * s:ox * s + k] for b, c, oy, ox in idx]).cpu()
    want = torch.stack([(patches[i] * wt[c]).sum() for i, (b, c, oy, ox) in enumerate(idx)])
    assert torch.equal(got, want)


@pytest.mark.parametrize('name,size', X.MODEL_CONFIGS)
def test_model_layers_bits(name, size):
    """The distinct conv layers (sources, cout, k, stride, map; two-destination launches as such) of the benchmark's models at
    B = 2 (the 1280 x 1280 model: 1), fp16 and bf16, none and ReLU with the layer's own residual: every variant that takes the layer, tile choices 0..3.
    The float64 reference of these big maps is computed on the device and spot-checked against CPU dot products.  For the
    block-tiled kernels the log also says which tile the planner picks at the benchmark's batch size and whether it ran here."""
    import ctypes
    from yolov6.hip import abi
    B = 2 if size <= 640 else 1                                      # (the 1280 x 1280 maps: one image keeps the test short)
    lib = abi.load()
    for cins, cout, k, s, use_res, h, w, sl in X.model_layer_signatures(name, size):
        pair = isinstance(cout, tuple)
        co = sum(cout) if pair else cout
        sig = '%s-%s-k%ds%d%s-%dx%d' % ('+'.join(map(str, cins)), '+'.join(map(str, cout)) if pair else cout, k, s, '-res' if use_res else '', h, w)
        conv = None
        for dtype in (F16, BF16):
            xs, wt, bias, res = X.grid_inputs(cins, co, k, B, h, w, dtype, res_hw=(h // s, w // s) if use_res else None, device='cuda')
            X.assert_grid_exact(xs, wt, bias, dtype)
            if conv is None:
                conv = _device_conv64(torch.cat(xs, 1), wt, k, s)
                _spot_check(conv, torch.cat(xs, 1), wt, k, s)
            pre = conv + bias.cuda().view(1, -1, 1, 1)
            _assert_rounding_exercised(pre, dtype, sig)
            tag = '%s-%d:%s-%s' % (name, size, sig, DT_ID[dtype])
            if pair:
                eng = _engine(dtype, None)                  # mfma16=None: the production default picks the first (default) kernel
                eng.autotune = False
                srcs = [eng.tensor(c, sl) for c in cins]
                dsts, wants = [], []
                for act, act_id in (('none', abi.LP_ACT_NONE), ('relu', abi.LP_ACT_RELU)):
                    dsts += eng.conv_pair(srcs, (wt[:cout[0]], bias[:cout[0]]), (wt[cout[0]:], bias[cout[0]:]), k, s, act_id, sl)
                    y = X.exact_epilogue(pre, act, dtype)
                    wants += [y[:, :cout[0]], y[:, cout[0]:]]
                eng.finish()
                eng.bind(B, size, size)
                for t, x in zip(srcs, xs):
                    _fill(eng, t, x)
                ops = [1, 2]
            else:
                epi = [('none', use_res), ('relu', use_res)]
                wants = [X.exact_epilogue(pre, a, dtype, res if r else None) for a, r in epi]
                eng, ops, dsts = _four_epilogue_engine(dtype, cins, co, k, s, sl, xs, wt, bias, res, B, size, size, epi, mfma16=None)
            x = _frame(B, size, size)
            eng.forward(x)
            _check(eng, dsts, wants, tag + ' default')
            ran = _walk(eng, ops, dsts, wants, ALL_VARIANTS, x, tag, B)
            assert 'generic' in ran
            for fam, variants in (('PIPE16_V', PIPE16_V), ('S2P16', S2P16)):        # coverage of the benchmark's planned tile
                if fam in ran:
                    th, tw = ctypes.c_int(), ctypes.c_int()
                    nct = -(-co // 128)
                    for cfg, _ in variants:
                        abi.check(lib.lp_plan_block_tile(cfg, h // s, w // s, BENCH_BATCH[name], nct, 0, ctypes.byref(th), ctypes.byref(tw), None))
                        _log('coverage %s variant=%d bench_B=%d planned=%dx%d covered=%s' % (tag, cfg, BENCH_BATCH[name], th.value, tw.value,
                                                                                           (th.value, tw.value) in ran[fam]))
            if dtype == F16:
                for fam in ('generic', 'PIPE', 'PIPE16'):                          # their tiles do not depend on B: choice 0 ran
                    if fam in ran:
                        _log('coverage %s family=%s tiles=%s covered=True (tile independent of B)' % (tag, fam, sorted(ran[fam])))


# ---- special values ------------------------------------------------------------------------------------------------------------
SPECIAL = [
    # (id, scale of x, scale of w and of the bias relative to x * w): powers of two keep every product and sum exact
    ('overflow', 2.0 ** 4, 2.0 ** 3),               # outputs up to ~2^17: beyond the largest finite fp16 value -> inf (bf16: finite)
    ('subnormal-out', 2.0 ** -10, 2.0 ** -10),      # outputs around 2^-20 ... 2^-10: fp16 subnormals below 2^-14, inputs normal
    ('subnormal-in', 2.0 ** -14, 2.0 ** 4),         # fp16 activations below 2^-14: subnormal MFMA inputs (bf16: normal)
]


def special_data(case, dtype):
    _, sx, sw = case
    xs, wt, bias, res = X.grid_inputs([64], 128, 3, 2, 16, 16, dtype, res_hw=(16, 16))
    xs, wt, bias, res = [x * sx for x in xs], wt * sw, bias * (sx * sw), res * (sx * sw)
    for t in xs + [wt, res]:
        assert torch.equal(t.to(dtype).double(), t)                  # the scaled grid values are still held exactly
    pre = F.conv2d(xs[0], wt, bias, padding=1)
    X.to_exact_f32(pre)
    return xs, wt, bias, res, [X.exact_epilogue(pre, a, dtype, res if r else None) for a, r in EPILOGUES]


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('case', SPECIAL, ids=[c[0] for c in SPECIAL])
def test_special_values(case, dtype):
    """fp16 overflow, fp16 subnormal outputs and subnormal inputs through the generic and the 16x16x32 kernels: the bits of torch's
    conversion of the exact reference (inf where the value exceeds the largest finite number, subnormals kept)."""
    name, sx, sw = case
    cins, cout, k, h, w, B, sl = [64], 128, 3, 16, 16, 2, 5
    xs, wt, bias, res, wants = special_data(case, dtype)
    if dtype == F16:
        y = wants[0].float()
        if name == 'overflow':
            assert torch.isinf(y).any() and torch.isfinite(y).any() and not torch.isnan(torch.cat([v.float() for v in wants])).any()
        if name == 'subnormal-out':
            assert ((y != 0) & (y.abs() < 2.0 ** -14)).float().mean() > 0.01
        if name == 'subnormal-in':
            assert ((xs[0] != 0) & (xs[0].abs() < 2.0 ** -14)).float().mean() > 0.1
    eng, ops, dsts = _four_epilogue_engine(dtype, cins, cout, k, 1, sl, xs, wt, bias, res, B, h << sl, w << sl)
    x = _frame(B, h << sl, w << sl)
    wants = [v.cuda() for v in wants]
    eng.forward(x)
    _check(eng, dsts, wants, name + ' default')
    ran = _walk(eng, ops, dsts, wants, GENERIC + PIPE + PIPE16 + PIPE16_V, x, 'special-%s-%s' % (name, DT_ID[dtype]), B)
    assert 'generic' in ran and 'PIPE16' in ran and 'PIPE16_V' in ran


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
def test_signed_zero(dtype):
    """All-zero activations, negative weights, bias -0.0: every product is -0.0 and so is, by IEEE 754, their sum (the accumulators
    start at the bias): -0.0 in front of the ReLU.  ReLU (the IEEE maximum with +0.0) must give +0.0, compared as the raw bit pattern.
    Without activation the result is a zero whose sign is NOT pinned: the matrix cores return +0.0 for this sum (measured on an
    MI355X: every kernel, fp16 and bf16), a property of the MFMA accumulation and not of the kernels (exact tests)."""
    from yolov6.hip import abi
    cin, cout, h, w, B, sl = 64, 128, 16, 16, 1, 5
    wt = -(X.grid_rand((cout, cin, 3, 3), 1, 0.25, 4.0))
    bias = torch.full((cout,), -0.0, dtype=torch.float64)
    xs = [torch.zeros(B, cin, h, w, dtype=torch.float64)]
    eng, ops, dsts = _four_epilogue_engine(dtype, [cin], cout, 3, 1, sl, xs, wt, bias, None, B, h << sl, w << sl, [('none', False), ('relu', False)])
    x = _frame(B, h << sl, w << sl)
    want = {0: None, 1: 0}                                            # ReLU: the int16 pattern of +0.0 in fp16 and bf16
    for cfg, nb in [(None, None)] + GENERIC + PIPE + PIPE16 + PIPE16_V:
        if cfg is not None:
            try:
                for op in ops:
                    eng.set_variant(op, cfg, nb)
            except RuntimeError:
                continue
        for d in dsts:
            eng.tensor_view(d).fill_(NAN)
        eng.forward(x)
        for i, d in enumerate(dsts):
            bits = eng.tensor_view(d).contiguous().view(torch.int16)
            assert bool(((bits & 0x7fff) == 0).all() if want[i] is None else (bits == want[i]).all()), (cfg, nb, i, bits.unique().tolist())


def test_every_tiled_family_reaches_a_second_tile():
    """Choices >= 1 reach a second tile in every kernel family with tiles.  Self-contained (the order and the selection of the other
    tests do not matter): one layer per family is run again here and the tiles it ran on are counted."""
    SEEN.clear()
    pick = lambda cins, cout, s, h: next(c for c in CASES if c[1:6] == (cins, cout, 3, s, h))
    test_conv_bits_every_variant_every_tile(pick((128,), 128, 1, 40), F16)          # generic, PIPE, PIPE16, PIPE16_V
    test_conv_bits_every_variant_every_tile(pick((64,), 128, 2, 160), F16)           # S2P16
    test_stem_bits(32, 256, 320, 'relu', F16)                                   # planar
    test_fused_stem_bits(32, 64, 320, 320, F16)
    test_fused_1x1_stride2_bits(64, 64, 40, 56, F16)
    few = {f: sorted(SEEN.get(f, ())) for f in ('generic', 'PIPE', 'PIPE16', 'PIPE16_V', 'S2P16', 'planar', 'fused_stem', 'fused_pw')
           if len(SEEN.get(f, ())) < 2}
    assert not few, few
