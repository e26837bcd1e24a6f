"""NaN and infinities through the engine's kernels, against the reference's semantics (tests/test_nonfinite_cpu.py has the CPU side).

The reference is IEEE arithmetic with nothing skipped and NaN-propagating ReLU and max pooling; the class of every output (NaN, +inf,
-inf, finite) then does not depend on the order of a sum, and on grid data the finite outputs keep the exact bits of the exact tests.
Conv families run on the machinery of test_exact_gpu.py (every variant that takes the layer, tile choices 0 and 1, NaN-filled
destinations, poisoned LDS) with lp_testing.assert_same_nonfinite as the comparison; what ran goes to exact_tiles.log."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lp_testing as X
import test_exact_gpu as E
import test_hip_kernels as T
from test_hip_kernels import _engine, _fill, _poison_lds

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT_ID = E.DT_ID
NAN, INF = float('nan'), float('inf')
ALL3 = pytest.mark.parametrize('dtype', [F16, BF16, F32], ids=['f16', 'bf16', 'f32'])
BITS16 = pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])


def _check(eng, dsts, wants, what):
    """_check of the exact tests with the NaN-aware comparison: one synchronisation, details only on a mismatch."""
    bad = sum(sum(X.same_nonfinite_mismatches(eng.tensor_view(d), w)) for d, w in zip(dsts, wants))
    if int(bad):
        for i, (d, w) in enumerate(zip(dsts, wants)):
            X.assert_same_nonfinite(eng.tensor_view(d), w, '%s, output %d' % (what, i))


def _walk(eng, ops, dsts, wants, variants, x, tag, B, fused_nan=()):
    return E._walk(eng, ops, dsts, wants, variants, x, 'nonfinite-' + tag, B, fused_nan=fused_nan, check=_check, choices=2)


def _log_counts(tag, want):
    E._log('nonfinite-%s expected %s' % (tag, X.nonfinite_counts(want)))


# ---- (a) conv families ---------------------------------------------------------------------------------------------------------------
CONV_VARIANTS = {'conv3x3': E.GENERIC + E.PIPE + E.PIPE16 + E.PIPE16_V, 'conv3x3s2': E.GENERIC + E.S2P16, 'stream1x1': E.GENERIC + E.STREAM,
                 'stream1x1-128': E.GENERIC + E.STREAM}
CONV_FAMILIES = {'conv3x3': ('generic', 'PIPE', 'PIPE16', 'PIPE16_V'), 'conv3x3s2': ('generic', 'S2P16'), 'stream1x1': ('generic',),
                 'stream1x1-128': ('generic',)}
# the streaming kernel's widths a layer takes (stream_fits): WC = 4 reads the 128-row weight packing, which a 64-channel layer does not
# have, and keeps all K-chunks of its 128 weight rows in LDS: the eight fp32 chunks of 256 input channels do not fit beside the staging
STREAM_TAKES = {('stream1x1', 2): [(16, 2)], ('stream1x1', 4): [(16, 2)], ('stream1x1-128', 2): [(16, 2), (17, 2)], ('stream1x1-128', 4): [(16, 2)]}


@ALL3
@pytest.mark.parametrize('name', list(CONV_VARIANTS))
def test_conv_families_propagate_nan_and_infinities(name, dtype):
    """64 -> 128 3x3 (the layer of test_special_values), its stride-2 form and the streaming 1x1 over a three-source concat (into 64
    channels: WC = 2; into 128: both widths), planted as lp_testing.NONFINITE_CONV_CASES says: none / ReLU x without / with residual,
    every variant that takes the layer."""
    d = X.nonfinite_conv_data(name, dtype)
    c = d['case']
    B, sl = 2, 5
    H, W = c['h'] << sl, c['w'] << sl
    wants = [d['wants'][e].cuda() for e in E.EPILOGUES]
    eng, ops, dsts = E._four_epilogue_engine(dtype, c['cins'], c['cout'], c['k'], c['s'], sl, d['xs'], d['wt'], d['bias'], d['res'], B, H, W)
    x = E._frame(B, H, W)
    tag = '%s-%s' % (name, DT_ID[dtype])
    _log_counts(tag, wants[0])
    eng.forward(x)
    _check(eng, dsts, wants, tag + ' default')
    ran = _walk(eng, ops, dsts, wants, CONV_VARIANTS[name], x, tag, B)
    for cfg, nb in STREAM_TAKES.get((name, torch.empty(0, dtype=dtype).element_size()), ()):                       # (no tiles: _walk does not count the streaming kernel as a family)
        for op in ops:
            eng.set_variant(op, cfg, nb)                              # _walk ran it: a refusal here fails the test
    for fam in CONV_FAMILIES[name] if dtype != F32 else ('generic',):
        assert fam in ran, (fam, ran)


@ALL3
def test_deconv2x2_propagates_nan_and_infinities(dtype):
    from yolov6.hip import abi
    from yolov6.hip.runtime import _f32
    d = X.nonfinite_conv_data('deconv2x2', dtype)
    c, B = d['case'], 2
    cin, cout, h, w = c['cins'][0], c['cout'], c['h'], c['w']
    want = d['wants'][('none', False)].cuda()
    eng = _engine(dtype)
    eng.autotune = False
    src, dst = eng.tensor(cin, 5), eng.tensor(cout, 4)
    abi.check(eng.lib.lp_engine_add_deconv2x2(eng.h, src, dst, eng._ptr(_f32(d['wt'])), eng._ptr(_f32(d['bias']))))
    eng.finish()
    eng.bind(B, h * 32, w * 32)
    _fill(eng, src, d['xs'][0])
    x = E._frame(B, h * 32, w * 32)
    eng.forward(x)
    _check(eng, [dst], [want], 'deconv default')
    _log_counts('deconv-' + DT_ID[dtype], want)
    assert 'generic' in _walk(eng, [1], [dst], [want], E.GENERIC, x, 'deconv-%s' % DT_ID[dtype], B)


@ALL3
def test_two_destination_conv_propagates_nan_and_infinities(dtype):
    from yolov6.hip import abi
    d = X.nonfinite_conv_data('pair', dtype)
    c, B, sl = d['case'], 2, 5
    c1, c2 = c['pair']
    assert (c['cins'], c1, c2, c['k'], c['h'], c['w'], B) in E.PAIRS
    eng = _engine(dtype)
    eng.autotune = False
    srcs = [eng.tensor(n, sl) for n in c['cins']]
    dsts, wants = [], []
    for act, act_id in (('none', abi.LP_ACT_NONE), ('relu', abi.LP_ACT_RELU)):
        dsts += eng.conv_pair(srcs, (d['wt'][:c1], d['bias'][:c1]), (d['wt'][c1:], d['bias'][c1:]), c['k'], 1, act_id, sl)
        y = d['wants'][(act, False)]
        wants += [y[:, :c1].cuda(), y[:, c1:].cuda()]
    eng.finish()
    assert eng.lib.lp_engine_num_ops(eng.h) == 3                     # input + two pair ops
    eng.bind(B, c['h'] << sl, c['w'] << sl)
    for t, xv in zip(srcs, d['xs']):
        _fill(eng, t, xv)
    x = E._frame(B, c['h'] << sl, c['w'] << sl)
    eng.forward(x)
    _check(eng, dsts, wants, 'pair default')
    assert 'generic' in _walk(eng, [1, 2], dsts, wants, E.ALL_VARIANTS, x, 'pair-%s' % DT_ID[dtype], B)


@BITS16
def test_infinite_weight_meets_the_zero_padding(dtype):
    """One weight +inf, clean activations: along the top row and the left column of that output channel the tap lies on the zero
    padding and inf * 0 is NaN -- the halo taps are multiplied by the zero page, not skipped.  The generic kernel and one pipelined."""
    d = X.nonfinite_weight_data(dtype)
    c, B, sl = d['case'], 2, 5
    wants = [d['wants'][e].cuda() for e in E.EPILOGUES]
    eng, ops, dsts = E._four_epilogue_engine(dtype, c['cins'], c['cout'], 3, 1, sl, d['xs'], d['wt'], d['bias'], d['res'], B, c['h'] << sl, c['w'] << sl)
    x = E._frame(B, c['h'] << sl, c['w'] << sl)
    ran = _walk(eng, ops, dsts, wants, [(0, 1), (32, 3)], x, 'weight-inf-%s' % DT_ID[dtype], B)
    assert 'generic' in ran and 'PIPE' in ran, ran


# ---- the stem: the caller's frame is the data -------------------------------------------------------------------------------------------
STEM_COUT, STEM_HW = 32, 32
BIG = 70000.0                                 # finite in fp32 and bf16, +inf in fp16 (largest finite fp16 value: 65504)
STEM_PLAN = [('nan', (0, 2, 0, 0)), ('+inf', (0, 0, 15, 17)), ('+inf', (0, 1, 21, 5)), ('+inf', (0, 2, 7, 25)), ('-inf', (0, 1, 15, 21)),
             ('-inf', (0, 0, 27, 11)), ('-inf', (0, 2, 25, 27)),
             ('nan', (1, 0, 31, 13)), ('+inf', (1, 2, 9, 9)), ('+inf', (1, 0, 3, 29)), ('+inf', (1, 1, 19, 3)), ('-inf', (1, 0, 21, 21)),
             ('-inf', (1, 1, 11, 19)), ('-inf', (1, 2, 29, 27))]
STEM_BIG = [(0, 1, 9, 13), (1, 2, 27, 5)]


def space_to_depth(x):
    """[B,3,H,W] -> [B,12,H/2,W/2], channel c*4 + py*2 + px = x[c][2Y+py][2X+px] (input_s2d_kernel)."""
    B, _, H, W = x.shape
    return x.reshape(B, 3, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(B, 12, H // 2, W // 2)


def lowered_stem_weights(wt):
    """The stem rewrite of lp_engine_finalize restated: the 3x3 stride-2 conv over 3 channels as a 3x3 stride-1 conv over the 12
    space-to-depth channels.  Image row 2 oy - 1 + ky = 2 (oy - 1 + dy) + py: ky 0 -> (dy 0, py 1), ky 1 -> (1, 0), ky 2 -> (1, 1), columns
    alike; every other (channel, tap) -- 81 of 108 -- is a structural ZERO weight that still multiplies its pixel."""
    w2 = torch.zeros(wt.shape[0], 12, 3, 3, dtype=wt.dtype)
    for ch in range(3):
        for ky in range(3):
            for kx in range(3):
                dy, py, dx, px = (0 if ky == 0 else 1), (0 if ky == 1 else 1), (0 if kx == 0 else 1), (0 if kx == 1 else 1)
                w2[:, ch * 4 + py * 2 + px, dy, dx] = wt[:, ch, ky, kx]
    return w2


def stem_data(dtype, xdt):
    """Frame [2,3,32,32] of grid values with the planted elements and two values of 70000, as a frame of type ``xdt`` arrives in an
    engine of type ``dtype`` (torch's conversions); the lowered weights; the pre-activation over the LOWERED weights (the engine's
    contract: its NaN set is wider than the reference's 3x3 stride-2 footprint) and the reference's own."""
    frame = X.grid_rand((2, 3, STEM_HW, STEM_HW), 3, -4.0, 4.0)
    _, wt, bias, _ = X.grid_inputs([3], STEM_COUT, 3, 1, 1, 1, dtype)
    X.assert_grid_exact([frame], wt, bias, dtype)
    w2 = lowered_stem_weights(wt)
    assert torch.equal(F.conv2d(space_to_depth(frame), w2, bias, padding=1), F.conv2d(frame, wt, bias, stride=2, padding=1))      # the same sums
    frame = X.plant_nonfinite(frame, STEM_PLAN)
    for idx in STEM_BIG:
        frame[idx] = BIG
    sent = frame.to(xdt)                                                # what the caller hands over
    x_eff = sent.to(dtype).double()                                     # what the input op stores
    pre = X.conv_nonfinite_ref([space_to_depth(x_eff)], w2, bias, 3, 1)
    pre_ref = X.conv_nonfinite_ref([x_eff], wt, bias, 3, 2)
    return sent, x_eff, wt, bias, pre, pre_ref


@ALL3
def test_input_op_keeps_nan_infinities_and_overflows_like_torch(dtype):
    """The input op alone, NCHW frame -> the engine's tensor: NaN, +inf, -inf arrive, 70000 arrives as +inf in an fp16 engine, all as
    torch's .to(dtype) gives them."""
    for xdt in (F32, F16):
        sent, x_eff, *_ = stem_data(dtype, xdt)
        eng = _engine(dtype)
        eng.finish()
        eng.forward(sent.cuda())
        X.assert_same_nonfinite(eng.tensor_view(eng.input_id), x_eff.to(dtype), 'input op %s <- %s' % (DT_ID[dtype], DT_ID[xdt]))
        cnt = X.nonfinite_counts(x_eff)
        assert cnt['nan'] == 2 and cnt['-inf'] == 6 and cnt['+inf'] == (8 if F16 in (dtype, xdt) else 6), cnt


@ALL3
@pytest.mark.parametrize('act', ['none', 'relu'])
def test_stem_propagates_over_its_lowered_footprint(act, dtype):
    """3 -> 32 through the input op with the space-to-depth rewrite (generic and pipelined kernels, frames of the engine's type and
    fp32 frames) and the planar stem reading a 16-bit frame itself: the product sum over the lowered weights, structural zeros
    included."""
    from yolov6.hip import abi
    B = 2
    eng = _engine(dtype)
    eng.autotune = False
    wt, bias = stem_data(dtype, F32)[2:4]
    dst = eng.conv([eng.input_id], wt, bias, 3, 2, {'none': abi.LP_ACT_NONE, 'relu': abi.LP_ACT_RELU}[act], 0)
    eng.finish()
    tag = 'stem-%s-%s' % (act, DT_ID[dtype])
    for xdt in dict.fromkeys((dtype, F32)):
        sent, _, _, _, pre, _ = stem_data(dtype, xdt)
        want = X.nonfinite_epilogue(pre, act, dtype).cuda()
        x = sent.cuda()
        eng.forward(x)
        _check(eng, [dst], [want], tag + ' default')
        _log_counts(tag + '<-' + DT_ID[xdt], want)
        assert 'generic' in _walk(eng, [1], [dst], [want], E.GENERIC + E.PIPE, x, tag, B)
    if dtype != F32:
        sent, _, _, _, pre, _ = stem_data(dtype, dtype)
        want = X.nonfinite_epilogue(pre, act, dtype).cuda()
        x = sent.cuda()
        assert x.data_ptr() % 16 == 0
        ran = _walk(eng, [1], [dst], [want], [(abi.LP_VARIANT_PIPE_P, 3)], x, tag, B)
        assert ran.get('planar'), 'the planar stem did not take the op'


# ---- the fused forms -------------------------------------------------------------------------------------------------------------------
FUSED_STEM = [(8, 24), (24, 64)]
FUSED_STEM_HW = 64                                               # frame 64 x 64 -> 32 x 32 -> 16 x 16
FUSED_STEM_PLAN = [('nan', (0, 2, 1, 1)), ('+inf', (0, 0, 31, 33)), ('+inf', (0, 1, 45, 13)), ('-inf', (0, 2, 13, 51)), ('+inf', (0, 2, 20, 40)),
                   ('nan', (1, 0, 63, 29)), ('+inf', (1, 1, 17, 17)), ('+inf', (1, 2, 7, 57)), ('-inf', (1, 0, 43, 41)), ('nan', (1, 1, 36, 10))]
# (even coordinates in the last plant of each image: only there do the reference's window, the fused kernel's four taps and the nine differ)
FUSED_PW = min(E.FUSED_PW_SHAPES, key=lambda s: s[2] * s[3])     # (32, 64, 16, 16)
FUSED_PW_PLAN = [('nan', (0, 63, 0, 0)), ('+inf', (0, 0, 7, 8)), ('+inf', (0, 31, 8, 8)), ('-inf', (0, 32, 15, 5)),
                 ('nan', (1, 5, 9, 15)), ('+inf', (1, 17, 3, 3)), ('+inf', (1, 40, 12, 11)), ('-inf', (1, 63, 5, 10))]


def fused_data(kind, c1, c2, H, W, dtype, relu=None, four_taps=False):
    """The two ReLU layers of test_exact_gpu.fused_data with planted inputs: (planted input, w1, b1, w2, b2, expected output of the
    first layer, expected output of the second) -- the propagating ReLU and ONE rounding between the layers
    (``relu='select'``: the mutant of the CPU test, v > 0 ? v : 0 in the inner layer).  ``four_taps``: the stem as the FUSED kernel
    runs it behind a ReLU, over the four live taps of the lowered form only -- image rows 2 oy - 2 .. 2 oy + 1: between the reference's
    window and the stand-alone stem's."""
    x0, w1, b1, w2, b2, _, _ = E.fused_data(kind, c1, c2, H, W, dtype, 2)
    if kind == 'stem':
        x0 = X.plant_nonfinite(x0, FUSED_STEM_PLAN)
        lw = lowered_stem_weights(w1)
        dead = torch.zeros_like(lw, dtype=torch.bool)
        if four_taps:                                  # stage A of stem2_fused_kernel does not run the five all-zero taps dy = 2 / dx = 2
            dead[:, :, 2, :] = dead[:, :, :, 2] = True
            assert not lw[dead].any()
        pre1 = X.conv_nonfinite_ref([space_to_depth(x0)], lw, b1, 3, 1, skip=dead if four_taps else None)
    else:
        x0 = X.plant_nonfinite(x0, FUSED_PW_PLAN)
        pre1 = X.conv_nonfinite_ref([x0], w1, b1, 1, 1)
    y1 = X.nonfinite_epilogue(pre1, 'relu', dtype, relu=relu)
    want2 = X.nonfinite_epilogue(X.conv_nonfinite_ref([y1.double()], w2, b2, 3, 2), 'relu', dtype)
    return x0, w1, b1, w2, b2, y1, want2


@BITS16
@pytest.mark.parametrize('c1,c2', FUSED_STEM)
def test_fused_stem_propagates_through_its_inner_relu(c1, c2, dtype):
    """LP_VARIANT_FUSED_STEM2 against the two-layer reference: a NaN behind the inner ReLU (kept in LDS) is a NaN in the output.  The
    separate ops carry the stand-alone stem's pattern (nine taps), the fused kernel the one of its four live taps."""
    from yolov6.hip import abi
    B, HW = 2, FUSED_STEM_HW
    frame, w1, b1, w2, b2, y1, want2 = fused_data('stem', c1, c2, HW, HW, dtype)
    fused2 = fused_data('stem', c1, c2, HW, HW, dtype, four_taps=True)[-1].cuda()
    want1, want2 = y1.cuda(), want2.cuda()
    eng = _engine(dtype)
    eng.autotune = False
    a = eng.conv([eng.input_id], w1, b1, 3, 2, abi.LP_ACT_RELU, 0)
    d = eng.conv([a], w2, b2, 3, 2, abi.LP_ACT_RELU, 1)
    eng.finish()
    x = frame.to(dtype).cuda()
    eng.forward(x)
    _check(eng, [a, d], [want1, want2], 'fused stem: separate ops')
    tag = 'fused_stem-%d-%d-%s' % (c1, c2, DT_ID[dtype])
    _log_counts(tag, want2)
    ran = _walk(eng, [2], [d], [fused2], [(abi.LP_VARIANT_FUSED_STEM2, 3)], x, tag, B, fused_nan=[a])
    assert ran.get('fused_stem'), 'the fused stem did not take the op'
    assert torch.isnan(eng.tensor_view(a).float()).all()             # the stem's output stayed on chip: the fused kernel ran


@BITS16
def test_fused_1x1_stride2_propagates_through_its_inner_relu(dtype):
    from yolov6.hip import abi
    c1, c2, h, w = FUSED_PW
    B, sl = 2, 3
    x0, w1, b1, w2, b2, y1, want2 = fused_data('pw', c1, c2, h, w, dtype)
    want1, want2 = y1.cuda(), want2.cuda()
    eng = _engine(dtype)
    eng.autotune = False
    src = eng.tensor(64, sl)
    a = eng.conv([src], w1, b1, 1, 1, abi.LP_ACT_RELU, sl)
    d = eng.conv([a], w2, b2, 3, 2, abi.LP_ACT_RELU, sl)
    eng.finish()
    eng.bind(B, h << sl, w << sl)
    _fill(eng, src, x0)
    x = E._frame(B, h << sl, w << sl)
    eng.forward(x)
    _check(eng, [a, d], [want1, want2], 'fused 1x1 + s2: separate ops')
    tag = 'fused_pw-%d-%d-%s' % (c1, c2, DT_ID[dtype])
    _log_counts(tag, want2)
    ran = _walk(eng, [2], [d], [want2], [(abi.LP_VARIANT_FUSED_PW_S2, 3)], x, tag, B, fused_nan=[a])
    assert ran.get('fused_pw'), 'the fused form did not take the op'
    assert torch.isnan(eng.tensor_view(a).float()).all()


BIFUSION_PLAN = {
    'x0': [('nan', (0, 3, 0, 0)), ('+inf', (0, 63, 5, 13)), ('-inf', (1, 0, 2, 7)), ('nan', (1, 40, 5, 0))],
    'x1': [('+inf', (0, 127, 0, 27)), ('-inf', (0, 64, 6, 6)), ('nan', (0, 0, 11, 20)), ('nan', (1, 127, 3, 3)), ('+inf', (1, 5, 9, 14)), ('-inf', (1, 6, 9, 14))],
    'd': [('nan', (0, 63, 7, 1)), ('-inf', (0, 0, 3, 19)), ('+inf', (1, 31, 11, 27)), ('+inf', (1, 32, 0, 0))],
}


@BITS16
def test_bifusion_fused_equals_its_three_ops_on_tainted_inputs(dtype):
    """LP_VARIANT_FUSED_BIFUSION at (6, 14, 2) with NaN / +-inf in all three inputs: the bits of its three ops at every non-NaN
    element, NaN exactly where they give NaN -- its to_operand ReLU propagates like the epilogue's.  The three ops themselves carry
    the class pattern (NaN / +inf / -inf / finite) of the torch reference on the stored values."""
    from yolov6.hip import abi
    from yolov6.hip.runtime import _f32
    h, w, B, sl = 6, 14, 2, 4
    C0, C1, C = 64, 128, 64
    eng = _engine(dtype)
    eng.autotune = False
    x0, x1, d = eng.tensor(C0, sl), eng.tensor(C1, sl - 1), eng.tensor(C, sl - 1)
    u = eng.tensor(C, sl - 1)
    wd, bd = T._rand((C0, C, 2, 2), 1, (1.0 / C0) ** 0.5), T._rand((C,), 2, 0.3)
    abi.check(eng.lib.lp_engine_add_deconv2x2(eng.h, x0, u, eng._ptr(_f32(wd)), eng._ptr(_f32(bd))))
    w1, b1 = T._rand((C, C1, 1, 1), 3, (2.0 / C1) ** 0.5), T._rand((C,), 4, 0.3)
    a = eng.conv([x1], w1, b1, 1, 1, abi.LP_ACT_RELU, sl - 1)
    w3, b3 = T._rand((C, 3 * C, 1, 1), 5, (2.0 / (3 * C)) ** 0.5), T._rand((C,), 6, 0.3)
    out = eng.conv([u, a, d], w3, b3, 1, 1, abi.LP_ACT_RELU, sl - 1)
    eng.finish()
    H, W = h << sl, w << sl
    eng.bind(B, H, W)
    data = {'x0': T._rand((B, C0, h, w), 10), 'x1': T._rand((B, C1, 2 * h, 2 * w), 11), 'd': T._rand((B, C, 2 * h, 2 * w), 12)}
    data = {k: X.plant_nonfinite(v.double(), BIFUSION_PLAN[k]).float() for k, v in data.items()}
    for t, k in ((x0, 'x0'), (x1, 'x1'), (d, 'd')):
        _fill(eng, t, data[k])
    op = eng.lib.lp_engine_num_ops(eng.h) - 1
    x = E._frame(B, H, W)
    eng.forward(x)
    want = eng.tensor_view(out).clone()
    q = lambda t: t.to(dtype).double()
    ru = q(F.conv_transpose2d(q(data['x0']), q(wd), bd.double(), stride=2))
    ra = q(F.relu(F.conv2d(q(data['x1']), q(w1), b1.double())))
    ref = F.relu(F.conv2d(torch.cat([ru, ra, q(data['d'])], 1), q(w3), b3.double()))
    got = want.double().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got == INF, ref == INF) and not (ref == -INF).any()
    cnt = X.nonfinite_counts(ref)
    assert cnt['nan'] >= 0.01 * ref.numel() and cnt['+inf'] > 0 and cnt['finite'] >= 0.30 * ref.numel(), cnt
    E._log('nonfinite-bifusion-%s expected %s' % (DT_ID[dtype], cnt))
    eng.set_variant(op, abi.LP_VARIANT_FUSED_BIFUSION, 3)
    assert eng.lib.lp_engine_op_carrier(eng.h, 1, 0) == op and eng.lib.lp_engine_op_carrier(eng.h, 2, 0) == op
    for rep in range(2):
        _poison_lds()
        for t in (u, a, out):
            eng.tensor_view(t).fill_(NAN)
        eng.forward(x)
        X.assert_same_nonfinite(eng.tensor_view(out), want, 'fused BiFusion, run %d' % rep)
        assert torch.isnan(eng.tensor_view(u).float()).all() and torch.isnan(eng.tensor_view(a).float()).all()


# ---- SiLU -------------------------------------------------------------------------------------------------------------------------------
SILU_CASES = [('generic', next(c for c in T.CONV_CASES if c[4] == 'silu' and c[2] == 1 and len(c[0]) == 3), None),
              ('PIPE16', next(c[:2] + (3, 1) + c[2:] for c in T.PIPE16_CASES if c[2] == 'silu'), (39, 3))]


@BITS16
@pytest.mark.parametrize('fam,case,variant', SILU_CASES, ids=[c[0] for c in SILU_CASES])
def test_silu_epilogue_has_the_references_nonfinite_pattern(fam, case, variant, dtype):
    """x * sigmoid(x) as v * rcp(1 + exp(-v)): NaN -> NaN, +inf -> +inf, -inf -> NaN (as torch: -inf * 0), and every finite element
    inside assert_elementwise's bound.  The shapes of the parity tests (the batch of the PIPE16 case trimmed to 3)."""
    from yolov6.hip import abi
    cins, cout, k, s, act, use_res, h, w, B = case
    assert act == 'silu' and not use_res
    B, sl = min(B, 3), 5
    eng = _engine(dtype)
    eng.autotune = False
    srcs = [eng.tensor(c, sl) for c in cins]
    cin = sum(cins)
    wt, bias = T._rand((cout, cin, k, k), 1, (2.0 / (cin * k * k)) ** 0.5), T._rand((cout,), 2, 0.5)
    dst = eng.conv(srcs, wt, bias, k, s, abi.LP_ACT_SILU, sl)
    eng.finish()
    eng.bind(B, h << sl, w << sl)
    xs = [T._rand((B, c, h, w), 10 + i) for i, c in enumerate(cins)]
    for i, xv in enumerate(xs):                                      # per source and image: a NaN, a +inf and a -inf in the last / first channels
        for b in range(B):
            y0 = (3 * b + 5 * i) % h
            xv[b, -1, y0, (2 + b) % w] = NAN
            xv[b, 0, (y0 + 4) % h, w - 1 - b] = INF
            xv[b, -1, (y0 + 8) % h, (5 + i) % w] = -INF
    for t, xv in zip(srcs, xs):
        _fill(eng, t, xv)
    if variant:
        for cfg in (variant[0], 41):                                 # the fixed-tile 16x16x32 kernel that takes the layer
            try:
                eng.set_variant(1, cfg, variant[1])
                break
            except RuntimeError:
                continue
        else:
            raise AssertionError('no PIPE16 variant took the layer')
        _poison_lds()
    eng.tensor_view(dst).fill_(NAN)
    eng.forward(E._frame(B, h << sl, w << sl))
    got = eng.tensor_view(dst).float().cpu()
    ref64, mag64, K, _ = X.conv_ref64(xs, wt, bias, dtype, s, k // 2, 'silu')
    g = got.double()
    assert torch.equal(torch.isnan(g), torch.isnan(ref64)), (int(torch.isnan(g).sum()), int(torch.isnan(ref64).sum()))
    assert torch.equal(g == INF, ref64 == INF) and not (ref64 == -INF).any() and not (g == -INF).any()
    cnt = X.nonfinite_counts(ref64)
    assert cnt['nan'] > 0 and cnt['+inf'] > 0 and cnt['finite'] >= 0.30 * ref64.numel(), cnt
    E._log('nonfinite-silu-%s-%s expected %s' % (fam, DT_ID[dtype], cnt))
    fin = torch.isfinite(ref64)
    X.assert_elementwise(got[fin], ref64[fin], mag64[fin], K, dtype, transcendental=True)


# ---- (b) the SPPF pool chain ------------------------------------------------------------------------------------------------------------
def _pool_engine(dtype, c, h, w, B):
    from yolov6.hip import abi
    eng = _engine(dtype)
    ids = [eng.tensor(c, 5) for _ in range(4)]
    abi.check(eng.lib.lp_engine_add_pool5_chain(eng.h, *ids))
    eng.finish()
    eng.bind(B, h * 32, w * 32)
    return eng, ids


@ALL3
@pytest.mark.parametrize('c,h,w,B', X.POOL_NONFINITE_SHAPES, ids=lambda v: str(v))
def test_pool_chain_propagates_nan_like_max_pool2d(c, h, w, B, dtype):
    """F.max_pool2d three times: a window that holds a NaN is NaN wherever the NaN sits in it (each of the 25 positions, windows clipped
    by each border), an all -inf window is -inf.  One granule per workgroup at B = 2, the 1024-thread form at (40, 40, 40), and the forms
    with 2, 4 and 8 granules per workgroup -- those also on finite random data, bit for bit."""
    gp = X.pool_granules(c, h, w, B, torch.empty(0, dtype=dtype).element_size())
    assert gp == X.POOL_GP.get((c, h, w, B), 1)                      # the launch rule restated: the case reaches the form it is here for
    eng, ids = _pool_engine(dtype, c, h, w, B)
    frame = E._frame(B, h * 32, w * 32)
    for finite in ((False, True) if gp > 1 else (False,)):
        y = X.pool_nonfinite_data(c, h, w, B, finite=finite)
        _fill(eng, ids[0], y)
        for t in ids[1:]:
            eng.tensor_view(t).fill_(NAN)
        eng.forward(frame)
        for n, t in enumerate(ids[1:]):
            y = F.max_pool2d(y, 5, 1, 2)
            X.assert_same_nonfinite(eng.tensor_view(t), y.to(dtype), 'pool %d of (%d, %d, %d) B = %d %s%s' % (n + 1, c, h, w, B, DT_ID[dtype],
                                                                                                           ' finite' if finite else ''))
    E._log('nonfinite-pool %s c=%d h=%d w=%d B=%d granules=%d%s' % (DT_ID[dtype], c, h, w, B, gp, ' threads=1024' if (c, h, w) == (40, 40, 40) else ''))


# ---- (d) the whole model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ['yololpn', 'yololps'])
def test_one_nan_pixel_is_not_laundered_by_the_model(key):
    """fp32 engine, deploy preparation, image 0 with one NaN pixel, image 1 clean: every element the float64 oracle predicts as NaN for
    image 0 is NaN in the engine's prediction; image 1 is, bit for bit, what the engine predicts for it in the clean batch; and neither
    route of detect_padded keeps a row on image 0 that the oracle does not keep.  (No upper bound on the NaN set here: the receptive
    field covers the image, the op-level tests carry that side.)"""
    from oracle import lp_oracle
    from yolov6.hip.runtime import detect_padded, nms_padded
    import test_e2e_gpu as G
    c = X.E2E_CASES[key]
    conf, iou, max_det = X.E2E_SETTINGS[key][0]
    clean = X.e2e_input(key)
    assert clean.shape[0] >= 2
    x = clean.clone()
    x[0, 1, x.shape[2] // 2 + 3, x.shape[3] // 3] = NAN
    p64, _ = lp_oracle.forward(X.e2e_model(key).state_dict(), lp_oracle.arch(c['arch']), x, precision=torch.float64)
    nan64 = torch.isnan(p64)
    assert not nan64[1:].any() and nan64[0].any()
    m = G._engine_model(key, 'deploy')
    with torch.no_grad():
        pred_clean = m(clean.cuda())[0].clone()
        pred = m(x.cuda())[0].clone()
    got_nan = torch.isnan(pred).cpu()
    share64, share = float(nan64[0].double().mean()), float(got_nan[0].double().mean())
    with open(os.path.join(X.log_dir(), 'parity.log'), 'a') as f:
        f.write('%-44s NaN share of image 0: oracle %.4f engine %.4f\n' % ('nonfinite %s %s' % (key, 'x'.join(map(str, x.shape))), share64, share))
    print(key, 'NaN share of image 0: oracle %.4f, engine %.4f' % (share64, share))
    lost = nan64[0] & ~got_nan[0]
    assert not lost.any(), 'the engine turned %d of the oracle\'s %d NaN predictions of image 0 into numbers' % (int(lost.sum()), int(nan64[0].sum()))
    assert torch.equal(pred[1:].view(torch.int32), pred_clean[1:].view(torch.int32)), 'the clean images changed'
    want_rows, want_keep = X.nms64(p64.numpy(), conf, iou, max_det)
    with torch.no_grad():
        outs = {'forward+nms': nms_padded(pred.clone(), conf, iou, max_det, want_keep=True),
                'det': detect_padded(m, x.cuda(), conf, iou, max_det, want_keep=True, route='det'),
                'pred': detect_padded(m, x.cuda(), conf, iou, max_det, want_keep=True, route='pred')}
    for path, (det, count, kept) in outs.items():
        extra = set(kept[0, :int(count[0])].cpu().tolist()) - set(np.asarray(want_keep[0]).tolist())
        assert not extra, (path, len(extra), len(want_keep[0]))
        assert int(count[1]) > 0, path


# ---- (c) the head's box path and NMS ---------------------------------------------------------------------------------------------------
import test_head_dfl_cpu as D                                          # noqa: E402  (geometry, decode64 and the coded DFL data)
import test_head_exact_gpu as HX                                       # noqa: E402

HEAD_W = (64, 128, 256)
# (image, level, pixel of the level, channel: 'cls' = the channel every class weight is +1/4 on, an int = that channel, kind).  A NaN
# or an infinity in ONE feature of an anchor reaches every output row of that anchor (under a zero weight as NaN).  On the 'cls'
# channel +inf saturates every class probability at 1 -- the anchor passes any threshold, with a non-finite box -- and -inf at 0; on
# any other channel of the coded DFL data the class weights are zero and the class probabilities NaN.  The last pixel of every level
# is planted; channel 0 and the last channel are DFL code channels (side 0 bit 0, side 3 bit 4).
HEAD_PLAN = [(0, 0, 17, 0, 'nan'), (0, 0, 100, 'cls', '+inf'), (0, 0, 239, 'cls', '-inf'), (0, 1, 59, 1, '+inf'), (0, 2, 6, 'cls', '+inf'),
             (1, 2, 14, -1, 'nan'), (1, 1, 3, 'cls', '+inf'), (1, 0, 7, -1, '-inf'), (1, 0, 150, 'cls', '+inf'),
             (2, 2, 0, 'cls', '+inf'), (2, 1, 30, 'cls', 'nan'), (2, 0, 200, 0, '+inf'), (2, 0, 201, 'cls', '+inf'), (2, 1, 31, 'cls', '-inf')]


def head_nonfinite_case(bins, dtype):
    """Head-only data of test_head_exact_gpu (bins 1) / the coded DFL data of test_head_dfl_cpu (bins 17) with HEAD_PLAN planted:
    dict of the planted ``data``, ``proj``, the expected prediction columns 0..12 ``pred`` (fp32: the oracle's decode in float64 on
    the planted logits -- a non-finite logit of a DFL side makes its whole softmax NaN --, every finite element the exact bits of the
    unplanted case), the mask of planted anchors, the float64 mask values ``mv`` and the threshold ``conf``."""
    if bins == 1:
        data, proj = HX.head_data(HEAD_W, 100), None
    else:
        data, proj = D.coded_data(bins, HEAD_W)[0], D.coded_proj(bins)
    data = [tuple(t.clone() for t in lvl) for lvl in data]
    cls_ch = []
    for x, wc, bc, wb, bb in data:
        code = set(D._code_channels(x.shape[1]).flatten().tolist())
        ch = next(c for c in range(3, x.shape[1]) if c not in code)
        wc[:, ch] = 0.25
        cls_ch.append(ch)

    def logits(levels):
        return torch.cat([F.conv2d(x, wb[..., None, None], bb).reshape(HX.B, wb.shape[0], -1) for x, _, _, wb, bb in levels], -1).permute(0, 2, 1)

    def decode(z):
        if bins == 1:
            dist = z[..., :4]
        else:
            dist = (torch.softmax(z[..., :4 * bins].reshape(HX.B, HX.N, 4, bins), -1) * proj).sum(-1)
        return D.decode64(dist, z[..., 4 * bins:])[0]
    clean = X.to_exact_f32(decode(logits(data))) if bins == 1 else D.coded_case(bins, dtype, HEAD_W)['pred']
    mv_clean = D.mask_value64(data)
    planted = torch.zeros(HX.B, HX.N, dtype=torch.bool)
    for b, lvl, pix, ch, kind in HEAD_PLAN:
        x = data[lvl][0]
        w = HX.MAPS[lvl][1]
        x[b, cls_ch[lvl] if ch == 'cls' else ch, pix // w, pix % w] = X.NONFINITE[kind]
        planted[b, HX.LEVEL_OFF[lvl] + pix] = True
    for lvl in range(3):
        assert planted[:, HX.LEVEL_OFF[lvl + 1] - 1].any()                      # the last pixel of every level
    pred = decode(logits(data))
    e = pred.float()
    fin = torch.isfinite(pred)
    assert torch.equal(e[~planted], clean[~planted]) or bins > 1               # (bins 17: the clean anchors are coded_case's idealised one-hot)
    assert torch.equal(e[planted][fin[planted]], clean[planted][fin[planted]])  # what stays finite at a planted anchor keeps its bits
    want = clean.clone()
    want[planted] = e[planted]
    cols = D.BOX_P + D.COR_P
    cnt = X.nonfinite_counts(want[planted][:, cols])
    assert cnt['nan'] > 0 and cnt['+inf'] > 0 and cnt['-inf'] > 0, cnt
    mv = D.mask_value64(data)
    assert torch.equal(mv[~planted], mv_clean[~planted])
    conf = HX.pick_threshold(mv_clean[~planted])
    return dict(data=data, proj=proj, pred=want, planted=planted, mv=mv, conf=conf, cls_ch=cls_ch)


@ALL3
@pytest.mark.parametrize('bins', [1, 17])
def test_head_box_path_and_nms_on_nonfinite_features(bins, dtype):
    """Prediction columns 0..3 and 5..12 carry the pattern of the oracle's decode in float64 (finite columns: the exact bits); lp_nms
    on that tensor equals the C oracle and lp_testing.nms64 -- the planted anchors that pass are kept, whatever their box: a box with
    NaN or infinite coordinates suppresses nothing and is suppressed by nothing --; the detections-only route equals lp_nms on a
    stale and on a 0xFF-filled workspace."""
    from yolov6.hip import abi, runtime
    from yolov6.hip.runtime import _f32
    import test_head_cls_gpu as HC
    B, N, H, W = HX.B, HX.N, HX.H, HX.W
    c = head_nonfinite_case(bins, dtype)
    conf, planted = c['conf'], c['planted']
    eng = _engine(dtype)
    eng.autotune = False
    feats = [eng.tensor(ch, 3 + i) for i, ch in enumerate(HEAD_W)]
    for i, (f, (_, wc, bc, wb, bb)) in enumerate(zip(feats, c['data'])):
        abi.check(eng.lib.lp_engine_add_head_cls(eng.h, f, i, HX.NCLS, eng._ptr(_f32(wc)), eng._ptr(_f32(bc))))
        abi.check(eng.lib.lp_engine_add_head_box(eng.h, f, i, bins, eng._ptr(_f32(wb)), eng._ptr(_f32(bb)), eng._ptr(_f32(c['proj'])) if bins > 1 else None))
    eng.finish()
    eng.bind(B, H, W)
    assert eng.n_anchors == N

    def fill(levels):
        for f, lvl in zip(feats, levels):
            _fill(eng, f, lvl[0])
    fill(c['data'])
    x = torch.zeros(B, 3, H, W, device='cuda:0')
    pred = eng.forward(x).clone()
    cols = D.BOX_P + D.COR_P
    what = 'head bins %d %s' % (bins, DT_ID[dtype])
    X.assert_same_nonfinite(pred[..., cols].contiguous(), c['pred'][..., cols].contiguous(), what + ': prediction columns 0..3, 5..12')
    assert torch.equal(pred[..., 4], torch.ones_like(pred[..., 4]))
    det, rows_c, keep_c = HC._assert_nms_equals_oracle(pred, conf, HX.IOU, HX.MAX_DET, what)
    _, keep64 = X.nms64(pred.double().cpu().numpy(), conf, HX.IOU, HX.MAX_DET)
    must = planted & (c['mv'] >= conf)                                  # (a NaN mask value passes nothing)
    assert int(must.sum()) >= 4 and int((planted & ~must).sum()) >= 4
    for b in range(B):
        assert np.array_equal(np.asarray(keep64[b]), keep_c[b]), (what, b)
        kept = set(keep_c[b].tolist())
        assert set(torch.nonzero(must[b]).flatten().tolist()) <= kept and not (set(torch.nonzero(planted[b] & ~must[b]).flatten().tolist()) & kept)
    assert int(det[1].sum()) > int(must.sum())
    other = HX.head_data(HEAD_W, 500) if bins == 1 else D.coded_data(bins, HEAD_W, seed=900)[0]
    ws = eng.det_workspace(B, H, W)
    for stale in (True, False):
        if stale:
            fill(other)
            eng.forward_det(x, conf, ws=ws)
            runtime.nms_candidates((ws, B, N), HX.IOU, HX.MAX_DET, want_keep=True)
            fill(c['data'])
        else:
            ws.fill_(0xFF)
        eng.forward_det(x, conf, ws=ws)
        got = runtime.nms_candidates((ws, B, N), HX.IOU, HX.MAX_DET, want_keep=True)
        assert torch.equal(got[1], det[1]), (what, stale)
        for b in range(B):
            n = int(det[1][b])
            assert torch.equal(got[2][b, :n], det[2][b, :n]), (what, stale, b)
            assert HC._same(got[0][b, :n].cpu().numpy(), det[0][b, :n].cpu().numpy()), (what, stale, b)
