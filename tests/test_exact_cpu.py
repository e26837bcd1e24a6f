"""CPU tests of the exact-arithmetic test machinery itself (tests/lp_testing.py): the grid-data generators meet the conditions the
GPU tests rely on, the exact reference does not depend on the fp32 summation order, and the checkers reject subtly wrong results
that the max-norm check of the parity tests lets pass.  No device, no library call besides the engine's host-side graph builder."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lp_testing as X
from lp_testing import rel_err
from test_hip_kernels import TOL

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
CASES = X.exact_conv_cases()
MIN_INEXACT, MIN_TIES = 0.25, 0.01      # stated conditions on the data: a quarter of the outputs need rounding, 1 % are ties


def _crop(h, w, s, cap=24):
    """The conditions are statistics of i.i.d. data: a map cropped to `cap` rows / columns has the same distribution."""
    return min(h, cap * s), min(w, cap * s)


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_grid_data_meets_its_conditions(case):
    """Every shape of the GPU bit-equality tests: inputs on their grids and held exactly by the storage type, the bound on
    sum|x||w| + |b| (checked with the float64 sum itself here, not only its analytic bound), the float64 reference an exact fp32
    value, and -- fp16 / bf16 -- enough outputs that need rounding and enough exact ties, for both epilogues."""
    _, cins, cout, k, s, h, w, B = case
    h, w = _crop(h, w, s)
    conv = None
    for dtype in (F16, BF16, F32):
        xs, wt, bias, res = X.grid_inputs(cins, cout, k, 1, h, w, dtype, res_hw=(h // s, w // s))
        X.assert_grid_exact(xs, wt, bias, dtype)
        if conv is None:                                 # x and w have the same range for every dtype: one float64 convolution
            conv = F.conv2d(torch.cat(xs, 1), wt, None, stride=s, padding=k // 2)
            mag = F.conv2d(torch.cat(xs, 1).abs(), wt.abs(), None, stride=s, padding=k // 2)
        pre = conv + bias.view(1, -1, 1, 1)
        assert float((mag + bias.abs().view(1, -1, 1, 1)).max()) < 2 ** 24 / 16
        for act in ('none', 'relu'):
            X.exact_epilogue(pre, act, dtype)             # asserts the exact float64 -> float32 round trip
            X.exact_epilogue(pre, act, dtype, res)        # ... and of the residual sum
            if dtype != F32:
                inexact, ties = X.rounding_stats(pre, act, dtype)
                assert inexact >= MIN_INEXACT and ties >= MIN_TIES, (dtype, act, inexact, ties)


@pytest.mark.parametrize('name,size', X.MODEL_CONFIGS)
def test_model_layer_data_meets_its_conditions(name, size):
    """The same for the distinct layers of the benchmark's models, as the engine's graph builder lowers them."""
    sigs = X.model_layer_signatures(name, size)
    assert len(sigs) >= 30
    assert any(isinstance(c[1], tuple) for c in sigs) and any(c[4] for c in sigs) == (name == 'yolov6m')
    for cins, cout, k, s, use_res, h, w, sl in sigs:
        co = sum(cout) if isinstance(cout, tuple) else cout
        assert h == size >> sl and h % s == 0
        h, w = _crop(h, w, s, cap=8)
        for dtype in (F16, BF16):
            xs, wt, bias, res = X.grid_inputs(cins, co, k, 1, h, w, dtype, res_hw=(h // s, w // s) if use_res else None)
            X.assert_grid_exact(xs, wt, bias, dtype)
            _, pre = X.exact_conv(xs, wt, bias, k, s, 'relu', dtype, res)
            inexact, ties = X.rounding_stats(pre, 'relu', dtype)
            assert inexact >= MIN_INEXACT and ties >= MIN_TIES, (cins, cout, k, s, dtype, inexact, ties)


def test_data_of_the_other_gpu_tests_meets_its_conditions():
    """Two-destination pairs, the transposed convolution, the stem on an NCHW frame, the two fused two-layer forms (the second sum
    stays exact on the ROUNDED first output), the batch sweep of the block-tiled kernels and the special-value cases."""
    import test_exact_gpu as G
    for dtype in (F16, BF16):
        pres = [G.pair_data(c, dtype)[3] for c in G.PAIRS]
        pres += [G.deconv_data(*c, dtype)[3] for c in G.DECONV_SHAPES]
        pres += [G.stem_data(*c, dtype)[3] for c in G.STEM_SHAPES]
        for stride in (1, 2):
            xs, wt, bias, _ = X.grid_inputs([64], 128, 3, 4, 20 * stride, 20 * stride, dtype)
            X.assert_grid_exact(xs, wt, bias, dtype)
            pres.append(F.conv2d(xs[0], wt, bias, stride=stride, padding=1))
        for pre in pres:
            X.to_exact_f32(pre)
            G._assert_rounding_exercised(pre, dtype, tuple(pre.shape))
        for c in G.FUSED_STEM_SHAPES:
            G.fused_data('stem', *c, dtype, B=1)                 # asserts exactness of both sums and the rounding statistics
        for c in G.FUSED_PW_SHAPES:
            G.fused_data('pw', *c, dtype, B=1)
        for case in G.SPECIAL:
            wants = G.special_data(case, dtype)[4]
            assert not any(torch.isnan(v.float()).any() for v in wants)
    y = G.special_data(G.SPECIAL[0], F16)[4][0].float()
    assert torch.isinf(y).any() and torch.isfinite(y).any()
    y = G.special_data(G.SPECIAL[1], F16)[4][0].float()
    assert ((y != 0) & (y.abs() < 2.0 ** -14)).float().mean() > 0.01
    x = G.special_data(G.SPECIAL[2], F16)[0][0]
    assert ((x != 0) & (x.abs() < 2.0 ** -14)).float().mean() > 0.1


def test_ulp_and_rounding_helpers():
    v = torch.tensor([0.0, 1.0, 1.5, 2047.0, 2048.0, 65504.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -15], dtype=torch.float64)
    assert X.ulp(v, F16).tolist() == [2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 1.0, 2.0, 32.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24]
    assert X.ulp(torch.tensor([1.0, 300.0], dtype=torch.float64), BF16).tolist() == [2.0 ** -7, 2.0]
    assert X.ulp(torch.tensor([1.0], dtype=torch.float64), F32).tolist() == [2.0 ** -23]
    # round-to-nearest-even of torch's conversion on exact ties: 2049 -> 2048, 2051 -> 2052 in fp16; 257 -> 256, 259 -> 260 in bf16
    assert torch.tensor([2049.0, 2051.0]).to(F16).tolist() == [2048.0, 2052.0]
    assert torch.tensor([257.0, 259.0]).to(BF16).tolist() == [256.0, 260.0]
    g = X.grid_rand((1000,), 3, -2.0, 2.0, 0.25)
    assert float(g.min()) == -2.0 and float(g.max()) == 2.0 and torch.equal(torch.round(g * 4), g * 4) and g.dtype == torch.float64
    with pytest.raises(AssertionError):
        X.grid_rand((4,), 0, -1, 1, 0.3)
    with pytest.raises(AssertionError):
        X.to_exact_f32(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
    a = torch.tensor([0.0, 1.0, float('nan')], dtype=F16)
    assert X.bit_mismatches(a, torch.tensor([-0.0, 1.0, float('nan')], dtype=F16)) == 0       # same NaN bits; zeros of either sign
    assert X.bit_mismatches(a, torch.tensor([0.0, 1.0, 2.0], dtype=F16)) == 1


@pytest.mark.parametrize('dtype', [F16, BF16, F32], ids=['f16', 'bf16', 'f32'])
def test_exact_reference_does_not_depend_on_the_fp32_summation_order(dtype):
    """im2col rows of a 96-channel 3x3 layer (K = 864 + bias) summed in fp32 sequentially in the natural, the reversed and three
    random K orders, bias first or last, and pairwise (numpy): always the float64 sum, bit for bit."""
    cin, cout, h, w = 96, 8, 6, 7
    xs, wt, bias, _ = X.grid_inputs([cin], cout, 3, 1, h, w, dtype)
    X.assert_grid_exact(xs, wt, bias, dtype)
    pre = F.conv2d(xs[0], wt, bias, padding=1)
    cols = F.unfold(xs[0], 3, padding=1)[0].t().numpy().astype(np.float32)          # [h*w, K]
    wk = wt.reshape(cout, -1).numpy().astype(np.float32)                             # [cout, K]
    want = X.to_exact_f32(pre)[0].reshape(cout, -1).t().numpy()                      # [h*w, cout]
    rng = np.random.default_rng(5)
    K = wk.shape[1]
    orders = [np.arange(K), np.arange(K)[::-1]] + [rng.permutation(K) for _ in range(3)]
    b32 = bias.numpy().astype(np.float32)
    for o in orders:
        prod = (cols[:, None, o] * wk[None, :, o]).astype(np.float32)                # [h*w, cout, K] exact products
        first = np.cumsum(np.concatenate([np.broadcast_to(b32[None, :, None], prod.shape[:2] + (1,)), prod], 2), axis=2, dtype=np.float32)[..., -1]
        last = (np.cumsum(prod, axis=2, dtype=np.float32)[..., -1] + b32[None]).astype(np.float32)
        pair = (prod.sum(2, dtype=np.float32) + b32[None]).astype(np.float32)
        for got in (first, last, pair):
            assert got.dtype == np.float32 and np.array_equal(got, want)


# ---- mutants: subtly wrong results, made on the CPU from the reference itself ------------------------------------------------
MUTANTS = ['one-ulp', 'dropped-product', 'truncation', 'missing-halo-pixel', 'unrounded-activation']


def _truncate(v64, dtype):
    """float64 -> storage type by truncation towards zero instead of round-to-nearest-even."""
    r = v64.float().to(dtype)
    over = r.double().abs() > v64.abs()
    bits = r.view(torch.int16)                            # sign-magnitude: the pattern minus one is the next value towards zero
    return torch.where(over, bits - 1, bits).view(dtype)


def _mutant_setup(dtype):
    """A 64-channel 3x3 ReLU layer with the residual epilogue on grid data: inputs, exact pre-activation sums, magnitudes."""
    cin, cout, h, w = 64, 32, 12, 10
    xs, wt, bias, res = X.grid_inputs([cin], cout, 3, 1, h, w, dtype, res_hw=(h, w))
    X.assert_grid_exact(xs, wt, bias, dtype)
    pre = F.conv2d(xs[0], wt, bias, padding=1)
    mag = F.conv2d(xs[0].abs(), wt.abs(), bias.abs(), padding=1)
    return xs[0], wt, bias, res, pre, mag, cin * 9


def _mutant(name, dtype):
    """(mutated result, correct result, float64 reference of the elementwise checker, magnitudes, K, extra slack)."""
    x, wt, bias, res, pre, mag, K = _mutant_setup(dtype)
    u = X.ulp(torch.relu(pre), dtype)
    acc = 1.1 * K * 2.0 ** -24 * mag                       # the accumulation term of the elementwise bound
    want = X.exact_epilogue(pre, 'relu', dtype)
    ref64 = torch.relu(pre)
    if name == 'one-ulp':
        # the elementwise bound allows one ulp on purpose (a boundary flip): the mutant moves AWAY from the reference, at the
        # element whose reference needed the most rounding beyond the accumulation term
        err = (want.double() - ref64)
        i = int(((err.abs() - acc) * (ref64 > 0)).flatten().argmax())
        assert float((err.abs() - acc).flatten()[i]) > 0
        got = want.clone()
        step = X.ulp(want.double(), dtype).flatten()[i] * (1.0 if float(err.flatten()[i]) > 0 else -1.0)
        got.view(-1)[i] = (want.double().flatten()[i] + step).float().to(dtype)
        assert X.bit_mismatches(got, want) == 1
        return got, want, ref64, mag, K, None
    if name == 'dropped-product':
        # one x * w with 2 <= |x w| <= 4 (a typical product), at an output that is positive and whose ulp is at most 1/2
        ok = (ref64 > 8) & (u <= 0.5)
        b, co, oy, ox = [int(t[0]) for t in torch.nonzero(ok[:, :, 1:-1, 1:-1], as_tuple=True)]
        oy, ox = oy + 1, ox + 1
        p = x[b, :, oy - 1:oy + 2, ox - 1:ox + 2] * wt[co]
        cand = torch.nonzero((p.abs() >= 2) & (p.abs() <= 4))
        c, ky, kx = cand[0].tolist()
        pre2 = pre.clone()
        pre2[b, co, oy, ox] -= p[c, ky, kx]
        return X.exact_epilogue(pre2, 'relu', dtype), want, ref64, mag, K, None
    if name == 'truncation':
        return _truncate(ref64, dtype), want, ref64, mag, K, None
    if name == 'missing-halo-pixel':
        # output pixel (0, 0) of image 0 without its neighbour (1, 1): all channels of one halo pixel of the corner tile
        pre2 = pre.clone()
        pre2[0, :, 0, 0] -= (x[0, :, 1, 1][None] * wt[:, :, 2, 2]).sum(1)
        return X.exact_epilogue(pre2, 'relu', dtype), want, ref64, mag, K, None
    if name == 'unrounded-activation':
        want = X.exact_epilogue(pre, 'relu', dtype, res)
        got = X.to_exact_f32(torch.relu(pre) + X.RES_ALPHA * res).to(dtype)            # ONE rounding instead of two
        y1 = torch.relu(pre).float().to(dtype).double()
        return got, want, y1 + X.RES_ALPHA * res, mag + X.RES_ALPHA * res.abs(), K, X.ulp(y1, dtype)
    raise KeyError(name)


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('name', MUTANTS)
def test_bit_checker_rejects_every_mutant(name, dtype):
    got, want, _, _, _, _ = _mutant(name, dtype)
    n = X.bit_mismatches(got, want)
    assert n >= 1
    if name in ('one-ulp', 'dropped-product'):
        assert n == 1                                     # a single element of 3840: the checker has no tolerance to hide it in
    with pytest.raises(AssertionError):
        X.assert_bits(got, want, name)
    X.assert_bits(want.clone(), want)


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('name', ['one-ulp', 'dropped-product', 'missing-halo-pixel'])
def test_elementwise_checker_rejects_the_mutants_above_one_ulp(name, dtype):
    got, want, ref64, mag, K, slack = _mutant(name, dtype)
    X.assert_elementwise(want, ref64, mag, K, dtype, slack64=slack)            # the correct result passes
    with pytest.raises(AssertionError):
        X.assert_elementwise(got, ref64, mag, K, dtype, slack64=slack)


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('name', ['truncation', 'unrounded-activation'])
def test_elementwise_bound_cannot_see_the_sub_ulp_mutants(name, dtype):
    """Stated limit of the elementwise bound, pinned here so that nobody relies on it for rounding: it grants one ulp of the storage
    type per element (half an ulp of rounding + a boundary flip of the fp32 sum), and truncation or a skipped intermediate rounding
    stay below one ulp in every element.  Worst error / bound of a mutant: below 1 (truncation: above the 1/2 that
    round-to-nearest-even cannot exceed on this data).  Only the bit-exact check on grid data (test_bit_checker_rejects_every_mutant) sees these two."""
    got, want, ref64, mag, K, slack = _mutant(name, dtype)
    worst_ok, _ = X.elementwise_excess(want, ref64, mag, K, dtype, slack64=slack)
    worst, _ = X.elementwise_excess(got, ref64, mag, K, dtype, slack64=slack)
    assert worst_ok <= 0.5 and worst_ok < worst < 1.0 and (worst > 0.5 or name != 'truncation'), (worst_ok, worst)
    assert X.bit_mismatches(got, want) > 0.1 * got.numel() or name == 'unrounded-activation'


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('name', MUTANTS[:3])
def test_max_norm_check_accepts_the_first_three_mutants(name, dtype):
    """What the parity tests assert (rel_err <= TOL against the fp32 reference) lets the one-ulp, the dropped-product and the
    truncation mutant pass -- the gap the exact tests close."""
    got, want, ref64, _, _, _ = _mutant(name, dtype)
    assert X.bit_mismatches(got, want) >= 1
    assert rel_err(got.float(), ref64.float()) <= TOL[dtype]
