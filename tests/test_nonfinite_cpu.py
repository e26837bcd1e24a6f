"""NaN and infinities through the engine's ops: the reference's semantics, the conditions on the planted data and the mutant checks of
tests/test_nonfinite_gpu.py -- all on the CPU, from the reference alone.

The reference (oracle/lp_oracle.py) is torch: F.conv2d, F.relu, F.silu, F.max_pool2d, softmax.  In all of them a NaN operand gives NaN,
inf * 0 gives NaN and +inf + -inf gives NaN; relu(-inf) = +0, silu(-inf) = NaN, a pooling window that holds a NaN is NaN.  The helpers
of lp_testing.py (conv_nonfinite_ref, nonfinite_epilogue, pool_chain_sep) restate that explicitly; here they are tied to torch, the
planted cases are shown to exercise every class and every way a NaN arises, and each wrong implementation the GPU tests are meant to
catch (the mutants) is shown to change what those tests assert, on the data of every case it applies to."""
import pytest
import torch
import torch.nn.functional as F

import lp_testing as X
import test_nonfinite_gpu as G

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
STORED = [F16, BF16, F32]
DT_ID = {F16: 'f16', BF16: 'bf16', F32: 'f32'}
NAN, INF = float('nan'), float('inf')
CASES = list(X.NONFINITE_CONV_CASES)


def _differs(a, b):
    """What assert_same_nonfinite counts between two expected tensors: (NaN-ness differs, bits of non-NaN elements differ)."""
    n, v = X.same_nonfinite_mismatches(a, b)
    return int(n), int(v)


# ---- the reference's semantics, restated against torch ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', STORED + [F64], ids=lambda d: str(d).split('.')[-1])
def test_reference_semantics_of_relu_silu_pool_conv_softmax(dtype):
    v = torch.tensor([NAN, INF, -INF, -0.0, -1.5, 2.0], dtype=dtype)
    r = torch.relu(v)
    assert torch.isnan(r[0]) and r[1] == INF and r[2] == 0 and r[3] == 0 and r[4] == 0 and r[5] == 2
    assert torch.equal(torch.isnan(F.relu(v)), torch.isnan(r))
    s = F.silu(v)
    assert torch.isnan(s[0]) and s[1] == INF and torch.isnan(s[2]) and s[3] == 0          # silu(-inf) = -inf * 0
    # a pooling window that holds a NaN is NaN wherever the NaN sits; an all -inf window is -inf
    x = torch.zeros(1, 1, 7, 7, dtype=dtype)
    x[0, 0, 3, 3] = NAN
    assert torch.isnan(F.max_pool2d(x, 5, 1, 2)[0, 0, 1:6, 1:6]).all() and int(torch.isnan(F.max_pool2d(x, 5, 1, 2)).sum()) == 25
    assert bool((F.max_pool2d(torch.full((1, 1, 5, 5), -INF, dtype=dtype), 5, 1, 2) == -INF).all())
    if dtype in (F32, F64):                                                                # (the CPU conv of the 16-bit types is the fp32 one)
        # conv: a zero weight under a NaN or an infinity gives NaN, and so does an infinite weight over the zero padding
        x = torch.ones(1, 1, 3, 3, dtype=dtype)
        x[0, 0, 1, 1] = NAN
        w = torch.ones(1, 1, 3, 3, dtype=dtype)
        w[0, 0, 1, 1] = 0
        assert torch.isnan(F.conv2d(x, w, padding=1)[0, 0, 1, 1])
        x[0, 0, 1, 1] = INF
        assert torch.isnan(F.conv2d(x, w, padding=1)[0, 0, 1, 1]) and F.conv2d(x, w, padding=1)[0, 0, 0, 0] == INF
        w = torch.ones(1, 1, 3, 3, dtype=dtype)
        w[0, 0, 0, 0] = INF
        y = F.conv2d(torch.ones(1, 1, 3, 3, dtype=dtype), w, padding=1)
        assert torch.isnan(y[0, 0, 0, :]).all() and torch.isnan(y[0, 0, :, 0]).all() and bool((y[0, 0, 1:, 1:] == INF).all())
    # softmax (the DFL decode): NaN or +inf among the logits, or nothing but -inf, make every weight NaN; a single -inf gets weight 0
    for logits, all_nan in (([0.0, NAN, 1.0], True), ([0.0, INF, 1.0], True), ([-INF, -INF, -INF], True), ([0.0, -INF, 1.0], False)):
        p = torch.softmax(torch.tensor(logits, dtype=dtype), 0)
        assert bool(torch.isnan(p).all()) == all_nan and (all_nan or (p[1] == 0 and torch.isfinite(p).all()))


def test_relu_of_the_helper_is_torchs():
    v = torch.tensor([NAN, INF, -INF, -0.0, 0.0, -1.5, 2.0, 70000.0], dtype=F64)
    for dtype in STORED:
        got, want = X.nonfinite_epilogue(v, 'relu', dtype), torch.relu(v).float().to(dtype)
        assert _differs(got, want) == (0, 0)
        assert torch.isnan(got[0]) and got[1] == INF and got[2] == 0 and not torch.signbit(got[2])
    assert X.nonfinite_epilogue(v, 'relu', F16)[7] == INF                                  # overflow of the ONE rounding
    # +inf in the activation and -inf in the residual: NaN; the other way round for 'none'
    pre, res = torch.tensor([INF, -INF, 1.0, -INF]), torch.tensor([-INF, INF, NAN, -INF])
    y = X.nonfinite_epilogue(pre.double(), 'none', F16, res.double())
    assert torch.isnan(y[:3]).all() and y[3] == -INF
    y = X.nonfinite_epilogue(pre.double(), 'relu', F16, res.double())
    assert torch.isnan(y[0]) and y[1] == INF and torch.isnan(y[2]) and y[3] == -INF       # relu(-inf) = 0, then 0 + alpha * res


def test_helpers_on_finite_data_are_the_exact_tests_helpers():
    for dtype in STORED:
        xs, wt, bias, res = X.grid_inputs([16], 24, 3, 2, 8, 8, dtype, res_hw=(8, 8))
        pre = X.conv_nonfinite_ref(xs, wt, bias, 3, 1)
        assert torch.equal(pre, F.conv2d(xs[0], wt, bias, padding=1))
        for act, r in X.EPILOGUES4:
            assert X.bit_mismatches(X.nonfinite_epilogue(pre, act, dtype, res if r else None), X.exact_epilogue(pre, act, dtype, res if r else None)) == 0
    wd = X.grid_rand((16, 24, 2, 2), 3)
    assert torch.equal(X.conv_nonfinite_ref(xs, wd, bias, 2, 2, transposed=True), F.conv_transpose2d(xs[0], wd, bias, stride=2))


def test_assert_same_nonfinite_notices_each_kind_of_difference():
    want = torch.tensor([NAN, INF, -INF, 0.0, 1.0, 2.0], dtype=F16)
    same = want.clone()
    same[0] = -torch.tensor(NAN, dtype=F16)                      # sign and payload of a NaN are free; +0.0 == -0.0
    same[3] = -0.0
    X.assert_same_nonfinite(same, want)
    for i, v in ((0, 0.0), (1, -INF), (2, INF), (1, 65504.0), (4, NAN), (5, 2.002)):
        bad = want.clone()
        bad[i] = v
        with pytest.raises(AssertionError) as e:
            X.assert_same_nonfinite(bad, want, 'probe')
        assert "'nan':" in str(e.value) and "'+inf':" in str(e.value) and "'-inf':" in str(e.value)      # the counts of each class


# ---- the planted conv cases: conditions from the reference alone ------------------------------------------------------------------
@pytest.mark.parametrize('dtype', STORED, ids=list(DT_ID.values()))
@pytest.mark.parametrize('name', CASES)
def test_planted_conv_case_exercises_every_class(name, dtype):
    d = X.nonfinite_conv_data(name, dtype)
    c, pre, (n_nan, n_pos, n_neg) = d['case'], d['pre'], d['terms']
    # the inputs: a handful of planted elements, everything else on the grid; image 1's plan is not image 0's
    for x, plan in zip(d['xs'], c['x']):
        assert 0 < int((~torch.isfinite(x)).sum()) <= 32 and plan
        assert not torch.equal(torch.isfinite(x[0]), torch.isfinite(x[1]))
    total = pre.numel()
    none = d['wants'][('none', False)].double()
    cnt = X.nonfinite_counts(none)
    for kind in ('nan', '+inf', '-inf'):
        assert cnt[kind] >= 0.01 * total, (kind, cnt)
    for key, want in d['wants'].items():
        k = X.nonfinite_counts(want)
        assert k['finite'] >= 0.30 * total, (key, k)
        for b in range(2):
            assert X.nonfinite_counts(want[b])['finite'] >= 0.30 * want[b].numel()
    # how the NaNs arise: a NaN term (a planted NaN, or an infinity under a zero weight) ...
    assert int(((n_nan > 0)).sum()) > 0 and torch.isnan(pre[n_nan > 0]).all()
    zero_w = (d['wt'] == 0).any()
    assert bool(zero_w)
    # ... and, with no NaN term at all, +inf and -inf terms meeting in one sum
    meet = (n_nan == 0) & (n_pos > 0) & (n_neg > 0)
    assert int(meet.sum()) > 0 and torch.isnan(pre[meet]).all()
    assert torch.equal(torch.isnan(pre), (n_nan > 0) | meet)
    assert torch.equal(pre == INF, (n_nan == 0) & (n_pos > 0) & (n_neg == 0)) and torch.equal(pre == -INF, (n_nan == 0) & (n_neg > 0) & (n_pos == 0))
    if ('relu', False) in d['wants']:
        relu = d['wants'][('relu', False)].double()
        m = pre == -INF
        assert int(m.sum()) > 0 and bool((relu[m] == 0).all()) and not torch.signbit(relu[m]).any()          # -inf -> +0
        assert torch.equal(torch.isnan(relu), torch.isnan(pre)) and torch.equal(relu == INF, pre == INF)
    for act in ('none', 'relu'):
        if (act, True) in d['wants']:
            plain, with_res = d['wants'][(act, False)].double(), d['wants'][(act, True)].double()
            only_res = torch.isnan(with_res) & ~torch.isnan(plain)
            by_meeting = only_res & ~torch.isnan(d['res'])                                  # +inf activation, -inf residual (or -inf, +inf)
            by_nan = only_res & torch.isnan(d['res'])
            assert int(by_meeting.sum()) > 0 and int(by_nan.sum()) > 0, (act, int(by_meeting.sum()), int(by_nan.sum()))
            assert bool(torch.isnan(with_res)[torch.isnan(plain)].all())


def test_weight_case_turns_the_padding_taps_into_nan():
    for dtype in STORED:
        d = X.nonfinite_weight_data(dtype)
        pre = d['pre']
        assert torch.isfinite(torch.cat(d['xs'], 1)).all() and int((~torch.isfinite(d['wt'])).sum()) == 1
        assert torch.isnan(pre[:, 5, 0, :]).all() and torch.isnan(pre[:, 5, :, 0]).all()          # the tap lies on the padding there
        inner, x_under = pre[:, 5, 1:, 1:], d['xs'][0][:, 20, :-1, :-1]
        assert torch.equal(inner == INF, x_under > 0) and torch.equal(inner == -INF, x_under < 0) and torch.equal(torch.isnan(inner), x_under == 0)
        assert int((x_under > 0).sum()) and int((x_under < 0).sum()) and int((x_under == 0).sum())
        rest = torch.ones(128, dtype=torch.bool)
        rest[5] = False
        assert torch.isfinite(pre[:, rest]).all()


@pytest.mark.parametrize('dtype', STORED, ids=list(DT_ID.values()))
def test_stem_case_and_the_wider_footprint_of_the_lowered_stem(dtype):
    """The expected tensor of the stem is the product sum over the LOWERED weights (3x3 stride 1 over the 12 space-to-depth channels, 81
    of 108 weights structural zeros): equal to the reference's 3x3 stride-2 sum wherever both are finite, NaN wherever the reference
    is NaN or infinite under a structural zero -- a strictly wider NaN set.  The conditions of the planted cases hold for it too."""
    for xdt in dict.fromkeys((dtype, F32, F16)):
        sent, x_eff, wt, bias, pre, pre_ref = G.stem_data(dtype, xdt)
        assert sent.dtype == xdt and float(sent[G.STEM_BIG[0]]) == float(torch.tensor(G.BIG).to(xdt)) and (xdt != F16 or float(sent[G.STEM_BIG[0]]) == INF)
        assert (x_eff[G.STEM_BIG[0]] == INF) == (F16 in (dtype, xdt))
        both = torch.isfinite(pre) & torch.isfinite(pre_ref)
        assert torch.equal(pre[both], pre_ref[both]) and torch.equal(torch.isfinite(pre) & ~both, torch.zeros_like(both))
        assert bool(torch.isnan(pre)[torch.isnan(pre_ref)].all()) and int(torch.isnan(pre).sum()) > int(torch.isnan(pre_ref).sum())
        wider = torch.isnan(pre) & ~torch.isnan(pre_ref)
        assert bool(torch.isfinite(pre_ref[wider]).any())                      # numbers in the reference, NaN in the engine: by design
        cnt = X.nonfinite_counts(X.nonfinite_epilogue(pre, 'none', dtype))
        for kind in ('nan', '+inf', '-inf'):
            assert cnt[kind] >= 0.01 * pre.numel(), (kind, cnt)
        assert cnt['finite'] >= 0.30 * pre.numel()
        relu = X.nonfinite_epilogue(pre, 'relu', dtype)
        assert int((pre == -INF).sum()) > 0 and bool((relu[pre == -INF] == 0).all())
        assert _differs(X.nonfinite_epilogue(pre, 'relu', dtype, relu='select'), relu)[0] > 0
        skipped = X.conv_nonfinite_ref([G.space_to_depth(x_eff)], G.lowered_stem_weights(wt), bias, 3, 1, skip='zero_weights')
        assert _differs(X.nonfinite_epilogue(skipped, 'none', dtype), X.nonfinite_epilogue(pre, 'none', dtype))[0] > 0


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('kind,c1,c2,H,W', [('stem',) + s + (G.FUSED_STEM_HW,) * 2 for s in G.FUSED_STEM] + [('pw',) + G.FUSED_PW])
def test_fused_cases_and_their_inner_relu_mutant(kind, c1, c2, H, W, dtype):
    """Two ReLU layers: most outputs stay finite, NaN and +inf both occur, and a select ReLU between the layers (what a fused kernel
    keeps in LDS) changes the NaN set of the second layer's output."""
    *_, y1, want2 = G.fused_data(kind, c1, c2, H, W, dtype)
    c1n, c2n = X.nonfinite_counts(y1), X.nonfinite_counts(want2)
    assert c1n['finite'] >= 0.30 * y1.numel() and c1n['nan'] > 0 and c1n['+inf'] > 0 and c1n['-inf'] == 0, c1n
    assert c2n['finite'] >= 0.30 * want2.numel() and c2n['nan'] >= 0.01 * want2.numel() and c2n['-inf'] == 0, c2n      # (NaN wins most sums)
    *_, m1, m2 = G.fused_data(kind, c1, c2, H, W, dtype, relu='select')
    assert _differs(m1, y1)[0] > 0 and _differs(m2, want2)[0] > 0
    if kind == 'stem':
        # the fused kernel runs the four live taps of the lowered stem: its NaN set lies between the reference's and the stand-alone stem's
        x0, w1, b1, w2, b2, f1, f2 = G.fused_data(kind, c1, c2, H, W, dtype, four_taps=True)
        ref1 = X.nonfinite_epilogue(X.conv_nonfinite_ref([x0], w1, b1, 3, 2), 'relu', dtype)
        n_ref, n_four, n_nine = torch.isnan(ref1), torch.isnan(f1), torch.isnan(y1)
        assert bool(n_four[n_ref].all()) and bool(n_nine[n_four].all()) and int(n_ref.sum()) < int(n_four.sum()) < int(n_nine.sum())
        both = ~n_four & ~n_nine
        assert _differs(f1[both], y1[both]) == (0, 0)
        cnt = X.nonfinite_counts(f2)
        assert cnt['finite'] >= 0.30 * f2.numel() and cnt['nan'] >= 0.01 * f2.numel(), cnt
        assert _differs(G.fused_data(kind, c1, c2, H, W, dtype, relu='select', four_taps=True)[-1], f2)[0] > 0


# ---- the mutants --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', STORED, ids=list(DT_ID.values()))
@pytest.mark.parametrize('name', CASES)
def test_conv_mutants_change_what_the_gpu_tests_assert(name, dtype):
    """ReLU as a select, a conv that skips zero weights, a residual added in front of the rounding: each changes the expected tensor
    of every case (and epilogue) it applies to -- in its NaN mask, or in the bits of finite elements for the residual order."""
    d = X.nonfinite_conv_data(name, dtype)
    c = d['case']
    tr = bool(c.get('transposed'))
    for act, r in c['epilogues']:
        want = d['wants'][(act, r)]
        res = d['res'] if r else None
        if act == 'relu':
            lost, _ = _differs(X.nonfinite_epilogue(d['pre'], act, dtype, res, relu='select'), want)
            assert lost > 0, (name, act, r)
        if r and dtype != F32:                                                 # (fp32 storage: the first rounding is the identity)
            nan_d, bits_d = _differs(X.nonfinite_epilogue(d['pre'], act, dtype, res, res_first=True), want)
            assert bits_d > 0, (name, act, r)
    skipped = X.conv_nonfinite_ref(d['xs'], d['wt'], d['bias'], c['k'], c['s'], transposed=tr, skip='zero_weights')
    for act, r in c['epilogues']:
        lost, _ = _differs(X.nonfinite_epilogue(skipped, act, dtype, d['res'] if r else None), d['wants'][(act, r)])
        assert lost > 0, (name, act, r)
    # skipping the taps outside the image changes nothing while the weights are finite: that mutant is the weight case's
    if not tr:
        unpadded = X.conv_nonfinite_ref(d['xs'], d['wt'], d['bias'], c['k'], c['s'], skip='padding')
        assert _differs(X.nonfinite_epilogue(unpadded, 'none', dtype), d['wants'][('none', False)]) == (0, 0)


def test_padding_mutant_changes_the_weight_case():
    for dtype in STORED:
        d = X.nonfinite_weight_data(dtype)
        unpadded = X.conv_nonfinite_ref(d['xs'], d['wt'], d['bias'], 3, 1, skip='padding')
        for (act, r), want in d['wants'].items():
            lost, _ = _differs(X.nonfinite_epilogue(unpadded, act, dtype, d['res'] if r else None), want)
            assert lost >= 2 * 31, (act, r, lost)                              # the top row and the left column of channel 5, both images


# ---- the pool chain -----------------------------------------------------------------------------------------------------------------
def _pool_ref(x):
    ys = []
    for _ in range(3):
        x = F.max_pool2d(x, 5, 1, 2)
        ys.append(x)
    return ys


@pytest.mark.parametrize('c,h,w,B', X.POOL_NONFINITE_SHAPES, ids=lambda v: str(v))
def test_pool_case_and_its_mutants(c, h, w, B):
    """The planted NaN sits at every position of some window (25 where the map has room), windows clipped by each border hold one, an
    all -inf window gives -inf through the three pools; the separable restatement with the propagating maximum IS F.max_pool2d; with
    maxNum or with c > a ? c : a it is not, in every one of the three outputs."""
    x = X.pool_nonfinite_data(c, h, w, B)
    ref = _pool_ref(x)
    for b in range(B):
        c0 = 8 * (b % (c // 8))
        y1 = ref[0][b]
        # channel c0: the NaN at (h//2, w//2) is in the window of every output within 2 of it: each of those sees it at another position
        ys, xs_ = torch.nonzero(torch.isnan(y1[c0]), as_tuple=True)
        offsets = {(int(h // 2 - yy), int(w // 2 - xx)) for yy, xx in zip(ys, xs_)}
        assert offsets == {(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3) if 0 <= h // 2 - dy < h and 0 <= w // 2 - dx < w}
        assert len(offsets) == 25 or h < 5 or w < 5
        # clipped windows: the corners and the left edge
        assert torch.isnan(y1[c0 + 1, 0, 0]) and torch.isnan(y1[c0 + 2, h - 1, w - 1]) and torch.isnan(y1[c0 + 3, h // 2, 0])
        assert bool((ref[2][b, c0 + 4] == INF).any()) and not torch.isnan(ref[2][b, c0 + 4]).any()
        for y in ref:
            assert y[b, c0 + 5, 0, 0] == -INF                                    # a window of nothing but -inf
    share = X.nonfinite_counts(ref[2])
    assert share['finite'] >= 0.30 * ref[2].numel() or c == 8, share
    good = X.pool_chain_sep(x, 'maximum')
    for g, r in zip(good, ref):
        assert _differs(g, r) == (0, 0)
    for mutant in ('maxnum', 'select'):
        for g, r in zip(X.pool_chain_sep(x, mutant), ref):
            lost, _ = _differs(g, r)
            assert lost > 0, mutant
    # on finite data all three are the same function
    xf = X.pool_nonfinite_data(c, h, w, B, finite=True)
    if xf.numel() <= 1 << 18:
        for op in ('maximum', 'maxnum', 'select'):
            for g, r in zip(X.pool_chain_sep(xf, op), _pool_ref(xf)):
                assert torch.equal(g, r)


def test_pool_launch_rule_restated():
    """(512, 4, 4, 16), (1024, 4, 4, 16) and (1024, 4, 4, 32) are the cases with 2, 4 and 8 granules per workgroup in every storage
    type; the B = 2 shapes all run one granule per workgroup."""
    for (c, h, w, B), gp in X.POOL_GP.items():
        for esz in (2, 4):
            assert X.pool_granules(c, h, w, B, esz) == gp
    for c, h, w, B in X.POOL_NONFINITE_SHAPES[:5]:
        assert X.pool_granules(c, h, w, B, 2) == 1 and X.pool_granules(c, h, w, B, 4) == 1
