"""The head's class path: the inputs of tests/test_head_cls_gpu.py are what they claim to be, and its checks can fail.

No GPU here.  The coded logits of lp_testing.cls_case_data are admissible (every column of a head either ties with the largest
logit in a way every fp32 sigmoid must reproduce, or is clear of it by twice the elementwise bound) and cover what the kernels
can get wrong: every class column as the arg-max, exact two-way ties inside and across the kernels' column tiles, saturated heads
whose first 1.0 is not the largest logit, all-saturated and all-zero heads, and 32-row tiles with 0, 6 and 7 passing anchors.  A
numpy emulation of the class path in head_det_kernel's operation order passes every check; six subtly wrong versions of it do
not.  The C oracle and its numpy restatement order NaN-scored candidates the same, well-defined way."""
import numpy as np
import pytest
import torch

import lp_testing as X
from test_head_exact_gpu import B, CASES, LEVEL_OFF, MAPS, N, NCLS, _case_id

NAN_WIDTH = 64
NAN_HEADS = (0, 6, 7)
NAN_DTYPES = (torch.float16, torch.bfloat16, torch.float32)


def test_geometry_is_that_of_the_box_path_tests():
    assert (B, tuple(MAPS), tuple(LEVEL_OFF), N, NCLS) == (X.CLS_B, X.CLS_MAPS, X.CLS_LEVEL_OFF, X.CLS_N, X.CLS_NC)
    assert X.CLS_HEAD0 == (0, 31, 55, 92, 129, 166, 203, 240, 277)


def test_saturation_limits_come_from_the_arithmetic():
    """1 + e^-20 rounds to 1 in fp32 with a factor of more than 25 to spare; e^128 overflows fp32 (so the reciprocal is +0); at 12 the
    sigmoid is still 50 ulps below 1, at -88 e^88 is still finite."""
    assert np.exp(-20.0) * 25 < 2.0 ** -24 and np.exp(128.0) > float(np.finfo(np.float32).max)
    assert 1.0 - 1.0 / (1.0 + np.exp(-12.0)) > 50 * 2.0 ** -24 and np.exp(88.0) < float(np.finfo(np.float32).max)
    assert X.sigmoid32(np.float32(20.0)).view(np.uint32) == 0x3f800000 and X.sigmoid32(np.float32(-128.0)).view(np.uint32) == 0


@pytest.mark.parametrize('seed', [100, 500])
@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_coded_logits_are_admissible_and_cover_the_class_path(case, seed):
    """cls_reference asserts exactness and admissibility; here the coverage (seed 100: the data under test, 500: what leaves the
    workspace stale)."""
    dtype, widths = case
    c = X.cls_case(dtype, widths, seed)
    cov, ref, confs = c['cov'], c['ref'], c['confs']
    assert cov['columns'] == NCLS, 'not every class column is the expected arg-max of a passing anchor'
    assert cov['tie2'] >= 0.10 and cov['sat_first'] >= 0.10 and cov['all_sat'] >= 0.05 and cov['all_zero'] >= 0.05, cov
    assert min(cov['cross_tile'], cov['cross_wave'], cov['cross_window']) >= 8, cov
    rates = [float((ref['mask'] >= t).mean()) for t in confs]
    assert 0.07 <= rates[0] <= 0.15 and 0.5 <= rates[1] <= 0.7, rates
    for seen in cov['tile_counts']:
        assert {0, 6, 7} <= seen, seen                        # an empty tile, the last sparse count (HEAD_DET_R), the first dense one
    for k in range(8):                                        # first and last column of every head
        ok = ref['mask'] >= confs[1]
        assert {0, X.CLS_HEAD0[k + 1] - X.CLS_HEAD0[k] - 1} <= set(ref['ci'][..., k][ok].tolist()), k
    # 'saturated with arg-max != largest logit' really separates the two rules
    sat = (ref['kind'] == 'S') & (ref['ci'] != ref['cmax'])
    assert int(sat.sum()) >= 0.10 * sat.size


def _emulated(ref, mutant=None):
    e = X.cls_emulate(ref['logits'].reshape(-1, NCLS), mutant)
    shape = ref['logits'].shape[:2]
    return dict(cf=e['cf'].reshape(shape + (8,)), ci=e['ci'].reshape(shape + (8,)), mask=e['mask'].reshape(shape),
                key=X.score_key_hi(e['score']).reshape(shape))


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_emulation_passes_and_every_mutant_is_noticed(case):
    """The emulation of the kernels' order meets every assertion at both thresholds; each mutant changes an asserted quantity
    on this case's data -- except 'nan_dropped', which cannot show on finite logits (admissibility rules NaN out): its data are
    the non-finite cases below."""
    dtype, widths = case
    c = X.cls_case(dtype, widths)
    ref = c['ref']
    e = _emulated(ref)
    for conf in c['confs']:
        assert X.cls_check(ref, conf, e['mask'] >= np.float32(conf), e['cf'], e['ci'], e['key']) == []
    expect = {'logit_argmax': 'arg-max', 'last_equal': 'arg-max', 'boundary': 'arg-max', 'mask_cf7': 'candidates', 'windows_desc': 'arg-max'}
    for mutant, what in expect.items():
        m = _emulated(ref, mutant)
        for conf in c['confs']:
            assert what in X.cls_check(ref, conf, m['mask'] >= np.float32(conf), m['cf'], m['ci'], m['key']), (mutant, conf)
    m = _emulated(ref, 'nan_dropped')
    assert all(np.array_equal(m[k], e[k]) for k in e)


def nan_case(dtype, head, seed=100):
    """(levels, weighted column, expectation, threshold) of a non-finite case; the threshold is the 60 % one of the finite masks."""
    levels, col = X.cls_nan_data(NAN_WIDTH, head, seed)
    for x, wc, _ in levels:
        assert torch.equal(x.to(dtype).double(), x) and torch.equal(wc.to(dtype).double(), wc)
    exp = X.cls_nan_expected(levels)
    finite = exp['mask'][~np.isnan(exp['mask'])]
    return levels, col, exp, X.cls_thresholds(finite)[1]


@pytest.mark.parametrize('head', NAN_HEADS)
def test_non_finite_case_expectation_and_nan_mutant(head):
    """torch.max's rule on the non-finite data: a NaN in heads 0..6 makes the mask NaN (no candidate); a NaN only in head 7 leaves
    the mask alone, the row carries NaN as its eighth maximum and the first NaN's index.  A +inf column ties with the saturated
    ones (the first wins), a -inf one with the zero ones.  The emulation agrees; the NaN-dropping mutant does not."""
    levels, col, exp, conf = nan_case(torch.float32, head)
    k_col = col - X.CLS_HEAD0[head]
    nan_rows = exp['nan'].any(-1)
    assert 0.2 <= float(nan_rows.mean()) <= 0.3 and bool((exp['nan'].sum(-1) <= 1).all())
    assert bool(np.isnan(exp['cf'][..., head][nan_rows]).all()) and bool((exp['ci'][..., head][nan_rows] == k_col).all())
    with np.errstate(invalid='ignore'):
        want = exp['mask'] >= conf
    if head < 7:
        assert bool(np.isnan(exp['mask'][nan_rows]).all()) and not bool(want[nan_rows].any())
    else:
        assert not bool(np.isnan(exp['mask']).any()) and int(want[nan_rows].sum()) >= 20
    L = exp['logits']
    pinf, ninf = np.isposinf(L[..., col]), np.isneginf(L[..., col])
    assert int(pinf.sum()) > 0 and int(ninf.sum()) > 0
    first_sat = (L[..., X.CLS_HEAD0[head]:X.CLS_HEAD0[head + 1]] >= X.CLS_SAT).argmax(-1)
    assert np.array_equal(exp['ci'][..., head][pinf], first_sat[pinf])
    assert int((first_sat[pinf] == k_col).sum()) > 0 and int((first_sat[pinf] < k_col).sum()) > 0     # inf is first, and is not
    for mutant, same in ((None, True), ('nan_dropped', False)):
        e = X.cls_emulate(L.reshape(-1, NCLS), mutant)
        with np.errstate(invalid='ignore'):
            got = (e['mask'] >= np.float32(conf)).reshape(want.shape)
        ci, cf = e['ci'].reshape(exp['ci'].shape)[want], e['cf'].reshape(exp['cf'].shape)[want]
        agrees = (np.array_equal(got, want) and np.array_equal(ci, exp['ci'][want])
                  and np.array_equal(np.isnan(cf), np.isnan(exp['cf'][want])))
        assert agrees == same, mutant


def synth_boxes(Bn, n, seed):
    """Prediction columns 0..12 for a class-path test: boxes that overlap in clusters, obj = 1."""
    return X.synth_pred(Bn, n, seed)[..., :13].numpy()


def test_oracles_order_nan_scores_first_by_anchor():
    """A NaN score (a NaN only in the last head) sorts before every number, as in torch's descending sort, NaNs among themselves by
    ascending anchor: cand_cmp is a strict weak order on such input, the numpy restatement follows the same order, score_key drops
    the NaN's sign, and the existing goldens (no NaN in them) are not affected (tests/test_oracle_golden.py keeps pinning them)."""
    from oracle import lp_post
    s = torch.tensor([0.5, float('nan'), 0.7, float('inf'), float('nan'), 0.7, -1.0])
    assert lp_post.order_desc(s.numpy()).tolist() == torch.sort(s, descending=True, stable=True).indices.tolist() == [1, 4, 3, 2, 5, 0, 6]
    neg_nan = np.array([0x7fc00000, 0xffc00000, 0x7f800001], np.uint32).view(np.float32)
    assert X.score_key_hi(neg_nan).tolist() == [0, 0, 0] and X.score_key_hi(np.float32([np.inf]))[0] > 0
    keys = X.score_key_hi(np.float32([np.inf, 1.0, 0.5, 0.0, -0.0, -1.0, -np.inf])).astype(np.int64)
    assert bool((np.diff(keys) > 0).all())
    levels, col, exp, conf = nan_case(torch.float32, 7)
    L64, _, _ = X.cls_logits64(levels)
    P = torch.where(L64 >= X.CLS_SAT, torch.ones_like(L64), torch.where(L64 <= X.CLS_ZERO, torch.zeros_like(L64), torch.sigmoid(L64)))
    pred = np.concatenate([synth_boxes(B, N, 3), P.float().numpy()], -1)
    # boxes far apart: nothing is suppressed, the kept order IS the sort order
    pred[..., 0] = np.arange(N)[None] * 200.0
    pred[..., 1] = 0.0
    rows_c, keep_c, _ = lp_post.nms_c(pred, conf, 0.45, N)
    rows_n, keep_n = lp_post.nms_np(pred, conf, 0.45, N)
    for b in range(B):
        with np.errstate(invalid='ignore'):
            want = np.nonzero(exp['mask'][b] >= conf)[0]
        sc = X.sum8_f32(exp['cf'][b][want].astype(np.float32), 7)
        nan = np.isnan(sc)
        assert int(nan.sum()) >= 5 and int((~nan).sum()) >= 5
        order = np.concatenate([want[nan], want[~nan][np.argsort(-sc[~nan], kind='stable')]])
        assert np.array_equal(keep_c[b], order) and np.array_equal(keep_n[b], order)
        assert np.array_equal(rows_c[b], rows_n[b].astype(np.float32), equal_nan=True)
        assert bool(np.isnan(rows_c[b][:int(nan.sum()), 19]).all())
        assert np.array_equal(rows_c[b][:int(nan.sum()), 27], np.full(int(nan.sum()), col - X.CLS_HEAD0[7], np.float32))
