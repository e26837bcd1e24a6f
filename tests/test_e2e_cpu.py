"""CPU side of the whole-model parity tests: the float64 mode of the forward oracle, the float64 post-processing, and the
decision-margin analyser that says which anchors' fate is firm under given error margins (tests/lp_testing.py).  The GPU side is
tests/test_e2e_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, GOLDEN
import lp_testing as T
from lp_testing import SEG, decision_margins, nms64, post64_scores, post64_select, synth_pred
from oracle import lp_oracle, lp_post
from test_oracle_golden import MODEL_CASES, P6_CASES

sys.path.insert(0, GOLDEN)


# ---- the oracle --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,weights,name', MODEL_CASES)
def test_fp64_oracle_matches_reference(case, weights, name):
    """The float64 mode against the reference's own outputs: the bars of test_forward_oracle_matches_reference."""
    g, sd = load_golden(case), load_golden(weights)
    pred, neck, bb = lp_oracle.forward(sd, lp_oracle.arch(name, width=0.0625), g['x'], return_stages=True, precision=torch.float64)
    assert pred.dtype == torch.float64 and all(t.dtype == torch.float64 for t in neck + bb)
    for i in range(4):
        torch.testing.assert_close(bb[i], g['bb%d' % i].double(), rtol=1e-4, atol=1e-4)
    for i in range(3):
        torch.testing.assert_close(neck[i], g['neck%d' % i].double(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(pred, g['pred'].double(), rtol=1e-4, atol=1e-3)
    assert torch.equal(pred[..., 4], torch.ones_like(pred[..., 4]))


@pytest.mark.parametrize('case,name,arch_kw,build_kw', P6_CASES, ids=[c[0] for c in P6_CASES])
def test_fp64_oracle_matches_reference_p6_and_pan(case, name, arch_kw, build_kw):
    g, sd = load_golden(case), load_golden(case + '_weights')
    a = lp_oracle.arch(name, width=0.0625, depth=0.25, **arch_kw)
    pred, neck = lp_oracle.forward(sd, a, g['x'], precision=torch.float64)
    assert len(neck) == (4 if a.p6 else 3) and pred.dtype == torch.float64
    for i, f in enumerate(neck):
        torch.testing.assert_close(f, g['neck%d' % i].double(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(pred, g['pred'].double(), rtol=1e-4, atol=1e-3)


def test_fp32_default_of_the_oracle_gives_the_bits_it_gave_before():
    """bench.py's CPU baseline and smoke() run the default path: its outputs on the tiny goldens, plain and rounding-aware, hash to
    what the oracle gave before it had a ``precision`` argument (make_golden_oracle_pin.py; 4 ATen threads, as recorded)."""
    import make_golden_oracle_pin as pin
    nthreads = torch.get_num_threads()
    torch.set_num_threads(4)
    try:
        with np.load(os.path.join(GOLDEN, 'oracle_fp32_pin.npz'), allow_pickle=False) as z:
            for case, weights, name, round_to in pin.PIN_CASES:
                assert pin.digests(case, weights, name, round_to) == z[pin.pin_key(case, round_to)].tolist(), (case, round_to)
    finally:
        torch.set_num_threads(nthreads)
    g, sd = load_golden('lps_tiny_64x160'), load_golden('lps_tiny_weights')
    a = lp_oracle.arch('yololps', width=0.0625)
    p0, n0 = lp_oracle.forward(sd, a, g['x'])
    p1, n1 = lp_oracle.forward(sd, a, g['x'], precision=torch.float32)
    assert p0.dtype == torch.float32 and torch.equal(p0, p1) and all(torch.equal(u, v) for u, v in zip(n0, n1))
    with pytest.raises(ValueError):
        lp_oracle.forward(sd, a, g['x'], precision=torch.float16)


def test_rounding_aware_fp64_oracle_keeps_16_bit_values():
    """round_to with precision=float64: every neck map still holds values of the 16-bit type (the roundings stay where they are)."""
    g, sd = load_golden('lps_tiny_64x160'), load_golden('lps_tiny_weights')
    for dt in (torch.float16, torch.bfloat16):
        pred, neck = lp_oracle.forward(sd, lp_oracle.arch('yololps', width=0.0625), g['x'].to(dt), round_to=dt, precision=torch.float64)
        assert pred.dtype == torch.float64
        for f in neck:
            assert f.dtype == torch.float64 and torch.equal(f.to(dt).double(), f)


# ---- float64 post-processing against the C oracle ----------------------------------------------------------------------------------
# Margins between the C oracle (fp32, op by op) and the float64 restatement ON THE SAME float32 prediction: the probabilities are the
# same numbers (eps_p = 0: only exact ties are not firm, and both sides take the first maximum); a mean of eight values <= 1 summed
# left to right in fp32 is within 8 * 2^-24 = 4.8e-7 of the exact one (eps_s = 1e-6); a corner x -+ w/2 below 1024 is rounded once,
# by <= 2^-15 = 3.1e-5 (delta = 1e-4, which also covers the fp32 rounding of the IoU itself: ~4 * 2^-24 relative, against a move of
# the IoU of ~4 delta / 30 px = 1.3e-5 that the margin already allows).
C_MARGINS = dict(eps_s=1e-6, eps_p=0.0, delta=1e-4)


@pytest.mark.parametrize('B,N,seed,hot,conf,iou,max_det,obj_one', [
    (3, 2100, 41, 0.05, 0.4, 0.45, 1000, True),
    (2, 2100, 42, 0.30, 0.03, 0.65, 300, True),        # every anchor is a candidate; the max_det cut is active
    (3, 600, 43, 0.50, 0.25, 0.50, 50, False),         # obj != 1
    (2, 77, 44, 1.00, 0.30, 0.10, 1000, True),
])
def test_nms64_equals_the_c_oracle_where_decisions_are_firm(B, N, seed, hot, conf, iou, max_det, obj_one):
    pred = synth_pred(B, N, seed, frac_hot=hot, obj_one=obj_one)
    rows_c, keep_c, _ = lp_post.nms_c(pred.numpy(), conf, iou, max_det)
    rows, keep = nms64(pred.double().numpy(), conf, iou, max_det)
    firm_images = 0
    for b in range(B):
        d = decision_margins(pred[b].double().numpy(), conf, iou, max_det, **C_MARGINS)
        assert np.array_equal(d['keep'], keep[b])
        changed = set(keep_c[b].tolist()) ^ set(keep[b].tolist())
        assert changed <= set(d['ambiguous'].tolist()), (b, sorted(changed))
        if len(d['ambiguous']) == 0:
            firm_images += 1
            for lo, hi in T.tie_runs(keep[b], d['order_ties']):
                assert sorted(keep[b][lo:hi].tolist()) == sorted(keep_c[b][lo:hi].tolist())
            if not d['order_ties']:
                assert np.array_equal(keep[b], keep_c[b])
                assert np.array_equal(rows[b][:, 20:], rows_c[b][:, 20:].astype(np.float64))        # class indices
                assert np.abs(rows[b][:, :12] - rows_c[b][:, :12]).max() <= C_MARGINS['delta']
                assert np.abs(rows[b][:, 12:20] - rows_c[b][:, 12:20]).max() == 0
    assert sum(len(k) for k in keep) > 0
    assert firm_images > 0, 'no image of this case has only firm decisions: it compares nothing'


# ---- planted cases -----------------------------------------------------------------------------------------------------------------
def _row(cx, cy, w, h, score, cls=0):
    """One anchor whose eight segment maxima all equal ``score`` (masked mean = score = ``score``), at class ``cls`` of each segment."""
    r = np.full(290, 0.01)
    r[:4], r[4] = (cx, cy, w, h), 1.0
    r[5:13] = np.tile((cx, cy), 4)
    for a in SEG[:-1]:
        r[a + cls] = score
    return r


def _iou_pair(iou, w=100.0, h=40.0):
    """Horizontal offset of two equal w x h boxes that gives them this IoU = (w - dx) / (w + dx)."""
    return w * (1 - 2 * iou / (1 + iou))


PLANT = dict(conf_thres=0.4, iou_thres=0.45, max_det=100, eps_s=1e-5, eps_p=1e-5, delta=1e-3)


def _planted():
    """Twelve groups, 1000 px apart: name -> (rows, names of the rows that must be flagged)."""
    e, thr = PLANT['eps_s'], PLANT['iou_thres']
    groups = {
        'near_threshold': ([_row(0, 0, 100, 40, PLANT['conf_thres'] + e / 2)], [0]),
        'firm_threshold': ([_row(0, 0, 100, 40, PLANT['conf_thres'] + 3 * e), _row(300, 0, 100, 40, PLANT['conf_thres'] - 3 * e)], []),
        # IoU within the interval the corner margin opens around the threshold: the lower-scored one can go either way
        'straddle': ([_row(0, 0, 100, 40, 0.9), _row(_iou_pair(thr) + 5e-4, 0, 100, 40, 0.8)], [1]),
        'firm_suppress': ([_row(0, 0, 100, 40, 0.9), _row(_iou_pair(0.6), 0, 100, 40, 0.8)], []),
        'firm_apart': ([_row(0, 0, 100, 40, 0.9), _row(_iou_pair(0.3), 0, 100, 40, 0.8)], []),
        # scores within 2 eps_s and overlapping: either can come first and suppress the other
        'near_tie': ([_row(0, 0, 100, 40, 0.7), _row(_iou_pair(0.7), 0, 100, 40, 0.7 - 1.5 * e)], [0, 1]),
        'near_tie_apart': ([_row(0, 0, 100, 40, 0.7), _row(_iou_pair(0.2), 0, 100, 40, 0.7 - 1.5 * e)], []),
        # cascade: b straddles with a; c overlaps b only (IoU 0.6), d overlaps c only: their fates follow b's
        'cascade': ([_row(0, 0, 100, 40, 0.9), _row(_iou_pair(thr) - 5e-4, 0, 100, 40, 0.8),
                     _row(_iou_pair(thr) + _iou_pair(0.6), 0, 100, 40, 0.7),
                     _row(_iou_pair(thr) + 2 * _iou_pair(0.6), 0, 100, 40, 0.6)], [1, 2, 3]),
        # the same chain behind a firm suppression: nothing is in doubt (b is dead, c is kept, d is dead)
        'firm_chain': ([_row(0, 0, 100, 40, 0.9), _row(_iou_pair(0.6), 0, 100, 40, 0.8),
                        _row(_iou_pair(0.6) + _iou_pair(0.7), 0, 100, 40, 0.7),
                        _row(_iou_pair(0.6) + 2 * _iou_pair(0.7), 0, 100, 40, 0.6)], []),
        # b and c are near-tied and overlap (IoU 0.54), but a surely suppresses b (0.54) and not c (0.25): b is dead, no doubt spreads
        'dead_ends_the_closure': ([_row(0, 0, 100, 40, 0.9), _row(30, 0, 100, 40, 0.8), _row(60, 0, 100, 40, 0.8 - 1.5 * e)], []),
        'inverted_box': ([_row(0, 0, -100, 40, 0.9), _row(10, 0, 100, 40, 0.8)], []),
        'below': ([_row(0, 0, 100, 40, 0.2), _row(5, 0, 100, 40, 0.39)], []),
    }
    rows, flagged, names = [], [], []
    for g, (name, (rs, fl)) in enumerate(groups.items()):
        for i, r in enumerate(rs):
            r = r.copy()
            r[0] += 1000.0 * g
            r[5:13:2] += 1000.0 * g
            if i in fl:
                flagged.append(len(rows))
            names.append('%s[%d]' % (name, i))
            rows.append(r)
    return np.stack(rows), flagged, names


def test_analyser_flags_exactly_the_planted_anchors():
    pred, flagged, names = _planted()
    d = decision_margins(pred, **PLANT)
    assert [names[i] for i in d['ambiguous']] == [names[i] for i in flagged]
    assert not d['nonfirm'].any()
    # the groups really are what their names say, in the float64 post-processing
    kept = set(names[i] for i in d['keep'])
    for n in ('straddle[0]', 'cascade[0]', 'firm_chain[0]', 'firm_chain[2]', 'firm_apart[1]', 'inverted_box[0]', 'inverted_box[1]',
              'dead_ends_the_closure[0]', 'dead_ends_the_closure[2]', 'near_tie[0]', 'firm_threshold[0]', 'near_threshold[0]'):
        assert n in kept, n
    for n in ('firm_suppress[1]', 'firm_chain[1]', 'firm_chain[3]', 'near_tie[1]', 'below[0]', 'below[1]', 'firm_threshold[1]',
              'dead_ends_the_closure[1]'):
        assert n not in kept, n
    # with margins of zero nothing is in doubt
    z = decision_margins(pred, PLANT['conf_thres'], PLANT['iou_thres'], PLANT['max_det'], 0.0, 0.0, 0.0)
    assert len(z['ambiguous']) == 0 and np.array_equal(z['keep'], d['keep'])


def test_analyser_reports_soft_argmax_and_order_ties():
    e = PLANT['eps_p']
    a, b, c = _row(0, 0, 100, 40, 0.9, cls=3), _row(1000, 0, 100, 40, 0.8), _row(2000, 0, 100, 40, 0.8 - 1e-5)
    a[SEG[2] + 7] = 0.9 - 1.5 * e            # segment 2 of row a: runner-up within 2 eps_p
    a[SEG[5] + 1] = 0.9 - 2.5 * e            # segment 5: outside
    d = decision_margins(np.stack([a, b, c]), **PLANT)
    assert d['keep'].tolist() == [0, 1, 2] and len(d['ambiguous']) == 0
    want = np.zeros((3, 8), bool)
    want[0, 2] = True
    assert np.array_equal(d['nonfirm'], want)
    assert d['order_ties'] == [(1, 2)]
    assert T.tie_runs(d['keep'], d['order_ties']) == [(0, 1), (1, 3)]


def test_analyser_at_the_max_det_cut():
    """Six separate anchors, max_det 3: ranks 3 and 4 in a near-tie can swap across the cut; firmly ordered ones cannot."""
    e = PLANT['eps_s']
    s = [0.9, 0.8, 0.7, 0.7 - e, 0.6, 0.5]
    pred = np.stack([_row(1000.0 * i, 0, 100, 40, v) for i, v in enumerate(s)])
    kw = dict(PLANT, max_det=3)
    d = decision_margins(pred, **kw)
    assert d['keep'].tolist() == [0, 1, 2] and d['ambiguous'].tolist() == [2, 3]
    pred[3, 13:] -= 0.05
    d = decision_margins(pred, **kw)
    assert d['keep'].tolist() == [0, 1, 2] and d['ambiguous'].tolist() == []
    # an anchor in doubt above the cut (0 and 6: a near-tied overlapping pair): the ranks behind it are not known
    pred = np.concatenate([pred, _row(_iou_pair(0.7), 0, 100, 40, 0.9 - e)[None]])
    assert decision_margins(pred, **kw)['ambiguous'].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert decision_margins(pred, **dict(PLANT, max_det=7))['ambiguous'].tolist() == [0, 6]


def test_analyser_at_the_max_nms_cut():
    """Five separate anchors, max_nms 3: the two in a near-tie at the cut can fall on either side, the one firmly behind it is out."""
    e = PLANT['eps_s']
    pred = np.stack([_row(1000.0 * i, 0, 100, 40, v) for i, v in enumerate([0.9, 0.8, 0.7, 0.7 - e, 0.6])])
    d = decision_margins(pred, max_nms=3, **PLANT)
    assert d['keep'].tolist() == [0, 1, 2] and d['ambiguous'].tolist() == [2, 3]
    pred[3, 13:] -= 0.05
    assert decision_margins(pred, max_nms=3, **PLANT)['ambiguous'].tolist() == []


# ---- soundness on the model cases --------------------------------------------------------------------------------------------------
def _perturbed(r, rng, kind, eps_s, eps_p, delta):
    """One move of an image's post-processing inputs within the margins: (box, cf, ci, mask, score).  kind 0: every probability of
    a row by the same amount of +-min(eps_s, eps_p) (mask and score move by exactly that much: the extreme for the score decisions),
    every corner by +-delta; kind 1: every probability independently within +-eps_p (the extreme for the argmax), rows whose mask or
    score would move by more than eps_s are left alone, corners uniform within +-delta."""
    n = len(r['score'])
    if kind == 0:
        prob = r['prob'] + rng.choice([-1.0, 1.0], (n, 1)) * min(eps_s, eps_p)
        box = r['box'] + rng.choice([-1.0, 1.0], (n, 4)) * delta
    else:
        prob = r['prob'] + rng.uniform(-eps_p, eps_p, r['prob'].shape)
        box = r['box'] + rng.uniform(-delta, delta, (n, 4))
    s = post64_scores(prob)
    far = (np.abs(s['mask'] - r['mask']) > eps_s) | (np.abs(s['score'] - r['score']) > eps_s)
    if far.any():
        prob[far] = r['prob'][far]
        s = post64_scores(prob)
    assert np.abs(s['mask'] - r['mask']).max() <= eps_s * (1 + 1e-9) and np.abs(s['score'] - r['score']).max() <= eps_s * (1 + 1e-9)
    return box, s


@pytest.mark.parametrize('key', list(T.E2E_CASES))
def test_analyser_is_sound_on_the_model_cases(key):
    """The cases of the GPU tests, their own margins, 50 seeded moves within them: where the analyser says nothing is ambiguous the kept
    set, its order outside near-ties and the firm argmax columns never change.  Then the same with margins 1000 times larger, where
    anchors ARE in doubt: only anchors the analyser flagged ever change their fate."""
    ref = T.e2e_reference(key)
    flagged_total = changed_total = 0
    for k, (conf, iou, max_det) in enumerate(T.E2E_SETTINGS[key]):
        dec = T.assert_e2e_inputs(key, k)
        for scale in (1.0, 1000.0):
            eps_s, eps_p, delta = (scale * ref[m] for m in ('eps_s', 'eps_p', 'delta'))
            for b, p in enumerate(ref['pred64'].numpy()):
                d = dec[b] if scale == 1.0 else decision_margins(p, conf, iou, max_det, eps_s, eps_p, delta)
                r = T.post64_rows(p)
                r['prob'] = p[:, 13:] * p[:, 4:5]
                amb, keep0 = set(d['ambiguous'].tolist()), d['keep']
                flagged_total += len(amb) if scale > 1 else 0
                rng = np.random.default_rng(1000 * k + b)
                for it in range(50):
                    box, s = _perturbed(r, rng, it % 2, eps_s, eps_p, delta)
                    keep = post64_select(box, s['mask'], s['score'], conf, iou, max_det)
                    changed = set(keep.tolist()) ^ set(keep0.tolist())
                    changed_total += len(changed) if scale > 1 else 0
                    assert changed <= amb, (key, k, scale, b, it, sorted(changed - amb))
                    if not amb:
                        for lo, hi in T.tie_runs(keep0, d['order_ties']):
                            assert sorted(keep[lo:hi].tolist()) == sorted(keep0[lo:hi].tolist()), (key, k, scale, b, it)
                        firm = ~d['nonfirm']
                        assert np.array_equal(s['ci'][keep0][firm], r['ci'][keep0][firm]), (key, k, scale, b, it)
    assert flagged_total > 0, 'the enlarged margins put nothing in doubt: the second half tests nothing'
    if key == 'yolov6m':            # (nearly every candidate is in doubt there: some fates do change)
        assert changed_total > 0
