"""The head's class path against a float64 reference of its own: arg-max ties, saturated sigmoids, NaN.

Head-only engines and geometry of tests/test_head_exact_gpu.py (B = 3, 96 x 160 input, N = 315: 32-anchor tiles straddle images, every
level ends in a partial tile; one, two, four, partial and -- past what the one-kernel forms take -- five K-chunks).  The class logits
are the coded ones of lp_testing.cls_case_data: exact fp32 sums whose arg-max, ties and saturation are known from float64 alone
(tests/test_head_cls_cpu.py asserts that, the coverage, and that the checks used here notice six subtly wrong class paths).
Three kernels are under test: the tiled MODE_PRED kernel, head_cls_rows_kernel (LP_VARIANT_ROWS) and head_det_kernel with its sparse
and dense tiles, and behind them score_kernel, on the prediction tensor and on a level's scratch.  Figures go to parity.log."""
import os

import numpy as np
import pytest
import torch

import lp_testing as X
from test_head_cls_cpu import NAN_DTYPES, NAN_HEADS, NAN_WIDTH, nan_case
from test_head_exact_gpu import B, CASES, H, IOU, MAX_DET, N, NCLS, W, _case_id, head_data
from test_hip_kernels import _engine, _fill

pytestmark = pytest.mark.gpu

F32 = torch.float32
ONE, ZERO = 0x3f800000, 0


def _log(line):
    with open(os.path.join(X.log_dir(), 'parity.log'), 'a') as f:
        f.write(line + '\n')


def _build(dtype, widths, levels):
    """Head-only engine: the class predictors of ``levels`` and grid-valued box / corner predictors (they only feed the NMS)."""
    from yolov6.hip import abi
    from yolov6.hip.runtime import _f32
    eng = _engine(dtype)
    eng.autotune = False
    feats = [eng.tensor(c, 3 + i) for i, c in enumerate(widths)]
    box = head_data(widths, 100)
    for i, (f, (_, wc, bc), (_, _, _, wb, bb)) in enumerate(zip(feats, levels, box)):
        abi.check(eng.lib.lp_engine_add_head_cls(eng.h, f, i, NCLS, eng._ptr(_f32(wc)), eng._ptr(_f32(bc))))
        abi.check(eng.lib.lp_engine_add_head_box(eng.h, f, i, 1, eng._ptr(_f32(wb)), eng._ptr(_f32(bb)), None))
    eng.finish()
    eng.bind(B, H, W)
    assert eng.n_anchors == N
    cls_ops = [i for i, k in enumerate(eng.op_kinds()) if k == 'head_cls']
    assert len(cls_ops) == 3
    return eng, feats, cls_ops


def _fill_levels(eng, feats, levels):
    for f, lvl in zip(feats, levels):
        _fill(eng, f, lvl[0])


def _chunks(dtype, c):
    kc = 128 // torch.empty(0, dtype=dtype).element_size()
    return (c + kc - 1) // kc, c % (kc // 4) == 0


def rows_fits(dtype, c):
    """head_rows_fits / the engine's rows_fits: at most three K-chunks of whole 32-byte K-steps."""
    n, whole = _chunks(dtype, c)
    return whole and n <= 3


def det_fits(dtype, c):
    """head_det_fits: four K-chunks of resident weights in 16 bit, three in fp32; else prediction rows to a scratch + score_kernel."""
    n, whole = _chunks(dtype, c)
    return whole and n <= (3 if dtype == F32 else 4)


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _same(a, b):
    """Bit for bit, a NaN equal to a NaN (the two routes and the oracle need not agree on a NaN's payload)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _assert_nms_equals_oracle(pred, conf, iou, max_det, what):
    """lp_nms on a copy of ``pred`` against the C oracle on the same tensor: rows, counts, kept anchors.  -> (det tuple, oracle rows, keep)"""
    from oracle import lp_post
    from yolov6.hip import runtime
    det = runtime.nms_padded(pred.clone(), conf, iou, max_det, want_keep=True)
    rows_c, keep_c, _ = lp_post.nms_c(pred.cpu().numpy(), conf, iou, max_det)
    for b in range(B):
        n = int(det[1][b])
        assert n == len(rows_c[b]), '%s: image %d: %d rows, the oracle has %d' % (what, b, n, len(rows_c[b]))
        assert np.array_equal(det[2][b, :n].cpu().numpy(), keep_c[b]), '%s: kept anchors, image %d' % (what, b)
        assert _same(det[0][b, :n].cpu().numpy(), rows_c[b]), '%s: rows, image %d' % (what, b)
    return det, rows_c, keep_c


def _check_pred_bits(prob, ref, what):
    """The properties of the class columns that hold bit for bit, and the elementwise bound.  -> worst error / bound"""
    L = ref['logits']
    bits = _bits(prob)
    assert bool((bits[L >= X.CLS_SAT] == ONE).all()), what + ': a logit >= 20 is not exactly 1.0f'
    assert bool((bits[L <= X.CLS_ZERO] == ZERO).all()), what + ': a logit <= -128 is not exactly +0.0f'
    vals, inv = np.unique(L, return_inverse=True)                   # equal logits -> equal bits; bits non-decreasing in the logit
    lo, hi = np.full(len(vals), 0xffffffff, np.uint32), np.zeros(len(vals), np.uint32)
    np.minimum.at(lo, inv.ravel(), bits.ravel())
    np.maximum.at(hi, inv.ravel(), bits.ravel())
    assert np.array_equal(lo, hi), what + ': equal logits, different bits'
    assert bool((np.diff(lo.astype(np.int64)) >= 0).all()), what + ': the sigmoid bits decrease where the logit grows'
    worst = 0.0
    for lv in range(3):                                            # (K, the number of summed terms, is the level's)
        s = slice(X.CLS_LEVEL_OFF[lv], X.CLS_LEVEL_OFF[lv + 1])
        K = int(ref['K'][s][0])
        args = (prob[:, s], torch.from_numpy(ref['prob'][:, s]), torch.from_numpy(ref['mag'][:, s]), K, F32)
        X.assert_elementwise(*args, transcendental=True)
        worst = max(worst, X.elementwise_excess(*args, transcendental=True)[0])
    return worst


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_prediction_tensor_class_columns(case):
    """Columns 13..289 from the tiled kernel and, where lp_engine_set_op_variant takes it (exactly where head_rows_fits holds), from
    the row writer: exact 1.0f / +0.0f where the logit saturates, equal bits for equal logits anywhere in the tensor and across the
    two kernels, bits monotone in the logit, every element inside the elementwise bound of the float64 sigmoid.  lp_nms on it
    equals the C oracle bit for bit at both thresholds, and with nothing suppressed (IoU threshold 1) the oracle's columns 20..27
    are the expected arg-max of every candidate: the tie to the reference's rule, not to the tensor."""
    from yolov6.hip import abi
    dtype, widths = case
    c = X.cls_case(dtype, widths)
    ref, confs = c['ref'], c['confs']
    eng, feats, cls_ops = _build(dtype, widths, c['levels'])
    _fill_levels(eng, feats, c['levels'])
    x = torch.zeros(B, 3, H, W, device='cuda:0')
    pred = eng.forward(x).clone()
    worst = _check_pred_bits(pred[..., 13:], ref, 'tiled kernel')
    took = []
    for op, cw in zip(cls_ops, widths):
        if rows_fits(dtype, cw):
            eng.set_variant(op, abi.LP_VARIANT_ROWS, 1)
            took.append(op)
        else:
            with pytest.raises(RuntimeError):
                eng.set_variant(op, abi.LP_VARIANT_ROWS, 1)
    if took:
        rows_pred = eng.forward(x)
        _check_pred_bits(rows_pred[..., 13:], ref, 'row writer')
        assert torch.equal(rows_pred.view(torch.int32), pred.view(torch.int32)), 'row writer and tiled kernel differ'
        for op in took:
            eng.set_variant(op, 2, 1)
    for conf in confs:
        _assert_nms_equals_oracle(pred, conf, IOU, MAX_DET, 'conf %g' % conf)
        _, rows_c, keep_c = _assert_nms_equals_oracle(pred, conf, 1.0, N, 'conf %g, nothing suppressed' % conf)
        want = ref['mask'] >= conf
        for b in range(B):
            assert np.array_equal(np.sort(keep_c[b]), np.nonzero(want[b])[0]), 'candidates of the oracle, image %d' % b
            assert np.array_equal(rows_c[b][:, 20:28].astype(np.int64), ref['ci'][b][keep_c[b]]), 'arg-max of the oracle, image %d' % b
    _log('head_cls pred %s: probability error / bound %.3g, row writer on %d of 3 levels, candidates %s' % (
        _case_id(case), worst, len(took), [int((ref['mask'] >= t).sum()) for t in confs]))


def _scratch_region(eng, feats):
    """Byte interval of the arena behind its tensors: where a level whose class predictors do not fit head_det_kernel gets its
    prediction scratch."""
    base = (eng.arena.data_ptr() + 255) // 256 * 256 - eng.arena.data_ptr()
    need = eng.lib.lp_engine_arena_bytes(eng.h, *eng.bound)
    end = max(X.engine_tensor_span(eng, t)[1] for t in [eng.input_id] + list(feats))
    assert len(feats) + 1 == 4 and eng.lib.lp_engine_tensor_info(eng.h, 4, None, None, None, None, None) < 0     # (no other tensor)
    return base + (end - base + 255) // 256 * 256, base + need - 256


def _run_det(eng, x, conf, ws, scratch):
    """One detections-only forward on ``ws``.  -> (counts [B], passed [B,N] bool, key high words [B,N] uint32 (0 where no key), bits
    of candidate-row columns 12..27 [B,N,16], candidate-row columns 12..27 as float32, prediction scratch written or not)."""
    cnt, keys, rows = X.det_workspace_views(ws, B, N)
    eng.arena[scratch[0]:scratch[1]].fill_(0xFF)
    eng.forward_det(x, conf, ws=ws)
    touched = bool((eng.arena[scratch[0]:scratch[1]] != 0xFF).any())
    cnt_h, keys_h = cnt.cpu().numpy(), keys.cpu().numpy()
    passed, hi = np.zeros((B, N), bool), np.zeros((B, N), np.uint32)
    for b in range(B):
        k = keys_h[b, :cnt_h[b]]
        a = (k & 0xFFFFFFFF).astype(np.int64)
        assert len(np.unique(a)) == len(a) and (len(a) == 0 or int(a.max()) < N), 'image %d: anchors of the keys' % b
        passed[b, a] = True
        hi[b, a] = ((k >> 32) & 0xFFFFFFFF).astype(np.uint32)
    vals = rows[..., 12:28].clone()
    return cnt_h, passed, hi, _bits(vals), vals.cpu().numpy(), touched


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_detections_only_class_path(case):
    """lp_engine_forward_det at both thresholds, once on a workspace another data set left stale and once on a 0xFF-filled one.  The
    route per level is named by rule: head_det_kernel where head_det_fits holds, else prediction rows in the arena's scratch +
    score_kernel (seen as writes to that scratch).  The candidates per image are exactly the reference's passing anchors; columns
    12..19 of their rows carry the bits the prediction tensor has at the head's expected arg-max (and the class they must: 1.0f,
    +0.0f, or inside the bound), columns 20..27 the expected arg-max; the key's high word is score_key of the left-to-right fp32
    sum of the eight / 8 recomputed in numpy, its low word the anchor; columns 12..27 of the anchors that do not pass are untouched
    on the poisoned workspace; lp_nms_candidates equals lp_nms on the prediction tensor bit for bit."""
    from yolov6.hip import runtime
    dtype, widths = case
    c, other = X.cls_case(dtype, widths), X.cls_case(dtype, widths, 500)
    ref, confs = c['ref'], c['confs']
    eng, feats, _ = _build(dtype, widths, c['levels'])
    routes = ['head_det_kernel' if det_fits(dtype, cw) else 'scratch + score_kernel' for cw in widths]
    scratch = _scratch_region(eng, feats)
    x = torch.zeros(B, 3, H, W, device='cuda:0')
    _fill_levels(eng, feats, c['levels'])
    pred = eng.forward(x).clone()
    col = 13 + np.array(X.CLS_HEAD0[:8])[None, None] + ref['ci']
    want_cf_bits = np.take_along_axis(_bits(pred), col, -1)                 # what (i) found for each head's expected arg-max
    ws = eng.det_workspace(B, H, W)
    for conf in confs:
        det0 = runtime.nms_padded(pred.clone(), conf, IOU, MAX_DET, want_keep=True)
        want = ref['mask'] >= conf
        for stale in (True, False):
            what = '%s, conf %g, %s workspace' % (' / '.join(routes), conf, 'stale' if stale else 'poisoned')
            if stale:
                _fill_levels(eng, feats, other['levels'])
                eng.forward_det(x, other['confs'][1], ws=ws)
                runtime.nms_candidates((ws, B, N), IOU, MAX_DET, want_keep=True)
                _fill_levels(eng, feats, c['levels'])
            else:
                ws.fill_(0xFF)
            before = _bits(X.det_workspace_views(ws, B, N)[2][..., 12:28].clone())
            cnt, passed, hi, bits, vals, touched = _run_det(eng, x, conf, ws, scratch)
            assert touched == any(r != 'head_det_kernel' for r in routes), what + ': the prediction scratch'
            assert cnt.tolist() == want.sum(1).tolist(), what
            ci = np.where(passed[..., None], vals[..., 8:], -1.0).astype(np.int64)      # (the poison of the other rows is a NaN)
            assert X.cls_check(ref, conf, passed, vals[..., :8], ci, hi) == [], what
            assert bool((vals[..., 8:][want] == np.floor(vals[..., 8:][want])).all())
            assert np.array_equal(bits[..., :8][want], want_cf_bits[want]), what + ': maxima differ from the prediction tensor'
            if not stale:
                assert np.array_equal(bits[~want], before[~want]), what + ': rows of anchors that do not pass were written'
            det = runtime.nms_candidates((ws, B, N), IOU, MAX_DET, want_keep=True)
            for t0, t1 in zip(det0, det):
                assert torch.equal(t0, t1), what + ': lp_nms_candidates differs from lp_nms'
    _log('head_cls det %s: routes %s, candidates %s of %d' % (_case_id(case), routes, [int((ref['mask'] >= t).sum()) for t in confs], B * N))


@pytest.mark.parametrize('head', NAN_HEADS)
@pytest.mark.parametrize('dtype', NAN_DTYPES, ids=['f16', 'bf16', 'f32'])
def test_non_finite_logits(dtype, head):
    """One class weight is +inf: its column is NaN where the feature is 0, +inf / -inf elsewhere.  The prediction tensor has NaN
    exactly there, 1.0f and +0.0f at the infinities.  A NaN in heads 0..6 makes the mask NaN: the anchor is no candidate on either
    route, and lp_nms equals the C oracle (it kept such anchors before score_heads propagated NaN).  A NaN only in head 7 leaves the
    mask alone: the candidate row carries NaN in column 19 and the index of the NaN column in column 27, its key sorts first, and
    both routes and the oracle agree on the order."""
    from yolov6.hip import runtime
    widths = (NAN_WIDTH,) * 3
    levels, col, exp, conf = nan_case(dtype, head)
    eng, feats, _ = _build(dtype, widths, levels)
    assert all(det_fits(dtype, cw) for cw in widths)
    _fill_levels(eng, feats, levels)
    x = torch.zeros(B, 3, H, W, device='cuda:0')
    pred = eng.forward(x).clone()
    prob = pred[..., 13:].cpu().numpy()
    L = exp['logits']
    assert np.array_equal(np.isnan(prob), exp['nan']), 'NaN columns of the prediction tensor'
    assert bool((prob.view(np.uint32)[np.isposinf(L)] == ONE).all()) and bool((prob.view(np.uint32)[np.isneginf(L)] == ZERO).all())
    with np.errstate(invalid='ignore'):
        want = exp['mask'] >= conf
    nan_rows = exp['nan'].any(-1)
    for iou, max_det in ((IOU, MAX_DET), (1.0, N)):
        det0, rows_c, keep_c = _assert_nms_equals_oracle(pred, conf, iou, max_det, 'head %d, iou %g' % (head, iou))
    for b in range(B):                                                     # (iou 1: nothing suppressed, every candidate is a row)
        assert np.array_equal(np.sort(keep_c[b]), np.nonzero(want[b])[0]), 'candidates of the oracle, image %d' % b
        assert np.array_equal(rows_c[b][:, 20:28].astype(np.int64), exp['ci'][b][keep_c[b]])
        assert np.array_equal(np.isnan(rows_c[b][:, 12:20]), np.isnan(exp['cf'][b][keep_c[b]]))
        n_nan = int(nan_rows[b][keep_c[b]].sum())
        assert n_nan == (0 if head < 7 else int((want[b] & nan_rows[b]).sum()))
        if n_nan:                                                          # NaN scores first, by ascending anchor
            assert bool(nan_rows[b][keep_c[b][:n_nan]].all()) and bool((np.diff(keep_c[b][:n_nan]) > 0).all())
    ws = eng.det_workspace(B, H, W)
    ws.fill_(0xFF)
    scratch = _scratch_region(eng, feats)
    cnt, passed, hi, bits, vals, touched = _run_det(eng, x, conf, ws, scratch)
    assert not touched and np.array_equal(passed, want), 'candidates of the detections-only forward'
    assert np.array_equal(vals[..., 8:][want].astype(np.int64), exp['ci'][want])
    assert np.array_equal(np.isnan(vals[..., :8][want]), np.isnan(exp['cf'][want]))
    assert np.array_equal(hi[want], X.score_key_hi(X.sum8_f32(vals[..., :8][want], 7)))
    if head == 7:
        assert int((want & nan_rows).sum()) >= 20 and bool((hi[want & nan_rows] == 0).all())
        assert bool((vals[..., 15][want & nan_rows] == col - X.CLS_HEAD0[7]).all())
    det = runtime.nms_candidates((ws, B, N), 1.0, N, want_keep=True)
    assert torch.equal(det[1], det0[1]) and torch.equal(det[2], det0[2])
    assert _same(det[0].cpu().numpy(), det0[0].cpu().numpy()), 'lp_nms_candidates differs from lp_nms'
    _log('head_cls nan %s head %d: %d NaN anchors, %d candidates, %d of them NaN-scored' % (
        {torch.float16: 'f16', torch.bfloat16: 'bf16', F32: 'f32'}[dtype], head, int(nan_rows.sum()), int(want.sum()),
        int((want & nan_rows).sum()) if head == 7 else 0))
