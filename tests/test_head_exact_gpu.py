"""The head's box / corner path against an exact reference, in every mix of the per-level sparse / dense box kernels.

Head-only engines (three levels, 277 classes, no DFL) on a 96 x 160 input, B = 3: level maps 12 x 20, 6 x 10, 3 x 5, N = 315 anchors, so
the 32-anchor tiles of the box kernels straddle images and levels.  Features are multiples of 1/4 in [-2, 2], box / corner weights
multiples of 1/4 in [-1, 1], biases multiples of 1/16: every accumulator and every step of the decode (ax +- d, / 2, * stride -- a power
of two --, cx - bw / 2) is an exact fp32 value, so the bits of prediction columns 0..3, 5..12 and of candidate-row columns 0..11 are
those of the oracle's decode evaluated in float64.  The class weights are on the same grid and the threshold sits where no reference
score comes within 1e-3 of it (a condition on the inputs, asserted on the CPU): the anchors that pass are known from the reference
alone."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import lp_testing as X
from test_hip_kernels import _engine, _fill

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
B, H, W, NCLS = 3, 96, 160, 277
MAPS = [(12, 20), (6, 10), (3, 5)]
LEVEL_OFF = [0, 240, 300, 315]
N = LEVEL_OFF[-1]
IOU, MAX_DET = 0.45, 100
MARGIN = 1e-3
CASES = [                                          # (dtype, channels per level)
    (F16, (64, 128, 256)), (BF16, (64, 128, 256)),         # one, two and four 128-byte K-chunks
    (F16, (32, 96, 192)), (BF16, (32, 96, 192)),           # partial chunks
    (F16, (320, 64, 64)), (BF16, (320, 64, 64)),           # level 0: five chunks, the generic decode kernel by rule
    (F32, (32, 64, 128)),                                  # one, two and four chunks
    (F32, (160, 32, 32)),                                  # level 0: five chunks
]
_case_id = lambda c: '%s-%s' % ({F16: 'f16', BF16: 'bf16', F32: 'f32'}[c[0]], '-'.join(map(str, c[1])))


def head_data(widths, seed):
    """Per level: features [B,C,h,w], class weights / bias, box + corner weights / bias (float64 grid values).  The class bias is
    -2.25 standard deviations of the level's logits (a multiple of 1/16): the largest of a head's ~35 logits then falls on
    either side of zero, so the mean of the heads' best probabilities spreads around 1/2 at every width."""
    out = []
    for i, (c, (h, w)) in enumerate(zip(widths, MAPS)):
        x = X.grid_rand((B, c, h, w), seed + 10 * i, -2.0, 2.0)
        wc = X.grid_rand((NCLS, c), seed + 10 * i + 1, -1.0, 1.0)
        sd = (c * 1.5 * 5.0 / 12.0) ** 0.5                   # var x = 3/2 (17 values), var w = 5/12 (9 values)
        bc = X.grid_rand((NCLS,), seed + 10 * i + 2, -0.5, 0.5, 1.0 / 16) - round(2.25 * sd * 16) / 16.0
        wb = X.grid_rand((12, c), seed + 10 * i + 3, -1.0, 1.0)
        bb = X.grid_rand((12,), seed + 10 * i + 4, -2.0, 2.0, 1.0 / 16)
        out.append((x, wc, bc, wb, bb))
    return out


def reference(data, dtype):
    """(pred columns 0..12 [B,N,13], candidate-row columns 0..11 [B,N,12], keep-mask value [B,N]) in float64: the oracle's decode and
    xywh2xyxy on exact sums, the class path as sigmoid -> best of each head -> the mask's mean (nms.py's: ad4 twice, ad5 omitted)."""
    from oracle import lp_oracle
    for x, wc, bc, wb, bb in data:
        for t in (x, wc, wb):
            assert torch.equal(t.to(dtype).double(), t) and torch.equal(torch.round(t * 4) / 4, t)
        assert torch.equal(torch.round(bb * 16) / 16, bb) and torch.equal(torch.round(bc * 16) / 16, bc)
    o = [F.conv2d(x, wb[..., None, None], bb).reshape(B, 12, -1) for x, _, _, wb, bb in data]
    cat = lambda parts: torch.cat(parts, -1).permute(0, 2, 1)
    pts, st = lp_oracle.anchors(MAPS)
    box, corners = lp_oracle.decode(cat([v[:, :4] for v in o]), cat([v[:, 4:] for v in o]), pts.double(), st.double())
    pred = torch.cat([box, torch.ones(B, N, 1, dtype=torch.float64), corners], -1)
    xyxy = torch.cat([box[..., :2] - box[..., 2:] / 2, box[..., :2] + box[..., 2:] / 2], -1)
    rows = torch.cat([xyxy, corners], -1)
    prob = cat([torch.sigmoid(F.conv2d(x, wc[..., None, None], bc)).reshape(B, NCLS, -1) for x, wc, bc, _, _ in data])
    best = [prob[..., a - 13:b - 13].max(-1).values for a, b in zip(X.SEG[:-1], X.SEG[1:])]
    mask_value = (sum(best[:7]) + best[6]) / 8.0
    return X.to_exact_f32(pred), X.to_exact_f32(rows), mask_value


def pick_threshold(mask_value):
    """The multiple of 2^-12 nearest the reference scores' 65 % quantile that no score comes within MARGIN of (a condition on the
    inputs; about a third of the anchors pass)."""
    v = mask_value.flatten()
    target = float(v.quantile(0.65))
    cands = sorted((k / 4096.0 for k in range(1, 4096)), key=lambda t: abs(t - target))
    return next(t for t in cands if float((v - t).abs().min()) > MARGIN)


def passing(mask_value, conf):
    """Per image the sorted anchors that pass; between 5 % and 60 % of every level of every image."""
    assert float((mask_value - conf).abs().min()) > MARGIN
    ok = mask_value >= conf
    for b in range(B):
        for l in range(3):
            share = float(ok[b, LEVEL_OFF[l]:LEVEL_OFF[l + 1]].double().mean())
            assert 0.05 <= share <= 0.60, (b, l, share)
    return [torch.nonzero(ok[b]).flatten() for b in range(B)]


def case_inputs(dtype, widths):
    """Data, reference and threshold of a case, and a second data set (what leaves stale content in a workspace)."""
    data = head_data(widths, 100)
    pred, rows, mv = reference(data, dtype)
    conf = pick_threshold(mv)
    return data, head_data(widths, 500), pred, rows, conf, passing(mv, conf)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_head_box_path_exact_in_every_mode_mix(case):
    """Prediction tensor: columns 0..3 and 5..12 carry the reference's bits, column 4 is 1 (the generic decode kernel at these widths).
    Detections-only forward, each of the eight requests sparse / dense per level, once on a workspace a preceding all-sparse run on
    OTHER data has used (stale snapshots, rows and kept indices) and once on one filled with 0xFF: per image the candidates are
    exactly the reference's passing anchors, their rows carry the reference's bits, a level requested dense has every row written
    and exact, a level requested sparse has its other rows either all untouched or all written and exact (untouched where the
    level before ran the streaming kernel), and counts, detections and kept indices are the same in all sixteen runs and equal to
    lp_nms on the prediction tensor."""
    from yolov6.hip import abi, runtime
    from yolov6.hip.runtime import _f32
    dtype, widths = case
    data, other, want_pred, want_rows, conf, want_pass = case_inputs(dtype, widths)
    eng = _engine(dtype)
    eng.autotune = False
    feats = [eng.tensor(c, 3 + i) for i, c in enumerate(widths)]
    for i, (f, (_, wc, bc, wb, bb)) in enumerate(zip(feats, data)):
        abi.check(eng.lib.lp_engine_add_head_cls(eng.h, f, i, NCLS, eng._ptr(_f32(wc)), eng._ptr(_f32(bc))))
        abi.check(eng.lib.lp_engine_add_head_box(eng.h, f, i, 1, eng._ptr(_f32(wb)), eng._ptr(_f32(bb)), None))
    eng.finish()
    eng.bind(B, H, W)
    assert eng.n_anchors == N
    boxes = [i for i, k in enumerate(eng.op_kinds()) if k == 'head_box']
    assert len(boxes) == 3
    x = torch.zeros(B, 3, H, W, device='cuda:0')

    def fill(which):
        for f, lvl in zip(feats, which):
            _fill(eng, f, lvl[0])

    fill(data)
    pred = eng.forward(x)
    want_pred, want_rows = want_pred.cuda(), want_rows.cuda()
    cols = [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12]
    assert torch.equal(_bits(pred[..., cols]), _bits(want_pred[..., cols])), 'prediction tensor: box / corner columns'
    assert torch.equal(pred[..., 4], torch.ones_like(pred[..., 4]))
    det0 = runtime.nms_padded(pred.clone(), conf, IOU, MAX_DET, want_keep=True)
    assert int(det0[1].sum()) > 0
    # the streaming box kernel takes a level of at most four 128-byte K-chunks; a wider one runs the generic decode kernel
    esz = torch.empty(0, dtype=dtype).element_size()
    streams = [c * esz <= 512 for c in widths]
    SP, DN = abi.LP_VARIANT_BOX_SPARSE, abi.LP_VARIANT_BOX_DENSE
    ws = eng.det_workspace(B, H, W)
    cnt, keys, rows = X.det_workspace_views(ws, B, N)
    for mix, stale in itertools.product(itertools.product((SP, DN), repeat=3), (True, False)):
        what = 'request %s on a %s workspace' % (''.join('S' if m == SP else 'D' for m in mix), 'stale' if stale else 'poisoned')
        if stale:
            for op in boxes:
                eng.set_variant(op, SP, 1)
            fill(other)
            eng.forward_det(x, conf, ws=ws)
            runtime.nms_candidates((ws, B, N), IOU, MAX_DET, want_keep=True)
            fill(data)
        else:
            ws.fill_(0xFF)
        before = _bits(rows[..., :12]).clone()
        for op, m in zip(boxes, mix):
            eng.set_variant(op, m, 1)
        eng.forward_det(x, conf, ws=ws)
        got_cnt, got_keys, got = cnt.clone(), keys.clone(), _bits(rows[..., :12]).clone()
        det = runtime.nms_candidates((ws, B, N), IOU, MAX_DET, want_keep=True)
        exact = got == _bits(want_rows)                              # [B,N,12]
        untouched = got == before
        for b in range(B):
            p = want_pass[b].cuda()
            assert int(got_cnt[b]) == len(p), (what, b, int(got_cnt[b]), len(p))
            assert torch.equal((got_keys[b, :len(p)] & 0xFFFFFFFF).sort().values, p), (what, b)
            assert bool(exact[b, p].all()), '%s: rows of passing anchors, image %d' % (what, b)
            rest = torch.ones(N, dtype=torch.bool, device='cuda:0')
            rest[p] = False
            for l, m in enumerate(mix):
                lvl = torch.zeros_like(rest)
                lvl[LEVEL_OFF[l]:LEVEL_OFF[l + 1]] = True
                r = rest & lvl
                assert bool(r.any())
                written = bool(exact[b, r].all())
                if m == DN:
                    assert written, '%s: level %d requested dense, image %d' % (what, l, b)
                    continue
                # (on a stale workspace a row may hold the same bits before and after: only the poisoned one tells them apart)
                kept_out = bool(untouched[b, r].all())
                assert written or kept_out, '%s: level %d requested sparse, image %d: neither all written nor all untouched' % (what, l, b)
                if not stale and streams[l] and (l == 0 or streams[l - 1]):
                    assert kept_out and not written, '%s: level %d must run sparse, image %d' % (what, l, b)
        for t0, t1 in zip(det0, det):                                # detections, counts, kept anchors
            assert torch.equal(t0, t1), what
    for op in boxes:
        eng.set_variant(op, SP, 1)
