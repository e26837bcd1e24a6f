"""The DFL branch of the head's box decode (MODE_DECODE with reg_bins > 1: per-side softmax over the bins, projection by proj[],
the four-threads-per-pixel quad exchange, the corner offset 4 * bins) in both forward forms, on head-only engines with the geometry
of test_head_exact_gpu.py.  Data, references, the bound and the proof that these checks can fail: tests/test_head_dfl_cpu.py.

Coded regime: the softmax is exactly one-hot or an exact two-way tie, so every box and corner bit is known.  Rounding regime: grid
data with a really soft softmax against float64, box columns within lp_testing.dfl_box_bounds (derived from the operation count,
independent of the storage type), corner columns bit-exact.  Bin counts 2 and 6 run the 32-cout tile (6: exactly full), 7 the
first row count of the 128-cout tile, 30 that tile exactly full."""
import os

import pytest
import torch

import lp_testing as X
import test_head_dfl_cpu as D
from test_head_exact_gpu import B, H, IOU, MAX_DET, N, NCLS, W, pick_threshold
from test_hip_kernels import _engine, _fill

pytestmark = pytest.mark.gpu


def _head_engine(dtype, widths, data, bins, proj):
    from yolov6.hip import abi
    from yolov6.hip.runtime import _f32
    eng = _engine(dtype)
    eng.autotune = False
    feats = [eng.tensor(c, 3 + i) for i, c in enumerate(widths)]
    for i, (f, (_, wc, bc, wb, bb)) in enumerate(zip(feats, data)):
        abi.check(eng.lib.lp_engine_add_head_cls(eng.h, f, i, NCLS, eng._ptr(_f32(wc)), eng._ptr(_f32(bc))))
        abi.check(eng.lib.lp_engine_add_head_box(eng.h, f, i, bins, eng._ptr(_f32(wb)), eng._ptr(_f32(bb)), eng._ptr(_f32(proj))))
    eng.finish()
    eng.bind(B, H, W)
    assert eng.n_anchors == N
    for f, lvl in zip(feats, data):
        _fill(eng, f, lvl[0])
    return eng


def _both_forms(eng, conf):
    """(prediction tensor, workspace, candidate rows [B,N,28] as the detections-only forward leaves them on a 0xFF-filled workspace)."""
    x = torch.zeros(B, 3, H, W, device='cuda:0')
    pred = eng.forward(x)
    ws = eng.det_workspace(B, H, W)
    ws.fill_(0xFF)
    eng.forward_det(x, conf, ws=ws)
    return pred, ws, X.det_workspace_views(ws, B, N)[2]


@pytest.mark.parametrize('case', D.CASES, ids=D.case_id)
def test_coded_logits_give_known_bits(case):
    """Prediction columns 0..3 and 5..12 carry the expected bits and column 4 is 1; columns 0..11 of ALL 315 candidate rows per image
    carry them after the detections-only forward on a poisoned workspace (the generic det_mode kernel writes every anchor of a DFL
    level); lp_nms_candidates on that workspace equals lp_nms on the prediction tensor bit for bit."""
    from yolov6.hip import runtime
    bins, dtype, widths = case
    want = D.coded_case(bins, dtype, widths)
    conf = pick_threshold(want['mask'])
    eng = _head_engine(dtype, widths, want['data'], bins, want['proj'])
    pred, ws, rows = _both_forms(eng, conf)
    cols = D.BOX_P + D.COR_P
    X.assert_bits(pred[..., cols].contiguous(), want['pred'][..., cols].contiguous(), 'prediction tensor: box / corner columns')
    assert torch.equal(pred[..., 4], torch.ones_like(pred[..., 4]))
    X.assert_bits(rows[..., :12].contiguous(), want['rows'], 'candidate rows: columns 0..11 of every anchor')
    assert D.coded_mismatches(pred, rows, want) == 0                  # (the count the CPU file's mutations are held against)
    det0 = runtime.nms_padded(pred.clone(), conf, IOU, MAX_DET, want_keep=True)
    det = runtime.nms_candidates((ws, B, N), IOU, MAX_DET, want_keep=True)
    assert int(det0[1].sum()) > 0
    for t0, t1 in zip(det0, det):
        assert torch.equal(t0, t1)


@pytest.mark.parametrize('case', D.CASES, ids=D.case_id)
def test_soft_logits_within_the_derived_bound(case):
    """With the model's proj = linspace and with a non-monotone one: the box columns of both forms within the derived elementwise
    bound of the float64 reference, the corner columns bit-exact.  The worst error / bound ratio goes to the parity log."""
    bins, dtype, widths = case
    soft = D.soft_case(bins, dtype, widths)
    for name, ref in zip(('linspace', 'coded'), soft['refs']):
        eng = _head_engine(dtype, widths, soft['data'], bins, ref['proj'])
        pred, _, rows = _both_forms(eng, 0.5)
        worst, bad = D.soft_check(pred, rows, ref)
        line = 'head-dfl gpu            %-24s proj %-8s box err/bound %.3f  corner mismatches %d' % (D.case_id(case), name, worst, bad)
        print(line)
        with open(os.path.join(X.log_dir(), 'parity.log'), 'a') as f:
            f.write(line + '\n')
        assert bad == 0, line
        assert worst <= 1.0, line


def test_add_head_box_refuses_bad_bin_arguments():
    """31 bins (132 outputs: past the 128-cout tile) and DFL without proj are refused when the op is added; nothing is launched."""
    from yolov6.hip import abi
    from yolov6.hip.runtime import _f32
    eng = _engine(torch.float16)
    f = eng.tensor(64, 3)
    w31, b31, p31 = torch.zeros(4 * 31 + 8, 64), torch.zeros(4 * 31 + 8), torch.linspace(0, 30, 31)
    with pytest.raises(RuntimeError, match='reg_bins'):
        abi.check(eng.lib.lp_engine_add_head_box(eng.h, f, 0, 31, eng._ptr(_f32(w31)), eng._ptr(_f32(b31)), eng._ptr(_f32(p31))))
    with pytest.raises(RuntimeError, match='proj'):
        abi.check(eng.lib.lp_engine_add_head_box(eng.h, f, 0, 17, eng._ptr(_f32(w31[:76])), eng._ptr(_f32(b31[:76])), None))
