"""GPU parity tests of the whole hot path: Model.forward through the HIP engine
and non_max_suppression through lp_nms, against the CPU oracle (oracle/) and the
golden vectors recorded from the reference (tests/golden/)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, REPO
from lp_testing import det_workspace_views, synth_pred, rel_err

pytestmark = pytest.mark.gpu

CFG = lambda n: os.path.join(REPO, 'configs', n + '.py')   # noqa: E731
MODEL_CASES = [('lps_tiny_128x96', 'lps_tiny_weights', 'yololps'),
               ('lps_tiny_64x160', 'lps_tiny_weights', 'yololps'),
               ('v6m_tiny_96x128', 'v6m_tiny_weights', 'yolov6m')]


def _tiny_model(name, weights, deploy):
    from yolov6.utils.synth import build_synthetic
    from yolov6.utils.torch_utils import fuse_model
    from yolov6.layers.common import RepVGGBlock
    m = build_synthetic(CFG(name), width=0.0625, sigma=1.5)
    m.load_state_dict(load_golden(weights))
    if deploy:                                       # the reference's inference preparation (inferer.py:25-68)
        m = fuse_model(m).eval()
        for layer in m.modules():
            if isinstance(layer, RepVGGBlock):
                layer.switch_to_deploy()
    return m.eval()


def _check_pred(pred, ref, extent, coord_tol, prob_tol, tag='', rms_tol=None):
    """Parity of a [B,N,290] prediction with the oracle / golden one.

    boxes + key-points (columns 0..12, pixels): max |d| <= coord_tol * extent, extent = max(H, W) of the input,
    i.e. the north-star's 1e-4 is read on coordinates normalised by the image size (the unit the reference writes
    to its label files, inferer.py:112-114).  An element-wise 1e-4 is not a meaningful bar in fp32: the
    reference's own fused-vs-unfused forward differs by up to 4e-4 px on the golden cases (make_golden.py log).
    probabilities (columns 13..): absolute."""
    assert pred.shape == ref.shape and pred.dtype == torch.float32
    assert torch.equal(pred[..., 4], torch.ones_like(pred[..., 4]))
    dc = pred[..., :13].double() - ref[..., :13].double()
    dp = (pred[..., 13:] - ref[..., 13:]).double()
    cerr, perr = float(dc.abs().max()), float(dp.abs().max())
    crms, prms = float(dc.pow(2).mean().sqrt()), float(dp.pow(2).mean().sqrt())
    os.makedirs(os.path.join(REPO, 'gpurun_out'), exist_ok=True)
    with open(os.path.join(REPO, 'gpurun_out', 'parity.log'), 'a') as f:
        f.write('%-60s coord max|d| %.3e px (%.3e of extent %d, |ref|max %.1f) rms %.3e of extent  prob max|d| %.3e rms %.3e\n'
                % (tag, cerr, cerr / extent, extent, float(ref[..., :13].abs().max()), crms / extent, perr, prms))
    assert cerr <= coord_tol * extent, (cerr, coord_tol * extent)
    assert perr <= prob_tol, perr
    if rms_tol is not None:      # (coordinate rms as a fraction of the extent, probability rms)
        assert crms <= rms_tol[0] * extent and prms <= rms_tol[1], (crms / extent, prms, rms_tol)


@pytest.mark.parametrize('deploy', [True, False], ids=['deploy', 'unfused'])
@pytest.mark.parametrize('case,weights,name', MODEL_CASES)
def test_tiny_model_fp32_matches_reference_golden(case, weights, name, deploy):
    g = load_golden(case)
    m = _tiny_model(name, weights, deploy).cuda()
    with torch.no_grad():
        pred, feats = m(g['x'].cuda())
    x = g['x']
    _check_pred(pred.cpu(), g['pred'], max(x.shape[2:]), 1e-4, 1e-4, 'fp32 %s %s' % (case, 'deploy' if deploy else 'unfused'))
    # element-wise relative check as well on these small cases
    c, r = pred.cpu()[..., :13].double(), g['pred'][..., :13].double()
    assert float(((c - r).abs() / r.abs().clamp(min=1.0)).max()) <= 1e-4
    for i, f in enumerate(feats):
        ref = g['neck%d' % i]
        assert f.shape == ref.shape
        assert rel_err(f.float().cpu(), ref) <= 1e-4


# Stated half-precision tolerances (coordinates as a fraction of the input extent, probabilities absolute): <= 3x the error
# measured on MI355X (gpurun_out/parity.log, round 2).  fp16: 7.7e-4 / 6.8e-4 / 4.4e-3 of the extent and 2.7e-4 / 1.7e-4 /
# 8.6e-3 in probability on the three cases; bf16: 5.5e-3 / 3.4e-3 / 5.2e-2 and 4.5e-3 / 2.0e-3 / 9.8e-2 (the yolov6m recipe
# produces distances of 500 grid units and 8 significant bits are rounded at ~60 chained layers).
HALF_TOL = {
    (torch.float16, 'lps_tiny_128x96'): (2.4e-3, 9e-4), (torch.float16, 'lps_tiny_64x160'): (2.1e-3, 6e-4),
    (torch.float16, 'v6m_tiny_96x128'): (1.4e-2, 2.6e-2),
    (torch.bfloat16, 'lps_tiny_128x96'): (1.7e-2, 1.4e-2), (torch.bfloat16, 'lps_tiny_64x160'): (1.1e-2, 6e-3),
    (torch.bfloat16, 'v6m_tiny_96x128'): (1.5e-1, 2.9e-1),
}


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('case,weights,name', MODEL_CASES)
def test_tiny_model_half_precision(case, weights, name, dtype):
    """fp16 / bf16 engines: activations and weights are rounded at every layer, so the stated tolerance is
    that of ~40 chained 11-bit / 8-bit roundings, not 1e-4."""
    box_tol, prob_tol = HALF_TOL[(dtype, case)]
    g = load_golden(case)
    m = _tiny_model(name, weights, True).cuda().to(dtype)
    with torch.no_grad():
        pred, feats = m(g['x'].cuda().to(dtype))
    assert feats[0].dtype == dtype
    _check_pred(pred.cpu(), g['pred'], max(g['x'].shape[2:]), box_tol, prob_tol, '%s %s' % (dtype, case))


# P6 and plain-PAN assemblies (tests/golden/make_golden_p6.py): (case, config, build overrides)
P6_CASES = [
    ('s6_tiny_128x192', 'yolov6s6', {}),
    ('m6_tiny_128x64', 'yolov6m6', {}),
    ('s6pan_tiny_64x128', 'yolov6s6', dict(neck='RepPANNeck6', fuse_P2=False)),
    ('s6csppan_tiny_128x128', 'yolov6s6', dict(neck='CSPRepPANNeck_P6', fuse_P2=False)),
    ('span_tiny_96x64', 'yololps', dict(neck='RepPANNeck', fuse_P2=False)),
    ('mpan_tiny_64x96', 'yolov6m', dict(neck='CSPRepPANNeck', fuse_P2=False)),
]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['f32', 'f16'])
@pytest.mark.parametrize('case,name,build_kw', P6_CASES, ids=[c[0] for c in P6_CASES])
def test_p6_and_pan_models_match_reference_golden(case, name, build_kw, dtype):
    """Four-level (stride 64) heads, six-stage backbones and the transpose-conv + concat necks through the engine,
    against the outputs of the reference's own model code (deploy-fused weights, fp32 within 1e-4 of the extent)."""
    from yolov6.utils.synth import build_synthetic
    from yolov6.utils.torch_utils import fuse_model
    from yolov6.layers.common import RepVGGBlock
    g, sd = load_golden(case), load_golden(case + '_weights')
    m = build_synthetic(CFG(name), width=0.0625, depth=0.25, sigma=1.5, **build_kw)
    m.load_state_dict(sd)
    m = fuse_model(m).eval()
    for layer in m.modules():
        if isinstance(layer, RepVGGBlock):
            layer.switch_to_deploy()
    m = m.cuda().to(dtype)
    x = g['x']
    with torch.no_grad():
        pred, feats = m(x.cuda().to(dtype))
    nlev = len([k for k in g if k.startswith('neck')])
    assert len(feats) == nlev and pred.shape == g['pred'].shape
    if dtype == torch.float32:
        _check_pred(pred.cpu(), g['pred'], max(x.shape[2:]), 1e-4, 1e-4, 'fp32 %s' % case)
        for i, f in enumerate(feats):
            assert rel_err(f.float().cpu(), g['neck%d' % i]) <= 1e-4
    else:
        # fp16: <= 3x measured (1.3e-3 of the extent on s6_tiny, 2.6e-3 in probability on s6pan_tiny)
        _check_pred(pred.cpu(), g['pred'], max(x.shape[2:]), 4e-3, 8e-3, 'f16 %s' % case)


def test_p6_engine_needs_multiples_of_64():
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yolov6s6'), width=0.0625, depth=0.25).cuda()
    with torch.no_grad():
        m(torch.zeros(1, 3, 128, 64, device='cuda'))
        with pytest.raises(ValueError, match='coarsest stride'):
            m(torch.zeros(1, 3, 96, 64, device='cuda'))


@pytest.mark.parametrize('name,B,H,W', [('yololps', 2, 640, 640), ('yololpn', 3, 640, 416), ('yolov6m', 1, 320, 320)])
def test_full_model_fp32_vs_oracle(name, B, H, W):
    from oracle import lp_oracle
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG(name), sigma=0.25)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(1234))
    ref, ref_feats = lp_oracle.forward(m.state_dict(), lp_oracle.arch(name), x)
    with torch.no_grad():
        pred, feats = m.cuda()(x.cuda())
    assert pred.shape == (B, (H // 8) * (W // 8) + (H // 16) * (W // 16) + (H // 32) * (W // 32), 290)
    _check_pred(pred.cpu(), ref, max(H, W), 1e-4, 1e-4, 'fp32 full %s B%d %dx%d' % (name, B, H, W))
    for f, rf in zip(feats, ref_feats):
        assert rel_err(f.float().cpu(), rf) <= 1e-4


def test_full_model_fp16_vs_oracle_and_determinism():
    from oracle import lp_oracle
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), sigma=0.25)
    x = torch.rand(2, 3, 640, 640, generator=torch.Generator().manual_seed(1234))
    ref, _ = lp_oracle.forward(m.state_dict(), lp_oracle.arch('yololps'), x)
    mh = m.cuda().half()
    with torch.no_grad():
        p1, _ = mh(x.cuda().half())
        p1 = p1.clone()
        p2, _ = mh(x.cuda().half())
    assert torch.equal(p1, p2)                       # no atomics / split-K: bitwise reproducible
    _check_pred(p1.cpu(), ref, 640, 2.4e-3, 9e-3, 'fp16 full yololps')       # <= 3x measured (7.7e-4 of the extent, 2.8e-3)
    # batch independence: image 1 alone gives the same rows as image 1 inside the batch
    with torch.no_grad():
        p3, _ = mh(x[1:2].cuda().half())
    assert torch.equal(p3[0], p1[1])


def test_full_model_fp16_with_the_stride2_family(monkeypatch):
    """LP_S2P16=1 (read when an engine is created): every eligible 3x3 stride-2 layer on conv3x3_s2p16_kernel, chosen by
    rule.  The same bars as the default engine: the fp32 oracle within the fp16 tolerance, bitwise reproducible, image k of a batch =
    image k alone; and the engine really runs the kernel (variant 48 / 49 on at least three ops of yololps)."""
    import ctypes
    from oracle import lp_oracle
    from yolov6.hip import abi, runtime
    from yolov6.utils.synth import build_synthetic
    monkeypatch.setenv('LP_S2P16', '1')
    m = build_synthetic(CFG('yololps'), sigma=0.25)
    x = torch.rand(2, 3, 640, 640, generator=torch.Generator().manual_seed(1234))
    ref, _ = lp_oracle.forward(m.state_dict(), lp_oracle.arch('yololps'), x)
    mh = m.cuda().half()
    with torch.no_grad():
        p1, _ = mh(x.cuda().half())
        p1 = p1.clone()
        p2, _ = mh(x.cuda().half())
        p3, _ = mh(x[1:2].cuda().half())
    eng = runtime.engine_for(mh)
    on = 0
    for i in range(eng.lib.lp_engine_num_ops(eng.h)):
        cfg, nb = ctypes.c_int(), ctypes.c_int()
        abi.check(eng.lib.lp_engine_op_variant(eng.h, i, ctypes.byref(cfg), ctypes.byref(nb)), 'lp_engine_op_variant')
        on += cfg.value in (abi.LP_VARIANT_PIPE16_S2A, abi.LP_VARIANT_PIPE16_S2B)
    assert on >= 3, on
    assert torch.equal(p1, p2)
    assert torch.equal(p3[0], p1[1])
    _check_pred(p1.cpu(), ref, 640, 2.4e-3, 9e-3, 'fp16 full yololps, stride-2 family')


def _prepared(name, dtype, sigma):
    """The reference's inference preparation (inferer.py:25-68): float -> fuse_model -> switch_to_deploy -> half."""
    from yolov6.utils.synth import build_synthetic
    from yolov6.utils.torch_utils import fuse_model
    from yolov6.layers.common import RepVGGBlock
    m = build_synthetic(CFG(name), sigma=sigma)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = fuse_model(m).eval()
    for layer in m.modules():
        if isinstance(layer, RepVGGBlock):
            layer.switch_to_deploy()
    return m.cuda().to(dtype), sd


def _batch_properties(m, x, conf, iou, max_det, probe):
    """Size-independent properties of one batch through the engine (autotuned kernel variants): bitwise determinism,
    image k of the batch == image k alone, lp_nms(engine pred) == the C oracle's NMS of that pred on the probed images;
    and the path bench.py times -- the detections-only forward (autotuned DET row kernels, the scratch + score_kernel route
    of the 256-channel level) + lp_nms_candidates on the FULL batch -- == lp_nms(forward) bit for bit and == the C oracle on
    the probed images, at the inference thresholds and at the evaluation thresholds (conf 0.03, iou 0.65, max_det 300)."""
    from oracle import lp_post
    from yolov6.hip.runtime import nms_padded, detect_padded
    with torch.no_grad():
        p1 = m(x)[0].clone()
        p2 = m(x)[0]
        assert torch.equal(p1, p2)
        for k in probe:
            pk = m(x[k:k + 1])[0]
            assert torch.equal(pk[0], p1[k]), k
    assert torch.isfinite(p1).all()
    sub = p1[probe].contiguous()
    rows, keep, _ = lp_post.nms_c(sub.cpu().numpy(), conf, iou, max_det)
    det, count, kept = nms_padded(p1.clone(), conf, iou, max_det, want_keep=True)
    det, count, kept = det.cpu().numpy(), count.cpu().numpy(), kept.cpu().numpy()
    assert sum(len(r) for r in rows) > 0
    for i, k in enumerate(probe):
        assert count[k] == len(rows[i])
        assert np.array_equal(kept[k, :count[k]], keep[i]) and np.array_equal(det[k, :count[k]], rows[i])
    for cf, io, md in ((conf, iou, max_det), (0.03, 0.65, 300)):
        d0, c0, k0 = nms_padded(p1.clone(), cf, io, md, want_keep=True)
        with torch.no_grad():
            for route in ('det', 'det', 'pred'):                    # twice: the workspace is reused
                d1, c1, k1 = detect_padded(m, x, cf, io, md, want_keep=True, route=route)
                assert torch.equal(c1, c0), (cf, route)
                assert torch.equal(k1, k0) and torch.equal(d1, d0), (cf, route)
        assert int(c0.sum()) > 0
        rows, keep, _ = lp_post.nms_c(sub.cpu().numpy(), cf, io, md)
        d1, c1, k1 = d1.cpu().numpy(), c1.cpu().numpy(), k1.cpu().numpy()
        for i, k in enumerate(probe):
            assert c1[k] == len(rows[i])
            assert np.array_equal(k1[k, :c1[k]], keep[i]) and np.array_equal(d1[k, :c1[k]], rows[i])
    return p1


def test_config_yololpn_640_fp16_vs_oracle_and_bs128_properties():
    """BASELINE configs[2]: yololpn 640x640 fp16 -- B=4 against the fp32 oracle, then the bs=128 batch through the
    autotuned engine: determinism, batch independence, NMS == oracle NMS."""
    from oracle import lp_oracle
    m, sd = _prepared('yololpn', torch.float16, 0.6)
    x = torch.rand(4, 3, 640, 640, generator=torch.Generator().manual_seed(1234))
    ref, _ = lp_oracle.forward(sd, lp_oracle.arch('yololpn'), x)
    with torch.no_grad():
        pred = m(x.cuda().half())[0]
    # measured on MI355X (round 2, gpurun_out/parity.log): 5.8e-4 of the extent, 4.0e-3 in probability; tolerance = 3x that
    _check_pred(pred.cpu(), ref, 640, 1.8e-3, 1.2e-2, 'fp16 full yololpn B4')
    xb = torch.rand(128, 3, 640, 640, generator=torch.Generator().manual_seed(77)).cuda().half()
    _batch_properties(m, xb, 0.4, 0.45, 1000, [0, 1, 63, 127])


def test_config_yololps_640_fp16_bs32_properties():
    """BASELINE configs[1] at its full batch: the autotuned variants the bench runs (B=32) keep determinism, batch
    independence and NMS parity."""
    m, _ = _prepared('yololps', torch.float16, 0.25)
    xb = torch.rand(32, 3, 640, 640, generator=torch.Generator().manual_seed(1234)).cuda().half()
    _batch_properties(m, xb, 0.4, 0.45, 1000, [0, 13, 31])


def test_config_yolov6m_1280_bf16_vs_oracle_and_nms():
    """BASELINE configs[4] per GPU: yolov6m 1280x1280 bf16 (DFL head, BottleRep residuals, N = 33600 anchors) against
    the fp32 oracle, and lp_nms on that prediction against the C oracle."""
    from oracle import lp_oracle, lp_post
    from yolov6.hip.runtime import nms_padded
    m, sd = _prepared('yolov6m', torch.bfloat16, 0.25)
    x = torch.rand(1, 3, 1280, 1280, generator=torch.Generator().manual_seed(5))
    ref, _ = lp_oracle.forward(sd, lp_oracle.arch('yolov6m'), x)
    with torch.no_grad():
        pred = m(x.cuda().bfloat16())[0]
        pred2 = m(torch.cat([x, x.flip(3)]).cuda().bfloat16())[0]
    assert pred.shape == (1, 33600, 290) and torch.equal(pred2[0], pred[0])       # batch independence at B=2
    # bf16 through ~90 chained layers: measured 5.8e-3 of the extent (7.4 px of |ref| up to 1467), 2.9e-2 in probability
    # (gpurun_out/parity.log, round 2); stated tolerance = 3x that
    _check_pred(pred.cpu(), ref, 1280, 1.8e-2, 9e-2, 'bf16 full yolov6m 1280 B1')
    for conf, iou, max_det in ((0.4, 0.45, 1000), (0.03, 0.65, 300)):
        rows, keep, _ = lp_post.nms_c(pred.cpu().numpy(), conf, iou, max_det)
        det, count, kept = nms_padded(pred.clone(), conf, iou, max_det, want_keep=True)
        n = int(count[0])
        assert n == len(rows[0])
        assert np.array_equal(kept[0, :n].cpu().numpy(), keep[0]) and np.array_equal(det[0, :n].cpu().numpy(), rows[0])


def test_config_yolov6m_1280_bf16_bs8_properties():
    """BASELINE configs[4] at its per-GPU batch (64 images over 8 GPUs = 8 per GPU): the autotuned variants of that shape keep
    determinism, batch independence, NMS == the C oracle, and the detections-only path == lp_nms(forward) (N = 33 600)."""
    m, _ = _prepared('yolov6m', torch.bfloat16, 0.25)
    xb = torch.rand(8, 3, 1280, 1280, generator=torch.Generator().manual_seed(6)).cuda().bfloat16()
    _batch_properties(m, xb, 0.4, 0.45, 1000, [0, 7])


# Rounding-aware oracle (oracle/lp_oracle.py, round_to=...): parameters and every layer output rounded to the engine's 16-bit type,
# fp32 accumulation -- the arithmetic contract of the fp16 / bf16 engines (the reference's --half path, inferer.py:46-50).  What is
# left between the two is the fp32 summation order inside a convolution (MFMA vs oneDNN) and the last bit of exp / rcp in SiLU: an
# fp32 difference of ~2^-22 moves an activation by one 16-bit ulp when the value sits on a rounding boundary -- about once per
# 2^11 (fp16) / 2^14 (bf16) elements and layer, i.e. ~100 / ~12 times per forward of a tiny model -- and behind the first such flip
# the two computations differ at the one-ulp level everywhere (measured: 45-83 % of the fp16 neck-map elements stay bit-equal;
# the one bf16 case without a flip, lps_tiny_64x160, agrees to 5e-6 of the extent with all three neck maps bit-equal).  So the
# MAXIMUM error against this oracle is that of a few ulps of the largest distances, like against the fp32 oracle; what it pins an
# order of magnitude tighter is the RMS error (measured 3e-5 of the extent for fp16, 3e-4 .. 2e-3 for bf16: 10-20x below the
# maxima), which a systematic difference -- a wrong rounding point, an unrounded parameter -- moves at once.
# (max coordinate error / extent, max probability error, rms coordinate error / extent, rms probability error): <= 3x measured on
# MI355X (gpurun_out/parity.log, round 3).
ROUND_TOL = {
    (torch.float16, 'lps_tiny_128x96'): (2.1e-3, 9e-4, 1.5e-4, 2.2e-5), (torch.float16, 'lps_tiny_64x160'): (2.1e-3, 9e-4, 1.5e-4, 2.2e-5),
    (torch.float16, 'v6m_tiny_96x128'): (1.1e-2, 2.5e-2, 9e-4, 1.1e-3),
    (torch.bfloat16, 'lps_tiny_128x96'): (1.7e-2, 6e-3, 9e-4, 1.2e-4), (torch.bfloat16, 'lps_tiny_64x160'): (1.7e-2, 6e-3, 9e-4, 1.2e-4),
    (torch.bfloat16, 'v6m_tiny_96x128'): (1.2e-1, 2.3e-1, 7e-3, 8.2e-3),
}


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('case,weights,name', MODEL_CASES)
def test_tiny_model_half_precision_vs_rounding_aware_oracle(case, weights, name, dtype):
    from oracle import lp_oracle
    g = load_golden(case)
    m = _tiny_model(name, weights, True)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = g['x'].to(dtype)
    ref, ref_feats = lp_oracle.forward(sd, lp_oracle.arch(name, width=0.0625), x, round_to=dtype)
    with torch.no_grad():
        pred, feats = m.cuda().to(dtype)(x.cuda())
    box_tol, prob_tol, box_rms, prob_rms = ROUND_TOL[(dtype, case)]
    _check_pred(pred.cpu(), ref, max(x.shape[2:]), box_tol, prob_tol, 'rounding-aware %s %s' % (dtype, case),
                rms_tol=None if box_rms is None else (box_rms, prob_rms))
    # the neck maps are 16-bit tensors on both sides: most elements agree exactly
    same = [float((f.float().cpu() == rf).float().mean()) for f, rf in zip(feats, ref_feats)]
    with open(os.path.join(REPO, 'gpurun_out', 'parity.log'), 'a') as f:
        f.write('%-60s neck maps bit-equal fractions %s\n' % ('rounding-aware %s %s' % (dtype, case), ['%.3f' % v for v in same]))
    assert min(same) > 0.3, same


@pytest.mark.parametrize('name,dtype,sigma,B,size,tol', [
    ('yololps', torch.float16, 0.25, 2, 640, (2e-3, 9e-3, 1e-4, 1.4e-4)),
    ('yololpn', torch.float16, 0.6, 2, 640, (1.7e-3, 8e-3, 1e-4, 2.2e-4)),
    ('yolov6m', torch.bfloat16, 0.25, 1, 1280, (2.2e-2, 1e-1, 8e-4, 2.4e-3)),
], ids=['yololps-f16', 'yololpn-f16', 'yolov6m-1280-bf16'])
def test_full_model_half_precision_vs_rounding_aware_oracle(name, dtype, sigma, B, size, tol):
    """The full-size fp16 / bf16 engines against the rounding-aware oracle (the fp32-oracle comparisons of the tests above stay
    as the accuracy statement; this one is the regression bar, see ROUND_TOL)."""
    from oracle import lp_oracle
    m, sd = _prepared(name, dtype, sigma)
    x = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(1234)).to(dtype)
    ref, _ = lp_oracle.forward(sd, lp_oracle.arch(name), x, round_to=dtype)
    with torch.no_grad():
        pred = m(x.cuda())[0]
    _check_pred(pred.cpu(), ref, size, tol[0], tol[1], 'rounding-aware full %s %s B%d %d' % (name, dtype, B, size),
                rms_tol=None if tol[2] is None else (tol[2], tol[3]))


def test_nms_more_than_max_nms_candidates():
    """nms.py:115-116: more than 30000 rows pass the mask (reachable at 1280x1280, N = 33600, eval conf 0.03): only the
    30000 best by score enter the greedy step.  Also the sort of a list longer than one LDS block (65 536 slots: four blocks)."""
    from oracle import lp_post
    from yolov6.hip.runtime import nms_padded
    pred = synth_pred(2, 33600, 31, frac_hot=1.0)
    conf = 0.03
    rows, keep, after = lp_post.nms_c(pred.numpy(), conf, 0.65, 300)
    seg_max = torch.stack([pred[..., a:b].max(-1).values for a, b in zip((13, 44, 68, 105, 142, 179, 216, 216), (44, 68, 105, 142, 179, 216, 253, 253))], -1)
    assert int(((seg_max.sum(-1) / 8.0) >= conf).sum(1).min()) > 30000          # the branch is really taken
    det, count, kept = nms_padded(pred.clone().cuda(), conf, 0.65, 300, want_keep=True)
    for b in range(2):
        n = int(count[b])
        assert n == len(rows[b]) == 300
        assert np.array_equal(kept[b, :n].cpu().numpy(), keep[b]) and np.array_equal(det[b, :n].cpu().numpy(), rows[b])
    # a selection that reaches the tail of the candidate list: a high IoU threshold keeps almost everything
    rows, keep, _ = lp_post.nms_c(pred[:1].numpy(), conf, 0.99, 31000)
    det, count, kept = nms_padded(pred[:1].clone().cuda(), conf, 0.99, 31000, want_keep=True)
    n = int(count[0])
    assert n == len(rows[0]) and n <= 30000
    assert np.array_equal(kept[0, :n].cpu().numpy(), keep[0]) and np.array_equal(det[0, :n].cpu().numpy(), rows[0])


def test_cuda_path_fails_loudly_without_extension(monkeypatch):
    from yolov6.hip import abi
    monkeypatch.setattr(abi, '_lib', None)
    monkeypatch.setattr(abi, 'LIB_PATH', '/nonexistent/libyololp_hip.so')
    with pytest.raises(RuntimeError, match='missing'):
        abi.load()


# ---------------------------------------------------------------------------------------------------
NMS_CASES = ['nms_model_tiny', 'nms_synth_600', 'nms_synth_maxdet5', 'nms_synth_obj', 'nms_crafted', 'nms_empty']


@pytest.mark.parametrize('case', NMS_CASES)
def test_nms_golden_bit_exact(case):
    from yolov6.utils.nms import non_max_suppression
    g = load_golden(case)
    p = g['pred'].clone().cuda()
    out = non_max_suppression(p, float(g['conf']), float(g['iou']), max_det=int(g['max_det']))
    assert len(out) == p.shape[0]
    for b, o in enumerate(out):
        assert o.is_cuda and o.dtype == torch.float32 and o.shape[1] == 28
        assert torch.equal(o.cpu(), g['det%d' % b]), case
    if 'pred_after' in g:                            # in-place obj*cls product on the caller's tensor
        assert torch.equal(p.cpu(), g['pred_after'])
    else:
        assert torch.equal(p.cpu(), g['pred'])


@pytest.mark.parametrize('B,N,seed,hot,conf,iou,max_det,obj_one', [
    (4, 8400, 21, 0.05, 0.4, 0.45, 1000, True),        # infer defaults
    (2, 8400, 22, 0.30, 0.03, 0.65, 300, True),        # eval defaults: every anchor is a candidate
    (3, 2100, 23, 0.50, 0.25, 0.50, 50, False),        # obj != 1, truncation by max_det
    (1, 33600, 24, 0.02, 0.4, 0.45, 1000, True),       # 1280x1280 anchor count
    (2, 77, 25, 1.00, 0.30, 0.10, 1000, True),         # fewer anchors than a wave; score runs of 16 rows straddle the images
    (2, 20000, 26, 1.00, 0.03, 0.60, 500, True),       # 20000 candidates: a sort of two LDS blocks (32 768 slots)
    (5, 8400, 27, 1.00, 0.03, 0.45, 1000, True),       # every anchor passes: one append per run of 16 rows
])
def test_nms_random_vs_oracle_bit_exact(B, N, seed, hot, conf, iou, max_det, obj_one):
    from oracle import lp_post
    from yolov6.hip.runtime import nms_padded
    pred = synth_pred(B, N, seed, frac_hot=hot, obj_one=obj_one)
    rows, keep, after = lp_post.nms_c(pred.numpy(), conf, iou, max_det)
    p = pred.clone().cuda()
    det, count, kept = nms_padded(p, conf, iou, max_det, want_keep=True)
    det, count, kept = det.cpu().numpy(), count.cpu().numpy(), kept.cpu().numpy()
    assert count.tolist() == [len(r) for r in rows]
    for b in range(B):
        n = count[b]
        assert np.array_equal(kept[b, :n], keep[b])            # bit-exact index selection, in order
        assert np.array_equal(det[b, :n], rows[b])
        assert not det[b, n:].any() and (kept[b, n:] == -1).all()
    assert np.array_equal(p.cpu().numpy(), after)
    # idempotence of the selection: feeding only the kept anchors back keeps all of them, in the same order
    b0 = 0
    if 0 < count[b0] <= 1000 and obj_one:
        sub = pred[b0:b0 + 1, torch.from_numpy(keep[b0].astype(np.int64))].clone().cuda()
        det2, count2, kept2 = nms_padded(sub, conf, iou, max_det, want_keep=True)
        assert int(count2[0]) == count[b0]
        assert kept2[0, :count[b0]].cpu().tolist() == list(range(count[b0]))


def test_nms_on_engine_output_matches_oracle():
    """End to end on one batch: pred from the HIP engine, NMS by lp_nms == oracle NMS of that same pred."""
    from oracle import lp_post
    from yolov6.utils.synth import build_synthetic
    from yolov6.utils.nms import non_max_suppression
    m = build_synthetic(CFG('yololps'), sigma=0.25).cuda().half()
    x = torch.rand(4, 3, 640, 640, generator=torch.Generator().manual_seed(99)).cuda().half()
    with torch.no_grad():
        pred, _ = m(x)
    rows, keep, _ = lp_post.nms_c(pred.cpu().numpy(), 0.4, 0.45, 1000)
    out = non_max_suppression(pred, 0.4, 0.45, max_det=1000)
    assert sum(len(r) for r in rows) > 0
    for o, r in zip(out, rows):
        assert np.array_equal(o.cpu().numpy(), r)


@pytest.mark.parametrize('name,kw,B,H,W,dtype', [
    ('yololps', dict(width=0.0625, sigma=1.5), 3, 128, 96, torch.float16),      # every level in the candidate-writing row kernel
    ('yololps', dict(sigma=0.25), 4, 640, 640, torch.float16),                   # level 2 (256 channels) goes through the scratch + score_kernel
    ('yololpn', dict(sigma=0.6), 5, 640, 416, torch.float16),
    ('yolov6m', dict(width=0.125, sigma=1.5), 2, 160, 128, torch.bfloat16),      # DFL head
    ('yololps', dict(width=0.125, sigma=1.5), 2, 256, 256, torch.float32),
    ('yolov6m', dict(sigma=0.25), 2, 192, 160, torch.bfloat16),                  # 96 / 192-channel towers: a partial last K-chunk in the row kernels
], ids=['lps-tiny', 'lps-full', 'lpn-full', 'v6m-dfl', 'lps-f32', 'v6m-full'])
def test_detections_only_forward_matches_forward_plus_nms(name, kw, B, H, W, dtype):
    """lp_engine_forward_det + lp_nms_candidates (the head writes NMS candidates, never the prediction tensor) == lp_nms on the
    prediction tensor of lp_engine_forward: detections, counts and kept anchor indices bit for bit, for the inference and
    the evaluation thresholds."""
    from yolov6.hip import runtime
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG(name), **kw).cuda().to(dtype)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(11)).cuda().to(dtype)
    with torch.no_grad():
        pred = m(x)[0]
    totals = {}
    for conf, iou, max_det in ((0.4, 0.45, 1000), (0.03, 0.65, 300), (0.9999, 0.5, 10)):
        d0, c0, k0 = runtime.nms_padded(pred.clone(), conf, iou, max_det, want_keep=True)
        for rep in range(2):
            d1, c1, k1 = runtime.detect_padded(m, x, conf, iou, max_det, want_keep=True, route='det')
            assert torch.equal(c1, c0), (conf, c0.tolist(), c1.tolist())
            assert torch.equal(k1, k0) and torch.equal(d1, d0), conf
        totals[conf] = int(c0.sum())
    # the evaluation threshold lets (nearly) every anchor through, the last one (nearly) nothing: both ends of the candidate lists
    assert totals[0.03] > 0 and totals[0.9999] < totals[0.03], totals
    out = runtime.detect(m, x, 0.03, 0.65, 300)
    ref = runtime.non_max_suppression(pred.clone(), 0.03, 0.65, 300)
    assert sum(len(o) for o in ref) > 0
    for o, r in zip(out, ref):
        assert torch.equal(o, r)


@pytest.mark.parametrize('name,kw,B,H,W,dtype', [
    ('yololps', dict(sigma=0.25), 3, 640, 640, torch.float16),
    ('yololpn', dict(sigma=0.6), 2, 320, 416, torch.float16),
    ('yololps', dict(width=0.125, sigma=1.5), 2, 256, 192, torch.bfloat16),
], ids=['lps-full', 'lpn', 'lps-tiny-bf16'])
def test_box_predictors_for_candidates_only_write_the_same_rows(name, kw, B, H, W, dtype):
    """LP_VARIANT_BOX_SPARSE (default) against LP_VARIANT_BOX_DENSE: in the detections-only forward the box predictors of a level run
    for the anchors its class predictors let pass only.  Columns 0..11 of every candidate's row are the dense form's bits, rows of
    anchors that did not pass are not written at all (the workspace is poisoned first), and detections are identical -- at the
    inference threshold, at the evaluation threshold (nearly every anchor passes) and at one nothing passes."""
    from yolov6.hip import runtime, abi
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG(name), **kw).cuda().to(dtype)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(5)).cuda().to(dtype)
    eng = runtime.engine_for(m)
    eng.autotune = False
    with torch.no_grad():
        eng.forward(x)                                            # binds the arena (op descriptions exist from then on)
    boxes = [i for i, k in enumerate(eng.op_kinds()) if k == 'head_box']
    assert len(boxes) == 3
    for conf in (0.4, 0.03, 1.0):
        got = {}
        for mode in (abi.LP_VARIANT_BOX_DENSE, abi.LP_VARIANT_BOX_SPARSE):
            for op in boxes:
                eng.set_variant(op, mode, 1)
            ws = eng.det_workspace(B, H, W)
            ws.fill_(0xFF)                                       # NaN rows: what the kernels do not write stays recognisable
            _, _, N = eng.forward_det(x, conf, ws=ws)
            torch.cuda.synchronize()
            cnt, keys, rows = [t.clone() for t in det_workspace_views(ws, B, N)]     # counts [B], keys [B][NP], candidate rows [B][N][28]
            det = runtime.nms_candidates((ws, B, N), 0.45, 300, want_keep=True)
            torch.cuda.synchronize()
            got[mode] = (cnt, keys, rows, det)
        (c0, k0, r0, d0), (c1, k1, r1, d1) = got[abi.LP_VARIANT_BOX_DENSE], got[abi.LP_VARIANT_BOX_SPARSE]
        assert torch.equal(c0, c1)
        written = 0
        for b in range(B):
            n = int(c0[b])
            a0 = (k0[b, :n] & 0xFFFFFFFF).sort().values
            a1 = (k1[b, :n] & 0xFFFFFFFF).sort().values
            assert torch.equal(a0, a1)                           # the same anchors pass (their order in the lists is arbitrary)
            assert torch.equal(r0[b, a0, :12].view(torch.int32), r1[b, a0, :12].view(torch.int32))
            assert not torch.isnan(r1[b, a0, :12]).any()
            mask = torch.ones(N, dtype=torch.bool, device=r1.device)
            mask[a0] = False
            assert torch.isnan(r1[b, mask, :12]).all()           # no row of an anchor that did not pass is touched
            assert not torch.isnan(r0[b, :, :12]).any()          # (the dense form writes them all)
            written += n
        if conf == 0.03:
            assert written > B * N // 2
        if conf == 1.0:
            assert written == 0
        for t0, t1 in zip(d0, d1):                                # detections, counts, kept anchors
            assert torch.equal(t0, t1)
    for op in boxes:
        eng.set_variant(op, abi.LP_VARIANT_BOX_SPARSE, 1)


def test_nms_rejects_bad_arguments():
    from yolov6.utils.nms import non_max_suppression
    from yolov6.hip.runtime import nms_padded
    with pytest.raises(AssertionError):
        non_max_suppression(torch.zeros(1, 8, 290, device='cuda'), conf_thres=2.0)
    with pytest.raises(ValueError):
        nms_padded(torch.zeros(1, 8, 100, device='cuda'), 0.4, 0.45, 10)
    out = non_max_suppression(torch.zeros(2, 0, 290, device='cuda'))
    assert [tuple(o.shape) for o in out] == [(0, 28), (0, 28)]


def test_infer_entry_point_on_gpu(tmp_path, monkeypatch):
    """tools/infer.py::run on the GPU (fp32 engine) reproduces its own CPU path: same detections after the
    reference's rescale + round (coordinates may flip by one pixel at a rounding boundary)."""
    import sys
    import importlib
    import numpy as np
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None}, str(ckpt))
    (tmp_path / 'imgs').mkdir()
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 255, (1160, 720, 3), dtype=np.uint8)).save(str(tmp_path / 'imgs' / 'a.png'))
    kw = dict(weights=str(ckpt), source=str(tmp_path / 'imgs'), yaml=None, img_size=[640, 640], conf_thres=0.06,
              iou_thres=0.45, max_det=50, save_txt=False, not_save_img=True)
    cpu = infer.run(device='cpu', save_dir=str(tmp_path / 'o1'), half=False, **kw)[0]
    gpu = infer.run(device='0', save_dir=str(tmp_path / 'o2'), half=False, **kw)[0]
    assert gpu.is_cuda and gpu.shape == cpu.shape and len(cpu) > 0
    assert float((gpu.cpu()[:, :12] - cpu[:, :12]).abs().max()) <= 1.0
    assert torch.equal(gpu.cpu()[:, 20:], cpu[:, 20:])               # the eight arg-max indices
    half = infer.run(device='0', save_dir=str(tmp_path / 'o3'), half=True, **kw)[0]
    assert half.shape[1] == 28


def test_eval_entry_point_speed_on_gpu(tmp_path, monkeypatch):
    """tools/eval.py::run --task speed on the GPU (row f4): the reference's three buckets (evaler.py:104-140, 507-513) come
    from HIP events on the current stream; the one-off engine set-up of a new batch shape stays outside them."""
    import sys
    import importlib
    import numpy as np
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    ev = importlib.import_module('eval')
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    rng = np.random.default_rng(2)
    for i in range(7):
        Image.fromarray(rng.integers(0, 255, (240, 320, 3), dtype=np.uint8)).save(str(img_dir / ('f%d.png' % i)))
    preds, speed, metrics = ev.run(str(img_dir), weights=str(ckpt), batch_size=4, img_size=128, conf_thres=0.4, iou_thres=0.45,
                                   task='speed', device='0', half=True, save_dir=str(tmp_path / 'sp'), name='exp')
    assert metrics is None and sum(len(b) for b in preds) == 7
    pre, inf, nms = speed
    # device time per image: a 128x128 forward of the tiny model is well under 5 ms once tuning (hundreds of timed launches,
    # seconds of host time) is kept out of the bucket; the last batch (3 images) is a second shape and is prepared untimed too
    assert 0 < inf < 5.0 and 0 < nms < 5.0 and 0 <= pre < 50.0, speed


def test_eval_entry_point_val_on_gpu(tmp_path, monkeypatch):
    """tools/eval.py::run --task val on the GPU: labels beside the images, Evaler.predict / eval with the metric counters
    from lp_eval_counts; the counters must equal the oracle's on the very detections the run produced."""
    import sys
    import importlib
    import numpy as np
    from PIL import Image
    from oracle import lp_metric as M
    from yolov6.utils import lp_metric
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    ev = importlib.import_module('eval')
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None}, str(ckpt))
    img_dir, lab_dir = tmp_path / 'ds' / 'images' / 'val', tmp_path / 'ds' / 'labels' / 'val'
    img_dir.mkdir(parents=True)
    lab_dir.mkdir(parents=True)
    rng = np.random.default_rng(1)
    for i in range(5):
        Image.fromarray(rng.integers(0, 255, (240, 320, 3), dtype=np.uint8)).save(str(img_dir / ('f%d.png' % i)))
    kw = dict(weights=str(ckpt), batch_size=2, img_size=128, conf_thres=0.03, iou_thres=0.65, task='val', half=False,
              name='exp')
    # first pass without labels: take some detections of the GPU run as labels (so that matches exist), second pass scores them
    preds, _, metrics = ev.run(str(img_dir), device='0', save_dir=str(tmp_path / 'v0'), **kw)
    assert metrics is None
    dets = [d for b in preds for d in b]
    assert sum(len(d) for d in dets) > 0
    for i, d in enumerate(dets):
        rows = []
        for det in d[:2].cpu().tolist():
            x1, y1, x2, y2 = det[:4]
            # invert the letterbox of a 240x320 frame in a 128x128 input: ratio 0.4, top pad 16
            box = [((x1 + x2) / 2) / 0.4 / 320, (((y1 + y2) / 2) - 16) / 0.4 / 240, (x2 - x1) / 0.4 / 320, (y2 - y1) / 0.4 / 240]
            cor = [(v / 0.4 / 320) if k % 2 == 0 else ((v - 16) / 0.4 / 240) for k, v in enumerate(det[4:12])]
            rows.append(' '.join('%.6f' % v for v in det[20:28] + box + cor))
        if rows:
            (lab_dir / ('f%d.txt' % i)).write_text('\n'.join(rows) + '\n')
    preds, _, metrics = ev.run(str(img_dir), device='0', save_dir=str(tmp_path / 'v1'), **kw)
    assert metrics is not None and len(metrics) == 7
    targets = [b[1] for b in ev.image_batches(str(img_dir), 128, 2)]
    from yolov6.core.evaler import Evaler
    val = Evaler(None, device=torch.device('cuda:0'), half=False)
    split = [val.split_targets(t, 2 if k < 2 else 1, 128, 128) for k, t in enumerate(targets)]
    ref_c = M.counts([[p.cpu().numpy() for p in b] for b in preds], [[t.cpu().numpy() for t in b] for b in split], strict=False)
    got_c = lp_metric.counts(preds, split)
    assert got_c.tolist() == ref_c.tolist()
    assert int(ref_c[M.I_TRUE]) > 0 and int(ref_c[M.I_PRED_BINS:M.I_PRED_BINS + 10].sum()) > 0
    assert metrics == lp_metric.finish(got_c)


def test_graph_mode_with_alternating_buffers():
    """hipGraph mode with two input buffers used in turn on a side stream, without host synchronisation: the engine keeps a
    captured graph per (input, output) pointer pair, so nothing is re-captured -- or destroyed while its last launch may
    still be running -- after the first two calls."""
    from yolov6.hip import runtime
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=0.25, sigma=1.0).cuda().half()
    xs = [torch.rand(4, 3, 256, 256, generator=torch.Generator().manual_seed(70 + i)).cuda().half() for i in range(2)]
    with torch.no_grad():
        ref = [m(x)[0].clone() for x in xs]
        eng = runtime.engine_for(m)
        eng.set_graph(True)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(side):
                for i in range(12):
                    pred = eng.forward(xs[i % 2])
                last = pred.clone()
            side.synchronize()
        finally:
            eng.set_graph(False)
    assert torch.equal(last, ref[11 % 2])


@pytest.mark.parametrize('dtype,shape,name,width', [(torch.float16, (3, 3, 160, 224), 'yololps', 0.5), (torch.bfloat16, (2, 3, 96, 128), 'yololps', 0.5),
                                                   (torch.float16, (1, 3, 640, 640), 'yololps', 0.5),
                                                   (torch.bfloat16, (2, 3, 160, 224), 'yolov6m', 0.75), (torch.float16, (1, 3, 320, 192), 'yolov6m', 0.625)],
                         ids=['lps-f16', 'lps-bf16', 'lps-640', 'v6m-48ch', 'v6m-40ch'])
def test_stem_reading_the_frame_itself_gives_the_same_bits(dtype, shape, name, width):
    """LP_VARIANT_PIPE_P: the stem gathers its pixels from the caller's NCHW frame (no input op, no space-to-depth tensor in
    between).  Same prediction bits as the input op + the stem's other kernels; a frame of another dtype takes that route."""
    import ctypes
    from yolov6.hip import runtime, abi
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG(name), width=width, sigma=1.0).cuda().to(dtype)      # (yolov6m: a 48- / 40-channel stem: the 64-row form of the kernel)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(91)).cuda().to(dtype)
    with torch.no_grad():
        eng = runtime.engine_for(m)
        eng.autotune = False
        base = eng.forward(x).clone()                               # input op + default stem kernel
        eng.set_variant(1, abi.LP_VARIANT_PIPE_P, 3)
        cfg, nb = ctypes.c_int(), ctypes.c_int()
        abi.check(eng.lib.lp_engine_op_variant(eng.h, 1, ctypes.byref(cfg), ctypes.byref(nb)), 'lp_engine_op_variant')
        assert cfg.value == abi.LP_VARIANT_PIPE_P
        assert torch.equal(eng.forward(x), base)
        assert torch.equal(eng.forward(x.float()), base)            # fp32 frame: input op + the stem's other kernel
        eng.set_variant(1, abi.LP_VARIANT_PIPE_C if name == 'yololps' else abi.LP_VARIANT_PIPE_B, 3)      # (also switches the planar form off again; the variant of the stem's packing: 32 / 64 rows)
        assert torch.equal(eng.forward(x), base)
        with pytest.raises(RuntimeError):
            eng.set_variant(2, abi.LP_VARIANT_PIPE_P, 3)            # only the stem has it


@pytest.mark.parametrize('dtype,width,shape', [(torch.float16, 0.5, (2, 3, 160, 224)), (torch.bfloat16, 0.25, (3, 3, 96, 128)),
                                               (torch.float16, 0.25, (1, 3, 64, 64)), (torch.float16, 0.5, (1, 3, 640, 640))])
def test_fused_stem_and_first_stride2_layer_give_the_same_bits(dtype, width, shape):
    """LP_VARIANT_FUSED_STEM2: input op + stem + ERBlock_2[0] as one kernel (the stem's output stays in LDS).  Same prediction bits
    as the three ops run one after the other; a frame of another dtype takes that route; tile borders, image borders and both
    template shapes (16 / 32 stem channels, 32 / 64 output channels) are covered by the sizes."""
    import ctypes
    from yolov6.hip import runtime, abi
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=width, sigma=1.0).cuda().to(dtype)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(92)).cuda().to(dtype)
    with torch.no_grad():
        eng = runtime.engine_for(m)
        eng.autotune = False
        base = eng.forward(x).clone()                               # input op + stem + conv, default kernels
        eng.set_variant(2, abi.LP_VARIANT_FUSED_STEM2, 3)
        cfg, nb = ctypes.c_int(), ctypes.c_int()
        abi.check(eng.lib.lp_engine_op_variant(eng.h, 2, ctypes.byref(cfg), ctypes.byref(nb)), 'lp_engine_op_variant')
        assert cfg.value == abi.LP_VARIANT_FUSED_STEM2
        assert torch.equal(eng.forward(x), base)
        assert torch.equal(eng.forward(x.float()), base)            # fp32 frame: the three ops
        xu = torch.empty(x.numel() + 8, dtype=dtype, device='cuda')[1:1 + x.numel()].view_as(x)
        xu.copy_(x)                                                  # a frame that is not 16-byte aligned: the three ops as well
        assert xu.data_ptr() % 16 != 0 and torch.equal(eng.forward(xu), base)
        assert torch.equal(eng.forward(x), base)
        with pytest.raises(RuntimeError):
            eng.set_variant(3, abi.LP_VARIANT_FUSED_STEM2, 3)       # only the layer behind the stem has it


@pytest.mark.parametrize('dtype,shape', [(torch.float16, (2, 3, 160, 224)), (torch.bfloat16, (1, 3, 96, 128)), (torch.float16, (1, 3, 640, 640))])
def test_fused_1x1_and_stride2_layer_give_the_same_bits(dtype, shape):
    """LP_VARIANT_FUSED_PW_S2: BiFusion's downsample(cv2(x)) -- a 1x1 layer and the 3x3 stride-2 layer behind it -- as one kernel
    (the 1x1 output stays in LDS): same prediction bits as the two launches."""
    import ctypes
    from yolov6.hip import runtime, abi
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=0.5, sigma=1.0).cuda().to(dtype)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(93)).cuda().to(dtype)
    with torch.no_grad():
        eng = runtime.engine_for(m)
        eng.autotune = False
        base = eng.forward(x).clone()
        took = []
        for op in range(eng.lib.lp_engine_num_ops(eng.h)):
            try:
                eng.set_variant(op, abi.LP_VARIANT_FUSED_PW_S2, 3)
                took.append(op)
            except RuntimeError:
                pass
        assert len(took) >= 1                                   # the 64-channel pair at the highest resolution of the neck
        cfg, nb = ctypes.c_int(), ctypes.c_int()
        abi.check(eng.lib.lp_engine_op_variant(eng.h, took[0], ctypes.byref(cfg), ctypes.byref(nb)), 'lp_engine_op_variant')
        assert cfg.value == abi.LP_VARIANT_FUSED_PW_S2
        assert torch.equal(eng.forward(x), base)


def test_inflight_pipeline_matches_single_engine():
    """Several batches in flight (yolov6/core/pipeline.py): every batch gets the bits a single engine gives it, the
    other engines take over the first engine's tuning, and the results do not depend on the interleaving."""
    from yolov6.core.pipeline import InflightForward
    from yolov6.hip import runtime
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=0.25, sigma=1.0).cuda().half()
    xs = [torch.rand(3, 3, 128, 192, generator=torch.Generator().manual_seed(50 + i)).cuda().half() for i in range(7)]
    with torch.no_grad():
        ref = [m(x)[0].clone() for x in xs]                      # one engine, one batch at a time
        pipe = InflightForward(m, depth=3)
        outs = [pipe.submit(x) for x in xs]
        for (pred, done), r in zip(outs, ref):
            done.synchronize()
            assert torch.equal(pred, r)
    eng0 = runtime.engine_for(m)
    assert pipe.engines[0] is eng0 and all(e.tuned == eng0.tuned and len(e.tuned) == 1 for e in pipe.engines)


def test_tuned_choices_survive_a_rebind_and_copy_tuning(monkeypatch):
    """What the library remembers of a tuned shape is the whole kernel choice of every op -- variant, tile and the fused forms (the
    full-width yololps has all four: test_graph_rules_gpu.py).  ``state`` reads it back through the ABI; every assertion holds
    whichever variants the timing prefers.  Binding another shape and the first one again, copy_tuning before and after a bind, and
    a refused set_variant all leave the tuned state, and the prediction bits with it; an accepted set_tile forgets the bound shape
    (both shapes are made to forget here: a shape that is not remembered runs with the choices of the shape bound before it)."""
    import lp_testing as X
    from yolov6.hip import runtime
    from yolov6.utils.synth import build_synthetic
    for name in ('LP_NO_MFMA16', 'LP_S2P16', 'LP_TUNE_CFG128', 'LP_TUNE_NBUF', 'LP_NO_STEM_S2D', 'LP_SINGLE_LANE', 'LP_LANES', 'LP_AUTOTUNE',
                 'LP_NO_PLANAR', 'LP_NO_FUSED_STEM', 'LP_NO_FUSED_PW', 'LP_NO_FUSED_BF'):
        monkeypatch.delenv(name, raising=False)
    forms = (X.PIPE_P, X.FUSED_STEM2, X.FUSED_PW_S2, X.FUSED_BIFUSION)
    A, B = (2, 128, 128), (2, 128, 192)
    m = build_synthetic(CFG('yololps')).eval()
    xA, xB = (torch.rand(s[0], 3, s[1], s[2], generator=torch.Generator().manual_seed(7)).cuda().half() for s in (A, B))
    new = lambda: runtime.Engine.from_model(m, torch.float16, torch.device('cuda:0'))   # noqa: E731

    def state(eng):
        out = []
        for i in range(eng.lib.lp_engine_num_ops(eng.h)):
            try:
                tile = eng.tile(i)
            except RuntimeError:
                tile = None
            out.append((eng.variant(i), tile, eng.lib.lp_engine_op_carrier(eng.h, i, 1)))
        return out

    def next_tile(eng):
        """An accepted set_tile: the next choice of the first op whose tile is its plain one (clamped, never refused)."""
        i, (_, tile, _) = next((i, s) for i, s in enumerate(state(eng)) if s[1] is not None and s[0][0] not in forms)
        eng.set_tile(i, tile[0] + 1)
        assert eng.tile(i)[0] == tile[0] + 1

    e1 = new()
    assert e1.autotune
    pA = e1.forward(xA).clone()                                  # binds, tunes, runs
    sA = state(e1)
    e1.forward(xB)
    assert B in e1.tuned
    e1.bind(*A)
    assert state(e1) == sA and A in e1.tuned and torch.equal(e1.forward(xA), pA)

    e2 = new()
    e2.copy_tuning(e1)                                           # before any bind: applied by the bind
    assert torch.equal(e2.forward(xA), pA) and state(e2) == sA
    e3 = new()
    e3.bind(*A)
    e3.copy_tuning(e1)                                           # bound already: applied at once
    assert state(e3) == sA

    with pytest.raises(RuntimeError, match='-4'):
        e1.set_variant(3, X.FUSED_STEM2, 3)                      # only the layer behind the stem has it
    assert state(e1) == sA
    e1.bind(*B)
    e1.bind(*A)
    assert state(e1) == sA                                       # ... and shape A is still remembered
    e1.bind(*B)
    next_tile(e1)                                                # forgets shape B
    e1.bind(*A)
    assert state(e1) == sA
    next_tile(e1)                                                # forgets shape A
    hand = state(e1)
    assert hand != sA
    e1.bind(*B)
    e1.bind(*A)
    assert state(e1) == hand


def test_inflight_detections_only_pipeline_with_a_shape_change():
    """``InflightForward.submit_det`` (bench.py's default path: several batches in flight, the head writes NMS candidates, the
    NMS runs on the caller's stream): every batch gets the detections ``detect_padded`` gives it, also when the batch shape
    changes in mid-pipeline (the slot's candidate workspace is replaced only behind the NMS that still reads the old one)."""
    from yolov6.core.pipeline import InflightForward
    from yolov6.hip import runtime
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=0.25, sigma=1.0).cuda().half()
    shapes = [(3, 128, 192)] * 5 + [(2, 192, 128)] * 4 + [(3, 128, 192)] * 3
    xs = [torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(80 + i)).cuda().half() for i, (b, h, w) in enumerate(shapes)]
    conf, iou, max_det = 0.1, 0.5, 200
    with torch.no_grad():
        ref = [runtime.nms_padded(m(x)[0].clone(), conf, iou, max_det)[:2] for x in xs]
        ref = [(d.clone(), c.clone()) for d, c in ref]
        assert sum(int(c.sum()) for _, c in ref) > 0
        pipe = InflightForward(m, depth=3)
        post = torch.cuda.Stream()
        outs = []
        for x in xs:
            handle, ready, release = pipe.submit_det(x, conf)
            post.wait_event(ready)
            with torch.cuda.stream(post):
                det, count, _ = runtime.nms_candidates(handle, iou, max_det)
                release(post)
            outs.append((det, count))
        torch.cuda.synchronize()
    for (d, c), (rd, rc) in zip(outs, ref):
        assert torch.equal(c, rc) and torch.equal(d, rd)


def test_detect_switches_to_the_prediction_tensor_at_high_candidate_density():
    """``runtime.detect`` (what Inferer.infer calls): while few anchors pass the confidence mask it runs the detections-only
    forward, once the previous batch showed a density above ``det_crossover`` it runs forward + lp_nms -- same detections."""
    from yolov6.hip import runtime
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=0.25, sigma=1.0).cuda().half()
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(8)).cuda().half()
    eng = runtime.engine_for(m)
    with torch.no_grad():
        ref = {c: runtime.non_max_suppression(m(x)[0].clone(), c, 0.5, 300) for c in (0.999, 0.01)}
        assert sum(len(o) for o in ref[0.01]) > 0
        routes = []
        for conf in (0.999, 0.999, 0.01, 0.01, 0.01, 0.999, 0.999):
            before = dict(eng.det_routes)
            out = runtime.detect(m, x, conf, 0.5, 300)          # (the list form synchronises: the density probe has landed)
            routes.append('pred' if eng.det_routes['pred'] > before['pred'] else 'det')
            for o, r in zip(out, ref[conf]):
                assert torch.equal(o, r), (conf, routes)
    # conf 0.01 lets every anchor through: the call after the first such batch takes the tensor route, and the call after the
    # first sparse batch is back on the detections-only forward
    assert eng.pass_rate is not None
    assert routes == ['det', 'det', 'det', 'pred', 'pred', 'pred', 'det'], routes


def test_bench_under_the_distributed_launcher():
    """The driver's multi-GPU launch line with one rank: ``python -m torch.distributed.run --nproc-per-node 1 bench.py --gpus 1``
    as a fresh child (the launcher starts before anything touches the GPU): RCCL process group, sharded step, one JSON line."""
    import json
    import subprocess
    import sys
    port = 29700 + os.getpid() % 200
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
           '--full', '--no-cpu-baseline']
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 1 and d['config']['parallelism'].startswith('dp1') and d['steps'] == 3
    assert np.isfinite(d['value']) and d['value'] > 0 and d['unit'] == 'images/s' and d['scaling'] == 'weak'
    assert 'roofline' in d and d['roofline']['bound'] in ('mfma', 'hbm')


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain ``bench.py`` run (no --full) times exactly --steps steps, prints the headline fields only, and --dump-outputs
    writes the detections of the last timed step: det [B, max_det, 28] fp32 with zeroed padding rows, counts [B]."""
    import json
    import subprocess
    import sys
    cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '4',
           '--dump-outputs', str(tmp_path)]
    r = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    d = json.loads(lines[0])
    assert d['steps'] == 2 and d['warmup'] == 1 and d['dtype'] == 'f16' and d['unit'] == 'images/s' and d['higher_is_better'] is True
    assert np.isfinite(d['value']) and d['value'] > 0 and d['ms_per_step'] > 0
    assert abs(d['value'] - 4 * 1e3 / d['ms_per_step']) <= 0.01 * d['value']
    for k in ('roofline', 'cpu_baseline', 'value_inflight1', 'step_ms_inflight1'):
        assert k not in d, k
    det, cnt = np.load(tmp_path / 'detections.npy'), np.load(tmp_path / 'counts.npy')
    assert det.dtype == np.float32 and det.shape == (4, 1000, 28) and cnt.dtype == np.float64 and cnt.shape == (4,)
    assert np.all(np.isfinite(det)) and np.all((cnt >= 0) & (cnt <= 1000)) and cnt.sum() > 0
    for b, n in enumerate(cnt.astype(int)):
        assert not det[b, n:].any() and det[b, :n].any(axis=1).all()
    assert abs(cnt.mean() - d['config']['mean_detections_per_image']) <= 0.051


def test_gather_detections_rccl_on_side_stream():
    """The all-gather of padded detections through RCCL (backend nccl), issued on a side stream like bench.py does;
    one rank is all a one-GPU box offers, so this checks the plumbing (RCCL loads, the collective runs on our tensors
    and stream), the multi-rank data movement itself is covered by the gloo test on CPU."""
    import torch.distributed as dist
    from yolov6.core.sharded import gather_detections
    from yolov6.hip.runtime import nms_padded
    port = 29600 + os.getpid() % 1000
    dist.init_process_group('nccl', init_method='tcp://127.0.0.1:%d' % port, rank=0, world_size=1,
                            device_id=torch.device('cuda:0'))
    try:
        pred = synth_pred(3, 2100, 31, frac_hot=0.2).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            det, count, _ = nms_padded(pred, 0.4, 0.45, 100)
            det_all, count_all = gather_detections(det, count, force_collective=True)
        side.synchronize()
        assert torch.equal(det_all, det) and torch.equal(count_all, count)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('h0,w0,size', [(1160, 720, [640, 640]), (480, 640, [640, 640]), (640, 640, [640, 640]),
                                         (300, 500, [320, 416]), (2000, 1500, [640, 640])])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_preprocess_letterbox_matches_host_mirror(h0, w0, size, dtype):
    """lp_preprocess_letterbox == the host mirror's letterbox + transpose + /255 (bit-exact: same integer bilinear).  bfloat16,
    which Inferer.precess_image does not produce, and the kernels' edge shapes: tests/test_letterbox_gpu.py."""
    from yolov6.hip.runtime import preprocess_letterbox
    from yolov6.core.inferer import Inferer
    rng = np.random.default_rng(h0 + w0)
    frame = rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8)
    ref, _ = Inferer.precess_image(frame, size, 32, dtype == torch.float16)
    got = preprocess_letterbox(torch.from_numpy(frame).cuda(), size, 32, dtype)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert torch.equal(got.cpu(), ref)


def test_rescale_round_matches_reference_formula():
    from yolov6.hip.runtime import rescale_round
    from yolov6.core.inferer import Inferer
    g = torch.Generator().manual_seed(5)
    det = torch.rand(300, 28, generator=g) * 700 - 30
    det[:7, :12] = torch.tensor([0.5, 1.5, 2.5, -0.5, 639.5, 415.5, 100.25, 100.75, 3.5, 4.5, 1e-3, 720.0])   # ties, edges
    for ori, tgt in (((640, 416), (1160, 720, 3)), ((640, 640), (480, 640, 3)), ((320, 416), (300, 500, 3))):
        ref = det.clone()
        ref[:, :12] = Inferer.rescale(ori, ref[:, :12], tgt).round()
        got = rescale_round(ori, det.clone().cuda(), tgt).cpu()
        assert torch.equal(got, ref)


def test_rescale_and_preprocess_kernels_match_the_reference_fixtures(golden):
    """lp_rescale_round / lp_preprocess_letterbox against the fixtures captured from the reference's own Inferer statics
    (tests/golden/make_golden_inferer.py): the rounded 12 coordinates bit for bit, the un-resized frames pixel for pixel."""
    from yolov6.hip.runtime import rescale_round, preprocess_letterbox
    z = golden('inferer_ref')
    for k in range(int(z['rescale_n'])):
        ori, tgt = tuple(z['rescale_%d_ori' % k].tolist()), tuple(z['rescale_%d_tgt' % k].tolist())
        det = torch.zeros(z['rescale_%d_in' % k].shape[0], 28)
        det[:, :12] = z['rescale_%d_in' % k]
        det[:, 12:] = 0.25
        got = rescale_round(ori, det.clone().cuda(), tgt).cpu()
        assert torch.equal(got[:, :12], z['rescale_%d_round' % k]), k
        assert torch.equal(got[:, 12:], det[:, 12:])
    for k in range(int(z['pre_n'])):
        frame = z['pre_%d_frame' % k].contiguous()
        size, half = int(z['pre_%d_size' % k]), bool(int(z['pre_%d_half' % k]))
        got = preprocess_letterbox(frame.cuda(), [size, size], 32, torch.float16 if half else torch.float32)
        assert torch.equal(got.float().cpu(), z['pre_%d_out' % k]), k


def test_engines_dropped_with_work_in_flight():
    """Engine lifetime (the round-1 abort was an object destroyed under in-flight work): drop a several-batches-in-flight
    pipeline and a standalone engine right after enqueueing forwards; lp_engine_destroy must wait for the side lanes."""
    import gc
    from yolov6.core.pipeline import InflightForward
    from yolov6.hip import runtime
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=0.125, sigma=1.5).cuda().half()
    x = torch.rand(8, 3, 256, 256, generator=torch.Generator().manual_seed(3)).cuda().half()
    with torch.no_grad():
        ref = m(x)[0].clone()
        pipe = InflightForward(m, 3)
        outs = [pipe.submit(x, fresh=False) for _ in range(9)]
        preds = [p for p, _ in outs]
        del pipe, outs
        gc.collect()
        eng = runtime.Engine.from_model(m, torch.float16, x.device)
        eng.copy_tuning(runtime.engine_for(m))
        p2 = eng.forward(x)
        del eng
        gc.collect()
    torch.cuda.synchronize()
    for p in preds + [p2]:
        assert torch.equal(p, ref)


def test_execution_lanes_give_the_same_bits_as_one_lane():
    """One lane is the default since round 3; the side lanes (independent branches of the graph on forked streams) stay
    selectable and must not change a bit, in the plain and in the detections-only forward, also with a graph replay."""
    from yolov6.hip import runtime
    from yolov6.utils.synth import build_synthetic
    for name in ('yololps', 'yolov6m'):
        m = build_synthetic(CFG(name), width=0.125, sigma=1.5).cuda().half()
        x = torch.rand(4, 3, 192, 256, generator=torch.Generator().manual_seed(5)).cuda().half()
        with torch.no_grad():
            eng = runtime.engine_for(m)
            assert eng.single_lane
            ref = m(x)[0].clone()
            det_ref = [t.clone() for t in runtime.detect_padded(m, x, 0.05, 0.45, 300, route='det')[:2]]
            eng.set_single_lane(False)
            got = m(x)[0].clone()
            det = runtime.detect_padded(m, x, 0.05, 0.45, 300, route='det')[:2]
            assert torch.equal(got, ref), name
            assert torch.equal(det[0], det_ref[0]) and torch.equal(det[1], det_ref[1]), name
            m.lp_graph = True                       # (what Inferer sets: the forward replayed as one hipGraph, lanes captured)
            got = m(x)[0].clone()
            got2 = m(x)[0].clone()
            m.lp_graph = False
            eng.set_single_lane(True)
            assert torch.equal(got, ref) and torch.equal(got2, ref), name
        assert int(det_ref[1].sum()) > 0


def test_nms_on_two_streams_at_once():
    """The NMS workspace is per (device, stream): two streams post-processing different batches must not share one."""
    from yolov6.hip.runtime import nms_padded
    preds = [synth_pred(4, 8400, 40 + k, frac_hot=0.3).cuda() for k in range(2)]
    ref = [nms_padded(p.clone(), 0.25, 0.5, 300)[:2] for p in preds]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    got = []
    for rep in range(3):
        for p, s in zip(preds, streams):
            with torch.cuda.stream(s):
                got.append(nms_padded(p.clone(), 0.25, 0.5, 300)[:2])
    torch.cuda.synchronize()
    for i, (d, c) in enumerate(got):
        assert torch.equal(d, ref[i % 2][0]) and torch.equal(c, ref[i % 2][1])


def test_input_too_large_for_the_pool_chain_is_refused_at_bind():
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=0.0625).cuda().half()
    with torch.no_grad(), pytest.raises(ValueError, match='pool chain'):
        m(torch.zeros(1, 3, 2080, 2080, device='cuda', dtype=torch.float16))


def test_graph_replay_matches_eager_launches():
    """hipGraph replay of the forward (lp_engine_set_graph) == re-issued launches, also after the input pointer or the
    shape changed (re-capture), and the persistent prediction buffer is overwritten by the next call."""
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5).cuda().half()
    xs = [torch.rand(1, 3, 128, 96, generator=torch.Generator().manual_seed(k)).cuda().half() for k in range(3)]
    xs.append(torch.rand(2, 3, 64, 160, generator=torch.Generator().manual_seed(9)).cuda().half())
    with torch.no_grad():
        ref = [m(x)[0].clone() for x in xs]
        m.lp_graph = True
        for _ in range(2):
            for x, r in zip(xs, ref):
                p, feats = m(x)
                assert torch.equal(p, r)
        p1, _ = m(xs[0])
        keep = p1.clone()
        p2, _ = m(xs[1])
        assert p2.data_ptr() == p1.data_ptr() and torch.equal(p2, ref[1]) and not torch.equal(keep, ref[1])
        m.lp_graph = False
        assert torch.equal(m(xs[2])[0], ref[2])
