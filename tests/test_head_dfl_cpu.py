"""The data, the references and the bound of the DFL box decode tests (tests/test_head_dfl_gpu.py), and the proof on the CPU that
those tests can fail: a numpy fp32 emulation of MODE_DECODE's DFL branch in the kernel's operation order passes both regimes, and
six deliberately wrong emulations fail both on the data of every case.

Geometry and helpers are those of test_head_exact_gpu.py (96 x 160 input, B = 3, maps 12 x 20 / 6 x 10 / 3 x 5, N = 315).

Coded regime.  For each side k and each bit j of a 5-bit code one feature channel holds +-32 by bit j of the pixel's target bin
t_k; bin row (k, i) has weight +-8 on that channel by bit j of i (zero on the other sides' code channels).  The code part of logit
(k, i) is 256 (5 - 2 hamming(i, t_k)): the target bin leads every other bin by at least 512.  A pixel whose code channel (k, j)
is zeroed has bins t_k and t_k ^ (1 << j) tied EXACTLY at 1024, 512 above the rest.  The other channels carry quarter-grid noise
whose bin-row weights and bias are the same for all bins of a side: an offset that z - m removes exactly (it would break the
ties otherwise).  All values are exact in bf16 and all sums in fp32, so expf(0) = 1 and expf(x <= -128) = 0 give p = 1 or
1/2, 1/2 and the distance is exactly proj[t] or (proj[a] + proj[b]) / 2, whatever the quality of the exponential.  proj holds
distinct multiples of 1/4 in [0, 16] in seeded order: a shifted index cannot pass as an offset.  Logits reach +-1300: a softmax
that does not subtract the maximum overflows.

Rounding regime.  head_data's grid ranges (features in [-2, 2], weights in [-1, 1], biases in [-2, 2]), logits exact fp32 sums,
reference softmax -> sum p_i proj_i -> decode in float64, bound lp_testing.dfl_box_bounds (derived, E = 1).  One addition to the
issue's data: the bias of a side's bin rows carries a common offset of +96 (sides 0, 1) or -96 (sides 2, 3).  It leaves the float64
softmax and z - m unchanged, and it is what makes a missing maximum visible here: with logits of a few tens expf neither overflows
nor underflows, and a softmax without the subtraction is then as accurate as one with it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lp_testing as X
from test_head_exact_gpu import B, BF16, F16, F32, LEVEL_OFF, MAPS, N, NCLS, head_data

BINS = (2, 6, 7, 17, 30)
W_A, W_B, W_C = (64, 128, 256), (96, 192, 384), (320, 64, 64)      # one to six K-chunks, partial chunks, yolov6m's own head widths
CASES = [                                                            # (bins, dtype, channels per level)
    (17, F16, W_A), (17, F16, W_B), (17, F16, W_C), (17, BF16, W_A), (17, BF16, W_B), (17, BF16, W_C), (17, F32, W_A), (17, F32, W_B),
    (2, F16, W_C), (2, BF16, W_A), (2, F32, W_B),                    # 2..6 bins: the 32-cout tile
    (6, F16, W_A), (6, BF16, W_B), (6, F32, W_A),                    # 6 bins = 32 couts: that tile exactly full
    (7, F16, W_B), (7, BF16, W_C), (7, F32, W_B),                    # 36 couts: the first of the 128-cout tile
    (30, F16, W_B), (30, BF16, W_C), (30, F32, W_A),                 # 128 couts: that tile exactly full
]
case_id = lambda c: 'bins%d-%s-%s' % (c[0], {F16: 'f16', BF16: 'bf16', F32: 'f32'}[c[1]], '-'.join(map(str, c[2])))
NBITS = 5
SOFT_OFFSET = 96.0
_cache = {}


def coded_proj(bins, seed=7):
    """``bins`` distinct multiples of 1/4 in [0, 16], in seeded order."""
    g = torch.Generator().manual_seed(seed + bins)
    return torch.randperm(65, generator=g)[:bins].double() / 4


def model_proj(bins):
    return torch.linspace(0, bins - 1, bins, dtype=torch.float64)


def _code_channels(c):
    """The 20 code channels of a c-channel level, spread from the first channel to the last (every K-chunk holds some)."""
    ch = np.round(np.linspace(0, c - 1, 4 * NBITS)).astype(np.int64)
    assert len(set(ch.tolist())) == 4 * NBITS
    return ch.reshape(4, NBITS)


def _targets(bins, rng):
    """Target bins [B,N,4] and the zeroed code bit [B,N,4] (-1: none).  Three pixels of four (and the last pixel of every level,
    and image 0's first ``bins`` pixels, where side k has target (n + k) % bins: every bin on every side) get min(4, bins)
    different targets; 30 % of the (pixel, side) pairs get one bit zeroed that has a partner bin below ``bins``."""
    t = rng.integers(0, bins, (B, N, 4))
    distinct = rng.random((B, N)) < 0.75
    distinct[:, [o - 1 for o in LEVEL_OFF[1:]]] = True
    for b, n in zip(*np.nonzero(distinct)):
        head = rng.permutation(bins)[:4]
        t[b, n] = rng.permutation(np.concatenate([head, rng.integers(0, bins, 4 - len(head))]))
    cover = np.arange(bins)
    t[0, :bins] = (cover[:, None] + np.arange(4)[None]) % bins
    bit = np.full((B, N, 4), -1)
    for b, n, k in zip(*np.nonzero(rng.random((B, N, 4)) < 0.30)):
        ok = [j for j in range(NBITS) if (t[b, n, k] ^ (1 << j)) < bins]
        bit[b, n, k] = ok[rng.integers(0, len(ok))]
    return t, bit


def coded_data(bins, widths, seed=300):
    """Per level (x, wc, bc, wb, bb) in float64 as head_data gives them, wb / bb with 4 * bins + 8 rows; and (targets, zeroed bits).
    The class weights are zero on the code channels (the class path sees the noise alone; its bias follows head_data's rule)."""
    rng = np.random.default_rng(seed + bins)
    t, bit = _targets(bins, rng)
    out = []
    for i, (c, (h, w)) in enumerate(zip(widths, MAPS)):
        code = _code_channels(c)
        noise = np.setdiff1d(np.arange(c), code.flatten())
        s = seed + 10 * i
        x = X.grid_rand((B, c, h, w), s, -2.0, 2.0)
        wc = X.grid_rand((NCLS, c), s + 1, -1.0, 1.0)
        wc[:, code.flatten()] = 0.0
        sd = (len(noise) * 1.5 * 5.0 / 12.0) ** 0.5
        bc = X.grid_rand((NCLS,), s + 2, -0.5, 0.5, 1.0 / 16) - round(2.25 * sd * 16) / 16.0
        wb = torch.zeros(4 * bins + 8, c, dtype=torch.float64)
        bb = torch.zeros(4 * bins + 8, dtype=torch.float64)
        side_w = X.grid_rand((4, len(noise)), s + 3, -1.0, 1.0)
        side_b = X.grid_rand((4,), s + 4, -2.0, 2.0, 1.0 / 16)
        wb[4 * bins:] = X.grid_rand((8, c), s + 5, -1.0, 1.0)         # the corner rows: independent, on every channel
        bb[4 * bins:] = X.grid_rand((8,), s + 6, -2.0, 2.0, 1.0 / 16)
        tl = t[:, LEVEL_OFF[i]:LEVEL_OFF[i + 1]].reshape(B, h, w, 4)
        zl = bit[:, LEVEL_OFF[i]:LEVEL_OFF[i + 1]].reshape(B, h, w, 4)
        for k in range(4):
            rows = slice(k * bins, (k + 1) * bins)
            wb[rows, torch.from_numpy(noise)] = side_w[k]
            bb[rows] = side_b[k]
            for j in range(NBITS):
                on = ((tl[..., k] >> j) & 1) * 2.0 - 1.0
                x[:, code[k, j]] = torch.from_numpy(np.where(zl[..., k] == j, 0.0, 32.0 * on))
                wb[rows, code[k, j]] = torch.from_numpy(((np.arange(bins) >> j) & 1) * 16.0 - 8.0)
        out.append((x, wc, bc, wb, bb))
    return out, t, bit


def soft_data(bins, widths, seed=700):
    """head_data's features and class predictors with box rows of 4 * bins + 8 outputs on the same grid; the bins of a side share a
    bias offset of +-SOFT_OFFSET (module docstring)."""
    out = []
    for i, (x, wc, bc, _, _) in enumerate(head_data(widths, seed)):
        c = x.shape[1]
        wb = X.grid_rand((4 * bins + 8, c), seed + 10 * i + 5, -1.0, 1.0)
        bb = X.grid_rand((4 * bins + 8,), seed + 10 * i + 6, -2.0, 2.0, 1.0 / 16)
        bb[:2 * bins] += SOFT_OFFSET
        bb[2 * bins:4 * bins] -= SOFT_OFFSET
        out.append((x, wc, bc, wb, bb))
    return out


def logits64(data, dtype):
    """[B,N,4 * bins + 8] float64: the box rows' sums, after the checks that they are exact in fp32 in any order."""
    for x, wc, _, wb, bb in data:
        for t in (x, wc, wb):
            assert torch.equal(t.to(dtype).double(), t) and torch.equal(torch.round(t * 4) / 4, t)
        assert torch.equal(torch.round(bb * 16) / 16, bb)
        assert float((x.abs().amax((0, 2, 3)) * wb.abs()).sum(1).max() + bb.abs().max()) < 2 ** 20       # 2^24 units of 1/16
    return torch.cat([F.conv2d(x, wb[..., None, None], bb).reshape(B, wb.shape[0], -1) for x, _, _, wb, bb in data], -1).permute(0, 2, 1)


def mask_value64(data):
    """The confidence mask's value [B,N] in float64 (nms.py's mean: ad4 twice, ad5 omitted), as test_head_exact_gpu.reference."""
    prob = torch.cat([torch.sigmoid(F.conv2d(x, wc[..., None, None], bc)).reshape(B, NCLS, -1) for x, wc, bc, _, _ in data], -1).permute(0, 2, 1)
    best = [prob[..., a - 13:b - 13].max(-1).values for a, b in zip(X.SEG[:-1], X.SEG[1:])]
    return (sum(best[:7]) + best[6]) / 8.0


def _anchors():
    from oracle import lp_oracle
    pts, st = lp_oracle.anchors(MAPS)
    return pts.double(), st.double()


def decode64(dist, cor):
    """(prediction columns 0..12 [B,N,13], candidate-row columns 0..11 [B,N,12]) in float64: the oracle's decode and xywh2xyxy."""
    from oracle import lp_oracle
    pts, st = _anchors()
    box, corners = lp_oracle.decode(dist, cor, pts, st)
    pred = torch.cat([box, torch.ones(B, N, 1, dtype=torch.float64), corners], -1)
    rows = torch.cat([box[..., :2] - box[..., 2:] / 2, box[..., :2] + box[..., 2:] / 2, corners], -1)
    return pred, rows


def coded_case(bins, dtype, widths):
    """Data, proj, logits and the expected bits of a coded case; the conditions on the data are asserted here."""
    key = ('coded', bins, dtype, widths)
    if key in _cache:
        return _cache[key]
    data, t, bit = coded_data(bins, widths)
    proj = coded_proj(bins)
    assert len(set(proj.tolist())) == bins and torch.equal(torch.round(proj * 4) / 4, proj) and 0 <= float(proj.min()) and float(proj.max()) <= 16
    z = logits64(data, dtype)
    zb = z[..., :4 * bins].reshape(B, N, 4, bins)
    top = zb == zb.amax(-1, keepdim=True)
    ntop = top.sum(-1)
    assert int(ntop.min()) >= 1 and int(ntop.max()) <= 2
    assert float((zb.amax(-1, keepdim=True) - zb)[~top].min()) >= 128.0                       # every other bin: expf gives 0
    tt, bb_ = torch.from_numpy(t), torch.from_numpy(bit)
    partner = torch.where(bb_ >= 0, tt ^ torch.bitwise_left_shift(torch.ones_like(bb_), bb_.clamp(min=0)), tt)
    want_top = F.one_hot(tt, bins).bool() | F.one_hot(partner, bins).bool()
    assert torch.equal(top, want_top)                                                          # the ties are where they were planted
    assert float((ntop == 2).double().mean()) >= 0.05
    for k in range(4):
        assert set(t[..., k].flatten().tolist()) == set(range(bins))                           # every bin is a target on every side
    ndiff = np.array([[len(set(t[b, n].tolist())) for n in range(N)] for b in range(B)])
    assert float((ndiff == min(4, bins)).mean()) >= 0.5                                       # (two bins cannot give four targets)
    assert float(z.abs().max()) > 1200.0
    dist = (top.double() * proj).sum(-1) / ntop
    pred, rows = decode64(dist, z[..., 4 * bins:])
    out = dict(data=data, proj=proj, z=z, pred=X.to_exact_f32(pred), rows=X.to_exact_f32(rows), ties=float((ntop == 2).double().mean()),
               mask=mask_value64(data))
    _cache[key] = out
    return out


def soft_case(bins, dtype, widths):
    """Data, logits, and per proj (the model's linspace, the coded regime's non-monotone one): float64 reference and bounds."""
    key = ('soft', bins, dtype, widths)
    if key in _cache:
        return _cache[key]
    data = soft_data(bins, widths)
    z = logits64(data, dtype)
    p = torch.softmax(z[..., :4 * bins].reshape(B, N, 4, bins), -1)
    pts, st = _anchors()
    refs = []
    for proj in (model_proj(bins), coded_proj(bins)):
        dist, mag = (p * proj).sum(-1), (p * proj.abs()).sum(-1)
        share = float(((dist[..., None] - proj).abs().amin(-1) > 1e-3).double().mean())
        assert share >= 0.25, share                                                            # the softmax is really soft
        pred, rows = decode64(dist, z[..., 4 * bins:])
        bp, br = X.dfl_box_bounds(dist, mag, pts, st, bins)
        refs.append(dict(proj=proj, dist=dist, dist_mag=mag, pred=pred, rows=rows, pred_bound=bp, rows_bound=br, soft_share=share, mag=float(mag.max()),
                         corners=X.to_exact_f32(pred[..., 5:])))
    out = dict(data=data, z=z, refs=refs, mask=mask_value64(data))
    _cache[key] = out
    return out


# ---- the two checks, as the GPU tests apply them ---------------------------------------------------------------------------------
BOX_P, COR_P, BOX_R, COR_R = [0, 1, 2, 3], list(range(5, 13)), [0, 1, 2, 3], list(range(4, 12))


def _bits(t):
    return t.contiguous().view(torch.int32)


def coded_mismatches(pred, rows, want):
    """Number of elements of prediction columns 0..3, 5..12 (+ column 4 != 1) and candidate-row columns 0..11 whose bits differ."""
    cols = BOX_P + COR_P
    n = int((_bits(pred[..., cols]) != _bits(want['pred'].to(pred.device)[..., cols])).sum()) + int((pred[..., 4] != 1).sum())
    return n + int((_bits(rows[..., :12]) != _bits(want['rows'].to(rows.device))).sum())


def soft_check(pred, rows, ref):
    """(worst |error| / bound over the box columns of both forms, number of corner elements whose bits differ)."""
    pred, rows = pred.cpu(), rows.cpu()
    worst = max(X.bound_excess(pred[..., BOX_P], ref['pred'][..., BOX_P], ref['pred_bound'])[0],
                X.bound_excess(rows[..., BOX_R], ref['rows'][..., BOX_R], ref['rows_bound'])[0])
    bad = int((_bits(pred[..., COR_P]) != _bits(ref['corners'])).sum()) + int((_bits(rows[..., COR_R]) != _bits(ref['corners'])).sum())
    return worst, bad


# ---- the kernel's DFL branch in numpy fp32, in its operation order -----------------------------------------------------------------
MUTATIONS = ('proj_shift', 'sum_short', 'swap_sides', 'no_max', 'corner_offset', 'quad_rotate')


def emulate(z64, proj64, bins, mutation=None, want_dist=False):
    """MODE_DECODE's DFL branch on fp32 logits [B,N,4 * bins + 8]: per side m = max, sum += expf(z - m), acc += expf(z - m) / sum *
    proj[i], the quad's four distances, then both forms of the decode in fp32.  -> (pred [B,N,13], rows [B,N,12]) as torch fp32
    (``want_dist``: the four distances [B,N,4] instead).
    ``mutation``: one of MUTATIONS -- proj[i + 1] on side 2; the sum over bins - 1 bins; the bins of sides 1 and 2 swapped; the
    maximum not subtracted; the corner offset 4 * bins - 1; the distances rotated by one side at the last pixel of every level."""
    f = np.float32
    z = z64.numpy().astype(f)
    assert np.array_equal(z.astype(np.float64), z64.numpy())
    proj = np.concatenate([proj64.numpy(), [0.0]]).astype(f)
    d = np.zeros((B, N, 4), f)
    with np.errstate(all='ignore'):
        for k in range(4):
            src = {1: 2, 2: 1}.get(k, k) if mutation == 'swap_sides' else k
            zk = z[..., src * bins:(src + 1) * bins]
            m = zk[..., 0].copy()
            for i in range(1, bins):
                m = np.maximum(m, zk[..., i])
            if mutation == 'no_max':
                m = np.zeros_like(m)
            s = np.zeros_like(m)
            for i in range(bins - 1 if mutation == 'sum_short' else bins):
                s = s + np.exp(zk[..., i] - m)
            acc = np.zeros_like(m)
            for i in range(bins):
                pi = proj[i + 1] if (mutation == 'proj_shift' and k == 2) else proj[i]
                acc = acc + (np.exp(zk[..., i] - m) / s) * pi
            d[..., k] = acc
        if want_dist:
            return torch.from_numpy(d)
        if mutation == 'quad_rotate':
            last = [o - 1 for o in LEVEL_OFF[1:]]
            d[:, last] = np.roll(d[:, last], -1, axis=-1)
        off = 4 * bins - (1 if mutation == 'corner_offset' else 0)
        cz = z[..., off:off + 8]
        pts, st = _anchors()
        ax, ay, sp = pts[:, 0].numpy().astype(f), pts[:, 1].numpy().astype(f), st[:, 0].numpy().astype(f)
        x1, y1, x2, y2 = ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]
        cor = []
        for k in range(4):
            cx_, cy_ = cz[..., 2 * k], cz[..., 2 * k + 1]
            cor += [(ax - cx_ if k < 2 else ax + cx_) * sp, (ay - cy_ if k in (0, 3) else ay + cy_) * sp]
        cx, cy, bw, bh = ((x1 + x2) / f(2)) * sp, ((y1 + y2) / f(2)) * sp, (x2 - x1) * sp, (y2 - y1) * sp
        pred = np.stack([cx, cy, bw, bh, np.ones_like(cx)] + cor, -1)
        rows = np.stack([cx - bw / f(2), cy - bh / f(2), cx + bw / f(2), cy + bh / f(2)] + cor, -1)
    assert pred.dtype == f and rows.dtype == f
    return torch.from_numpy(pred), torch.from_numpy(rows)


def _log(line):
    import os
    with open(os.path.join(X.log_dir(), 'parity.log'), 'a') as fh:
        fh.write(line + '\n')


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_emulation_passes_and_every_mutation_fails_both_regimes(case):
    """The data conditions of both regimes (asserted while the cases are built), the un-mutated emulation against both checks, and
    each of the six mutations against both: it must change bits of the coded regime AND leave the rounding regime's bound (or, for
    the corner offset, which no box column sees, its bit-exact corner columns) with both proj arrays.  The emulation's own error /
    bound ratio is logged: the calibration the GPU's ratio is read against."""
    bins, dtype, widths = case
    coded, soft = coded_case(bins, dtype, widths), soft_case(bins, dtype, widths)
    assert coded_mismatches(*emulate(coded['z'], coded['proj'], bins), coded) == 0
    for ref in soft['refs']:
        worst, bad = soft_check(*emulate(soft['z'], ref['proj'], bins), ref)
        assert worst <= 1.0 and bad == 0, (worst, bad)
        d_err = (emulate(soft['z'], ref['proj'], bins, want_dist=True).double() - ref['dist']).abs()
        d_units = float((d_err / (2.0 ** -24 * ref['dist_mag'].clamp(min=1e-30))).max())
        assert d_units <= 1.1 * (4 * X.DFL_EXP_ULPS + 2 * bins)
        _log('head-dfl cpu-emulation %-24s proj %-8s box err/bound %.3f  distance err %.2f u mag (bound %.1f, max mag %.1f)  soft share %.2f  ties %.2f'
             % (case_id(case), 'linspace' if ref is soft['refs'][0] else 'coded', worst, d_units, 1.1 * (4 * X.DFL_EXP_ULPS + 2 * bins),
                ref['mag'], ref['soft_share'], coded['ties']))
    for mut in MUTATIONS:
        assert coded_mismatches(*emulate(coded['z'], coded['proj'], bins, mut), coded) > 0, mut
        for ref in soft['refs']:
            worst, bad = soft_check(*emulate(soft['z'], ref['proj'], bins, mut), ref)
            if mut == 'corner_offset':
                assert bad > 0, mut
            else:
                assert worst > 1.0, (mut, worst)


def test_cases_cover_what_the_issue_asks():
    """Every bin count meets every storage type, every width set meets 17 bins, and the 320-channel set stays with the 16-bit types."""
    for bins in BINS:
        assert {c[1] for c in CASES if c[0] == bins} == {F16, BF16, F32}
    assert {c[2] for c in CASES if c[0] == 17} == {W_A, W_B, W_C}
    assert all(c[1] != F32 for c in CASES if c[2] == W_C)
    assert LEVEL_OFF[-1] == N == 315


def test_bound_is_the_derived_one():
    """dfl_box_bounds on a hand-computed element: 17 bins, anchor (0.5, 0.5) of stride 8, all four distances 4 with magnitude 4."""
    u = 2.0 ** -24
    pts, st = torch.tensor([[0.5, 0.5]], dtype=torch.float64), torch.tensor([[8.0]], dtype=torch.float64)
    d = torch.full((1, 4), 4.0, dtype=torch.float64)
    bp, br = X.dfl_box_bounds(d, d, pts, st, 17)
    ed = 1.1 * (4 * X.DFL_EXP_ULPS + 34) * u * 4.0
    e1, e2 = ed + u * (3.5 + ed), ed + u * (4.5 + ed)                         # x1 = -3.5, x2 = 4.5
    es, ew = e1 + e2 + u * (1.0 + e1 + e2), e1 + e2 + u * (8.0 + e1 + e2)     # x1 + x2 = 1, x2 - x1 = 8
    assert abs(float(bp[0, 0]) - es / 2 * 8) < 1e-18 and abs(float(bp[0, 2]) - ew * 8) < 1e-18
    e_row = (es / 2 + ew / 2) * 8
    assert abs(float(br[0, 0]) - (e_row + u * (28.0 + e_row))) < 1e-18        # cx - bw / 2 = 4 - 32
    assert abs(float(br[0, 2]) - (e_row + u * (36.0 + e_row))) < 1e-18


def test_add_head_box_refuses_bad_bin_arguments_on_a_cpu_engine():
    """The two argument checks need no device: 31 bins (132 outputs, past the 128-cout tile) and DFL without proj are refused, 30 bins
    and 2 bins with a proj are taken."""
    from yolov6.hip import abi
    from yolov6.hip.runtime import Engine, _f32
    eng = Engine(F16, 'cpu')
    f = eng.tensor(64, 3)
    add = lambda bins, proj: eng.lib.lp_engine_add_head_box(eng.h, f, 0, bins, eng._ptr(_f32(torch.zeros(4 * bins + 8, 64))),
                                                            eng._ptr(_f32(torch.zeros(4 * bins + 8))), proj)
    with pytest.raises(RuntimeError, match='reg_bins'):
        abi.check(add(31, eng._ptr(_f32(model_proj(31)))))
    with pytest.raises(RuntimeError, match='proj'):
        abi.check(add(17, None))
    abi.check(add(30, eng._ptr(_f32(model_proj(30)))))
    abi.check(add(2, eng._ptr(_f32(model_proj(2)))))
