"""Shared helpers of the test-suite (own code; nothing here comes from the reference)."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SEG = (13, 44, 68, 105, 142, 179, 216, 253, 290)


def synth_pred(B, N, seed, frac_hot=0.2, obj_one=True, extent=560.0):
    """Random [B,N,290] head output: clustered boxes (IoUs straddle the threshold) and sparse high scores.
    Same construction as tests/golden/make_golden.py::synth_pred."""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(B, N, 290, generator=g) * 0.2
    centers = torch.rand(B, N // 8 + 1, 2, generator=g) * extent + 40
    cxy = centers[:, torch.arange(N) % (N // 8 + 1)] + torch.randn(B, N, 2, generator=g) * 6
    wh = torch.rand(B, N, 2, generator=g) * 60 + 30
    p[..., 0:2], p[..., 2:4] = cxy, wh
    p[..., 4] = 1.0 if obj_one else torch.rand(B, N, generator=g) * 0.5 + 0.5
    p[..., 5:13] = cxy.repeat(1, 1, 4) + torch.randn(B, N, 8, generator=g) * 20
    hot = torch.rand(B, N, generator=g) < frac_hot
    for a, b in zip(SEG[:-1], SEG[1:]):
        cls = torch.randint(0, b - a, (B, N), generator=g)
        val = torch.rand(B, N, generator=g) * 0.7 + 0.3
        cur = p[..., a:b]
        cur.scatter_(2, cls[..., None], torch.where(hot, val, cur.gather(2, cls[..., None])[..., 0])[..., None])
    return p.half().float()


def nhwc(t, cs=None):
    """NCHW torch tensor -> NHWC with channels zero-padded to ``cs``."""
    t = t.permute(0, 2, 3, 1).contiguous()
    if cs is not None and cs != t.shape[-1]:
        t = torch.nn.functional.pad(t, (0, cs - t.shape[-1]))
    return t


def rel_err(a, b):
    """max |a-b| / max(1, max|b|)"""
    return float((a.double() - b.double()).abs().max() / max(1.0, float(b.double().abs().max())))


def unpack_lists(z, prefix, width):
    """Inverse of tests/golden/make_golden_metric.py::pack: per batch, per image float32 tensors [n, width]."""
    rows, lens, batch = z[prefix + '_rows'], z[prefix + '_len'].tolist(), z[prefix + '_batch'].tolist()
    out, o, i = [], 0, 0
    for b in batch:
        cur = []
        for _ in range(b):
            cur.append(rows[o:o + lens[i]].reshape(-1, width).float().clone())
            o += lens[i]
            i += 1
        out.append(cur)
    return out


def synth_metric_batch(seed, B, max_pred, max_tgt, hw=640.0):
    """Seeded detections [n,28] / labels [m,20] per image with IoUs spread over the metric's bins (same recipe as the
    golden generator, kept separate on purpose)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    pb, tb = [], []
    for _ in range(B):
        n = 0 if r(1).item() < 0.1 else int(torch.randint(1, max_pred + 1, (1,), generator=g))
        m = 0 if r(1).item() < 0.1 else int(torch.randint(1, max_tgt + 1, (1,), generator=g))
        cxy, wh = r(n, 2) * (hw - 120) + 60, r(n, 2) * 80 + 20
        box = torch.cat([cxy - wh / 2, cxy + wh / 2], 1)
        cor = torch.cat([box[:, :2], box[:, 2:3], box[:, 1:2], box[:, 2:], box[:, 0:1], box[:, 3:4]], 1) + (r(n, 8) - 0.5) * 4
        cls = torch.randint(0, 24, (n, 8), generator=g).float()
        pred = torch.cat([box, cor, r(n, 8), cls], 1)
        if n > 0 and m > 0:
            src = torch.randint(0, n, (m,), generator=g)
            tbox = box[src] + (r(m, 4) - 0.5) * wh[src].repeat(1, 2) * r(m, 1) * 0.9
            tcor = cor[src] + (r(m, 8) - 0.5) * wh[src].mean(1, keepdim=True) * r(m, 1) * 0.5
            tcls = cls[src].clone()
            flip = r(m) < 0.3
            tcls[flip, 0] = (tcls[flip, 0] + 1) % 24
            tgt = torch.cat([tcls, tbox, tcor], 1)
        else:
            tgt = torch.cat([torch.randint(0, 24, (m, 8), generator=g).float(), r(m, 2) * 300, r(m, 2) * 300 + 320, r(m, 8) * hw], 1)
        pb.append(pred.float())
        tb.append(tgt.float())
    return pb, tb


# ---- exact-arithmetic helpers (tests/test_exact_cpu.py, tests/test_exact_gpu.py) ---------------------------------------
# Grid data: every tensor holds multiples of a power of two.  Products x*w are multiples of step_x*step_w (the "grid unit"),
# and as long as sum|x||w| + |b| stays below 2^24 units every product and every partial sum, in ANY order, is an integer
# number of units below 2^24, i.e. exact in fp32.  The result of a convolution then does not depend on the summation order
# and its bits are known: the float64 sum, converted to float32 (exact) and rounded ONCE to the storage type.
SIG_BITS = {torch.float16: 11, torch.bfloat16: 8, torch.float32: 24}
MIN_EXP = {torch.float16: -14, torch.bfloat16: -126, torch.float32: -126}
INT_VIEW = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
RES_ALPHA = 0.75                 # residual weight of the exact tests: a multiple of 1/4, so alpha * res stays on the grid
# value ranges of the grid data per storage type: (|x|, |w| bound, |bias| bound, |residual| bound).  x, w and the residual are
# multiples of 1/4 that the 16-bit type holds exactly; the bias (fp32 in the engine) is a multiple of 1/16 and sets the scale of
# the outputs so that they need rounding: outputs are multiples of 1/16, fp16 cannot hold those from |v| >= 128, bf16 from 16.
GRID_RANGE = {torch.float16: (4.0, 1024.0, 256.0), torch.bfloat16: (4.0, 128.0, 32.0), torch.float32: (4.0, 1024.0, 256.0)}


def grid_rand(shape, seed, lo=-4.0, hi=4.0, step=0.25, device='cpu'):
    """Seeded float64 tensor of multiples of ``step`` (a power of two) drawn uniformly from [lo, hi] (``device``: where it is
    drawn and kept; the sequence of a seed differs between devices, each is reproducible)."""
    m, _ = np.frexp(step)
    assert m == 0.5 and lo <= hi, 'step must be a power of two'
    g = torch.Generator(device).manual_seed(seed)
    return torch.randint(int(round(lo / step)), int(round(hi / step)) + 1, tuple(shape), generator=g, device=device).double() * step


def grid_inputs(cins, cout, k, B, h, w, dtype, res_hw=None, seed=0, wshape=None, device='cpu'):
    """Grid-valued activations (one per source), weights, bias and residual (or None) of one layer for storage type ``dtype``."""
    xw, bb, rb = GRID_RANGE[dtype]
    xs = [grid_rand((B, c, h, w), seed + 10 + i, -xw, xw, device=device) for i, c in enumerate(cins)]
    wt = grid_rand(wshape or (cout, sum(cins), k, k), seed + 1, -xw, xw)
    bias = grid_rand((cout,), seed + 2, -bb / 4, bb, 1.0 / 16)       # mostly positive: ReLU leaves four outputs of five
    res = grid_rand((B, cout) + tuple(res_hw), seed + 20, -rb, rb, device=device) if res_hw else None
    return xs, wt, bias, res


def assert_grid_exact(xs, wt, bias, dtype, unit=1.0 / 16, fan_in=None):
    """The conditions ON THE INPUTS under which the result is independent of the summation order: everything on its grid and
    held exactly by the storage type, and fan_in * max|x| * max|w| + max|b| (an upper bound of sum|x||w| + |b|) below 2^24
    grid units."""
    for t in list(xs) + [wt]:
        assert torch.equal(t.to(dtype).double(), t), 'the storage type does not hold the grid values'
    assert torch.equal(bias.float().double(), bias)
    fan_in = fan_in or wt[0].numel()
    bound = fan_in * max(float(x.abs().max()) for x in xs) * float(wt.abs().max()) + float(bias.abs().max())
    assert bound < 2 ** 24 * unit, bound
    for t in list(xs) + [wt]:
        assert torch.equal(torch.round(t * 4) / 4, t)              # x * w: multiples of 1/16
    assert unit <= 1.0 / 16 and torch.equal(torch.round(bias / unit) * unit, bias)


def to_exact_f32(t64):
    """float64 -> float32, asserting that nothing is rounded (the value was an exact fp32 sum)."""
    t32 = t64.float()
    assert torch.equal(t32.double(), t64), 'the float64 reference is not an fp32 value: the data left the exact regime'
    return t32


def exact_epilogue(pre64, act, dtype, res64=None, alpha=RES_ALPHA):
    """Expected bits for a pre-activation float64 sum on grid data: activation (none / relu), ONE round-to-nearest-even step
    to the storage type, then the residual epilogue from_f32<T>(to_f32(T(act)) + alpha * to_f32(res)) -- an exact fp32 sum
    of grid values rounded once more."""
    assert act in ('none', 'relu')
    v = torch.where(pre64 > 0, pre64, torch.zeros_like(pre64)) if act == 'relu' else pre64
    y = to_exact_f32(v).to(dtype)
    if res64 is not None:
        assert torch.equal(res64.to(dtype).double(), res64)
        y = to_exact_f32(y.double() + alpha * res64).to(dtype)
    return y


def exact_conv(xs, wt, bias, k, s, act, dtype, res64=None, alpha=RES_ALPHA):
    """(expected tensor in ``dtype``, float64 values before the activation and the rounding) of a grid-valued conv layer."""
    pre = torch.nn.functional.conv2d(torch.cat(xs, 1), wt, bias, stride=s, padding=k // 2)
    return exact_epilogue(pre, act, dtype, res64, alpha), pre


# ---- non-finite values (tests/test_nonfinite_cpu.py, tests/test_nonfinite_gpu.py) ------------------------------------------------
# The reference (oracle/lp_oracle.py: F.conv2d, F.relu, F.silu, F.max_pool2d, softmax) is plain IEEE 754 arithmetic: a NaN operand
# gives NaN, inf * 0 gives NaN, +inf + -inf gives NaN.  None of that depends on the order of a sum, so on grid data with a few planted
# NaN / +-inf the expected tensor is still known bit for bit at every finite element and by class at every other.
NONFINITE = {'nan': float('nan'), '+inf': float('inf'), '-inf': float('-inf')}


def plant_nonfinite(t, plan):
    """A copy of the grid-valued float64 tensor ``t`` with NaN / +inf / -inf written at named positions: ``plan`` is a list of
    (kind, index) with kind in NONFINITE and index what ``t[index] = value`` takes (integers and slices).  The rest stays on the grid."""
    assert t.dtype == torch.float64
    out = t.clone()
    for kind, idx in plan:
        out[idx] = NONFINITE[kind]
    return out


def nonfinite_counts(t):
    """{'nan', '+inf', '-inf', 'finite'} -> number of elements of ``t``."""
    v = t.double()
    n, p, m = int(torch.isnan(v).sum()), int((v == NONFINITE['+inf']).sum()), int((v == NONFINITE['-inf']).sum())
    return {'nan': n, '+inf': p, '-inf': m, 'finite': v.numel() - n - p - m}


def conv_nonfinite_ref(xs, wt, bias, k, s, transposed=False, skip=None, terms=False):
    """Pre-activation sum of a conv layer on data that holds NaN / +-inf, as an explicit float64 product-then-sum over unfolded
    patches with zero padding, (patches * w).sum(...): IEEE arithmetic with nothing skipped -- a padding tap under an infinite weight
    is inf * 0 = NaN, a zero weight over a NaN is NaN.  The class of a sum (NaN / +inf / -inf / finite) does not depend on its order,
    and grid data cannot overflow, so this is the authority; F.conv2d in float64 must show the same NaN / +inf / -inf masks (asserted:
    a BLAS that skips zero operands would not).  ``transposed``: the 2x2 stride-2 transposed conv (wt [cin, cout, 2, 2]).
    ``skip`` restates a WRONG convolution for the mutant checks: 'zero_weights' drops the terms whose weight is 0, 'padding' the taps
    that fall outside the image.  A boolean tensor shaped like ``wt`` drops exactly the marked terms: a kernel that by design does not
    run some all-zero taps (the fused stem).  ``terms=True`` also returns, per output, the numbers of NaN, +inf and -inf terms of its sum."""
    import torch.nn.functional as F
    x = torch.cat(list(xs), 1)
    B, cin = x.shape[:2]
    if transposed:
        cout = wt.shape[1]
        pat = x.reshape(B, cin, 1, -1)                                           # one term per input channel and output phase
        wm = wt.permute(1, 2, 3, 0).reshape(cout * 4, cin)                       # [(co, dy, dx), cin]
        inside = torch.ones(1, cin, x.shape[2] * x.shape[3], dtype=torch.bool)
    else:
        cout = wt.shape[0]
        pat = F.unfold(x, k, padding=k // 2, stride=s).reshape(B, cin * k * k, -1)
        wm = wt.reshape(cout, cin * k * k)
        inside = F.unfold(torch.ones(1, cin, x.shape[2], x.shape[3], dtype=torch.float64), k, padding=k // 2, stride=s) > 0
    pat = pat.reshape(B, 1, wm.shape[1], -1)
    rows = wm.shape[0]
    out = torch.empty(B, rows, pat.shape[-1], dtype=torch.float64)
    cnt = torch.zeros(3, B, rows, pat.shape[-1], dtype=torch.int32) if terms else None
    step = max(1, int(3e7 // (B * wm.shape[1] * pat.shape[-1])))                # bounds the product tensor at ~240 MB
    for r0 in range(0, rows, step):
        wv = wm[r0:r0 + step].reshape(1, -1, wm.shape[1], 1)
        prod = pat * wv
        if skip == 'zero_weights':
            prod = torch.where(wv == 0, torch.zeros_like(prod), prod)
        elif skip == 'padding':
            prod = torch.where(inside.reshape(1, 1, wm.shape[1], -1), prod, torch.zeros_like(prod))
        elif torch.is_tensor(skip):
            prod = torch.where(skip.reshape(wm.shape)[r0:r0 + step].reshape(1, -1, wm.shape[1], 1), torch.zeros_like(prod), prod)
        else:
            assert skip is None
        out[:, r0:r0 + step] = prod.sum(2)
        if terms:
            cnt[0, :, r0:r0 + step] = torch.isnan(prod).sum(2)
            cnt[1, :, r0:r0 + step] = (prod == NONFINITE['+inf']).sum(2)
            cnt[2, :, r0:r0 + step] = (prod == NONFINITE['-inf']).sum(2)
    if transposed:
        h, w = x.shape[2:]

        def shape(t):                                                            # [..., (co, dy, dx), (y, x)] -> [..., co, 2y + dy, 2x + dx]
            lead, n = tuple(t.shape[:-2]), t.dim() - 2
            t = t.reshape(lead + (cout, 2, 2, h, w)).permute(list(range(n)) + [n, n + 3, n + 1, n + 4, n + 2])
            return t.reshape(lead + (cout, 2 * h, 2 * w))
        lib = F.conv_transpose2d(x, wt, None, stride=2)
    else:
        ho, wo = (x.shape[2] + 2 * (k // 2) - k) // s + 1, (x.shape[3] + 2 * (k // 2) - k) // s + 1
        shape = lambda t: t.reshape(t.shape[:-1] + (ho, wo))
        lib = F.conv2d(x, wt, None, stride=s, padding=k // 2)
    out = shape(out)
    if skip is None:
        for kind in ('+inf', '-inf'):
            assert torch.equal(lib == NONFINITE[kind], out == NONFINITE[kind]), 'F.conv2d and the explicit product sum differ in ' + kind
        assert torch.equal(torch.isnan(lib), torch.isnan(out)), 'F.conv2d and the explicit product sum differ in their NaN masks'
        fin = torch.isfinite(out)
        assert torch.equal(lib[fin], out[fin]), 'F.conv2d and the explicit product sum differ at finite elements of grid data'
    out = out + bias.view(1, -1, 1, 1)
    return (out, shape(cnt)) if terms else out


def nonfinite_epilogue(pre64, act, dtype, res64=None, alpha=RES_ALPHA, relu=None, res_first=False):
    """``exact_epilogue`` with the reference's semantics for NaN and infinities: relu maps NaN to NaN, -inf to +0 and +inf to +inf
    (torch.relu), ONE rounding to the storage type, then from_f32<T>(to_f32(T(act)) + alpha * res) in IEEE arithmetic -- +inf in
    the activation and -inf in the residual give NaN.  Finite values must still be exact fp32 sums.  ``relu`` / ``res_first``
    restate WRONG epilogues for the mutant checks: relu='select' is v > 0 ? v : 0, res_first adds the residual in front of the
    rounding."""
    assert act in ('none', 'relu')

    def exact32(v64):
        fin = torch.isfinite(v64)
        v32 = v64.float()
        assert torch.equal(v32.double()[fin], v64[fin]), 'the float64 reference is not an fp32 value: the data left the exact regime'
        return v32

    v = pre64
    if act == 'relu':
        sel = torch.where(pre64 > 0, pre64, torch.zeros_like(pre64))
        v = sel if relu == 'select' else torch.where(torch.isnan(pre64), pre64, sel)      # (= torch.relu: test_nonfinite_cpu.py)
    if res64 is not None and res_first:
        return exact32(v + alpha * res64).to(dtype)
    y = exact32(v).to(dtype)
    if res64 is not None:
        fin = torch.isfinite(res64)
        assert torch.equal(res64.to(dtype).double()[fin], res64[fin])
        y = exact32(y.double() + alpha * res64).to(dtype)
    return y


def same_nonfinite_mismatches(got, want):
    """0-d integer tensors (on the device of ``got``) for assert_same_nonfinite: elements whose NaN-ness differs, and non-NaN
    elements whose bits differ (infinities with their sign; zeros of either sign equal, as in bit_mismatch_count)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    iv = torch.int64 if got.dtype == torch.float64 else INT_VIEW[got.dtype]
    g, w = got.contiguous(), want.to(got.device).contiguous()
    gn, wn = torch.isnan(g), torch.isnan(w)
    same = (g.view(iv) == w.view(iv)) | ((g == 0) & (w == 0))
    return (gn != wn).sum(), (~gn & ~wn & ~same).sum()


def assert_same_nonfinite(got, want, what=''):
    """``got`` (a tensor of a storage type, any device) against the expected tensor of the same type: NaN exactly where ``want`` is
    NaN (payload and sign free), +inf and -inf equal with their sign, equal bits at every finite element (+0.0 == -0.0, as the exact
    tests treat it).  The message counts each class on both sides."""
    nan_bad, bit_bad = same_nonfinite_mismatches(got, want)
    if int(nan_bad) or int(bit_bad):
        g, w = got.cpu().double(), want.cpu().double()
        gn, wn = torch.isnan(g), torch.isnan(w)
        lost, extra = wn & ~gn, gn & ~wn
        inf_bad = ~gn & ~wn & (torch.isinf(g) | torch.isinf(w)) & (g != w)
        fin_bad = torch.isfinite(g) & torch.isfinite(w) & (g != w)
        first = torch.nonzero(lost | extra | inf_bad | fin_bad)[:4].tolist()
        raise AssertionError('%s: NaN lost at %d elements (got there: %s), NaN where the reference has none at %d, infinities differ at %d, '
                             'finite bits differ at %d; got %s, want %s; first at %s'
                             % (what, int(lost.sum()), g[lost][:4].tolist(), int(extra.sum()), int(inf_bad.sum()), int(fin_bad.sum()),
                                nonfinite_counts(g), nonfinite_counts(w), first))


EPILOGUES4 = (('none', False), ('relu', False), ('none', True), ('relu', True))
_ALL = slice(None)
# The planted conv cases: layer, map of the SOURCES, B = 2, and where NaN / +inf / -inf go -- per source tensor (``x``) and in the residual
# (``res``), image 1 differently from image 0.  A planted element taints its 3x3 footprint for every output channel (an infinity as
# +inf / -inf by the sign of the weight, as NaN under a zero weight), so a handful per image leaves most outputs finite and still gives
# each class its share; two infinities with overlapping footprints meet in one sum; an infinite residual sits on a pixel whose
# activation is infinite too.  test_nonfinite_cpu.py asserts all of that from the reference alone.
NONFINITE_CONV_CASES = {
    # 64 -> 128, 3x3: a corner, edges, the interior pixel (7, 8) -- on the boundary of every tile whose height or width divides 8 -- and
    # channels 15 | 16, the last of one K-chunk and the first of the next (16 channels per chunk in the 16-bit types, 8 in fp32)
    'conv3x3': dict(cins=[64], cout=128, k=3, s=1, h=16, w=16, epilogues=EPILOGUES4,
                    x=[[('nan', (0, 15, 0, 0)), ('+inf', (0, 16, 7, 8)), ('+inf', (0, 40, 7, 9)), ('-inf', (0, 63, 15, 5)),
                        ('nan', (1, 0, 8, 15)), ('+inf', (1, 31, 0, 15)), ('+inf', (1, 32, 4, 4)), ('-inf', (1, 63, 12, 7))]],
                    res=[('nan', (0, slice(5, 9), 3, 12)), ('-inf', (0, _ALL, 6, 7)), ('+inf', (1, slice(0, 64), 12, 7)), ('nan', (1, 100, 0, 0))]),
    # stride 2, 32 x 32 in: a pixel at odd coordinates reaches four outputs, one at even coordinates a single one
    'conv3x3s2': dict(cins=[64], cout=128, k=3, s=2, h=32, w=32, epilogues=EPILOGUES4,
                      x=[[('nan', (0, 15, 1, 1)), ('nan', (0, 3, 31, 17)), ('+inf', (0, 16, 15, 17)), ('+inf', (0, 40, 15, 19)), ('+inf', (0, 5, 21, 5)),
                          ('+inf', (0, 50, 25, 25)), ('-inf', (0, 63, 9, 27)), ('-inf', (0, 7, 27, 11)),
                          ('nan', (1, 0, 17, 31)), ('nan', (1, 20, 5, 9)), ('+inf', (1, 31, 1, 31)), ('+inf', (1, 32, 11, 11)), ('+inf', (1, 33, 21, 21)),
                          ('-inf', (1, 63, 25, 7)), ('-inf', (1, 2, 7, 23)), ('+inf', (1, 9, 30, 0))]],
                      res=[('nan', (0, slice(5, 9), 3, 3)), ('-inf', (0, _ALL, 7, 8)), ('+inf', (1, slice(0, 64), 12, 3)), ('nan', (1, 100, 0, 0))]),
    # the streaming 1x1 kernel over a concat: the last channel of one source and the first of the next
    'stream1x1': dict(cins=[128, 64, 64], cout=64, k=1, s=1, h=16, w=16, epilogues=EPILOGUES4,
                      x=[[('nan', (0, 127, 2, slice(3, 6))), ('nan', (1, 127, 15, slice(13, 16)))],
                         [('+inf', (0, 0, 5, slice(0, 8))), ('-inf', (0, 63, 9, slice(4, 12))), ('+inf', (1, 0, 0, slice(8, 16))), ('-inf', (1, 63, 7, slice(0, 8)))],
                         [('+inf', (0, 0, 9, slice(8, 14))), ('+inf', (1, 63, 12, slice(2, 10)))]],
                      res=[('nan', (0, slice(10, 12), 14, 14)), ('-inf', (0, _ALL, 5, 3)), ('+inf', (1, _ALL, 7, 2)), ('nan', (1, 5, 3, 3))]),
    # the same concat into 128 output channels: the 128-row weight packing, which the wide streaming kernel (WC = 4) needs
    'stream1x1-128': dict(cins=[128, 64, 64], cout=128, k=1, s=1, h=16, w=16, epilogues=EPILOGUES4,
                          x=[[('nan', (0, 127, 2, slice(3, 6))), ('nan', (1, 127, 15, slice(13, 16)))],
                             [('+inf', (0, 0, 5, slice(0, 8))), ('-inf', (0, 63, 9, slice(4, 12))), ('+inf', (1, 0, 0, slice(8, 16))), ('-inf', (1, 63, 7, slice(0, 8)))],
                             [('+inf', (0, 0, 9, slice(8, 14))), ('+inf', (1, 63, 12, slice(2, 10)))]],
                          res=[('nan', (0, slice(10, 12), 14, 14)), ('-inf', (0, _ALL, 5, 3)), ('+inf', (1, _ALL, 7, 2)), ('nan', (1, 5, 3, 3))]),
    # 2x2 stride-2 transposed conv: +inf and -inf in two channels of one pixel meet in every output of that pixel
    'deconv2x2': dict(cins=[16], cout=24, k=2, s=2, h=6, w=6, transposed=True, epilogues=(('none', False),),
                      x=[[('nan', (0, 15, 0, 0)), ('+inf', (0, 0, 2, 3)), ('-inf', (0, 8, 2, 3)), ('+inf', (0, 7, 5, 5)), ('-inf', (0, 3, 3, 0)),
                          ('nan', (1, 0, 5, 2)), ('+inf', (1, 15, 0, 5)), ('+inf', (1, 4, 3, 3)), ('-inf', (1, 9, 4, 0))]], res=None),
    # two sibling layers in one launch (PAIR_CASES' narrow one: 8 + 24 output channels in one 32-row cout tile)
    'pair': dict(cins=[16], cout=32, pair=(8, 24), k=3, s=1, h=12, w=20, epilogues=(('none', False), ('relu', False)),
                 x=[[('nan', (0, 15, 0, 19)), ('+inf', (0, 0, 6, 10)), ('+inf', (0, 8, 6, 11)), ('-inf', (0, 7, 11, 3)),
                     ('nan', (1, 3, 5, 0)), ('+inf', (1, 15, 0, 0)), ('+inf', (1, 1, 9, 15)), ('-inf', (1, 12, 3, 8))]], res=None),
}
_nonfinite_cache = {}


def nonfinite_conv_data(name, dtype):
    """One planted case for storage type ``dtype``: dict of the planted sources ``xs`` and residual ``res``, ``wt``, ``bias``, the float64
    pre-activation ``pre`` (conv_nonfinite_ref), the (NaN, +inf, -inf) term counts of every sum ``terms``, and ``wants``: the expected
    tensor per epilogue of the case.  Activations and weights are the same grid values for every dtype: the product sums are computed
    once per case and never modified."""
    c = NONFINITE_CONV_CASES[name]
    B, tr = 2, bool(c.get('transposed'))
    cin = sum(c['cins'])
    xs, wt, bias, res = grid_inputs(c['cins'], c['cout'], c['k'], B, c['h'], c['w'], dtype, wshape=(cin, c['cout'], 2, 2) if tr else None,
                                    res_hw=(c['h'] // c['s'], c['w'] // c['s']) if c['res'] else None)
    assert_grid_exact(xs, wt, bias, dtype, fan_in=cin if tr else None)
    xs = [plant_nonfinite(x, plan) for x, plan in zip(xs, c['x'])]
    if c['res']:
        res = plant_nonfinite(res, c['res'])
    if name not in _nonfinite_cache:
        _nonfinite_cache[name] = conv_nonfinite_ref(xs, wt, torch.zeros_like(bias), c['k'], c['s'], transposed=tr, terms=True)
    acc, terms = _nonfinite_cache[name]
    pre = acc + bias.view(1, -1, 1, 1)
    wants = {(a, r): nonfinite_epilogue(pre, a, dtype, res if r else None) for a, r in c['epilogues']}
    return dict(case=c, xs=xs, wt=wt, bias=bias, res=res, pre=pre, terms=terms, wants=wants)


def nonfinite_weight_data(dtype):
    """The layer of 'conv3x3' on clean activations with ONE weight +inf, the top-left tap of (cout 5, cin 20): output channel 5 is
    +-inf by the sign of the activation under that tap, NaN where that activation is 0 and -- the point -- NaN along the top row and
    the left column, where the tap lies on the zero padding (inf * 0): a kernel that skipped halo taps would give a number there."""
    c = NONFINITE_CONV_CASES['conv3x3']
    xs, wt, bias, res = grid_inputs(c['cins'], c['cout'], 3, 2, c['h'], c['w'], dtype, res_hw=(c['h'], c['w']))
    assert_grid_exact(xs, wt, bias, dtype)
    wt = plant_nonfinite(wt, [('+inf', (5, 20, 0, 0))])
    if 'weight' not in _nonfinite_cache:
        _nonfinite_cache['weight'] = conv_nonfinite_ref(xs, wt, torch.zeros_like(bias), 3, 1)
    pre = _nonfinite_cache['weight'] + bias.view(1, -1, 1, 1)
    wants = {(a, r): nonfinite_epilogue(pre, a, dtype, res if r else None) for a, r in EPILOGUES4}
    return dict(case=c, xs=xs, wt=wt, bias=bias, res=res, pre=pre, wants=wants)


# ---- the SPPF pool chain on non-finite data --------------------------------------------------------------------------------------
POOL_NONFINITE_SHAPES = [(8, 4, 3, 2), (32, 2, 1, 2), (16, 1, 5, 2), (64, 13, 7, 2), (40, 40, 40, 2),          # (c, h, w, B); the last: 1024 threads
                         (512, 4, 4, 16), (1024, 4, 4, 16), (1024, 4, 4, 32)]                                    # 2, 4 and 8 granules per workgroup
POOL_GP = {(512, 4, 4, 16): 2, (1024, 4, 4, 16): 4, (1024, 4, 4, 32): 8}


def pool_granules(c, h, w, B, esz):
    """Restatement of pool_launch_t's rule (lp_aux.hip): granules (8 channels) per workgroup = the largest of 8, 4, 2 that divides the
    granule count, keeps the two LDS planes within 64 KiB and still gives 512 workgroups; else 1."""
    cs = (c + 7) // 8 * 8
    for cand in (8, 4, 2):
        if (cs // 8) % cand == 0 and h * w * cand * 8 * esz * 2 <= 64 * 1024 and B * (cs // 8 // cand) >= 512:
            return cand
    return 1


def pool_nonfinite_data(c, h, w, B, finite=False):
    """[B, c, h, w] float64 of values every storage type holds (normal deviates rounded to bf16) and, unless ``finite``, in the eight
    channels of granule g = image index (so the images differ): channel 0 a NaN in the middle of the map -- it sits at each of the up to
    25 positions of the windows around it --, channels 1..3 a NaN in the first pixel, in the last pixel and on the middle of the left
    edge (windows clipped by every border), channel 4 one +inf, channel 5 a 7 x 7 (or the whole map's) block of -inf in the top-left
    corner: the windows inside it are all -inf through the three pools."""
    g = torch.Generator().manual_seed(c * 1000 + h * 10 + w)
    x = torch.randn(B, c, h, w, generator=g).to(torch.bfloat16).double()
    if finite:
        return x
    plan = []
    for b in range(B):
        c0 = 8 * (b % (c // 8))
        plan += [('nan', (b, c0, h // 2, w // 2)), ('nan', (b, c0 + 1, 0, 0)), ('nan', (b, c0 + 2, h - 1, w - 1)), ('nan', (b, c0 + 3, h // 2, 0)),
                 ('+inf', (b, c0 + 4, h // 3, w - 1 - w // 3)), ('-inf', (b, c0 + 5, slice(0, 7), slice(0, 7)))]
    return plant_nonfinite(x, plan)


def pool_chain_sep(x, op):
    """The three chained 5x5 stride-1 pools as lp_aux.hip computes them -- a row pass and a column pass over the taps inside the image,
    left to right / top to bottom -- with the two-operand maximum ``op``: 'maximum' (IEEE 754-2019: NaN propagates), 'maxnum' (a NaN
    operand is dropped) or 'select' (c > a ? c : a).  -> [y1, y2, y3]."""
    f = {'maximum': torch.maximum, 'maxnum': torch.fmax, 'select': lambda a, c: torch.where(c > a, c, a)}[op]

    def axis_pass(t, dim):
        n = t.shape[dim]
        out = []
        for i in range(n):
            m = t.select(dim, max(0, i - 2))
            for j in range(max(0, i - 2) + 1, min(n - 1, i + 2) + 1):
                m = f(m, t.select(dim, j))
            out.append(m)
        return torch.stack(out, dim)
    ys = []
    for _ in range(3):
        x = axis_pass(axis_pass(x, 3), 2)
        ys.append(x)
    return ys


def rounding_stats(pre64, act, dtype):
    """Fractions of the pre-rounding outputs (after the activation) that the storage type cannot hold, and that are exact ties."""
    v = (torch.relu(pre64) if act == 'relu' else pre64)
    r = v.float().to(dtype).double()
    inexact = r != v
    u = ulp(v, dtype)
    tie = inexact & ((r - v).abs() * 2 == u)
    return float(inexact.double().mean()), float(tie.double().mean())


def ulp(v64, dtype):
    """Spacing of the storage type at |v| (float64 tensor): 2^(max(floor(log2|v|), emin) - (p - 1))."""
    _, e = torch.frexp(v64.abs())
    e = torch.where(v64 == 0, torch.full_like(e, -10000), e) - 1
    e = e.clamp(min=MIN_EXP[dtype], max=15 if dtype == torch.float16 else 127)
    return torch.ldexp(torch.ones_like(v64), e - (SIG_BITS[dtype] - 1))


def bit_mismatch_count(got, want):
    """0-d integer tensor (on the device of ``got``): number of elements whose bit patterns differ.  Zeros of either sign compare
    equal (the sign of zero has its own test); a NaN is equal only to the identical NaN pattern."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    iv = INT_VIEW[got.dtype]
    g, w = got.contiguous(), want.to(got.device).contiguous()
    same = (g.view(iv) == w.view(iv)) | ((g == 0) & (w == 0))
    return (~same).sum()


def bit_mismatches(got, want):
    return int(bit_mismatch_count(got, want))


def assert_bits(got, want, what=''):
    n = bit_mismatches(got, want)
    if n:
        g, w = got.cpu().double(), want.cpu().double()
        bad = torch.nonzero((g != w) | torch.isnan(g))[:4].tolist()
        raise AssertionError('%s: %d of %d elements differ from the exact reference, max |diff| %g, first at %s'
                             % (what, n, got.numel(), float((g - w).abs().nan_to_num(float('inf')).max()), bad))


def elementwise_bound(ref64, mag64, K, dtype, transcendental=False, slack64=None):
    """The bound of ``elementwise_excess`` per element (float64); ``K`` may be a tensor that broadcasts against ``mag64``."""
    r, m = ref64.double(), mag64.double()
    bound = ulp(r, dtype) + 1.1 * K * 2.0 ** -24 * m
    if transcendental:
        bound = bound + 4 * 2.0 ** -23 * r.abs()
    if slack64 is not None:
        bound = bound + slack64.double()
    return bound


def elementwise_excess(got, ref64, mag64, K, dtype, transcendental=False, slack64=None):
    """max over elements of |got - ref64| / bound, bound = ulp_T(ref64) + 1.1 K 2^-24 mag64 (+ 4 * 2^-23 |ref64|):
    one ulp of the storage type (half an ulp of rounding + a boundary flip), the standard bound K u sum|x||w| of an fp32
    accumulation of K terms in any order (u = 2^-24) times the Lipschitz constant 1.1 of SiLU (1 for none / ReLU: covered), and
    for an epilogue with v_exp_f32, v_rcp_f32 (1 ulp each) and a multiply, 4 * 2^-23 relative.  ``slack64``: a further derived
    absolute term (the residual epilogue rounds the activation to the storage type BEFORE the add: one more ulp_T of it)."""
    g, r = got.cpu().double(), ref64.double()
    bound = elementwise_bound(ref64, mag64, K, dtype, transcendental, slack64)
    ratio = (g - r).abs() / bound
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float('inf')))
    return float(ratio.max()), ratio


def assert_elementwise(got, ref64, mag64, K, dtype, transcendental=False, slack64=None):
    assert got.shape == ref64.shape == mag64.shape, (got.shape, ref64.shape, mag64.shape)
    worst, ratio = elementwise_excess(got, ref64, mag64, K, dtype, transcendental, slack64)
    if not worst <= 1.0:
        i = int(ratio.flatten().argmax())
        idx = np.unravel_index(i, tuple(ratio.shape))
        raise AssertionError('element %s: got %r, reference %r, error / bound = %g (%d of %d elements over the bound)'
                             % (idx, float(got.cpu().double().flatten()[i]), float(ref64.flatten()[i]), worst,
                                int((ratio > 1).sum()), ratio.numel()))


# The precise expf of the device library (the build has no fast-math): its documented maximum error is 1 ulp (HIP's math API
# tables); no copy of that document ships with the toolchain, so the figure is restated here, not read from it.
DFL_EXP_ULPS = 1


def dfl_box_bounds(dist64, mag64, pts64, st64, nb, exp_ulps=DFL_EXP_ULPS):
    """Elementwise bounds of the box columns of a DFL head whose logits are exact fp32 values, derived from the operation count of
    MODE_DECODE's DFL branch; nothing here is measured, and nothing depends on the engine's storage type (everything after the
    logits is fp32).  ``dist64`` [..,N,4]: the float64 distances sum_i p_i proj_i of the four sides, ``mag64`` the same sum over
    |proj_i|, ``pts64`` [N,2] / ``st64`` [N,1] the anchors.  -> (bound of prediction columns 0..3 (cx, cy, w, h), bound of
    candidate-row columns 0..3 (x1, y1, x2, y2)), float64 [..,N,4].

    With u = 2^-24 and E = ``exp_ulps``:
      e_i = expf(z_i - m)     z_i - m is exact; E ulps = 2 E u relative
      s = e_0 + ... (nb - 1 adds)      (2 E + nb - 1) u relative (all terms positive)
      p_i = e_i / s           2 E + (2 E + nb - 1) + 1 = (4 E + nb) u
      p_i * proj_i, then nb - 1 adds of same-signed or mixed terms: + nb u relative to sum p_i |proj_i|
      => |d^ - d| <= 1.1 (4 E + 2 nb) u sum p_i |proj_i|          (1.1: the second-order terms)
    Every fp32 operation of the decode then adds half an ulp of ITS result (<= u |result|, the result being within the incoming
    error of the float64 one) and passes the incoming errors on linearly: c = ax -+ d, s = c1 + c2, w = c2 - c1, and for the
    candidate rows cx -+ bw / 2; / 2 and * stride (a power of two) are exact."""
    u = 2.0 ** -24
    d, mag = dist64.double(), mag64.double()
    a = torch.cat([pts64, pts64], -1).double()
    st = st64.double()
    half_ulp = lambda v, e: u * (v.abs() + e)
    ed = 1.1 * (4 * exp_ulps + 2 * nb) * u * mag
    c = a + d * torch.tensor([-1.0, -1.0, 1.0, 1.0], dtype=torch.float64)           # x1 y1 x2 y2 in grid units
    ec = ed + half_ulp(c, ed)
    e_in = ec[..., :2] + ec[..., 2:]
    s, w = c[..., :2] + c[..., 2:], c[..., 2:] - c[..., :2]
    es, ew = e_in + half_ulp(s, e_in), e_in + half_ulp(w, e_in)
    pred_bound = torch.cat([es / 2, ew], -1) * st
    cxy, wh = s / 2 * st, w * st
    e_row = (es / 2 + ew / 2) * st
    rows_bound = torch.cat([e_row + half_ulp(cxy - wh / 2, e_row), e_row + half_ulp(cxy + wh / 2, e_row)], -1)
    return pred_bound, rows_bound


def bound_excess(got, ref64, bound64):
    """(max over elements of |got - ref64| / bound64, the ratios); a non-finite ``got`` counts as infinitely far."""
    g = got.cpu().double()
    ratio = (g - ref64.double()).abs() / bound64.double()
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float('inf')))
    return float(ratio.max()), ratio


def _trim(B, h, w, cin, cout, k, budget=0.5e9):
    """Batch size of the exact test for a case of the parity tests: as many images as keep the float64 CPU reference under
    ``budget`` multiply-adds (the tile geometry of the block-tiled kernels depends on B: it gets a sweep of its own)."""
    per_image = h * w * cin * cout * k * k
    return max(1, min(B, int(budget // per_image)))


def exact_conv_cases():
    """(id, cins, cout, k, s, h, w, B) of the exact tests: the shapes of the parity tests (CONV_ / PIPE_ / PIPE16_ /
    S2P16_ / RING_CASES of test_hip_kernels.py; the epilogue is the exact tests' own) with the batch trimmed."""
    import test_hip_kernels as T
    out, seen = [], set()

    def add(cins, cout, k, s, res, h, w, B):
        B = _trim(B, h // s, w // s, sum(cins), cout, k)
        key = (tuple(cins), cout, k, s, h, w, B)
        if key not in seen:
            seen.add(key)
            out.append(('%s-%d-k%ds%d-%dx%dx%d' % ('+'.join(map(str, cins)), cout, k, s, B, h, w),) + key)
    for cins, cout, k, s, act, res, h, w, B in T.CONV_CASES:
        add(cins, cout, k, s, res, h, w, B)
    for cins, cout, act, res, h, w, B in T.PIPE_CASES + T.PIPE16_CASES:
        add(cins, cout, 3, 1, res, h, w, B)
    for cins, cout, act, h, w, B in T.S2P16_CASES:
        add(cins, cout, 3, 2, False, h, w, B)
    for cin, cout, h, w, B in T.RING_CASES:
        add([cin], cout, 3, 1, False, h, w, B)
    return out


MODEL_CONFIGS = (('yololpn', 640), ('yololps', 640), ('yolov6m', 1280))     # the benchmark's configurations


def model_layer_signatures(name, size):
    """Distinct conv layers of a model as the engine lowers them (deploy form), found by walking its modules with the engine's
    own graph builder on the CPU: (cins, cout or (cout1, cout2) for a two-destination launch, k, stride, residual, h, w of the
    layer's INPUT map, log2 stride of that map).  The network input's own reader (the stem) is left to the stem tests."""
    import os
    from yolov6.hip import runtime
    from yolov6.utils.synth import build_synthetic

    class Recorder(runtime.Engine):
        def __init__(self):
            self.chan, self.sigs = {}, []
            super().__init__(torch.float16, 'cpu')

        def tensor(self, channels, sl):
            tid = super().tensor(channels, sl)
            self.chan[tid] = int(channels)
            return tid

        def _add_conv(self, srcs, w, b, k, s, act, dst, dst2=-1, res=None, alpha=0.0):
            if srcs != [self.input_id]:
                cout = (self.chan[dst], self.chan[dst2]) if dst2 >= 0 else self.chan[dst]
                sig = (tuple(self.chan[t] for t in srcs), cout, k, s, res is not None, size >> self._sl, size >> self._sl, self._sl)
                if sig not in self.sigs:
                    self.sigs.append(sig)
            super()._add_conv(srcs, w, b, k, s, act, dst, dst2, res, alpha)

        def conv(self, srcs, weight, bias, k, s, act, sl, res=None, alpha=0.0):
            self._sl = sl
            return super().conv(srcs, weight, bias, k, s, act, sl, res, alpha)

        def conv_pair(self, srcs, wb1, wb2, k, s, act, sl):
            self._sl = sl
            return super().conv_pair(srcs, wb1, wb2, k, s, act, sl)

    m = build_synthetic(os.path.join(REPO, 'configs', name + '.py'))
    rec = Recorder()
    with torch.no_grad():
        rec._build(m)
    return rec.sigs


# Layers at the edges of the kernel selection rules (pick_cfg, conv_pipe_fits, op_fam16): 3x3 layers as (id, sources, cout, stride,
# families that take the op besides the generic kernel, family of the default the rule picks at finalize with the production
# settings).  The LDS tables of the kernels decide them: PIPE / PIPE16 hold 1024 biases and 64 K-chunks of 16 stored channels
# (PIPE_MAXC, PIPE_MAXCHUNKS), PIPE16_V 512 and 32, S2P16 512 and 64; PIPE16 wants the 128-row packing and K-chunks a multiple of four.
RULE_ROWS = [
    ('576-128-s1', [576], 128, 1, {'PIPE', 'PIPE16'}, 'PIPE16'),               # 36 chunks: past PIPE16_V's table
    ('1024-128-s1', [1024], 128, 1, {'PIPE', 'PIPE16'}, 'PIPE16'),             # 64 chunks: the chunk table exactly full
    ('512+512-128-s1', [512, 512], 128, 1, {'PIPE', 'PIPE16'}, 'PIPE16'),
    ('1088-128-s1', [1088], 128, 1, set(), 'generic'),                         # 68 chunks: past every chunk table
    ('64-640-s1', [64], 640, 1, {'PIPE', 'PIPE16'}, 'PIPE16'),                 # 5 cout tiles of 128: past PIPE16_V's bias table
    ('64-1024-s1', [64], 1024, 1, {'PIPE', 'PIPE16'}, 'PIPE16'),               # 8 tiles: the bias table exactly full
    ('64-1152-s1', [64], 1152, 1, set(), 'generic'),                           # 9 tiles
    ('64-960-s1', [64], 960, 1, {'PIPE'}, 'generic'),                          # 64-row packing, 15 tiles: PIPE_B only
    ('64-1088-s1', [64], 1088, 1, set(), 'generic'),                           # 64-row packing, 17 tiles
    ('1024-128-s2', [1024], 128, 2, {'S2P16'}, 'generic'),                     # 64 chunks (the stride-2 family is opt-in: not the default)
    ('1088-128-s2', [1088], 128, 2, set(), 'generic'),
    ('64-640-s2', [64], 640, 2, set(), 'generic'),                             # 5 tiles: past S2P16's bias table
]
CONV3_FAMILIES = {'generic', 'PIPE', 'PIPE16', 'PIPE16_V', 'S2P16'}             # kernel families with 3x3 variants a test can ask for


def det_workspace_views(ws, B, N):
    """The detections-only workspace as lp_nms.hip carves it (256-byte aligned pieces): views of the candidate counts [B] int32, the
    sort keys [B][NP] int64 (NP = N rounded up to a power of two, at least 64) and the candidate rows [B][N][28] fp32."""
    off = (ws.data_ptr() + 255) // 256 * 256 - ws.data_ptr()
    cnt = ws[off:][:4 * B].view(torch.int32)
    NP = 1 << max(6, (N - 1).bit_length())
    keys_off = off + (4 * B + 255) // 256 * 256
    keys = ws[keys_off:][:8 * B * NP].view(torch.int64).view(B, NP)
    rows_off = keys_off + (8 * B * NP + 255) // 256 * 256
    rows = ws[rows_off:][:4 * B * N * 28].view(torch.float32).view(B, N, 28)
    return cnt, keys, rows


def ref_images(B, most=3):
    """Images of a batch the float64 reference of the elementwise check is computed for: all of a small batch, else the first,
    the middle and the last one (the kernels still run the whole batch; the max-norm check beside it covers every image)."""
    return list(range(B)) if B <= most else [0, B // 2, B - 1]


def conv_ref64(xs, wt, bias, dtype, stride=1, padding=0, act='none', res=None, alpha=0.0, transposed=False):
    """(ref64, mag64, K, slack64) for assert_elementwise: the layer in float64 on the values the engine stores (activations and
    weights rounded to ``dtype``, fp32 bias), the same operation on absolute values, the number of summed terms, and -- residual
    epilogue, which rounds the activation to the storage type before the add -- that rounding applied to the reference plus one
    ulp of it as slack (a boundary flip of the first rounding)."""
    import torch.nn.functional as F
    q = lambda t: t.to(dtype).double()
    x, w, b = torch.cat([q(t) for t in xs], 1), q(wt), bias.float().double()
    if transposed:
        op, K = (lambda a, c, d: F.conv_transpose2d(a, c, d, stride=stride)), w.shape[0] + 1
    else:
        op, K = (lambda a, c, d: F.conv2d(a, c, d, stride=stride, padding=padding)), w[0].numel() + 1
    pre, mag = op(x, w, b), op(x.abs(), w.abs(), b.abs())
    ref = {'none': lambda v: v, 'relu': torch.relu, 'silu': lambda v: v * torch.sigmoid(v), 'sigmoid': torch.sigmoid}[act](pre)
    slack = None
    if res is not None:
        y1 = ref.float().to(dtype).double()
        slack, ref, mag = ulp(y1, dtype), y1 + alpha * q(res), mag + abs(alpha) * q(res).abs()
    return ref, mag, K, slack


def log_dir():
    """Folder the GPU tests append their logs to (the parity log, the tile log of the exact tests): LP_TEST_LOG_DIR if set, else the
    output folder the repository's .gitignore keeps out of git (its first ``<name>_out/`` entry), else ``test_out`` in the tree."""
    import re
    d = os.environ.get('LP_TEST_LOG_DIR')
    if not d:
        d = os.path.join(REPO, 'test_out')
        try:
            with open(os.path.join(REPO, '.gitignore')) as f:
                for line in f:
                    if re.fullmatch(r'/?\w+_out/', line.strip()):
                        d = os.path.join(REPO, line.strip().strip('/'))
                        break
        except OSError:
            pass
    os.makedirs(d, exist_ok=True)
    return d


# ---- float64 post-processing and its decision margins (tests/test_e2e_cpu.py, tests/test_e2e_gpu.py) ----------------------------
# The steps and the operation order of oracle/lp_post_ref.c (nms.py:68-125) on a float64 prediction.  The reference uses TWO means
# of the eight segment maxima c0..c7: the confidence mask tests (c0+...+c6+c6)/8 (ad4 twice, ad5 omitted), the sort key and the
# greedy step use (c0+...+c7)/8.  Both are restated; "score" below is the sort key, "mask" the masked mean.
MAX_NMS = 30000


def post64_rows(x):
    """One image's float64 prediction [N,290] -> dict of float64 arrays: box [N,4] xyxy, corners [N,8], cf [N,8] segment maxima,
    ci [N,8] first-maximum indices, mask [N] and score [N] (see above).  ``x`` is not modified."""
    x = np.array(x, dtype=np.float64)
    assert x.ndim == 2 and x.shape[1] == SEG[-1]
    x[:, 13:] *= x[:, 4:5]
    box = np.stack([x[:, 0] - x[:, 2] / 2, x[:, 1] - x[:, 3] / 2, x[:, 0] + x[:, 2] / 2, x[:, 1] + x[:, 3] / 2], 1)
    return dict(post64_scores(x[:, 13:]), box=box, corners=x[:, 5:13].copy())


def post64_scores(prob):
    """cf, ci, mask, score of the (obj-multiplied) probability columns [N,277]."""
    cf = np.stack([prob[:, a - 13:b - 13].max(1) for a, b in zip(SEG[:-1], SEG[1:])], 1)
    ci = np.stack([prob[:, a - 13:b - 13].argmax(1) for a, b in zip(SEG[:-1], SEG[1:])], 1)
    c = [cf[:, k] for k in range(8)]
    mask = (c[0] + c[1] + c[2] + c[3] + c[4] + c[5] + c[6] + c[6]) / 8.0
    score = (c[0] + c[1] + c[2] + c[3] + c[4] + c[5] + c[6] + c[7]) / 8.0
    return dict(cf=cf, ci=ci, mask=mask, score=score)


def _conf64(conf_thres):
    return float(np.float32(conf_thres))          # torch casts the python scalar to the tensor's dtype: the engine compares with this


def post64_select(box, mask, score, conf_thres, iou_thres, max_det, max_nms=MAX_NMS):
    """Mask, stable descending sort, max_nms cut, greedy step (strict >, fp64 IoU = inter / (a_i + a_j - inter)), max_det cut.
    -> kept anchor indices in output order (int64)."""
    sel = np.nonzero(mask >= _conf64(conf_thres))[0]
    order = sel[np.argsort(-score[sel], kind='stable')][:max_nms]
    b = box[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    sup = np.zeros(len(order), bool)
    keep = []
    for a in range(len(order)):
        if sup[a]:
            continue
        if len(keep) == max_det:
            break
        keep.append(order[a])
        w = np.maximum(0.0, np.minimum(b[a, 2], b[a + 1:, 2]) - np.maximum(b[a, 0], b[a + 1:, 0]))
        h = np.maximum(0.0, np.minimum(b[a, 3], b[a + 1:, 3]) - np.maximum(b[a, 1], b[a + 1:, 1]))
        inter = w * h
        with np.errstate(divide='ignore', invalid='ignore'):
            sup[a + 1:] |= inter / (area[a] + area[a + 1:] - inter) > float(iou_thres)
    return np.asarray(keep, np.int64)


def nms64(pred, conf_thres, iou_thres, max_det, max_nms=MAX_NMS):
    """float64 restatement of the post-processing for a batch [B,N,290] (float64; not modified):
    (list of [n_i,28] float64 rows, list of kept anchor-index arrays), rows laid out as lp_post_ref.c writes them."""
    out, kept = [], []
    for x in np.asarray(pred, np.float64):
        r = post64_rows(x)
        k = post64_select(r['box'], r['mask'], r['score'], conf_thres, iou_thres, max_det, max_nms)
        out.append(np.concatenate([r['box'][k], r['corners'][k], r['cf'][k], r['ci'][k].astype(np.float64)], 1))
        kept.append(k)
    return out, kept


def iou_bounds(box, delta):
    """Lower and upper bounds [n,n] of the IoU of every pair of xyxy boxes when every corner coordinate may move by <= delta:
    intersection of the boxes grown by delta over the union of the boxes shrunk by delta, and the other way round.  The intersection
    bounds hold for any corner order (an inverted box, x2 < x1, intersects nothing); a pair that CAN intersect and has a box thinner
    than 2 delta on either side (its area may change sign after the move: the formula is then not monotone) gets (-inf, inf)."""
    x1, y1, x2, y2 = (box[:, k] for k in range(4))

    def pair(lo):                       # lo: shrink (+delta on the near corner), else grow
        d = delta if lo else -delta
        a1, b1, a2, b2 = x1 + d, y1 + d, x2 - d, y2 - d
        w = np.maximum(0.0, np.minimum(a2[:, None], a2[None]) - np.maximum(a1[:, None], a1[None]))
        h = np.maximum(0.0, np.minimum(b2[:, None], b2[None]) - np.maximum(b1[:, None], b1[None]))
        return w * h, np.maximum(0.0, a2 - a1) * np.maximum(0.0, b2 - b1)
    i_lo, a_lo = pair(True)
    i_up, a_up = pair(False)
    with np.errstate(divide='ignore', invalid='ignore'):
        den_up = a_lo[:, None] + a_lo[None] - i_up
        up = np.where(i_up == 0, 0.0, np.where(den_up > 0, i_up / den_up, np.inf))
        den_lo = a_up[:, None] + a_up[None] - i_lo
        lo = np.where(i_lo == 0, 0.0, i_lo / den_lo)
    thin = (x2 - x1 <= 2 * delta) | (y2 - y1 <= 2 * delta)
    bad = (thin[:, None] | thin[None]) & (i_up > 0)      # (no possible intersection: the IoU is 0, or 0 / 0 -- never over a threshold)
    return np.where(bad, -np.inf, lo), np.where(bad, np.inf, up)


def decision_margins(pred, conf_thres, iou_thres, max_det, eps_s, eps_p, delta, max_nms=MAX_NMS):
    """Which decisions of the post-processing of ONE image's float64 prediction [N,290] are firm when every probability may move by
    <= eps_p, the masked mean and the score by <= eps_s and every box corner by <= delta.

    Returns a dict: ``keep`` the float64 kept anchors (post64_select), ``ambiguous`` the sorted anchor indices whose fate (kept or
    not) could change, ``nonfirm`` bool [len(keep),8]: class segments of a kept row whose two largest probabilities are within
    2 eps_p (the argmax is not firm there), ``order_ties``: pairs of kept rows that follow each other with scores within 2 eps_s (their
    ORDER in the output is not firm), ``candidates``: number of anchors that pass the mask.

    How: P = anchors that can pass the mask (mask >= conf - eps_s); two anchors are NEAR-scored when their scores are within 2 eps_s,
    i is FIRMLY before j when score_i - score_j > 2 eps_s.  A THREAT of i is another anchor of P, before or near i, whose IoU with
    i can exceed the threshold (upper bound > iou_thres).  To a fixed point:
      sure-kept = firmly passes the mask and every threat of it is dead;  dead = some sure-kept anchor firmly before it has an IoU
      lower bound > iou_thres with it.
    Under any move within the margins a sure-kept anchor is kept (whatever could suppress it is never kept) and a dead one is not
    (its suppressor is kept, stays before it and stays over the threshold); by induction over the fixed-point rounds.  Every other
    anchor of P is ambiguous, and it is so for one of these reasons: its mask value is within eps_s of conf (1); a sure-kept
    anchor firmly before it straddles the IoU threshold with it (2); a near-scored anchor can overlap it (2, 3); a threat of it is
    itself ambiguous (5, the closure).  An anchor within eps_s of conf is reported even when it is dead.  (4) the cuts: with more
    than max_nms anchors in P and the last one in near-scored to the first one out, those near either can fall on either side and are
    treated like (1); with more possible survivors than max_det, the kept rows whose rank can cross the cut are ambiguous."""
    r = post64_rows(pred)
    conf, iou = _conf64(conf_thres), float(iou_thres)
    keep = post64_select(r['box'], r['mask'], r['score'], conf_thres, iou_thres, max_det, max_nms)
    score = r['score']
    P = np.nonzero(r['mask'] >= conf - eps_s)[0]
    P = P[np.argsort(-score[P], kind='stable')]
    unsure = np.abs(r['mask'][P] - conf) <= eps_s                       # (1)
    if len(P) > max_nms:                                                # (4) the max_nms cut
        cut, out = score[P[max_nms - 1]], score[P[max_nms]]            # the last one in, the first one out
        if cut - out <= 2 * eps_s:
            unsure |= (np.abs(score[P] - cut) <= 2 * eps_s) | (np.abs(score[P] - out) <= 2 * eps_s)
        inside = unsure | (np.arange(len(P)) < max_nms)
        P, unsure = P[inside], unsure[inside]
    s = score[P]
    lo, up = iou_bounds(r['box'][P], delta)
    gap = s[:, None] - s[None]                                          # gap[i, j] > 2 eps_s: i firmly before j
    threat = (gap >= -2 * eps_s) & (up > iou) & ~np.eye(len(P), dtype=bool)      # threat[b, i]: b threatens i
    kills = (gap > 2 * eps_s) & (lo > iou)                              # kills[i, j]: i, if kept, surely suppresses j
    sure, dead = np.zeros(len(P), bool), np.zeros(len(P), bool)
    while True:
        new_sure = ~unsure & ~dead & ~(threat & ~dead[:, None]).any(0)
        new_dead = (kills & new_sure[:, None]).any(0)
        if np.array_equal(new_sure, sure) and np.array_equal(new_dead, dead):
            break
        sure, dead = new_sure, new_dead
    amb = (~sure & ~dead) | unsure
    if int((~dead).sum()) > max_det:                                    # (4) the max_det cut: ranks among the survivors
        alive = np.nonzero(~dead)[0]                                    # in score order
        if amb[alive].any():
            first = alive[amb[alive]][0]                                # from the first ambiguous survivor on, no rank is known
            amb[alive[s[alive] <= s[first] + 2 * eps_s]] = True
        elif s[alive[max_det - 1]] - s[alive[max_det]] <= 2 * eps_s:    # all sure: only the order at the cut matters
            amb[alive[np.abs(s[alive] - s[alive[max_det - 1]]) <= 2 * eps_s]] = True
            amb[alive[np.abs(s[alive] - s[alive[max_det]]) <= 2 * eps_s]] = True
    prob = np.array(pred, dtype=np.float64)[keep]
    prob = prob[:, 13:] * prob[:, 4:5]
    nonfirm = np.zeros((len(keep), 8), bool)
    for k, (a, b) in enumerate(zip(SEG[:-1], SEG[1:])):
        top = np.sort(prob[:, a - 13:b - 13], 1)[:, -2:]
        nonfirm[:, k] = top[:, 1] - top[:, 0] <= 2 * eps_p
    ks = score[keep]
    ties = [(int(keep[i]), int(keep[i + 1])) for i in range(len(keep) - 1) if ks[i] - ks[i + 1] <= 2 * eps_s]
    return dict(keep=keep, ambiguous=np.sort(P[amb]), nonfirm=nonfirm, order_ties=ties,
                candidates=int((r['mask'] >= conf).sum()))


# ---- whole-model cases of the end-to-end parity tests ------------------------------------------------------------------------------
# Synthetic weights (build_synthetic's seeded recipe at ``sigma``), input torch.rand(B,3,H,W) of ``seed``: the smallest shapes that
# reach three head levels (four for P6) and more than one tile of the tiled kernels.
E2E_CASES = {
    'yololps': dict(arch='yololps', sigma=0.25, shape=(2, 320, 320), seed=1234),
    'yololpn': dict(arch='yololpn', sigma=0.6, shape=(2, 320, 256), seed=1234),
    'yolov6m': dict(arch='yolov6m', sigma=0.25, shape=(1, 320, 320), seed=1234),          # DFL, BottleRep
    # the P6 case, four head levels: yolov6s6 at its own width (0.5) -- its float64 forward takes under 2 s, no reduction is needed
    'yolov6s6': dict(arch='yolov6s6', sigma=0.25, shape=(1, 320, 256), seed=1234),
}
# Post-processing settings per case: the inference thresholds, and -- where the case meets the input conditions with it (fewer
# candidates than max_det; at the evaluation confidence 0.03 every anchor is a candidate) -- the evaluation IoU and max_det at conf 0.25.
E2E_SETTINGS = {
    'yololps': [(0.4, 0.45, 1000), (0.25, 0.65, 300)], 'yololpn': [(0.4, 0.45, 1000)], 'yolov6m': [(0.4, 0.45, 1000)],
    'yolov6s6': [(0.4, 0.45, 1000), (0.25, 0.65, 300)],
}
# What the float64 oracle and the analyser give for these cases (seed search on the CPU; asserted before an engine is consulted).
# The synthetic models' outputs hardly depend on the input, so the input seed moves these counts by a few rows only; the seed stays
# 1234 everywhere.  Per (case, setting): per image (candidates, kept rows) -- these come from the float64 oracle alone and are asserted.
# Suppressed share = 1 - kept / candidates: yolov6m 93 %, yolov6s6 49 % / 21 % (the two cases that exercise the greedy step), yololpn
# 4 %, yololps 0 % (its synthetic boxes are inverted, x2 < x1: such a box intersects nothing).  Ambiguous anchors: 0 everywhere, and
# still 0 with margins 4 x larger (8 x except yololps' second setting).  Non-firm (row, segment) pairs: 0 of 392 .. 2400.  Pairs of
# kept rows in a near-tie of scores (their ORDER is not firm: they may swap) -- these depend on the margins, i.e. on the fp32 oracle's
# error on the machine at hand, so they are bounded, not pinned: yololps 0 / 4-7 of 305 rows, yololpn 4-5 of 522, the others 0.
E2E_EXPECT = {
    ('yololps', 0): [(49, 49), (49, 49)], ('yololps', 1): [(169, 169), (136, 136)], ('yololpn', 0): [(271, 260), (271, 262)],
    ('yolov6m', 0): [(323, 21)], ('yolov6s6', 0): [(39, 20)], ('yolov6s6', 1): [(68, 54)],
}
E2E_FACTOR = 4.0          # engine error <= 4 x the fp32 oracle's own error against the fp64 oracle (see DESIGN, 4.2)
_e2e_cache = {}


def parity_stats(pred, necks, ref64, necks64):
    """Error figures of a prediction [B,N,290] and its neck maps against the float64 oracle's: max and rms over the coordinate
    columns 0..12 (pixels) and over the probability columns, max relative error (rel_err) of the neck maps (``neck_max``; per map as
    well), and the largest moves of
    the post-processing's inputs: masked mean / score, and box corner (xyxy)."""
    p, r = pred.double(), ref64.double()
    dc, dp = (p - r)[..., :13], (p - r)[..., 13:]
    out = dict(coord_max=float(dc.abs().max()), coord_rms=float(dc.pow(2).mean().sqrt()),
               prob_max=float(dp.abs().max()), prob_rms=float(dp.pow(2).mean().sqrt()))
    for i, (f, rf) in enumerate(zip(necks, necks64)):
        out['neck%d' % i] = rel_err(f.float().cpu(), rf)
    out['neck_max'] = max(out['neck%d' % i] for i in range(len(necks64)))
    s_err = b_err = 0.0
    for a, b in zip(p.numpy(), r.numpy()):
        ra, rb = post64_rows(a), post64_rows(b)
        s_err = max(s_err, float(np.abs(ra['score'] - rb['score']).max()), float(np.abs(ra['mask'] - rb['mask']).max()))
        b_err = max(b_err, float(np.abs(ra['box'] - rb['box']).max()))
    out.update(score_max=s_err, box_max=b_err)
    return out


def e2e_model(key):
    """The case's model on the CPU, unfused (its state dict is what the oracle folds)."""
    from yolov6.utils.synth import build_synthetic
    c = E2E_CASES[key]
    return build_synthetic(os.path.join(REPO, 'configs', c['arch'] + '.py'), sigma=c['sigma']).eval()


def e2e_input(key):
    c = E2E_CASES[key]
    B, H, W = c['shape']
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(c['seed']))


def e2e_reference(key, round_to=None):
    """One case's references, computed once per process and never modified: the float64 oracle (pred64, necks64, backbone64), the
    fp32 oracle of today, ``e_ref`` = parity_stats(fp32 oracle against fp64 oracle): the reference's own error, and the margins of
    the decision analysis eps_p, eps_s, delta = 4 x e_ref's prob_max, score_max, box_max.  With ``round_to`` both are the rounding-
    aware oracle (fp32 accumulation against fp64 between the same 16-bit roundings)."""
    from oracle import lp_oracle
    if (key, round_to) not in _e2e_cache:
        c = E2E_CASES[key]
        sd = e2e_model(key).state_dict()
        a = lp_oracle.arch(c['arch'])
        x = e2e_input(key)
        if round_to is not None:
            x = x.to(round_to)
        p64, n64, b64 = lp_oracle.forward(sd, a, x, return_stages=True, round_to=round_to, precision=torch.float64)
        p32, n32 = lp_oracle.forward(sd, a, x, round_to=round_to)
        e_ref = parity_stats(p32, n32, p64, n64)
        _e2e_cache[(key, round_to)] = dict(
            x=x, pred64=p64, necks64=n64, bb64=b64, pred32=p32, necks32=n32, e_ref=e_ref, eps_p=E2E_FACTOR * e_ref['prob_max'],
            eps_s=E2E_FACTOR * e_ref['score_max'], delta=E2E_FACTOR * e_ref['box_max'])
    return _e2e_cache[(key, round_to)]


def e2e_decisions(key, k):
    """decision_margins of every image of a case at its k-th setting, with the case's own margins (cached with the reference)."""
    r = e2e_reference(key)
    if ('dec', k) not in r:
        conf, iou, max_det = E2E_SETTINGS[key][k]
        r[('dec', k)] = [decision_margins(p, conf, iou, max_det, r['eps_s'], r['eps_p'], r['delta']) for p in r['pred64'].numpy()]
    return r[('dec', k)]


def assert_e2e_inputs(key, k):
    """The conditions on the INPUTS of the kept-set tests, from the float64 oracle alone: no ambiguous anchor, >= 16 kept rows per
    case, fewer candidates than max_det, at most 2 % of the (row, segment) pairs without a firm argmax and at most 5 % of the kept rows
    in a near-tie of scores; and the recorded counts of E2E_EXPECT."""
    dec, exp = e2e_decisions(key, k), E2E_EXPECT[(key, k)]
    max_det = E2E_SETTINGS[key][k][2]
    assert [len(d['ambiguous']) for d in dec] == [0] * len(dec), [d['ambiguous'] for d in dec]
    assert sum(len(d['keep']) for d in dec) >= 16
    assert all(d['candidates'] < max_det for d in dec)
    nonfirm, pairs = sum(int(d['nonfirm'].sum()) for d in dec), sum(d['nonfirm'].size for d in dec)
    ties = sum(len(d['order_ties']) for d in dec)
    assert nonfirm <= 0.02 * pairs and 2 * ties <= 0.05 * sum(len(d['keep']) for d in dec), (nonfirm, pairs, ties)
    got = [(d['candidates'], len(d['keep'])) for d in dec]
    assert got == exp, (got, exp)
    return dec


def tie_runs(keep, order_ties):
    """Positions of ``keep`` split into runs: consecutive rows linked by a near-tie of scores form one run (they may come out in any
    order), every other row is a run of its own.  -> list of (start, stop)."""
    linked = set(order_ties)
    runs, start = [], 0
    for i in range(len(keep)):
        if i + 1 == len(keep) or (int(keep[i]), int(keep[i + 1])) not in linked:
            runs.append((start, i + 1))
            start = i + 1
    return runs


# ---- the bilinear resize by its definition, and the bar of the 8-bit fixed-point scheme against it ------------------------------
# (tests/test_letterbox_cpu.py, tests/test_letterbox_gpu.py)
def _axis64(dst, src, coord=None):
    """Per destination index of one axis: the two neighbours and the weight of the second, in float64.  ``coord(d, src, dst)``
    gives the source coordinate; the default is the definition, pixel centres at half-integers: (d + 0.5) * src / dst - 0.5.
    The coordinate is clamped to [0, src - 1] (replicate border)."""
    d = np.arange(dst, dtype=np.float64)
    c = (d + 0.5) * src / dst - 0.5 if coord is None else coord(d, src, dst)
    c = np.clip(c, 0.0, float(src - 1))
    i0 = np.floor(c).astype(np.int64)
    return i0, np.minimum(i0 + 1, src - 1), c - i0


def bilinear64(im_u8, new_wh, coord=None):
    """uint8 [h, w, C] (or [h, w]) -> float64 [nh, nw, C], unrounded: bilinear interpolation written from its definition (half-pixel
    centres, replicate border, a linear blend of the two neighbours per axis).  No fixed point, no 11-bit weights; nothing of
    ``data_augment`` is used.  ``coord``: another coordinate rule, for the deliberately wrong resizes of the tests."""
    im = np.asarray(im_u8).astype(np.float64)
    if im.ndim == 2:
        im = im[:, :, None]
    h, w = im.shape[:2]
    nw, nh = int(new_wh[0]), int(new_wh[1])
    y0, y1, ty = _axis64(nh, h, coord)
    x0, x1, tx = _axis64(nw, w, coord)
    if nh * w <= h * nw:                                     # the smaller intermediate first; the blend is separable
        rows = im[y0] * (1.0 - ty)[:, None, None] + im[y1] * ty[:, None, None]
        return rows[:, x0] * (1.0 - tx)[None, :, None] + rows[:, x1] * tx[None, :, None]
    cols = im[:, x0] * (1.0 - tx)[None, :, None] + im[:, x1] * tx[None, :, None]
    return cols[y0] * (1.0 - ty)[:, None, None] + cols[y1] * ty[:, None, None]


def linear_u8_bar(src_hw):
    """(lo, hi): the interval that (8-bit fixed-point INTER_LINEAR result) - (float64 bilinear) must stay in, in grey levels, for
    a source of ``src_hw``; derived from the scheme, not measured (the derivation: tests/test_letterbox_cpu.py).
      weights   per axis the second weight is rint(f * 2048) with a0 + a1 = 2048, f the fraction of the float32 coordinate:
                |a1 / 2048 - f_true| <= 0.5 / 2048 + (half a float32 ulp of the coordinate, at most spacing(src) / 2); a blend
                of two values in 0..255 moves by at most 255 times that, and the vertical blend of two such rows adds its own
      >> 4      loses less than 1/128 level in all (the two rows' losses are weighted by b0 + b1 = 2048)
      >> 16     twice, each loses less than 1/4 level
      (+2) >> 2 of an integer number of quarter levels: the result minus the quarter-level value is one of 0, -1/4, +1/4, +1/2"""
    w = sum(255.0 * (0.5 / 2048 + float(np.spacing(np.float32(s))) / 2) for s in src_hw)
    return -(0.25 + 0.5 + 1.0 / 128 + w) - 1e-9, 0.5 + w + 1e-9


# ---- containment: which bytes of a buffer did a run change (tests/test_containment_cpu.py, tests/test_containment_gpu.py) ---------
def merge_intervals(intervals):
    """Sorted union of half-open byte intervals [a, b): empty ones dropped, overlapping and adjacent ones merged."""
    out = []
    for a, b in sorted((int(a), int(b)) for a, b in intervals):
        if b <= a:
            continue
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]


def layout_regions(base, need, total, tensors):
    """Named regions (name, a, b) that tile a buffer of ``total`` bytes holding an arena of ``need`` bytes at offset ``base`` (the
    256-byte aligned start inside the allocation): ``tensors`` = (name, offset in the arena, bytes) back to back, each rounded up to
    256 bytes.  'unaligned head', the tensors, 'slack after <name>' (the rounding), 'behind the tensors' (whatever the arena holds
    behind its last tensor, e.g. a prediction scratch), 'arena tail' (the arena's last 256 bytes) and 'allocation slack'."""
    out = [('unaligned head', 0, base)]
    end = 0
    for name, off, nbytes in sorted(tensors, key=lambda t: t[1]):
        if nbytes == 0:
            continue
        assert off >= end and off % 256 == 0, (name, off, end)
        if off > end:
            out.append(('gap before ' + name, base + end, base + off))
        out.append((name, base + off, base + off + nbytes))
        end = (off + nbytes + 255) // 256 * 256
        out.append(('slack after ' + name, base + off + nbytes, base + end))
    assert end + 256 <= need <= total - base, (end, need, total, base)
    out += [('behind the tensors', base + end, base + need - 256), ('arena tail', base + need - 256, base + need),
            ('allocation slack', base + need, total)]
    return [r for r in out if r[2] > r[1]]


class ByteWatch:
    """Which bytes of a 1-D uint8 buffer changed since a snapshot, outside a set of allowed byte intervals.  The comparison runs on
    the buffer's device; a check that finds nothing costs one synchronisation (the count), one that finds something reads the
    offsets back as well.  ``regions``: (name, a, b) of the buffer, used to say where a changed byte lies."""

    def __init__(self, buf, regions=()):
        assert buf.dtype == torch.uint8 and buf.dim() == 1 and buf.is_contiguous()
        self.buf, self.regions = buf, sorted((str(n), int(a), int(b)) for n, a, b in regions)
        self._masks = {}
        self.snapshot()

    def snapshot(self):
        self.snap = self.buf.clone()

    def _watched(self, allowed):
        key = tuple(merge_intervals((max(0, a), min(self.buf.numel(), b)) for a, b in allowed))
        if key not in self._masks:
            m = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
            for a, b in key:
                m[a:b] = False
            self._masks = {key: m}                       # one mask at a time: a walk repeats the same allowed set
        return self._masks[key]

    def changed(self, allowed):
        """bool [n] on the device: changed and not allowed."""
        return (self.buf != self.snap) & self._watched(allowed)

    def count(self, allowed):
        """0-d tensor on the device (no synchronisation): number of changed bytes outside ``allowed``."""
        return self.changed(allowed).sum()

    def region_of(self, off):
        for name, a, b in self.regions:
            if a <= off < b:
                return name
        return 'unnamed'

    def report(self, allowed):
        """dict: ``count``, ``first``, ``last`` (offsets, None when nothing changed), ``offsets`` (int64 numpy array of every changed
        byte outside ``allowed``) and ``regions``: [(name, count, first, last)] in buffer order."""
        bad = self.changed(allowed)
        n = int(bad.sum())
        if n == 0:
            return dict(count=0, first=None, last=None, offsets=np.zeros(0, np.int64), regions=[])
        offs = torch.nonzero(bad).flatten().cpu().numpy().astype(np.int64)
        per = {}
        for o in offs.tolist():
            name = self.region_of(o)
            c, f, _ = per.get(name, (0, o, o))
            per[name] = (c + 1, f, o)
        return dict(count=n, first=int(offs[0]), last=int(offs[-1]), offsets=offs,
                    regions=[(name,) + per[name] for name in sorted(per, key=lambda k: per[k][1])])

    def assert_contained(self, allowed, what=''):
        r = self.report(allowed)
        if r['count']:
            raise AssertionError('%s: %d byte(s) changed outside the allowed intervals, first at %d, last at %d: %s' % (
                what, r['count'], r['first'], r['last'],
                '; '.join('%s: %d byte(s), offsets %d..%d' % reg for reg in r['regions'])))


def engine_tensor_span(eng, tid):
    """(a, b, view) of engine tensor ``tid`` for the bound shape, from lp_engine_tensor_info: its full stored byte interval
    [a, b) = [off, off + B*h*w*cs*esz) inside ``eng.arena`` (offsets of that uint8 buffer, the aligned base included) and a
    [B,h,w,cs] view that includes the padding channels.  (A network input that the space-to-depth rewrite replaced is not placed:
    its offset is that of the tensor behind it, and the interval means nothing.)"""
    import ctypes
    from yolov6.hip import abi
    off, c, cs, h, w = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    abi.check(eng.lib.lp_engine_tensor_info(eng.h, tid, ctypes.byref(off), ctypes.byref(c), ctypes.byref(cs), ctypes.byref(h),
                                            ctypes.byref(w)), 'lp_engine_tensor_info')
    B = eng.bound[0]
    esz = torch.empty(0, dtype=eng.dtype).element_size()
    a = (eng.arena.data_ptr() + 255) // 256 * 256 - eng.arena.data_ptr() + off.value
    b = a + B * h.value * w.value * cs.value * esz
    return a, b, eng.arena[a:b].view(eng.dtype).view(B, h.value, w.value, cs.value)


def arena_regions(eng, names, placed=None):
    """layout_regions of ``eng.arena`` for the bound shape: ``names`` = {tensor id: name}; ``placed``: ids that lie in the arena
    (default: all of ``names``)."""
    base = (eng.arena.data_ptr() + 255) // 256 * 256 - eng.arena.data_ptr()
    need = eng.lib.lp_engine_arena_bytes(eng.h, *eng.bound)
    tensors = []
    for tid in (names if placed is None else placed):
        a, b, _ = engine_tensor_span(eng, tid)
        tensors.append((names[tid], a - base, b - a))
    return layout_regions(base, need, eng.arena.numel(), tensors)


def spill_case(first_rank, n_orig=6000, n_copy=2000):
    """One crafted image for the greedy step's spilled kept list: ``n_orig`` pairwise disjoint 8 x 8 boxes on a 10-px grid with
    strictly decreasing, distinct scores (row r has rank r), then ``n_copy`` lower-scored copies of the boxes ranked
    first_rank .. first_rank + n_copy - 1, each shifted by 1 px in x: IoU 56 / 72 with its original, disjoint from every other
    box.  obj = 1 and the same single probability in every class segment, a multiple of 2^-14 below 1: the eight-term sums are exact,
    so mask value = score = that probability.  -> (pred float32 [1, n_orig + n_copy, 290], float64 xyxy boxes, scores)."""
    n = n_orig + n_copy
    assert first_rank + n_copy <= n_orig and n < 16000
    r = np.arange(n_orig)
    cx, cy = 10.0 * (r % 100) + 4.0, 10.0 * (r // 100) + 4.0
    src = np.arange(first_rank, first_rank + n_copy)
    cx, cy = np.concatenate([cx, cx[src] + 1.0]), np.concatenate([cy, cy[src]])
    score = (16000.0 - np.arange(n)) / 16384.0
    p = np.zeros((1, n, 290), np.float32)
    p[0, :, 0], p[0, :, 1], p[0, :, 2], p[0, :, 3], p[0, :, 4] = cx, cy, 8.0, 8.0, 1.0
    p[0, :, 5:13] = np.stack([cx - 4, cy - 4, cx + 4, cy - 4, cx + 4, cy + 4, cx - 4, cy + 4], 1)
    for a in SEG[:-1]:
        p[0, :, a + 1] = score
    box = np.stack([cx - 4.0, cy - 4.0, cx + 4.0, cy + 4.0], 1)
    return p, box, score


def assert_spill_preconditions(p, box, score, first_rank, n_orig, n_copy, conf, iou, max_det, cache=4096):
    """What the spilled-list test needs, from the C oracle and float64 geometry alone: the oracle keeps exactly the originals in rank
    order; the only box over the IoU threshold with a copy is its original; returns the kept ranks of those originals."""
    from oracle import lp_post
    rows, keep, _ = lp_post.nms_c(p, conf, iou, max_det)
    assert max_det > cache - 64 and float(score.min()) > conf
    assert np.array_equal(keep[0], np.arange(n_orig)), 'the oracle does not keep exactly the originals in order'
    assert np.all(np.diff(score) < 0)
    c = box[n_orig:]
    w = np.maximum(0.0, np.minimum(c[:, None, 2], box[None, :, 2]) - np.maximum(c[:, None, 0], box[None, :, 0]))
    h = np.maximum(0.0, np.minimum(c[:, None, 3], box[None, :, 3]) - np.maximum(c[:, None, 1], box[None, :, 1]))
    inter = w * h
    over = inter / (64.0 + 64.0 - inter) > iou
    over[np.arange(n_copy), n_orig + np.arange(n_copy)] = False            # a box and itself
    assert np.array_equal(over.sum(1), np.ones(n_copy, np.int64))
    orig = over.argmax(1)
    assert np.array_equal(orig, first_rank + np.arange(n_copy))
    assert np.allclose(inter[np.arange(n_copy), orig], 56.0) and int((inter > 0).sum()) == 2 * n_copy
    return rows, keep, orig                                              # (kept rank of original r is r: the oracle keeps 0..n_orig-1)


# ---- the head's class path on coded logits (tests/test_head_cls_cpu.py, tests/test_head_cls_gpu.py) ---------------------
# Logits whose arg-max, ties and saturation are known from float64 alone.  Six CODE channels carry +-s by the bits of a per-anchor
# code t; column i of head k weighs them +-1 by the bits of its own code perm_k(i) (a seeded draw per head and level), so its logit is
# (6 - 2 d) s, d the Hamming distance of the two codes.  Zeroing code channel j at an anchor ties the columns coded t and
# t ^ (1 << j) exactly.  One OFFSET channel per head (weight 1 on that head's columns only) sets the category of each
# (anchor, head); a few NOISE channels per head (weights +-1/4 and a bias shared by the head's columns: order and ties survive) move
# the head's logits by |n| <= 1.  Every value is an integer or a multiple of 1/16 far below 2^8, so every storage type holds it and
# every sum is exact in fp32.
#   anchors with s = 4:   resolved: the offset that puts the head's largest logit at 11, 7, 3, -1 or -3 (the next one is 8 lower)
#                         +48 all saturated (every logit >= 23), -160 all zero (every logit <= -135)
#   anchors with s = 12:  offset +1: the columns at distance <= 2 are saturated (>= 24), those at distance 3 are at 0 .. 2; the
#                         first saturated column is then rarely the column of the largest logit.  +96 all saturated, -208 all zero.
# Two scales because the rule of admissibility below wants a clear gap in PROBABILITY under every saturated column (s = 4 would put
# a column at logit 12 beneath one at 20), while a resolved head must keep all its logits inside [-88, 12] (s = 12 spans 144).
CLS_B, CLS_MAPS = 3, ((12, 20), (6, 10), (3, 5))
CLS_LEVEL_OFF = (0, 240, 300, 315)
CLS_N = CLS_LEVEL_OFF[-1]
CLS_NC = SEG[-1] - SEG[0]                                  # 277
CLS_HEAD0 = tuple(a - SEG[0] for a in SEG)                 # first class column of each head, and 277
CLS_SAT, CLS_ZERO = 20.0, -128.0                           # logits from which the fp32 sigmoid is exactly 1.0f / +0.0f
CLS_MARGIN = 1e-3
CLS_PLANTED_TILES = {2: 0, 7: 6, 12: 7}                    # 32-row tile of level 0 -> number of its anchors that pass at any threshold
RES, PSAT, ASAT, AZERO = 0, 1, 2, 3
_RES_TOP = np.array([11.0, 7.0, 3.0, -1.0, -3.0])


def _cls_codes(rng):
    """perm_k for the eight heads: distinct 6-bit codes, drawn as whole pairs {2a, 2a + 1} so that the bit-0 partner of a code is
    (nearly) always a column of the same head, in random column order."""
    out = []
    for w in (b - a for a, b in zip(SEG[:-1], SEG[1:])):
        pairs = rng.permutation(32)[:(w + 1) // 2]
        codes = np.concatenate([2 * pairs, 2 * pairs + 1])[:w]
        out.append(rng.permutation(codes))
    return out


def cls_case_data(widths, seed):
    """The coded data of one case.  -> dict: ``levels`` [(x [B,C,h,w], wc [277,C], bc [277])] float64 tensors, ``plan``: the
    categories drawn (numpy, [B,N,8]; nothing asserts them -- every expectation comes from ``cls_reference``)."""
    rng = np.random.RandomState(seed)
    B, N = CLS_B, CLS_N
    codes = [_cls_codes(rng) for _ in CLS_MAPS]                     # [level][head] -> codes of the head's columns
    level_of = np.searchsorted(np.array(CLS_LEVEL_OFF[1:]), np.arange(N), side='right')
    big = np.zeros((B, N), bool)                                    # s = 12 anchors
    t = np.zeros((B, N), np.int64)
    zj = np.full((B, N), -1)                                        # zeroed code channel, or -1
    cat = np.zeros((B, N, 8), np.int64)
    off = np.zeros((B, N, 8))
    free = np.ones((B, N), bool)
    hw0 = CLS_MAPS[0][0] * CLS_MAPS[0][1]

    def set_all(b, n, big_, c, o):
        big[b, n], zj[b, n], cat[b, n], off[b, n], free[b, n] = big_, -1, c, o, False
        t[b, n] = rng.randint(64)
    def res_off(b, n, top):
        """Per head the offset that puts the largest logit of a resolved head of an s = 4 anchor at ``top``."""
        bits = 63 if zj[b, n] < 0 else 63 & ~(1 << zj[b, n])
        dmin = np.array([min(bin((int(c) ^ int(t[b, n])) & bits).count('1') for c in codes[level_of[n]][k]) for k in range(8)])
        return top - 4.0 * (bin(bits).count('1') - 2 * dmin)
    for tile, npass in CLS_PLANTED_TILES.items():                   # planted tiles: (32 - npass) anchors at 0, npass anchors at 1
        for r in range(32):
            b, n = divmod(32 * tile + r, hw0)
            if r < 32 - npass:
                set_all(b, n, True, AZERO, -208.0)
            else:
                set_all(b, n, True, PSAT, 1.0)
    order = [divmod(f, N) for f in rng.permutation(B * N) if free.flat[f]]
    for c, (b, n) in zip(range(CLS_NC), order):                     # one anchor per class column: resolved there, strong elsewhere
        k = int(np.searchsorted(np.array(CLS_HEAD0[1:]), c, side='right'))
        sat = rng.rand(8) < 0.2
        low = rng.choice([h for h in range(7) if h != k])            # (see below: an s = 4 anchor stays clear of mask value 1)
        sat[k] = sat[low] = False
        cat[b, n] = np.where(sat, ASAT, RES)
        t[b, n] = codes[level_of[n]][k][c - CLS_HEAD0[k]]
        top = rng.choice(_RES_TOP[:3], 8)
        top[low] = -1.0
        off[b, n] = np.where(sat, 48.0, res_off(b, n, top))
        off[b, n, k] = rng.choice(_RES_TOP[:2]) - 24.0
        free[b, n] = False
    for b, n in order[CLS_NC:]:
        lv = level_of[n]
        kk = rng.randint(8)
        t[b, n] = rng.choice(codes[lv][kk])
        u = rng.rand(8)
        if rng.rand() < 0.35:
            big[b, n] = True
            cat[b, n] = np.where(u < 0.74, PSAT, np.where(u < 0.90, ASAT, AZERO))
            off[b, n] = np.choose(cat[b, n], [0.0, 1.0, 96.0, -208.0])
        else:
            if rng.rand() < 0.65:
                zj[b, n] = 0 if rng.rand() < 0.6 else rng.randint(1, 6)
            cat[b, n] = np.where(u < 0.70, RES, np.where(u < 0.80, ASAT, AZERO))
            # one of the heads the mask reads is resolved at a logit <= 0: the s = 4 anchors' mask values stay below 15/16, the
            # s = 12 anchors without a zero head are at exactly 1, and the threshold of the 10 % pass rate fits between the two
            low = rng.randint(7)
            cat[b, n, low] = RES
            off[b, n] = np.choose(cat[b, n], [0.0, 0.0, 48.0, -160.0])
            res = cat[b, n] == RES
            top = rng.choice(_RES_TOP, 8)
            top[low] = rng.choice(_RES_TOP[3:])
            off[b, n][res] = res_off(b, n, top)[res]
    levels = []
    for lv, (C, (h, w)) in enumerate(zip(widths, CLS_MAPS)):
        n0, n1 = CLS_LEVEL_OFF[lv], CLS_LEVEL_OFF[lv + 1]
        nchunk = max(1, (C + 31) // 32)                             # 32 channels: the fp32 K-chunk (the 16-bit one is two of them)
        special = [(i % nchunk) * 32 + (i // nchunk) * 2 + 1 for i in range(14)]      # code 0..5, offset 0..7, over all chunks
        assert len(set(special)) == 14 and max(special) < C, special
        noise = np.array([c for c in range(C) if c not in special])
        x = np.zeros((B, n1 - n0, C))
        x[:, :, noise] = rng.randint(-4, 5, (B, n1 - n0, len(noise))) / 4.0
        s = np.where(big[:, n0:n1], 12.0, 4.0)
        for j in range(6):
            bit = (t[:, n0:n1] >> j) & 1
            x[:, :, special[j]] = np.where(zj[:, n0:n1] == j, 0.0, s * (2 * bit - 1))
        wc, bc = np.zeros((CLS_NC, C)), np.zeros(CLS_NC)
        for k in range(8):
            a, e = CLS_HEAD0[k], CLS_HEAD0[k + 1]
            x[:, :, special[6 + k]] = off[:, n0:n1, k]
            wc[a:e, special[6 + k]] = 1.0
            for j in range(6):
                wc[a:e, special[j]] = 2.0 * ((codes[lv][k] >> j) & 1) - 1.0
            wc[a:e, rng.choice(noise, 3, replace=False)] = rng.choice([-0.25, 0.25], 3)
            bc[a:e] = rng.randint(-4, 5) / 16.0
        levels.append((torch.from_numpy(x.reshape(B, h, w, C)).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(wc), torch.from_numpy(bc)))
    return dict(levels=levels, plan=dict(big=big, t=t, zj=zj, cat=cat, off=off))


def cls_logits64(levels):
    """(logits, sum |x||w| + |b|, number of summed terms) of the class predictors in float64: [B,N,277], [B,N,277], [N]."""
    L, M, K = [], [], []
    for x, wc, bc in levels:
        Bn, C = x.shape[:2]
        xf = x.permute(0, 2, 3, 1).reshape(Bn, -1, C)
        L.append(xf @ wc.T + bc)
        M.append(xf.abs() @ wc.abs().T + bc.abs())
        K.append(torch.full((xf.shape[1],), C + 1.0, dtype=torch.float64))
    return torch.cat(L, 1), torch.cat(M, 1), torch.cat(K)


def _head_slices():
    return [slice(a, b) for a, b in zip(CLS_HEAD0[:-1], CLS_HEAD0[1:])]


def cls_reference(levels, dtype):
    """Everything the class-path tests expect, from float64 alone.  Asserts the exactness of the sums (as ``assert_grid_exact``)
    and the rule of ADMISSIBILITY: for every (anchor, head) with largest logit m, every column either ties with m --
      (a) its logit equals m, (b) it and m are >= 20 (both sigmoids are exactly 1.0f), (c) it and m are <= -128 (both exactly +0.0f)
    -- or (d) its float64 sigmoid lies below that of m by at least twice the slack ``elementwise_bound`` grants it (fp32 output,
    transcendental); and no logit lies in (12, 20) or (-128, -88), where the fp32 result depends on the implementation.
    -> dict (numpy): ``logits`` float32 [B,N,277] (exact), ``prob`` float64, ``bound`` the elementwise bound of the probabilities,
    ``ci`` [B,N,8] the expected arg-max (the first tying column), ``cmax`` [B,N,8] the column of the largest logit (its first),
    ``kind`` [B,N,8]: 'S' saturated (1.0f), 'Z' zero (+0.0f), 'V' a value inside the bound, ``ntie`` [B,N,8] the number of tying
    columns, ``tie2`` [B,N,8,2] the two columns of an exact two-way tie (-1 elsewhere), ``best`` float64 [B,N,8] the largest
    sigmoid, ``mask`` float64 [B,N] (ad4 twice)."""
    for x, wc, bc in levels:
        assert_grid_exact([x], wc, bc, dtype, fan_in=wc.shape[1])
    L, M, K = cls_logits64(levels)
    to_exact_f32(L)
    assert not bool(((L > 12) & (L < CLS_SAT)).any()) and not bool(((L > CLS_ZERO) & (L < -88)).any())
    P = torch.sigmoid(L)
    bound = elementwise_bound(P, M, K[None, :, None], torch.float32, transcendental=True)
    n = L.shape[:2]
    ci, cmax, ntie = (np.zeros(n + (8,), np.int64) for _ in range(3))
    kind = np.full(n + (8,), 'V')
    tie2 = np.full(n + (8, 2), -1)
    best = np.zeros(n + (8,))
    for k, sl in enumerate(_head_slices()):
        l, p, bd = L[..., sl], P[..., sl], bound[..., sl]
        m = l.max(-1, keepdim=True).values
        a, b, c = l == m, (l >= CLS_SAT) & (m >= CLS_SAT), (l <= CLS_ZERO) & (m <= CLS_ZERO)
        tie = a | b | c
        d = torch.sigmoid(m) - p >= 2 * bd
        assert bool((tie != d).all()), 'head %d: a column neither ties with the largest logit nor is clear of it' % k
        ci[..., k] = tie.int().argmax(-1).numpy()
        cmax[..., k] = a.int().argmax(-1).numpy()
        ntie[..., k] = tie.sum(-1).numpy()
        kind[..., k] = np.where(m[..., 0].numpy() >= CLS_SAT, 'S', np.where(m[..., 0].numpy() <= CLS_ZERO, 'Z', 'V'))
        two = (a.sum(-1) == 2) & (tie.sum(-1) == 2)
        idx = torch.nonzero(a & two[..., None])                           # rows come in column order: two per tying pair
        tie2[..., k, :][two.numpy()] = idx[:, -1].reshape(-1, 2).numpy()
        best[..., k] = p.max(-1).values.numpy()
    mask = (best[..., :7].sum(-1) + best[..., 6]) / 8.0
    return dict(logits=L.float().numpy(), prob=P.numpy(), bound=bound.numpy(), mag=M.numpy(), K=K.numpy(), ci=ci, cmax=cmax,
                kind=kind, ntie=ntie, tie2=tie2, best=best, mask=mask)


def cls_thresholds(mask):
    """Two confidence thresholds: of the multiples of 2^-12 that no mask value of the reference comes within CLS_MARGIN of, the
    two whose pass rates are nearest 10 % and 60 % (the larger threshold of equally good ones)."""
    v = mask.flatten()
    cands = np.arange(1, 4096) / 4096.0
    cands = cands[np.abs(v[None] - cands[:, None]).min(1) > CLS_MARGIN]
    rate = (v[None] >= cands[:, None]).mean(1)
    return [float(cands[len(cands) - 1 - np.abs(rate - r)[::-1].argmin()]) for r in (0.10, 0.60)]


def cls_coverage(ref, confs):
    """Shares and counts the tests assert (DESIGN 4.1 has the table), from the reference: over the (anchor, head) pairs -- ``tie2``
    exact two-way ties, ``sat_first`` saturated with arg-max != column of the largest logit, ``all_sat`` / ``all_zero`` (arg-max 0);
    ``columns``: class columns that are the expected arg-max at an anchor passing the lower threshold; ``cross_tile`` /
    ``cross_wave`` / ``cross_window``: two-way ties of passing anchors whose columns lie in different 32-column tiles / on different
    sides of column 96 or 192 / in different 64-column windows; ``tile_counts``: per threshold the set of pass counts of the
    32-row tiles of every level."""
    ci, cmax, kind, ntie = ref['ci'], ref['cmax'], ref['kind'], ref['ntie']
    pairs = float(ci.size)
    nc = np.array([b - a for a, b in zip(CLS_HEAD0[:-1], CLS_HEAD0[1:])])
    ok = ref['mask'] >= min(confs)
    cols = set()
    for k in range(8):
        cols |= set((CLS_HEAD0[k] + ci[..., k][ok]).tolist())
    t2 = ref['tie2'] + np.array(CLS_HEAD0[:8])[None, None, :, None]
    t2 = t2[(ref['tie2'][..., 0] >= 0) & ok[..., None]]
    wave = lambda c: (c >= 96).astype(int) + (c >= 192)
    counts = []
    for conf in confs:
        seen = set()
        for lv in range(len(CLS_MAPS)):
            rows = (ref['mask'][:, CLS_LEVEL_OFF[lv]:CLS_LEVEL_OFF[lv + 1]] >= conf).flatten()
            seen |= set(int(rows[i:i + 32].sum()) for i in range(0, len(rows), 32))
        counts.append(seen)
    return dict(tie2=float((ref['tie2'][..., 0] >= 0).sum()) / pairs,
                sat_first=float(((kind == 'S') & (ci != cmax) & (ntie < nc)).sum()) / pairs,
                all_sat=float(((kind == 'S') & (ntie == nc)).sum()) / pairs, all_zero=float((kind == 'Z').sum()) / pairs,
                columns=len(cols), cross_tile=int((t2[:, 0] // 32 != t2[:, 1] // 32).sum()),
                cross_wave=int((wave(t2[:, 0]) != wave(t2[:, 1])).sum()), cross_window=int((t2[:, 0] // 64 != t2[:, 1] // 64).sum()),
                tile_counts=counts)


def score_key_hi(sc32):
    """High word of lp_score.inc::score_key for float32 scores (numpy uint32): descending-orderable bits, a NaN of either sign 0."""
    sc32 = np.ascontiguousarray(sc32, np.float32)
    u = sc32.view(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(sc32), np.uint32(0), ~u).astype(np.uint32)


def sum8_f32(cf, last=7):
    """Left-to-right fp32 sum of cf[..., 0..6] and cf[..., last], / 8 (score_mask_value: last = 6, score_value: last = 7)."""
    cf = np.asarray(cf, np.float32)
    s = cf[..., 0] + cf[..., 1]
    for k in (2, 3, 4, 5, 6, last):
        s = (s + cf[..., k]).astype(np.float32)
    return (s / np.float32(8.0)).astype(np.float32)


def sigmoid32(v):
    """rcp(1 + exp(-v)) in numpy float32: not the device's bits, but the same properties (1.0f from 20 up, +0.0f from -128 down,
    monotone, NaN for NaN)."""
    v = np.asarray(v, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-v))).astype(np.float32)


CLS_MUTANTS = ('logit_argmax', 'last_equal', 'boundary', 'nan_dropped', 'mask_cf7', 'windows_desc')


def cls_emulate(logits32, mutant=None):
    """numpy emulation of the class path in head_det_kernel's operation order on fp32 logits [R,277]: per head the NaN-propagating
    maximum of the LOGITS, its sigmoid, the mask (ad4 twice) and the score as left-to-right fp32 sums, and the FIRST column whose
    sigmoid equals the maximum (both NaN: the first NaN), looked for in the 64-column windows in ascending order.  ``mutant``: one
    of CLS_MUTANTS, the same path subtly wrong.  -> dict cf [R,8] float32, ci [R,8], mask [R], score [R] float32."""
    assert mutant is None or mutant in CLS_MUTANTS
    x = np.asarray(logits32, np.float32)
    sg = sigmoid32(x)
    edges = list(CLS_HEAD0)
    if mutant == 'boundary':
        edges = [0] + [e + 1 for e in edges[1:-1]] + [edges[-1]]
    cf, ci = np.zeros((len(x), 8), np.float32), np.zeros((len(x), 8), np.int64)
    for k in range(8):
        a, b = edges[k], edges[k + 1]
        with np.errstate(invalid='ignore'):
            mx = np.fmax.reduce(x[:, a:b], 1) if mutant == 'nan_dropped' else x[:, a:b].max(1)
        cf[:, k] = sigmoid32(mx)
        hit = sg[:, a:b] == cf[:, k:k + 1]
        if mutant != 'nan_dropped':
            hit |= np.isnan(cf[:, k:k + 1]) & np.isnan(x[:, a:b])
        if mutant == 'logit_argmax':
            hit = (x[:, a:b] == mx[:, None]) | (np.isnan(mx)[:, None] & np.isnan(x[:, a:b]))
        if mutant == 'windows_desc':
            win = np.where(hit, (np.arange(a, b) // 64)[None], -1)
            hit &= win == win.max(1, keepdims=True)
        ci[:, k] = (b - a - 1 - hit[:, ::-1].argmax(1)) if mutant == 'last_equal' else hit.argmax(1)
    return dict(cf=cf, ci=ci, mask=sum8_f32(cf, 7 if mutant == 'mask_cf7' else 6), score=sum8_f32(cf, 7))


def cls_nan_data(dtype_width, head, seed):
    """The small non-finite case: the coded data of ``cls_case_data`` at width ``dtype_width`` on every level, plus ONE channel
    (a noise channel no head weighs) with weight +inf on the middle column of ``head`` and 0 elsewhere.  Its feature cycles over
    the pixels through 0 (0 * inf: that column is NaN), +1 (+inf: probability 1.0, a tie with every saturated column), -1 (-inf:
    probability 0) and +1.  -> (levels, class column 0..276 that carries the weight)"""
    d = cls_case_data((dtype_width,) * 3, seed)
    col = (CLS_HEAD0[head] + CLS_HEAD0[head + 1]) // 2
    levels = []
    for x, wc, bc in d['levels']:
        free = [c for c in range(wc.shape[1]) if float(wc[:, c].abs().sum()) == 0]
        ch = free[len(free) // 2]
        wc = wc.clone()
        wc[col, ch] = float('inf')
        x = x.clone()
        Bn, C, h, w = x.shape
        pat = torch.tensor([0.0, 1.0, -1.0, 1.0], dtype=torch.float64)[torch.arange(Bn * h * w) % 4].reshape(Bn, h, w)
        x[:, ch] = pat
        levels.append((x, wc, bc))
    return levels, col


def cls_nan_expected(levels):
    """Expectation of the non-finite case from the reference's torch.max: the float64 logits, the probabilities every admissible
    implementation must return -- 1.0 from logit 20 up, 0.0 from -128 down, NaN for NaN, else the float64 sigmoid --, and per head
    torch.max of them (the first maximum; a NaN wins, the first one).  -> dict (numpy) cf [B,N,8] float64, ci [B,N,8], mask [B,N]
    (NaN where a head 0..6 is NaN), ``nan`` [B,N,277] bool."""
    L, _, _ = cls_logits64(levels)
    P = torch.where(L >= CLS_SAT, torch.ones_like(L), torch.where(L <= CLS_ZERO, torch.zeros_like(L), torch.sigmoid(L)))
    assert bool((torch.isnan(P) == torch.isnan(L)).all())
    cf, ci = zip(*[torch.max(P[..., sl], -1) for sl in _head_slices()])
    cf, ci = torch.stack(cf, -1).numpy(), torch.stack(ci, -1).numpy()
    return dict(logits=L.float().numpy(), cf=cf, ci=ci, mask=(cf[..., :7].sum(-1) + cf[..., 6]) / 8.0, nan=torch.isnan(L).numpy())


_cls_cache = {}


def cls_case(dtype, widths, seed=100):
    """Data, reference, thresholds and coverage of a case, computed once per process and never modified."""
    key = (dtype, tuple(widths), seed)
    if key not in _cls_cache:
        d = cls_case_data(widths, seed)
        ref = cls_reference(d['levels'], dtype)
        confs = cls_thresholds(ref['mask'])
        _cls_cache[key] = dict(levels=d['levels'], ref=ref, confs=confs, cov=cls_coverage(ref, confs))
    return _cls_cache[key]


def cls_check(ref, conf, passed, cf, ci, key_hi=None):
    """What the tests assert of a class path's result at threshold ``conf``, against ``cls_reference``: ``passed`` [B,N] bool is
    the reference's set; at the passing anchors ``ci`` [B,N,8] is the expected arg-max, ``cf`` [B,N,8] float32 is exactly 1.0f
    for a saturated head, exactly +0.0f for a zero one and else inside the elementwise bound of the largest float64 sigmoid, and
    ``key_hi`` [B,N] is score_key of the left-to-right fp32 sum of the eight / 8.  -> list of the quantities that differ (empty:
    all hold), so that a test can also require that a wrong result IS noticed."""
    bad = []
    want = ref['mask'] >= conf
    assert float(np.abs(ref['mask'] - conf).min()) > CLS_MARGIN
    if not np.array_equal(np.asarray(passed, bool), want):
        bad.append('candidates')
    cf, ci = np.asarray(cf, np.float32)[want], np.asarray(ci)[want]
    if not np.array_equal(ci, ref['ci'][want]):
        bad.append('arg-max')
    kind, best = ref['kind'][want], ref['best'][want]
    col = np.array(CLS_HEAD0[:8])[None] + ref['ci'][want]
    bound = np.take_along_axis(ref['bound'][want], col, -1)
    bits = cf.view(np.uint32)
    ok = np.where(kind == 'S', bits == 0x3f800000, np.where(kind == 'Z', bits == 0, np.abs(cf.astype(np.float64) - best) <= bound))
    if not ok.all():
        bad.append('maximum')
    if key_hi is not None and not np.array_equal(np.asarray(key_hi)[want], score_key_hi(sum8_f32(cf, 7))):
        bad.append('key')
    return bad


# ---- graphs at the edges of the fused forms' legality rules (tests/test_graph_rules_cpu.py, tests/test_graph_rules_gpu.py) ------------
# Four engine forms skip writing a tensor because a scan of the frozen graph says nobody else reads it: the planar stem and the
# fused stem (LP_VARIANT_PIPE_P on op 1, LP_VARIANT_FUSED_STEM2 on op 2), the fused 1x1 + 3x3 stride-2 form (LP_VARIANT_FUSED_PW_S2)
# and the fused BiFusion form (LP_VARIANT_FUSED_BIFUSION).  Per form one builder: ``change`` None is the BASE graph the form must
# accept, every other value of its *_CHANGES table a graph that differs from the base in that one thing and must be refused.  The
# builders record what they add (``RuleGraph.nodes``), so that ``rule_graph_expected`` can state every tensor's bits in float64.
RULE_MARK = 0x7FA5                      # a NaN in fp16 and in bf16 that no kernel produces from finite data: "never written"
PIPE_P, FUSED_STEM2, FUSED_PW_S2, FUSED_BIFUSION = 36, 37, 38, 45          # lp_hip.h's variant codes of the four forms


def _zero_data(name, wshape, nbias, stage):
    return np.zeros(wshape, np.float32), np.zeros(nbias, np.float32)


class RuleGraph:
    """Records a small op graph while adding it to ``eng`` (a runtime.Engine that is not finished yet).  Tensors are named;
    ``t[name]`` is the id, ``op[name]`` the op index of the layer that writes it.  ``data(name, weight shape, bias length, stage)``
    -> (weight, bias) supplies the layers' parameters (default: zeros); stage 1 = a layer over network inputs, 2 = over the outputs
    of stage 1, 3 = anything later (grid_rule_data keeps each stage's sums exact)."""

    def __init__(self, eng, data=None):
        self.eng, self.data = eng, data or _zero_data
        self.t, self.chan, self.sl = {'input': eng.input_id}, {eng.input_id: 3}, {eng.input_id: 0}
        self.op, self.nodes, self.sources = {'input': 0}, [dict(kind='input', op=0, dsts=[eng.input_id])], []
        self.form = self.form_op = None
        self.carried_ops, self.carried_tensors = [], []

    def _tensor(self, name, c, sl):
        assert name not in self.t, name
        tid = self.eng.tensor(c, sl)
        self.t[name], self.chan[tid], self.sl[tid] = tid, c, sl
        return tid

    def source(self, name, c, sl):
        """A tensor no op writes: the test fills it.  A multiple of 8 channels, so that it has no padding channels."""
        assert c % 8 == 0
        self.sources.append(name)
        return self._tensor(name, c, sl)

    def conv(self, name, srcs, cout, k, s, act, res=None, stage=3, also=None):
        """act(conv(cat(srcs)) + b) [+ RES_ALPHA * res] -> tensor ``name``; ``also`` = (name2, cout2): a two-destination launch."""
        from yolov6.hip import abi
        ids = [self.t[n] for n in srcs]
        sl = self.sl[ids[0]]
        cin, c2 = sum(self.chan[i] for i in ids), (also[1] if also else 0)
        w, b = self.data(name, (cout + c2, cin, k, k), cout + c2, stage)
        wn, bn = (np.ascontiguousarray(np.asarray(v, dtype=np.float32)) for v in (w, b))
        dst = self._tensor(name, cout, sl + (s == 2))
        dst2 = self._tensor(also[0], c2, sl + (s == 2)) if also else -1
        self.eng._add_conv(ids, wn, bn, k, s, {'none': abi.LP_ACT_NONE, 'relu': abi.LP_ACT_RELU}[act], dst, dst2,
                           res=None if res is None else self.t[res], alpha=RES_ALPHA if res is not None else 0.0)
        self.op[name] = len(self.nodes)
        self.nodes.append(dict(kind='conv', op=len(self.nodes), name=name, srcs=ids, res=None if res is None else self.t[res], k=k, s=s,
                               act=act, w=w, b=b, dsts=[dst] + ([dst2] if also else []), split=cout))
        return dst

    def deconv(self, name, src, cout, stage=3):
        """2x2 stride-2 transposed convolution with bias, no activation."""
        from yolov6.hip import abi
        sid = self.t[src]
        w, b = self.data(name, (self.chan[sid], cout, 2, 2), cout, stage)
        wn, bn = (np.ascontiguousarray(np.asarray(v, dtype=np.float32)) for v in (w, b))
        dst = self._tensor(name, cout, self.sl[sid] - 1)
        abi.check(self.eng.lib.lp_engine_add_deconv2x2(self.eng.h, sid, dst, self.eng._ptr(wn), self.eng._ptr(bn)), 'lp_engine_add_deconv2x2')
        self.op[name] = len(self.nodes)
        self.nodes.append(dict(kind='deconv', op=len(self.nodes), name=name, srcs=[sid], res=None, w=w, b=b, dsts=[dst]))
        return dst

    def tail(self, name):
        """Two downstream readers of tensor ``name`` (the output of a fused kernel): one reads it as a source, one as a residual."""
        c = self.chan[self.t[name]]
        self.conv('t1', [name], c, 1, 1, 'relu')
        self.conv('t2', ['t1'], c, 1, 1, 'relu', res=name)

    def carries(self, form, form_op, ops, tensors):
        """What the accepted form does: ``form`` on op ``form_op`` carries the ops ``ops``; the named ``tensors`` stay unwritten."""
        self.form, self.form_op, self.carried_ops, self.carried_tensors = form, self.op[form_op], [self.op[o] for o in ops], list(tensors)
        return self


# change -> does the PLANAR stem still take op 1 (the fused stem must refuse every one of them)
STEM_CHANGES = {
    'stem_read_by_later_conv': True, 'stem_second_source_of_later_conv': True, 'stem_residual_of_later_op': True,
    'l2_residual': True, 'l2_two_destinations': True, 'l2_two_sources': True, 'stem_act_none': True, 'l2_act_none': True,
    'stem_two_destinations': False, 'input_second_reader': False,
}


def stem_rule_graph(eng, change=None, data=None):
    """input -> stem 3x3 s2 ReLU 3 -> 24 (op 1) -> l2 3x3 s2 ReLU 24 -> 64 (op 2) -> two readers of l2 only."""
    assert change is None or change in STEM_CHANGES, change
    g = RuleGraph(eng, data)
    s_act, l_act = ('none' if change == 'stem_act_none' else 'relu'), ('none' if change == 'l2_act_none' else 'relu')
    g.conv('stem', ['input'], 24, 3, 2, s_act, stage=1, also=('stem_b', 8) if change == 'stem_two_destinations' else None)
    if change in ('l2_two_sources', 'stem_second_source_of_later_conv'):
        g.source('e1', 8, 1)
    if change == 'l2_residual':
        g.source('r2', 64, 2)
    g.conv('l2', ['stem', 'e1'] if change == 'l2_two_sources' else ['stem'], 64, 3, 2, l_act, stage=2,
           res='r2' if change == 'l2_residual' else None, also=('l2_b', 8) if change == 'l2_two_destinations' else None)
    g.tail('l2')
    if change == 'stem_read_by_later_conv':
        g.conv('x1', ['stem'], 8, 1, 1, 'relu')
    if change == 'stem_second_source_of_later_conv':
        g.conv('x1', ['e1', 'stem'], 8, 1, 1, 'relu')
    if change == 'stem_residual_of_later_op':                 # a 1x1 layer at the stem's scale: over a transposed conv of l2's output
        g.deconv('up', 'l2', 24)
        g.conv('x1', ['up'], 24, 1, 1, 'relu', res='stem')
    if change == 'input_second_reader':
        g.conv('x1', ['input'], 8, 3, 2, 'relu', stage=1)
    return g.carries(FUSED_STEM2, 'l2', ['input', 'stem'], ['stem'])


PW_CHANGES = ('p_read_by_later_conv', 'p_residual_of_later_op', 'op_between', 'lanes_differ', 'p_read_on_other_lane', 'p_two_destinations',
              'p_residual', 'p_two_sources', 'c_residual', 'c_two_destinations')


def pw_rule_graph(eng, change=None, data=None):
    """x (64 channels, stride 8) -> p 1x1 ReLU 64 -> 64 -> c 3x3 s2 ReLU 64 -> 64 (the op right behind p) -> two readers of c only."""
    assert change is None or change in PW_CHANGES, change
    g = RuleGraph(eng, data)
    g.source('x', 64, 3)
    for name, c, sl, when in (('x2', 8, 3, 'p_two_sources'), ('rp', 64, 3, 'p_residual'), ('rc', 64, 4, 'c_residual')):
        if change == when:
            g.source(name, c, sl)
    if change == 'lanes_differ':
        eng.lane(1)
    g.conv('p', ['x', 'x2'] if change == 'p_two_sources' else ['x'], 64, 1, 1, 'relu', stage=1, res='rp' if change == 'p_residual' else None,
           also=('p_b', 8) if change == 'p_two_destinations' else None)
    eng.lane(0)
    if change == 'op_between':
        g.conv('x1', ['x'], 8, 1, 1, 'relu', stage=1)
    g.conv('c', ['p'], 64, 3, 2, 'relu', stage=2, res='rc' if change == 'c_residual' else None,
           also=('c_b', 8) if change == 'c_two_destinations' else None)
    g.tail('c')
    if change == 'p_read_by_later_conv':
        g.conv('x1', ['p'], 8, 1, 1, 'relu')
    if change == 'p_residual_of_later_op':
        g.conv('x1', ['x'], 64, 1, 1, 'relu', stage=1, res='p')
    if change == 'p_read_on_other_lane':
        eng.lane(1)
        g.conv('x1', ['p'], 8, 1, 1, 'relu')
        eng.lane(0)
    return g.carries(FUSED_PW_S2, 'c', ['p'], ['p'])


BF_CHANGES = ('u_read_by_later_conv', 'a_read_by_later_conv', 'u_residual_of_later_op', 'a_residual_of_later_op', 'cv3_residual',
              'cv3_two_destinations', 'cv3_act_none', 'sources_reordered', 'third_source_128', 'cv1_first_of_two_destinations')


def bifusion_rule_graph(eng, change=None, data=None):
    """The graph of test_bifusion_fused_equals_its_three_ops: x0 (64 channels, stride 16), x1 (128, stride 8), d (64, stride 8);
    u = transposed conv of x0 (op 1), a = cv1 = 1x1 ReLU 128 -> 64 of x1 (op 2), cv3 = 1x1 ReLU over [u, a, d] -> 64 (op 3), then
    two readers of cv3 only."""
    assert change is None or change in BF_CHANGES, change
    g = RuleGraph(eng, data)
    g.source('x0', 64, 4)
    g.source('x1', 128, 3)
    g.source('d', 128 if change == 'third_source_128' else 64, 3)
    if change == 'cv3_residual':
        g.source('r3', 64, 3)
    g.deconv('u', 'x0', 64, stage=1)
    g.conv('a', ['x1'], 64, 1, 1, 'relu', stage=1, also=('a_b', 8) if change == 'cv1_first_of_two_destinations' else None)
    g.conv('cv3', ['a', 'u', 'd'] if change == 'sources_reordered' else ['u', 'a', 'd'], 64, 1, 1, 'none' if change == 'cv3_act_none' else 'relu',
           stage=2, res='r3' if change == 'cv3_residual' else None, also=('cv3_b', 8) if change == 'cv3_two_destinations' else None)
    g.tail('cv3')
    for name, src in (('u_read_by_later_conv', 'u'), ('a_read_by_later_conv', 'a')):
        if change == name:
            g.conv('x1r', [src], 8, 1, 1, 'relu')
    for name, src in (('u_residual_of_later_op', 'u'), ('a_residual_of_later_op', 'a')):
        if change == name:
            g.conv('x1r', ['d'], 64, 1, 1, 'relu', stage=1, res=src)
    return g.carries(FUSED_BIFUSION, 'cv3', ['u', 'a'], ['u', 'a'])


RULE_GRAPHS = {'stem': (stem_rule_graph, tuple(STEM_CHANGES)), 'pw': (pw_rule_graph, PW_CHANGES), 'bifusion': (bifusion_rule_graph, BF_CHANGES)}


def engine_state(eng, tiles=False):
    """What a refused request must leave alone: per op (variant, ring depth), the carrier with and without a direct frame, and --
    ``tiles``: an arena is bound -- the tile choice and the prepared tile (None where the op's kernel has no tiles)."""
    out = []
    for i in range(eng.lib.lp_engine_num_ops(eng.h)):
        row = [eng.variant(i), eng.lib.lp_engine_op_carrier(eng.h, i, 1), eng.lib.lp_engine_op_carrier(eng.h, i, 0)]
        if tiles:
            try:
                row.append(eng.tile(i))
            except RuntimeError:
                row.append(None)
        out.append(tuple(row))
    return out


def grid_unit(t64):
    """The largest power of two (at most 1) that every element of ``t64`` is a multiple of."""
    for k in range(0, 24):
        s = t64 * float(2 ** k)
        if torch.equal(torch.round(s), s):
            return 2.0 ** -k
    raise AssertionError('not grid data')


def grid_rule_data(dtype, seed=0):
    """``data`` of a RuleGraph whose sums stay exact over three and more chained layers: stage 1 and 2 as E.fused_data draws them
    (x, w multiples of 1/4 in [-2, 2], the second layer's bias sized so that its outputs need rounding), later layers four weights
    of +-1 per output channel (and tap / phase) and a small bias, so that neither the grid unit nor the magnitudes grow much."""
    import zlib
    xw, bb, _ = GRID_RANGE[dtype]

    def data(name, wshape, nbias, stage):
        s = seed + zlib.crc32(name.encode()) % 100000
        if stage == 1:
            return grid_rand(wshape, s, -2.0, 2.0), grid_rand((nbias,), s + 1, -8.0, 32.0, 1.0 / 16)
        if stage == 2:
            lim = 2.0 if wshape[1] * wshape[2] * wshape[3] <= 9 * 32 else 1.0          # by fan-in, as E.fused_data
            return grid_rand(wshape, s, -lim, lim), grid_rand((nbias,), s + 1, -bb / 4, bb, 1.0 / 16)
        g = torch.Generator().manual_seed(s)
        w = torch.zeros(wshape, dtype=torch.float64)
        transposed = wshape[2] == 2                                   # [Cin][Cout][2][2], else [Cout][Cin][k][k]
        nout, nin = (wshape[1], wshape[0]) if transposed else (wshape[0], wshape[1])
        for o in range(nout):
            for tap in range(wshape[2] * wshape[3]):
                idx = torch.randperm(nin, generator=g)[:4]
                sign = torch.randint(0, 2, (len(idx),), generator=g).double() * 2 - 1
                if transposed:
                    w[idx, o, tap // wshape[3], tap % wshape[3]] = sign
                else:
                    w[o, idx, tap // wshape[3], tap % wshape[3]] = sign
        return w, grid_rand((nbias,), s + 1, -8.0, 32.0, 1.0 / 16)
    return data


def rule_graph_inputs(g, dtype, B, H, W, seed=0):
    """Grid values for the frame and every source tensor of a RuleGraph at frame size H x W: {tensor id: float64 [B,C,h,w]};
    multiples of 1/4 in [-2, 2], residual sources (names starting with 'r') in the storage type's residual range."""
    vals = {g.t['input']: grid_rand((B, 3, H, W), seed + 3, -2.0, 2.0)}
    for i, name in enumerate(g.sources):
        tid = g.t[name]
        lim = GRID_RANGE[dtype][2] if name.startswith('r') else 2.0
        vals[tid] = grid_rand((B, g.chan[tid], H >> g.sl[tid], W >> g.sl[tid]), seed + 10 + i, -lim, lim)
    return vals


def rule_graph_expected(g, vals, dtype):
    """Expected bits of every tensor an op of the RuleGraph writes, from float64: {tensor id: tensor of ``dtype``}.  Per layer the
    sum is asserted to be exact in fp32 in ANY order: every product and the bias are multiples of unit = unit(x) * unit(w), and
    sum |x||w| + |b| -- the actual magnitudes, per output element -- stays below 2^24 units; the expected tensor is then the
    float64 sum under exact_epilogue (one rounding, a second one behind the residual add).  ``vals`` is not modified."""
    import torch.nn.functional as F
    val = {t: v.clone() for t, v in vals.items()}
    for t, v in val.items():
        assert torch.equal(v.to(dtype).double(), v), 'the storage type does not hold an input'
    want = {}
    for n in g.nodes[1:]:
        x = torch.cat([val[s] for s in n['srcs']], 1)
        w, b = torch.as_tensor(n['w']).double(), torch.as_tensor(n['b']).double()
        assert torch.equal(w.to(dtype).double(), w) and torch.equal(b.float().double(), b), n['name']
        if n['kind'] == 'deconv':
            op = lambda a, c, d: F.conv_transpose2d(a, c, d, stride=2)
        else:
            op = lambda a, c, d, n=n: F.conv2d(a, c, d, stride=n['s'], padding=n['k'] // 2)
        pre, mag = op(x, w, b), op(x.abs(), w.abs(), b.abs())
        unit = grid_unit(x) * grid_unit(w)
        assert grid_unit(b) >= unit and float(mag.max()) < 2 ** 24 * unit, (n['name'], float(mag.max()), unit)
        res = None if n['res'] is None else val[n['res']]
        y = exact_epilogue(pre, n.get('act', 'none'), dtype, res)
        assert bool(torch.isfinite(y.float()).all()), n['name']
        parts = [y] if len(n['dsts']) == 1 else [y[:, :n['split']], y[:, n['split']:]]
        for t, p in zip(n['dsts'], parts):
            want[t], val[t] = p.contiguous(), p.double()
    return want


# ---- scenes at the edges of the greedy NMS schedule, and a model of that schedule (tests/test_nms_schedule_cpu.py, _gpu.py) ----
# greedy_kernel (csrc/lp_nms.hip) resolves the sorted candidates 64 at a time: chunk c's candidates are struck by the kept list
# through chunk c - 2 (fifteen waves, each a 1-in-15 share of the list, eight entries per trip = 120 list entries per trip of the
# block, then a remainder loop; a ring of three masks), by the SURVIVORS of chunk c - 1 (xt & kept_prev) and by the earlier survivors
# of their own chunk (mt, resolved in candidate order); candidates are staged 1024 = 16 chunks at a time.  The scenes below put one
# decision on every such edge.  Their geometry is spill_case's, denser: 8 x 8 boxes in CELLS of a 16-px grid, 128 cells per row; a
# cell holds a CHAIN, member s being the cell's box shifted by s px in x.  With iou_thres 0.7 the only pairs over the threshold are
# members one shift apart (IoU 56/72) and identical boxes; two apart 48/80, three apart 40/88, other cells 0: every decision has a
# margin of more than 0.07.  Row r of a scene has rank r (strictly decreasing exact scores); to_pred scatters the ranks over the
# anchors of a prediction tensor, so the sort is part of every case.
NMS_IOU, NMS_CONF = 0.7, 0.25
NMS_CHAIN_IOU = (1.0, 56.0 / 72.0, 48.0 / 80.0, 40.0 / 88.0)          # by the difference of two members' shifts
NMS_MUTANTS = ('no_remainder', 'last_share', 'stale_T', 'ring2', 'late_batch', 'xt_alive', 'xt_any', 'no_xt', 'no_mt', 'mt_dead_kills',
               'no_cut')
SHARE_KS = (1, 14, 15, 16, 105, 119, 120, 121, 135, 240, 241)
CUT_MS = (1, 63, 64, 65, 190, 200)
NC_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025)
SORT_EDGES = (16383, 16384, 16385)


def chain(*ranks):
    """rank -> (cell, shift) of one chain: its members in rank order share the cell of the first, member s shifted by s px."""
    assert len(ranks) <= 4 and list(ranks) == sorted(ranks)
    return {r: (ranks[0], s) for s, r in enumerate(ranks)}


def copies(ranks, of):
    """rank -> (cell, shift) making ``ranks`` copies (1 px to the right) of the singles ranked ``of``."""
    return {int(r): (int(o), 1) for r, o in zip(ranks, of)}


def cell_expect(cell, shift, max_det):
    """The kept ranks in closed form: cells are independent; inside a cell, in rank order, a member is kept unless a kept member of
    the cell is at most one shift away (NMS_CHAIN_IOU: differences 0 and 1 are over the threshold, 2 and 3 are not)."""
    held, keep = {}, []
    for r in range(len(cell)):
        h = held.setdefault(int(cell[r]), [])
        if all(abs(int(shift[r]) - s) > 1 for s in h):
            h.append(int(shift[r]))
            keep.append(r)
    return np.asarray(keep[:max_det], np.int64)


def nms_scene(name, n, special=None, sort_scores=False, max_det=None, score=None):
    """A scene of ``n`` ranks: ``special`` maps rank -> (cell, shift); every other rank is a single in the cell of its own number
    (cells named by a special rank are therefore cells of lower ranks, or stay empty).  Scores (16000 - r) / 16384, or
    (32767 - r) / 32768 with ``sort_scores``: multiples of 2^-14 / 2^-15 below 1, so the eight-term sums are exact and mask value =
    score.  -> dict(name, n, cell, shift, box [n,4] float64 xyxy, score float64, iou, conf, max_det, expect = kept ranks)."""
    cell, shift = np.arange(n), np.zeros(n, np.int64)
    for r, (c, s) in (special or {}).items():
        assert 0 <= r < n and 0 <= c <= r and 0 <= s <= 3, (name, r, c, s)
        cell[r], shift[r] = c, s
    x1, y1 = 16.0 * (cell % 128) + shift, 16.0 * (cell // 128)
    if score is None:
        score = (32767.0 - np.arange(n)) / 32768.0 if sort_scores else (16000.0 - np.arange(n)) / 16384.0
        assert n < 16000 or sort_scores
    max_det = n if max_det is None else max_det
    return dict(name=name, n=n, cell=cell, shift=shift, box=np.stack([x1, y1, x1 + 8.0, y1 + 8.0], 1), score=np.asarray(score, np.float64),
                iou=NMS_IOU, conf=2.0 ** -16 if sort_scores else NMS_CONF, max_det=max_det, expect=cell_expect(cell, shift, max_det))


def _edge_chains(b, in_chunk=True):
    """The chains around the chunk boundary b (rank b is lane 0 of a chunk); all offsets are distinct mod 64."""
    sp = {}
    for ch in ((b - 1, b, b + 1),             # killer in lane 63, victim lane 0 of the next chunk, the victim's copy must live
               (b - 4, b - 3, b + 2),         # the victim dies inside its chunk (mt): its xt bit on b + 2 must not count
               (b - 6, b + 6),                # a plain kill across the edge (xt)
               (b - 130, b - 8, b + 8),       # the victim is dead by the kept list; its copy in the next chunk lives
               (b - 71, b - 10, b + 10),      # the victim dies in wave 0 through xt & kept_prev; its copy in the next chunk lives
               (b - 133, b + 12)):            # a kill through the kept list
        sp.update(chain(*ch))
    if in_chunk:
        sp.update(chain(b + 20, b + 21, b + 22, b + 23))      # keep, kill, keep, kill inside one chunk
    return sp


def scene_chunk_edges(bounds=(192, 256, 320), max_det=None, name='chunk_edges'):
    sp = {}
    for b in bounds:
        sp.update(_edge_chains(b))
    return nms_scene(name, bounds[-1] + 128, sp, max_det=max_det)


def scene_share(K):
    """K singles (kept position = rank), 128 copies of rank 0 (they die, and keep the ranks behind them clear of the xt path), then one
    copy of every single in a seeded order: each has exactly one killer, at kept position = its rank."""
    order = np.random.default_rng(900 + K).permutation(K)
    sp = copies(range(K, K + 128), [0] * 128)
    sp.update(copies(range(K + 128, 2 * K + 128), order))
    return nms_scene('share_%d' % K, 2 * K + 128, sp)


def scene_ring(pattern='SSCSSSCCSCSSCSS'):
    """Chunks of 64 singles (S) and of 64 copies of the first chunk (C: the whole chunk is dead by the kept list)."""
    assert pattern[0] == 'S'
    sp = {}
    for c, kind in enumerate(pattern):
        if kind == 'C':
            sp.update(copies(range(64 * c, 64 * c + 64), range(64)))
    return nms_scene('ring', 64 * len(pattern), sp)


def scene_batch_edges():
    """The cross-edge chains at the first chunks of the second and third staged batch, and in each of those chunks 16 candidates
    that only the kept list suppresses."""
    sp = {}
    for i, b in enumerate((1024, 2048)):
        sp.update(_edge_chains(b, in_chunk=False))
        sp.update(copies(range(b + 30, b + 46), range(200 + 16 * i, 216 + 16 * i)))
    return nms_scene('batch_edges', 2176, sp)


def scene_nc(n):
    """n candidates, every third one a copy of the one before it."""
    return nms_scene('nc_%d' % n, n, copies(range(2, n, 3), range(1, n, 3)))


def scene_sort(n):
    return nms_scene('sort_%d' % n, n, sort_scores=True, max_det=31000)


def scene_ties():
    """130 candidates of ONE score: the order is the anchor order.  Rank 0 and rank 129 are singles, (1, 2), (3, 4), ... (127, 128)
    overlapping pairs -- (63, 64) and (127, 128) across a chunk edge -- whose winner is the lower anchor."""
    return nms_scene('ties', 130, copies(range(2, 129, 2), range(1, 128, 2)), score=np.full(130, 0.5))


def scene_threshold(below):
    """Two 8 x 6 boxes 2 px apart in y: IoU = 32 / 64 = 0.5 exactly.  At iou_thres 0.5 the second is kept (the test is a strict >), at
    the next double below 0.5 it is suppressed."""
    sc = nms_scene('thr_below' if below else 'thr_at', 2)
    sc['box'] = np.array([[0.0, 0.0, 8.0, 6.0], [0.0, 2.0, 8.0, 8.0]])
    sc['iou'] = float(np.nextafter(0.5, 0.0)) if below else 0.5
    sc['expect'] = np.array([0] if below else [0, 1], np.int64)
    return sc


_NMS_SCENES = {}


def nms_schedule_scenes():
    """name -> scene, every scene whose overlap matrix the schedule model is run on (the sort scenes are singles only)."""
    if not _NMS_SCENES:
        sc = [scene_chunk_edges()] + [scene_share(K) for K in SHARE_KS] + [scene_ring(), scene_batch_edges()]
        sc += [scene_chunk_edges((192, 256), M, 'cut_%d' % M) for M in CUT_MS] + [scene_nc(n) for n in NC_EDGES] + [scene_ties()]
        _NMS_SCENES.update((s['name'], s) for s in sc)
    return _NMS_SCENES


def scene_perm(sc, N, seed):
    """Anchors of the ranks: a seeded draw of n of the N anchors, ascending where all scores are equal (ties go by the anchor)."""
    a = np.random.default_rng(seed).permutation(N)[:sc['n']]
    return np.sort(a) if sc['n'] > 1 and sc['score'][0] == sc['score'][-1] else a


def to_pred(sc, N, perm):
    """float32 [1, N, 290]: rank r at anchor perm[r], obj = 1, in each class segment one column with the rank's score; the other
    anchors keep score 0 (below conf) and an empty box."""
    assert len(perm) == sc['n'] <= N and len(np.unique(perm)) == sc['n']
    b = sc['box']
    cx, cy, w, h = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    p = np.zeros((1, N, 290), np.float32)
    p[0, :, 4] = 1.0
    p[0, perm, 0], p[0, perm, 1], p[0, perm, 2], p[0, perm, 3] = cx, cy, w, h
    p[0, perm, 5:13] = np.stack([b[:, 0], b[:, 1], b[:, 2], b[:, 1], b[:, 2], b[:, 3], b[:, 0], b[:, 3]], 1)
    for a in SEG[:-1]:
        p[0, perm, a + 1] = sc['score']
    return p


def assert_scene_geometry(sc):
    """From float64 geometry alone: the scores are fp32 values whose eight-term fp32 sum is exact, strictly decreasing (or all equal)
    and above conf; every pair of boxes with a common point lies in one cell and has the IoU of its shift difference; no IoU is
    within 0.07 of the threshold.  -> the boolean overlap matrix (IoU > iou_thres) in rank order; None for a scene of more than
    4096 singles, whose boxes are shown disjoint cell by cell instead."""
    s, b, n = sc['score'], sc['box'], sc['n']
    s32 = s.astype(np.float32)
    eight = s32.copy()
    for _ in range(7):
        eight = eight + s32
    assert np.array_equal(s32.astype(np.float64), s) and np.array_equal(eight / np.float32(8.0), s32), sc['name']
    assert np.all(np.diff(s) < 0) or np.all(s == s[0]), sc['name']
    assert float(s.min()) > sc['conf'] and np.array_equal(b.astype(np.float32).astype(np.float64), b), sc['name']
    if n > 4096:
        cx, cy = b[:, 0] // 16, b[:, 1] // 16
        assert not sc['shift'].any() and len(np.unique(cy * 128 + cx)) == n, sc['name']
        assert np.all(b[:, 2] <= 16 * cx + 16) and np.all(b[:, 3] <= 16 * cy + 16) and np.all(b[:, 2] > b[:, 0]), sc['name']
        return None
    w = np.maximum(0.0, np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]))
    h = np.maximum(0.0, np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]))
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    inter = w * h
    iou = inter / (area[:, None] + area[None, :] - inter)
    if sc['name'].startswith('thr_'):
        assert iou[0, 1] == 0.5 and inter[0, 1] == 32.0, sc['name']
    else:
        same = sc['cell'][:, None] == sc['cell'][None, :]
        assert np.array_equal(inter > 0, same), sc['name']
        want = np.asarray(NMS_CHAIN_IOU)[np.abs(sc['shift'][:, None] - sc['shift'][None, :])]
        assert np.allclose(iou[same], want[same], rtol=0, atol=1e-15) and float(np.abs(iou - sc['iou']).min()) > 0.07, sc['name']
    over = iou > sc['iou']
    np.fill_diagonal(over, False)
    return over


def greedy_plain_np(over, max_det):
    """The textbook greedy loop over a boolean overlap matrix in rank order -> kept ranks."""
    sup, keep = np.zeros(len(over), bool), []
    for i in range(len(over)):
        if sup[i]:
            continue
        if len(keep) == max_det:
            break
        keep.append(i)
        sup[i + 1:] |= over[i, i + 1:]
    return np.asarray(keep, np.int64)


def greedy_schedule_np(over, max_det, mutant=None):
    """greedy_kernel's decomposition of the same loop, restated (see the head of this section); ``mutant`` names ONE defect of
    NMS_MUTANTS.  The model exists to show that the scenes discriminate; the reference of the GPU tests is the C oracle."""
    assert mutant is None or mutant in NMS_MUTANTS
    n, NSW = len(over), 15
    kept, T_after, dead_of = [], [], []
    pidx, alive_prev, kept_prev = np.zeros(0, np.int64), np.zeros(0, bool), np.zeros(0, bool)
    for c in range((n + 63) // 64):
        idx = np.arange(64 * c, min(n, 64 * c + 64))
        # dead: the kept list as it stood when chunk c - 1 was resolved, i.e. through chunk c - 2; wave w tests entries w, w + 15, ...
        back = 3 if mutant == 'stale_T' else 2
        T = T_after[c - back] if c >= back else 0
        tested = []
        for w in range(NSW):
            k = w
            while k + 7 * NSW < T:                                     # a trip of eight tests
                tested += [k + u * NSW for u in range(8)]
                k += 8 * NSW
            if mutant != 'no_remainder':
                tested += list(range(k, T, NSW))
        if mutant == 'last_share':
            tested = [k for k in tested if k % NSW != NSW - 1]
        assert mutant in ('no_remainder', 'last_share') or sorted(tested) == list(range(T))
        dead = over[np.ix_(np.asarray(kept, np.int64)[np.asarray(tested, np.int64)], idx)].any(0)
        if mutant == 'ring2' and c >= 3:
            dead |= dead_of[c - 3][:len(idx)]
        # xt: the candidates of chunk c - 1 that overlap; honoured for its survivors only
        src = {'xt_alive': alive_prev, 'xt_any': np.ones(len(pidx), bool), 'no_xt': np.zeros(len(pidx), bool)}.get(mutant, kept_prev)
        hit = over[np.ix_(pidx[src], idx)].any(0)
        # mt: the earlier candidates of the chunk itself
        mt = np.triu(over[np.ix_(idx, idx)], 1)
        if mutant == 'late_batch' and c and c % 16 == 0:
            dead[:], hit[:], mt[:] = False, False, False
        alive = ~dead & ~hit
        todo, keptmask = alive.copy(), np.zeros(len(idx), bool)
        for k in range(len(idx)):
            if todo[k]:
                keptmask[k] = True
            if (todo[k] and mutant != 'no_mt') or (alive[k] and mutant == 'mt_dead_kills'):
                todo &= ~mt[k]
        kept += idx[keptmask].tolist()
        T_after.append(len(kept))
        dead_of.append(dead)
        pidx, alive_prev, kept_prev = idx, alive, keptmask
        if len(kept) >= max_det:
            break
    return np.asarray(kept if mutant == 'no_cut' else kept[:max_det], np.int64)


# ---- the tracker's add-ons together (tests/test_all_on_cpu.py, tests/test_all_on_gpu.py) ---------------------------------------------
# One scene through a tracker with best shot, stack, hold, look-back, watchlist, live watch and sightings all enabled.  The numpy chain
# ``AllOnNp`` composes the single specifications (PlateTrackerNp with every enable_*, BestShotNp, LookbackNp) in the order the product
# enqueues them; with a subset of ``ALL_ON_FEATURES`` it is the single-feature chain, with a ``mutant`` one deliberate mis-composition.
ALL_ON_FEATURES = ('shot', 'stack', 'hold', 'lookback', 'watch', 'live', 'sight')
ALL_ON_NEEDS = {'stack': ('shot',), 'lookback': ('hold',)}                       # what a feature cannot be enabled without
ALL_ON_OUTPUTS = {                                                               # feature -> the outputs of a step that are its own
    'track': ('det_out', 'tid', 'slot', 'ended_i', 'ended_f', 'ended_count'), 'hold': ('det_hold', 'count_hold', 'tid_hold'),
    'watch': ('match_i',), 'live': ('live_i', 'q_i', 'q_f', 'q_slot', 'q_count'), 'sight': ('sight_i',),
    'shot': ('shot_crops', 'shot_i', 'shot_q', 'shot_det'), 'stack': ('stack_crops', 'stack_i'), 'lookback': ('released',),
}
ALL_ON_MUTANTS = ('redact_first', 'stale_ended', 'stale_slot', 'lookback_no_copy', 'reset_skips_tracker', 'reset_skips_gallery',
                  'reset_skips_stack', 'reset_skips_memo', 'reset_skips_lookback')
ALL_ON = dict(n_streams=3, max_det=6, Bs=(1, 3, 70, 2, 0), frame_hw=(40, 120), crop_hw=(8, 24), max_crops=6, max_ended=2, depth=4, seed=2269,
              reset_before=3, reset_streams=(1,), poison=0xAB,
              track=dict(max_tracks=70, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=18),
              shot=dict(min_score=0.2), stack=dict(search=2, max_frames=5, min_width=8.0, min_sharp=1), hold=dict(min_hits=2),
              redact=dict(mode='mosaic', cell=4, margin=0.1), watch=dict(max_mismatch=1, max_cost=0.75), live=dict(min_hits=2),
              sight=dict(window=5, min_hits=1, max_mismatch=8, max_cost=6.0), sight_capacity=64)
_all_on_cache = {}


def all_on_scene(seed):
    """The calls [(det, count, stream_of, flush, frames)] of the all-on tests: ``test_track_cpu.random_track_case`` on the shapes of
    ALL_ON (two objects per stream that live inside the frame), plus, in every frame of stream 0, a passer-by in each free row: a
    5 x 3 box on its own cell of an 8 x 5 grid, seen once, so that stream 0 fills its 70 slots past lane 64 and its tracks end by age,
    many more per call than ``max_ended``; call 3 flushes stream 2 without showing it a frame; seeded frames that move from call to
    call, so that every crop sees other pixels."""
    import test_track_cpu as C
    p = ALL_ON
    calls = C.random_track_case(seed, n_streams=p['n_streams'], max_det=p['max_det'], n_obj=2, extent=40, Bs=p['Bs'])
    rng = np.random.default_rng(seed + 1000)
    H, W = p['frame_hw']
    base = rng.integers(0, 256, (H + 16, W + 64, 3), dtype=np.uint8)
    base[::2] //= 3                                                             # rows of two brightnesses: sharpness differs with the cut
    out, k, f = [], 0, 0
    for c, (det, count, stream_of, flush) in enumerate(calls):
        det, count, flush = det.copy(), count.copy(), list(flush)
        if c == 3:
            stream_of = [s if s != 2 else 1 for s in stream_of]
            flush[2] = 1
        for b, s in enumerate(stream_of):
            n = int(count[b])
            if s != 0 or not 0 <= n < p['max_det']:
                continue
            for r in range(n, p['max_det']):
                cell = k % 120
                x, y = 1 + 8 * (cell % 15), 1 + 5 * (cell // 15)
                det[b, r] = C.make_row((x, y, x + 5, y + 3), ids=rng.integers(0, 24, 8), conf=(rng.integers(3, 9, 8) / 8.0))
                k += 1
            count[b] = p['max_det']
        frames = []
        for b in range(len(det)):
            dy, dx = (5 * f) % 16, (7 * f) % 64
            frames.append(np.ascontiguousarray(base[dy:dy + H, dx:dx + W]))
            f += 1
        out.append((det, count, list(stream_of), flush, frames))
    return out


def all_on_watchlist(calls):
    """Entries for the scene: every other read that a plain run ends within ``max_ended`` and every third read a live track of at least
    two hits shows, unchanged, between random entries."""
    from yolov6.utils.track import PlateTrackerNp
    p = ALL_ON
    rng = np.random.default_rng(5)
    trk, ended, live = PlateTrackerNp(p['n_streams'], **p['track']), [], []
    for det, count, stream_of, flush, _ in calls:
        _, _, ei, _, ec = trk.update(det, count, stream_of, flush, p['max_ended'])
        ended += [ei[s, j, 4:] for s in range(p['n_streams']) for j in range(min(int(ec[s]), p['max_ended']))]
        live += [trk.read(s, t)[0] for s, t in np.argwhere(trk.hits >= 2)]
    rows = []
    for r in ended[::2] + live[::3]:
        if ((r >= 0) & (r < 64)).all():
            rows += [r, rng.integers(0, 24, 8)]
    return np.array(rows, np.uint8).reshape(-1, 8)


def all_on_case():
    """(calls, watchlist entries, confusion table) of the all-on tests, made once per process and never modified."""
    if 'case' not in _all_on_cache:
        from yolov6.utils.watch import confuse_table
        calls = all_on_scene(ALL_ON['seed'])
        _all_on_cache['case'] = (calls, all_on_watchlist(calls), confuse_table([(1, 2), (3, 8), (0, 13)], weight=3))
    return _all_on_cache['case']


def all_on_features(features):
    """``features`` with what they need, in the order of ALL_ON_FEATURES."""
    on = set(features)
    for f in features:
        on |= set(ALL_ON_NEEDS.get(f, ()))
    assert on <= set(ALL_ON_FEATURES), on
    return tuple(f for f in ALL_ON_FEATURES if f in on)


class AllOnNp:
    """The numpy chain of one tracker call with ``features`` enabled, in the product's order:
      1. the frames are uploaded into the slots of a ring that every call reuses (``FrameBatcher``);
      2. the tracker's update: rules 1..11, then the watchlist, the live watch and the sightings on the records it ended;
      3. the crops are cut from the uploaded frames; the gallery, then the stack, read them with this call's tid, slot and records;
      4. COPIES of the frames enter the delay line, and the frames that leave it are redacted along the rows released for them.
    ``step`` returns the outputs by name (ALL_ON_OUTPUTS), each a copy.  ``mutant``: one of ALL_ON_MUTANTS."""

    def __init__(self, features=ALL_ON_FEATURES, mutant=None, entries=None, confuse=None):
        from yolov6.utils.best_shot import BestShotNp
        from yolov6.utils.lookback import LookbackNp
        from yolov6.utils.sight import SightLogNp
        from yolov6.utils.track import PlateTrackerNp
        from yolov6.utils.watch import WatchlistNp
        assert mutant is None or mutant in ALL_ON_MUTANTS
        p = ALL_ON
        self.on, self.mutant = all_on_features(features), mutant
        S, T = p['n_streams'], p['track']['max_tracks']
        self.trk = trk = PlateTrackerNp(S, **p['track'])
        self.gal = self.lb = self.log = None
        if entries is None:
            _, entries, confuse = all_on_case()
        wl = WatchlistNp(entries, confuse)
        if 'hold' in self.on:
            trk.enable_hold(**p['hold'])
        if 'watch' in self.on:
            trk.enable_watch(wl, **p['watch'])
        if 'live' in self.on:
            trk.enable_live_watch(wl, p['live']['min_hits'], **p['watch'])
        if 'sight' in self.on:
            self.log = SightLogNp(p['sight_capacity'], S, confuse)
            trk.enable_sightings(self.log, **p['sight'])
        if 'shot' in self.on:
            self.gal = BestShotNp(S, T, p['crop_hw'], p['shot']['min_score'])
        if 'stack' in self.on:
            trk.enable_stack(crop_hw=p['crop_hw'], max_crops=p['max_crops'], min_score=p['shot']['min_score'], **p['stack'])
        if 'lookback' in self.on:
            self.lb = LookbackNp(trk, p['depth'], **p['redact'])
        self.ring = {}                  # slot b of the upload ring -> its persistent array
        self.prev_ended = None          # (ended_i, ended_count) of the previous call
        self.slot_cache = {}            # (B, max_det) -> (tid, slot) as the previous call of that shape left them

    def reset(self, streams):
        """``PlateTracker.reset(streams)`` plus the delay line's: tracker, live memo, stack, gallery, delay line."""
        skip = {'reset_skips_tracker': (self.trk, self.trk._SLOT_ARRAYS + ('frame', 'next_id', 'dropped')),
                'reset_skips_gallery': (self.gal, self.gal._ARRAYS if self.gal is not None else ()),
                'reset_skips_stack': (self.trk._stack['np'], self.trk._stack['np']._ARRAYS) if self.trk._stack is not None else (None, ()),
                'reset_skips_memo': (self.trk._live, ('memo',))}.get(self.mutant, (None, ()))
        kept = {name: getattr(skip[0], name).copy() for name in skip[1]} if skip[0] is not None else {}
        self.trk.reset(streams)
        if self.gal is not None:
            self.gal.reset(streams)
        if self.lb is not None and self.mutant != 'reset_skips_lookback':
            self.lb.reset(streams)
        for name, a in kept.items():
            getattr(skip[0], name)[...] = a

    def step(self, det, count, stream_of, flush, frames):
        from yolov6.utils.redact import redact_plates_np
        p, trk, B = ALL_ON, self.trk, len(det)
        up = []
        for b, fr in enumerate(frames):                                         # 1
            buf = self.ring.get(b)
            if buf is None:
                buf = self.ring[b] = np.empty_like(fr)
            buf[:] = fr
            up.append(buf)
        o = trk.update(det, count, stream_of, flush, p['max_ended'])            # 2
        out = dict(zip(ALL_ON_OUTPUTS['track'], (o[0], o[1], trk.last_slot, o[2], o[3], o[4])))
        if 'hold' in self.on:
            out.update(zip(ALL_ON_OUTPUTS['hold'], trk.last_hold))
            if self.mutant == 'redact_first' and B:                             # the frames are redacted where they lie, before the cut
                for buf, red in zip(up, redact_plates_np(up, trk.last_hold[0], trk.last_hold[1], **p['redact'])[0]):
                    buf[:] = red
        if 'watch' in self.on:
            out['match_i'] = trk.last_watch
        if 'live' in self.on:
            out.update(zip(ALL_ON_OUTPUTS['live'], (trk.last_live,) + tuple(trk.last_live_reads)))
        if 'sight' in self.on:
            out['sight_i'] = trk.last_sight
        ended = (o[2], o[4])
        if self.mutant == 'stale_ended' and self.prev_ended is not None:
            ended = self.prev_ended
        tid, slot = o[1], trk.last_slot
        if self.mutant == 'stale_slot':                                         # the cached buffer of the shape, as it was before this call
            tid, slot = self.slot_cache.get(det.shape[:2], (np.full_like(tid, -1), np.full_like(slot, -1)))
        self.prev_ended, self.slot_cache[det.shape[:2]] = (o[2].copy(), o[4].copy()), (o[1].copy(), trk.last_slot.copy())
        poison = lambda: np.full((p['n_streams'], p['max_ended']) + tuple(p['crop_hw']) + (3,), p['poison'], np.uint8)   # noqa: E731
        if self.gal is not None:                                                # 3
            out.update(zip(ALL_ON_OUTPUTS['shot'], self.gal.update_from_frames(up, det, count, tid, slot, stream_of, ended[0], ended[1],
                                                                                p['max_crops'], shot_crops=poison())))
        if 'stack' in self.on:
            if self.mutant in ('stale_ended', 'stale_slot'):
                res = trk._stack['np'].update_from_frames(up, det, count, tid, slot, stream_of, ended[0], ended[1], p['max_crops'],
                                                          stack_crops=poison())
            else:
                trk._stack['out'][p['max_ended']] = poison()
                res = trk.update_stack(up, det, count, stream_of)
            out.update(zip(ALL_ON_OUTPUTS['stack'], res))
        if self.lb is not None:                                                 # 4
            held = up if self.mutant == 'lookback_no_copy' else [f.copy() for f in up]
            out['released'] = self.lb.push(held, stream_of, flush)
        return {k: ([(s, g, f.copy()) for s, g, f in v] if k == 'released' else np.array(v, copy=True)) for k, v in out.items()}


def all_on_run(features=ALL_ON_FEATURES, mutant=None, reset=True, first=0):
    """The scene's calls from call ``first`` on through a fresh AllOnNp: (chain, [outputs of each call]); ``reset``: with the reset of
    ALL_ON['reset_streams'] in front of call ALL_ON['reset_before']."""
    calls = all_on_case()[0]
    chain, outs = AllOnNp(features, mutant), []
    for c, call in enumerate(calls):
        if c < first:
            continue
        if reset and c == ALL_ON['reset_before']:
            chain.reset(ALL_ON['reset_streams'])
        outs.append(chain.step(*call))
    return chain, outs


def all_on_reference():
    """(chain, outputs per call) of the all-on run with the reset, once per process."""
    if 'ref' not in _all_on_cache:
        _all_on_cache['ref'] = all_on_run()
    return _all_on_cache['ref']


def all_on_differences(a, b, names=None):
    """The names of the outputs in which two runs (lists of step outputs) differ anywhere, sorted; a name only one run has counts."""
    diff = set()
    for x, y in zip(a, b):
        for k in (set(x) | set(y)) if names is None else names:
            if k not in x or k not in y:
                diff.add(k)
            elif k == 'released':
                same = [(s, g) for s, g, _ in x[k]] == [(s, g) for s, g, _ in y[k]] and all(np.array_equal(f, h) for (_, _, f), (_, _, h) in zip(x[k], y[k]))
                if not same:
                    diff.add(k)
            elif x[k].shape != y[k].shape or x[k].dtype != y[k].dtype or x[k].tobytes() != y[k].tobytes():
                diff.add(k)
    return sorted(diff)


def all_on_conditions(seed=None):
    """What the scene of ``seed`` (None: the tests' own) reaches, counted on the all-on numpy chain alone: a dict of counters, each of
    which the CPU test wants above zero before anything else runs."""
    from yolov6.utils.lookback import LookbackNp
    from yolov6.utils.watch_live import alerts_of
    p = ALL_ON
    if seed is None:
        calls, entries, confuse = all_on_case()
    else:
        from yolov6.utils.watch import confuse_table
        calls = all_on_scene(seed)
        entries, confuse = all_on_watchlist(calls), confuse_table([(1, 2), (3, 8), (0, 13)], weight=3)
    chain = AllOnNp(entries=entries, confuse=confuse)
    near = LookbackNp(chain.trk, p['depth'], max_back=0, **p['redact'])          # the same delay line without the frames before the first detection
    n = dict(by_age=0, by_flush=0, overflow=0, held=0, back_before_first=0, shot_replaced=0, stack_n2=0, watch_hit=0, alert=0, resighting=0,
             slot_64=0, split=0, untracked=0, idle_flush=0, dropped=0, shot_valid=0, cut_with_entry=0)
    for c, (det, count, stream_of, flush, frames) in enumerate(calls):
        if c == p['reset_before']:
            chain.reset(p['reset_streams'])
            near.reset(p['reset_streams'])
        live_before = [int(chain.trk.live(s).sum()) for s in range(p['n_streams'])]
        o = chain.step(det, count, stream_of, flush, frames)
        near.push([f.copy() for f in frames], stream_of, flush)
        ec = o['ended_count']
        n['overflow'] += int((ec > p['max_ended']).sum())
        n['held'] += int((o['count_hold'] - np.clip(count, 0, p['max_det'])).sum())
        n['watch_hit'] += int((o['match_i'][..., 0] >= 0).sum())
        n['alert'] += len(alerts_of(o['live_i']))
        n['resighting'] += int((o['sight_i'][..., 0] >= 0).sum())
        n['stack_n2'] += int(((o['stack_i'][..., 3] == 1) & (o['stack_i'][..., 0] >= 2)).sum())
        n['shot_valid'] += int(o['shot_i'][..., 3].sum())
        n['slot_64'] += int((chain.trk.hits[:, 64:] > 0).sum())                   # live after the call
        n['untracked'] += sum(1 for s in stream_of if s < 0)
        n['idle_flush'] += sum(1 for s in range(p['n_streams']) if flush[s] and s not in stream_of and live_before[s] > 0)
        n['by_flush'] += sum(int(ec[s]) for s in range(p['n_streams']) if flush[s] and s not in stream_of)
        n['by_age'] += sum(int(ec[s]) for s in range(p['n_streams']) if not flush[s])
        if len(stream_of) > 64:
            n['split'] += sum(1 for s in range(p['n_streams']) if s in stream_of[:64] and s in stream_of[64:])
    n['back_before_first'] = chain.lb.stats['back_rows'] - near.stats['back_rows']
    n['shot_replaced'] = chain.gal.stats['replaced']
    n['dropped'] = int(chain.trk.dropped.sum())
    n['cut_with_entry'] = int((chain.gal.idp1 != 0).sum())
    return n


# The Inferer with every flag (tests/test_all_on_cpu.py on the CPU path, tests/test_all_on_gpu.py on the GPU paths): feature sets of
# tools/infer.py's keywords; 'all' is their union.  A watchlist file is added to 'watch' and 'live' by ``all_on_infer``.
INFER_CROP = (16, 48)
INFER_SETS = {
    'crops': dict(save_crops=True),
    'shots': dict(best_shots=True),
    'stacks': dict(best_shots=True, stack_shots=True, stack_search=1, stack_max_frames=4, stack_min_width=8.0),
    'sightings': dict(sightings=4, sight_window=12, sight_mismatch=8),
    'watch': dict(), 'live': dict(watch_live=True, watch_live_min_hits=2),
    'hold': dict(redact='mosaic', redact_cell=8, redact_hold=True),
    'lookback': dict(redact='mosaic', redact_cell=8, redact_hold=True, redact_lookback=4),
}
INFER_FRAMES = 12


def all_on_infer_source(tmp):
    """(checkpoint, image folder) under ``tmp``: the tiny synthetic yololps and twelve 128 x 160 frames of ``test_sight_cpu.
    blinking_frames`` (the plate is hidden for four frames: its track breaks and comes back)."""
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    import test_sight_cpu as SC
    m = build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5)
    torch.save({'model': m.half(), 'ema': None, 'epoch': 0}, str(tmp / 'tiny.pt'))
    (tmp / 'imgs').mkdir()
    for k, f in enumerate(SC.blinking_frames(INFER_FRAMES, range(3, 7))):
        Image.fromarray(f).save(str(tmp / 'imgs' / ('f%02d.png' % k)))
    return tmp / 'tiny.pt', tmp / 'imgs'


def files_under(root):
    """{path relative to ``root``: bytes} of every file below it."""
    out = {}
    for d, _, names in os.walk(str(root)):
        for n in names:
            p = os.path.join(d, n)
            with open(p, 'rb') as f:
                out[os.path.relpath(p, str(root))] = f.read()
    return out


def all_on_infer(infer, tmp, ckpt, src, tag, names=None, **kw):
    """``infer.run`` with the sets ``names`` of INFER_SETS alone (default: tracking alone and every set) and with all of INFER_SETS at
    once, under ``tmp / tag``: {set name: its files}.  The plates.txt of the first run gives the watchlist: the first read, the last
    read with a wildcard, one read that nothing shows."""
    base = dict(weights=str(ckpt), source=str(src), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
                not_save_img=True, save_txt=True, track=True, track_max_age=2, track_iou=0.25, track_expand=0.25, crop_size=INFER_CROP)
    base.update(kw)
    root, out = tmp / tag, {}
    sets = dict(INFER_SETS, track={})
    names = (('track',) + tuple(INFER_SETS)) if names is None else tuple(names)
    assert 'watchlist' not in sets[names[0]] and names[0] not in ('watch', 'live')
    for name in names + ('all',):
        s = {k: v for n in INFER_SETS for k, v in sets[n].items()} if name == 'all' else dict(sets[name])
        if name in ('watch', 'live', 'all'):
            s['watchlist'] = str(root / 'watch.txt')
        infer.run(save_dir=str(root / name), **dict(base, **s))
        out[name] = files_under(root / name)
        if name == names[0]:
            reads = [line.split()[4:12] for line in out[name]['plates.txt'].decode().splitlines()]
            assert reads, 'the run ended no track'
            rows = [reads[0], ['255'] + reads[-1][1:], [str((int(v) + 5) % 24) for v in reads[0]]]
            (root / 'watch.txt').write_text('\n'.join(' '.join(r) for r in rows) + '\n')
    return out


def assert_all_on_files(files, what=''):
    """Every file of every single-feature run is byte-identical in the all-on run (of the hold-only run all but the redacted frames,
    which the look-back redacts further); every feature left something to compare.  -> {set name: files compared}."""
    both = files['all']
    n = {}
    for name, own in files.items():
        if name == 'all':
            continue
        names = [p for p in own if not (name == 'hold' and p.startswith('redacted' + os.sep))]
        missing = [p for p in names if p not in both]
        assert not missing, '%s %s: the all-on run has no %s' % (what, name, missing[:4])
        differ = [p for p in names if own[p] != both[p]]
        assert not differ, '%s %s: %d of %d files differ in the all-on run, first %s' % (what, name, len(differ), len(names), sorted(differ)[:4])
        n[name] = len(names)
    has = lambda pre: sum(1 for p in both if p.startswith(pre))                 # noqa: E731
    assert has('shots' + os.sep) >= 1 and has('stacks' + os.sep) >= 1 and has('redacted' + os.sep) == INFER_FRAMES, (what, sorted(both)[:8])
    assert has(os.path.join('imgs', 'crops') + os.sep) >= INFER_FRAMES // 2
    for name in ('hits.txt', 'alerts.txt', 'resightings.txt', 'plates.txt', 'tracks.txt', 'shots.txt', 'stacks.txt'):
        assert both[name].strip(), '%s: %s of the all-on run is empty' % (what, name)
    return n


def all_on_stream_part(out, stream_of, s):
    """The part of one step's outputs that belongs to stream ``s``: the rows of its frames, its lines of the per-stream outputs and
    the frames it released; the sightings (one log for all streams) are left out."""
    rows = [b for b, v in enumerate(stream_of) if v == s]
    part = {}
    for k, v in out.items():
        if k == 'released':
            part[k] = [(t, g, f) for t, g, f in v if t == s]
        elif k in ('det_out', 'tid', 'slot', 'det_hold', 'count_hold', 'tid_hold'):
            part[k] = v[rows]
        elif k != 'sight_i':
            part[k] = v[s]
    return part
