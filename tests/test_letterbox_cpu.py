"""The letterbox's resize rule against its definition, on the CPU.  ``resize_linear_u8`` (yolov6/data/data_augment.py) restates
OpenCV's 8-bit INTER_LINEAR fixed-point scheme; every kernel and every numpy specification of the letterbox is built on it.  Here
it is held to ``lp_testing.bilinear64``, a float64 bilinear written from the definition, within a bar derived from the scheme:

    the scheme, per channel:  h_y = t(y, x0) * a0 + t(y, x1) * a1                     (horizontal pass, scaled by 2048)
                              S   = (b0 * (h_y0 >> 4) >> 16) + (b1 * (h_y1 >> 4) >> 16)  (quarter levels)
                              out = (S + 2) >> 2
    weights    a1 = rint(f * 2048), a0 = rint((1 - f) * 2048), a0 + a1 = 2048 (asserted below), f the fraction of the float32
               source coordinate.  |a1 / 2048 - f_true| <= 0.5 / 2048 + e32, e32 = half a float32 ulp of the coordinate
               <= spacing(src) / 2: 2^-13 for a source of 2048..4095 px, 2^-12 from 4096 on, as much as the 11-bit step itself.
               The interpolant is continuous in the coordinate, so a coordinate rounded across an integer (another index pair) or
               across a clamp costs no more than its distance.  A blend of two values in 0..255 moves by <= 255 * that: 0.062 level
               per axis for small sources; the vertical blend is a convex combination of two such rows plus its own error.
    >> 4       loses < 1 unit of 1/128 level per row, weighted by b0 / 2048 and b1 / 2048, which sum to 1: < 1/128 in all
    >> 16      twice, each loses < 1 quarter level: < 1/2 in all; only ever downwards
    (+2) >> 2  S is an INTEGER number of quarter levels, so out - S / 4 is one of 0, -1/4, +1/4, +1/2 (not any value in +-1/2)
    hence      -(1/4 + 1/2 + 1/128 + 255 (dx + dy)) <= restatement - bilinear64 <= 1/2 + 255 (dx + dy),
               d = 0.5 / 2048 + spacing(src) / 2 per axis: [-0.886, +0.628] for a source of 97 x 131, [-0.945, +0.687] for one of 40 x 4100.
The lower end is 1/4 tighter than the sum of one "+-0.5 rounding" and the truncations, because of the quarter-level step; the
>> 4 term is 1/128, not 2/128, because the two rows' weights sum to one.  Observed extremes per case go to letterbox_cpu.log in
the suite's log folder; they are figures, the bar is ``lp_testing.linear_u8_bar``."""
import functools
import os

import numpy as np
import pytest

import lp_testing as T
from yolov6.data import data_augment
from yolov6.data.data_augment import _linear_coef, letterbox, letterbox_geometry, resize_linear_u8

LOG_NAME = 'letterbox_cpu.log'

# (source (h, w), destination (h, w))
CASES = [
    ((1, 1), (5, 7)), ((1, 37), (4, 90)), ((37, 1), (90, 3)), ((1, 37), (3, 11)), ((2, 2), (7, 9)), ((2, 2), (1, 1)),
    ((5, 7), (48, 67)), ((5, 8), (48, 77)), ((3, 4), (40, 50)),               # enlargements up to 12.5x: runs of clamped pixels at both ends
    ((700, 900), (33, 42)), ((400, 1000), (11, 29)),                          # reductions of 21x and 34x
    ((40, 4100), (3, 260)), ((8, 4100), (8, 4099)), ((4, 4100), (5, 6000)),   # beyond 4096 columns: float32 coordinates in steps of 2^-11
    ((6, 9000), (6, 9001)),
    ((97, 131), (98, 73)), ((97, 131), (96, 132)), ((131, 97), (130, 98)),    # sizes that differ by one
    ((1160, 720), (640, 397)), ((300, 500), (250, 416)), ((2000, 1500), (640, 480)),   # the resizes of test_preprocess_letterbox_
    ((480, 640), (480, 640)), ((640, 640), (640, 640)),                       # matches_host_mirror; two of its five are ratio 1
    ((300, 1700), (46, 260)), ((2160, 3840), (234, 416)),
]
CONTENTS = ('noise', 'zeros', 'full', 'checker', 'ramp_x', 'ramp_y')


def _content(kind, h, w, seed):
    if kind == 'noise':
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind in ('zeros', 'full'):
        return np.full((h, w, 3), 0 if kind == 'zeros' else 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'checker':
        v = ((yy + xx) & 1) * 255
    else:
        n, i = (w, xx) if kind == 'ramp_x' else (h, yy)
        v = i * 255 // max(n - 1, 1)
    return np.stack([v, 255 - v, v], -1).astype(np.uint8)                      # the channels are not all alike


def _id(case):
    return '%dx%d-%dx%d' % (case[0] + case[1])


def _log(line):
    with open(os.path.join(T.log_dir(), LOG_NAME), 'a') as f:
        f.write(line + '\n')


def test_the_bar_of_a_small_source_is_what_the_derivation_gives():
    lo, hi = T.linear_u8_bar((97, 131))
    w = 2 * 255 * (0.5 / 2048 + 2.0 ** -17 / 2)                                # spacing(float32) is 2^-17 in [64, 128), 2^-16 in [128, 256)
    assert -(0.7578125 + w + 255 * 2.0 ** -18 + 1e-6) < lo < -(0.7578125 + w) and 0.5 + w < hi < 0.5 + w + 255 * 2.0 ** -18 + 1e-6
    assert -0.8853 < lo < -0.8852 and 0.6274 < hi < 0.6275


def _outside(got_u8, ref64, bar):
    """How many pixels of ``got_u8 - ref64`` leave the bar, and the extremes of the difference."""
    d = got_u8.astype(np.float64) - ref64
    return int(((d < bar[0]) | (d > bar[1])).sum()), float(d.min()), float(d.max())


@functools.lru_cache(maxsize=None)
def _weights_sum_to_2048(dst, src):
    _, _, a0, a1 = _linear_coef(dst, src)
    return bool((a0 + a1 == 2048).all() and (a0 >= 0).all() and (a1 >= 0).all())


# ---- a. the bound ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_restatement_stays_within_the_derived_bar_of_the_float64_definition(case):
    (h, w), (nh, nw) = case
    assert _weights_sum_to_2048(nw, w) and _weights_sum_to_2048(nh, h)         # the derivation relies on it
    bar = T.linear_u8_bar((h, w))
    lo, hi = 0.0, 0.0
    for k, kind in enumerate(CONTENTS):
        im = _content(kind, h, w, 100 + k)
        ref = T.bilinear64(im, (nw, nh))
        got = resize_linear_u8(im, (nw, nh))
        assert got.shape == (nh, nw, 3) and got.dtype == np.uint8
        bad, dmin, dmax = _outside(got, ref, bar)
        _log('%-22s %-8s restatement - float64 in [%+.4f, %+.4f]  bar [%+.4f, %+.4f]' % (_id(case), kind, dmin, dmax, bar[0], bar[1]))
        assert bad == 0, (kind, dmin, dmax, bar)
        assert int(np.abs(got.astype(np.int64) - np.rint(ref).astype(np.int64)).max()) <= 1, kind
        assert _outside(np.rint(ref).astype(np.uint8), ref, bar)[0] == 0       # the bar admits the correctly rounded definition
        lo, hi = min(lo, dmin), max(hi, dmax)
    _log('%-22s %-8s restatement - float64 in [%+.4f, %+.4f]' % (_id(case), 'all', lo, hi))


# ---- d. the bound can fail --------------------------------------------------------------------------------------------------------
WRONG = {'no half-pixel offset': lambda d, src, dst: d * src / dst,
         'align-corners': lambda d, src, dst: d * (src - 1) / max(dst - 1, 1)}


def _wrong_rule_reach(case):
    """An upper limit, in grey levels, of how far either wrong rule can move a pixel of the float64 result: each shifts the
    coordinate of an axis by at most |src / dst - 1| / 2 source pixels (none on an axis of one source pixel), and a pixel of
    shift moves a blend of 0..255 values by at most 255."""
    (h, w), (nh, nw) = case
    return sum(127.5 * abs(s / d - 1.0) for s, d in ((h, nh), (w, nw)) if s > 1)


def _detectable(case):
    """After its own rounding (0.5) a wrong rule can leave the bar only if its reach exceeds hi - 0.5.  The two cases that
    resize 4100 -> 4099 and 9000 -> 9001 px fall short of that (reach 0.03 and 0.014 level): no test can tell those rules apart
    there.  Every other resized case must reject both."""
    return _wrong_rule_reach(case) + 0.5 > T.linear_u8_bar(case[0])[1]


def test_which_cases_can_tell_a_wrong_rule():
    assert [c for c in CASES if not _detectable(c)] == [((1, 1), (5, 7)), ((8, 4100), (8, 4099)), ((6, 9000), (6, 9001)),
                                                        ((480, 640), (480, 640)), ((640, 640), (640, 640))]


@pytest.mark.parametrize('case', [c for c in CASES if _detectable(c)], ids=_id)
@pytest.mark.parametrize('rule', sorted(WRONG))
def test_the_bar_rejects_a_wrong_coordinate_rule(case, rule):
    """The two classic mistakes, correctly rounded from float64, on the inputs of the bound test: each leaves the bar (on the noise,
    the checkerboard or a ramp; constant images cannot tell any two resizes apart)."""
    (h, w), (nh, nw) = case
    bar = T.linear_u8_bar((h, w))
    rejected = {}
    for k, kind in enumerate(CONTENTS):
        im = _content(kind, h, w, 100 + k)
        wrong = np.rint(T.bilinear64(im, (nw, nh), coord=WRONG[rule])).astype(np.uint8)
        bad, dmin, dmax = _outside(wrong, T.bilinear64(im, (nw, nh)), bar)
        rejected[kind] = bad
        if kind in ('zeros', 'full'):
            assert bad == 0
    _log('%-22s wrong rule %-22s pixels outside the bar: %s' % (_id(case), rule, rejected))
    assert max(rejected.values()) > 0, rejected


# ---- b. exact properties ----------------------------------------------------------------------------------------------------------
def test_equal_size_returns_the_source():
    for h, w in ((1, 1), (2, 2), (33, 60), (97, 131), (16, 4100)):
        im = _content('noise', h, w, h + w)
        assert np.array_equal(resize_linear_u8(im, (w, h)), im)
        for axis_only in ((w, 2 * h + 1), (3 * w + 2, h)):                     # one axis unresized: that axis blends nothing
            got = resize_linear_u8(im, axis_only)
            ref = T.bilinear64(im, axis_only)
            assert _outside(got, ref, T.linear_u8_bar((h, w)))[0] == 0


def test_exact_halving_is_the_rounded_mean_of_four():
    for h, w in ((2, 2), (4, 6), (96, 130), (10, 8200)):
        for kind in ('noise', 'checker', 'full', 'ramp_x'):
            im = _content(kind, h, w, 7).astype(np.int32)
            want = (im[0::2, 0::2] + im[0::2, 1::2] + im[1::2, 0::2] + im[1::2, 1::2] + 2) >> 2
            assert np.array_equal(resize_linear_u8(im.astype(np.uint8), (w // 2, h // 2)), want.astype(np.uint8)), (h, w, kind)


def test_constant_images_stay_constant_and_one_pixel_fills():
    for (h, w), (nh, nw) in CASES[:18]:
        for v in (0, 1, 113, 114, 127, 128, 254, 255):
            got = resize_linear_u8(np.full((h, w, 3), v, np.uint8), (nw, nh))
            assert got.shape == (nh, nw, 3) and bool((got == v).all()), (h, w, nh, nw, v)
    px = np.array([[[3, 250, 114]]], np.uint8)
    for nh, nw in ((1, 1), (5, 7), (1, 300), (300, 1), (48, 260)):
        assert np.array_equal(resize_linear_u8(px, (nw, nh)), np.broadcast_to(px, (nh, nw, 3)))


def _mirror_equivalent(dst, src):
    """Per destination index d: does the coefficient table give d and its mirror image dst - 1 - d mirrored taps with swapped
    weights?  (A tap of weight 0 does not count: an index pair (s, s + 1) with weights (2048, 0) is the pair (s - 1, s) with
    (0, 2048).)  The coordinate of the mirror image is src - 1 - c in exact arithmetic, but both are rounded to float32 where
    the scheme takes their fraction, at different magnitudes: the 11-bit weight of some d is one unit off its mirror's."""
    s0, s1, a0, a1 = _linear_coef(dst, src)

    def taps(i0, i1, w0, w1):
        """Per destination index: {source index: weight}, taps of weight 0 left out."""
        out = []
        for d in range(dst):
            t = {}
            for i, w in ((int(i0[d]), int(w0[d])), (int(i1[d]), int(w1[d]))):
                if w:
                    t[i] = t.get(i, 0) + w
            out.append(t)
        return out

    mirrored = taps((src - 1 - s1)[::-1], (src - 1 - s0)[::-1], a1[::-1], a0[::-1])
    return np.array([a == b for a, b in zip(taps(s0, s1, a0, a1), mirrored)])


# coordinates that float32 holds exactly in both orientations: enlargements by 2 and 8, reductions by 2, 3 and 4
EXACT_FLIP_CASES = [((6, 10), (12, 20)), ((5, 7), (40, 56)), ((96, 130), (48, 65)), ((63, 30), (21, 10)), ((64, 4104), (16, 1026)), ((1, 37), (1, 74))]


@pytest.mark.parametrize('case', EXACT_FLIP_CASES + CASES[:21], ids=_id)
def test_resize_commutes_with_flips(case):
    """Bit for bit wherever a destination index and its mirror image get mirrored coefficients: everywhere for the scales whose
    coordinates float32 holds exactly, and on most rows and columns otherwise (fewer the wider the source: from 4096 px on a
    float32 ulp is a whole weight step).  On the others the flipped result is within one level: the scheme itself (OpenCV's, which takes the fraction of a float32 coordinate) is not mirror-symmetric."""
    (h, w), (nh, nw) = case
    mx, my = _mirror_equivalent(nw, w), _mirror_equivalent(nh, h)
    if case in EXACT_FLIP_CASES:
        assert mx.all() and my.all()
    for kind in ('noise', 'checker'):
        im = _content(kind, h, w, 11)
        base = resize_linear_u8(im, (nw, nh)).astype(np.int32)
        hf = resize_linear_u8(im[:, ::-1], (nw, nh))[:, ::-1].astype(np.int32)
        vf = resize_linear_u8(im[::-1], (nw, nh))[::-1].astype(np.int32)
        assert np.array_equal(hf[:, mx], base[:, mx]) and np.array_equal(vf[my], base[my]), kind
        assert int(np.abs(hf - base).max()) <= 1 and int(np.abs(vf - base).max()) <= 1, kind
    _log('%-22s flips: %d of %d columns and %d of %d rows have a weight one unit off their mirror image\'s'
         % (_id(case), int((~mx).sum()), nw, int((~my).sum()), nh))


def test_source_indices_are_monotone_and_inside():
    pairs = set()
    for (h, w), (nh, nw) in CASES:
        pairs |= {(nh, h), (nw, w)}
    pairs |= {(d, s) for s in (1, 2, 3, 7, 640, 4097) for d in (1, 2, 5, 640, 641, 5000)}
    for dst, src in sorted(pairs):
        s0, s1, a0, a1 = _linear_coef(dst, src)
        assert s0.shape == (dst,) and int(s0.min()) >= 0 and int(s1.max()) <= src - 1, (dst, src)
        assert bool((np.diff(s0) >= 0).all()) and bool((np.diff(s1) >= 0).all()), (dst, src)
        assert bool(((s1 == s0 + 1) | (s1 == src - 1)).all()), (dst, src)
        assert bool((a0 + a1 == 2048).all()) and int(a1.min()) >= 0 and int(a1.max()) <= 2048, (dst, src)
        assert bool((a1[s0 == src - 1] == 0).all()), (dst, src)                # a clamped tap takes no weight from its neighbour


# ---- c. a second witness ----------------------------------------------------------------------------------------------------------
def test_enlargements_agree_with_pil_bilinear_within_one_level():
    from PIL import Image
    probe = np.array([[0, 255]], np.uint8)
    if not np.array_equal(np.asarray(Image.fromarray(probe).resize((4, 1), Image.BILINEAR)), np.array([[0, 64, 191, 255]], np.uint8)):
        pytest.skip('this PIL does not resize (0, 255) -> 4 px to 0, 64, 191, 255: not the half-pixel-centre bilinear of its documentation')
    for (h, w), (nh, nw) in [c for c in CASES if c[1][0] >= c[0][0] and c[1][1] >= c[0][1] and c[0][0] * c[0][1] <= 200000]:
        for k, kind in enumerate(('noise', 'checker', 'ramp_x')):
            im = _content(kind, h, w, 300 + k)
            pil = np.asarray(Image.fromarray(im).resize((nw, nh), Image.BILINEAR))
            d = int(np.abs(pil.astype(np.int32) - resize_linear_u8(im, (nw, nh)).astype(np.int32)).max())
            _log('%-22s %-8s |restatement - PIL| max %d' % (_id(((h, w), (nh, nw))), kind, d))
            assert d <= 1, (h, w, nh, nw, kind)


# ---- e. letterbox() as a whole ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('auto', [False, True])
def test_letterbox_places_the_resize_in_its_rectangle(auto, monkeypatch):
    monkeypatch.setattr(data_augment, 'cv2', None)                             # the fixed-point scheme, wherever the suite runs
    calls = []
    monkeypatch.setattr(data_augment, 'resize_linear_u8', lambda im, wh: calls.append(wh) or resize_linear_u8(im, wh))
    shapes = [((1160, 720), [640, 640]), ((480, 640), [640, 640]), ((640, 640), [640, 640]), ((300, 500), [320, 416]),
              ((2000, 1500), [640, 640]), ((5, 7), [48, 260]), ((1, 1), [33, 98]), ((300, 1700), [48, 260]), ((33, 60), [33, 98]),
              ((97, 131), [96, 128])]
    for (h, w), size in shapes:
        im = _content('noise', h, w, h * w)
        del calls[:]
        out, r, (dw, dh) = letterbox(im, size, auto=auto, stride=32)
        r2, (rw, rh), (top, bottom, left, right), (dw2, dh2) = letterbox_geometry((h, w), size, auto=auto, stride=32)
        assert (r, dw, dh) == (r2, dw2, dh2) and out.dtype == np.uint8
        assert out.shape == (rh + top + bottom, rw + left + right, 3)
        if auto:
            assert out.shape[0] <= size[0] and out.shape[1] <= size[1] and top + bottom < 32 and left + right < 32
        else:
            assert out.shape[:2] == tuple(size)
        inside = np.zeros(out.shape[:2], bool)
        inside[top:top + rh, left:left + rw] = True
        assert bool((out[~inside] == 114).all())
        if (rh, rw) == (h, w):
            assert calls == [] and np.array_equal(out[inside].reshape(rh, rw, 3), im)
        else:
            assert calls == [(rw, rh)]
            want = resize_linear_u8(im, (rw, rh))
            assert np.array_equal(out[inside].reshape(rh, rw, 3), want)
            assert _outside(want, T.bilinear64(im, (rw, rh)), T.linear_u8_bar((h, w)))[0] == 0
        got2, _, (l2, t2) = letterbox(im, size, auto=auto, stride=32, return_int=True)
        assert (l2, t2) == (left, top) and np.array_equal(got2, out)
