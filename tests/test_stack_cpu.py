"""One denoised picture per plate track on the CPU: ``StackNp`` (yolov6/utils/stack.py), the specification of lp_stack_update,
against a plain-loop restatement over Python integers, the quality the feature is there for, the edges of the rule, the numpy
tracker's ``enable_stack``, the argument checks of the C entry point and ``tools/infer.py --stack-shots`` on the CPU path.
"""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import test_track_cpu as C
import test_best_shot_cpu as S

LP_ERR_ARG = -1
f32 = np.float32
SIGMA = 16.0


# ---- the rule once more, in plain loops over Python integers -------------------------------------------------------------------
class StackLoops:
    """The rules of yolov6/utils/stack.py restated without numpy arithmetic: every value a Python int.  ``cost_bits``: keep only so
    many low bits of every cost (64: the rule; 32: what a 32-bit accumulator would make of it)."""

    def __init__(self, S_, T, crop_hw, search=2, max_frames=64, min_score=0.0, min_width=0.0, min_sharp=0, cost_bits=64):
        self.S, self.T, (self.Hc, self.Wc) = S_, T, crop_hw
        self.R, self.max_frames, self.min_score, self.min_width, self.min_sharp = search, max_frames, min_score, min_width, min_sharp
        self.cost_bits = cost_bits
        self.frame = [0] * S_
        self.entry = [[dict(idp1=0, n=0, first=0, last=0, acc=None) for _ in range(T)] for _ in range(S_)]
        self.shifts = []

    def _acc(self, en):
        if en['acc'] is None:
            en['acc'] = [[[0, 0, 0] for _ in range(self.Wc)] for _ in range(self.Hc)]
        return en['acc']

    def candidates(self):
        R = self.R
        out = []
        for d2 in range(2 * R * R + 1):
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    if dy * dy + dx * dx == d2:
                        out.append((dy, dx))
        return out

    def costs(self, crop, acc, n):
        R, Hc, Wc = self.R, self.Hc, self.Wc
        y = lambda p: 29 * int(p[0]) + 150 * int(p[1]) + 77 * int(p[2])   # noqa: E731
        out = []
        for dy, dx in self.candidates():
            c = 0
            for i in range(R, Hc - R):
                for j in range(R, Wc - R):
                    c += abs(n * y(crop[i + dy][j + dx]) - y(acc[i][j]))
            out.append(c & ((1 << self.cost_bits) - 1))
        return out

    def align(self, crop, acc, n):
        R = self.R
        if n == 0 or R == 0 or self.Hc <= 2 * R or self.Wc <= 2 * R:
            return 0, 0
        costs, best = self.costs(crop, acc, n), 0
        for k in range(1, len(costs)):
            if costs[k] < costs[best]:
                best = k
        return self.candidates()[best]

    def retire(self, s, g, ids, stack_crops, stack_i):
        en = self.entry[s][g]
        e = next((k for k, v in enumerate(ids) if v == en['idp1'] - 1), None)
        n = en['n']
        if e is not None and n >= 1:
            for i in range(self.Hc):
                for j in range(self.Wc):
                    for c in range(3):
                        stack_crops[s, e, i, j, c] = (en['acc'][i][j][c] + (n >> 1)) // n
            stack_i[s, e] = (n, en['first'], en['last'], 1)
        en['idp1'] = en['n'] = 0

    def update(self, inp, stack_crops):
        det, count, tid, slot = inp['det'], inp['count'], inp['tid'], inp['slot']
        crops, status, sharp = inp['crops'], inp['status'], inp['sharp']
        ended_i, ended_count = inp['ended_i'], inp['ended_count']
        max_det, max_crops, max_ended = det.shape[1], crops.shape[1], ended_i.shape[1]
        stack_i = np.zeros((self.S, max_ended, 4), np.int32)
        ids = [[int(v) for v in ended_i[s, :min(max(int(ended_count[s]), 0), max_ended), 0]] for s in range(self.S)]
        self.shifts = []
        for b, s in enumerate(inp['stream_of']):
            if s < 0:
                continue
            for r in range(min(max(int(count[b]), 0), max_det, max_crops, 128)):
                t, g = int(tid[b, r]), int(slot[b, r])
                if t < 0 or not 0 <= g < self.T:
                    continue
                en = self.entry[s][g]
                if en['idp1'] != t + 1:
                    if en['idp1'] != 0:
                        self.retire(s, g, ids[s], stack_crops, stack_i)
                    en['idp1'], en['n'] = t + 1, 0
                row = det[b, r]
                with np.errstate(all='ignore'):
                    sc = row[12] + row[13]
                    for c in range(14, 20):
                        sc = sc + row[c]
                    sc = float(sc / f32(8.0))
                    width = float(row[2] - row[0])
                if int(status[b, r]) != 1 or not sc >= self.min_score or not width >= self.min_width or int(sharp[b, r]) < self.min_sharp \
                        or en['n'] >= self.max_frames:
                    continue
                crop, acc, n = crops[b, r].tolist(), self._acc(en), en['n']
                dy, dx = self.align(crop, acc, n)
                for i in range(self.Hc):
                    si = min(max(i + dy, 0), self.Hc - 1)
                    for j in range(self.Wc):
                        sj = min(max(j + dx, 0), self.Wc - 1)
                        for c in range(3):
                            acc[i][j][c] = crop[si][sj][c] + (acc[i][j][c] if n else 0)
                if n == 0:
                    en['first'] = self.frame[s]
                en['n'], en['last'] = n + 1, self.frame[s]
                self.shifts.append((s, g, t, dy, dx))
            self.frame[s] += 1
        for s in range(self.S):
            for g in range(self.T):
                en = self.entry[s][g]
                if en['idp1'] != 0 and en['idp1'] - 1 in ids[s]:
                    self.retire(s, g, ids[s], stack_crops, stack_i)
        return stack_crops, stack_i


# ---- random cases (shared with the GPU tests): the inputs of test_best_shot_cpu.shot_case through StackNp --------------------------
# parallel to S.SHOT_CASES: the stack's parameters per case
STACK_KW = [
    dict(search=2, max_frames=64, min_score=0.3, min_width=0.0, min_sharp=0),
    dict(search=1, max_frames=2, min_score=0.0, min_width=0.0, min_sharp=0),         # entries fill up
    dict(search=2, max_frames=64, min_score=0.0, min_width=40.0, min_sharp=3),       # width and sharpness thresholds
    dict(search=2, max_frames=64, min_score=0.3, min_width=0.0, min_sharp=0),        # 64 x 192, max_crops < max_det, truncation
]


def snapshot(stk):
    return {name: getattr(stk, name).copy() for name in stk._ARRAYS}


def stack_case(k):
    """Case k of ``S.SHOT_CASES`` for the stack: (StackNp after the calls, calls) with calls[c] = (inputs dict, (stack_crops,
    stack_i) of StackNp on stack_crops poisoned with 0xAB, the state arrays after the call)."""
    from yolov6.utils.stack import StackNp
    seed, n_streams, T, max_det, Bs, crop_hw, max_crops, max_ended, kw = S.SHOT_CASES[k]
    _, shot_calls = S.shot_case(seed, n_streams, T, max_det, Bs, crop_hw, max_crops, max_ended, **kw)
    stk = StackNp(n_streams, T, crop_hw, **STACK_KW[k])
    calls = []
    for inp, _ in shot_calls:
        if k == 1:
            inp['status'] = np.minimum(inp['status'], 1)      # every counted row is rectified: the entries fill up
        poison = np.full((n_streams, max_ended) + tuple(crop_hw) + (3,), 0xAB, np.uint8)
        want = stk.update(inp['det'], inp['count'], inp['tid'], inp['slot'], inp['crops'], inp['status'], inp['sharp'], inp['stream_of'],
                          inp['ended_i'], inp['ended_count'], stack_crops=poison)
        calls.append((inp, want, snapshot(stk)))
    return stk, calls


def check_stack_case(k, stk, calls):
    """What case k is there for happened."""
    st = stk.stats
    assert st['summed'] > 0 and st['with_stack'] > 0 and st['without_stack'] > 0, st
    if STACK_KW[k]['search'] > 0:
        assert st['shifted'] > 0, st
    if k == 0:
        assert st['reused'] > 0, st
    if k == 1:
        assert st['full'] > 0, st
    if k == 3:
        assert st['truncated'] > 0, st
    for _, (sc, si), _ in calls:
        assert np.all(sc[si[..., 3] == 0] == 0xAB) and set(np.unique(si[..., 3]).tolist()) <= {0, 1}
        assert (si[..., 0][si[..., 3] == 1] >= 1).all() and not si[si[..., 3] == 0].any()


@pytest.mark.parametrize('k', [0, 1, 2], ids=[S.SHOT_IDS[k] for k in (0, 1, 2)])
def test_stack_np_equals_the_plain_loops_on_random_calls(k):
    """(The 64 x 192 case is left to the GPU test: its searches take minutes in plain loops.)"""
    seed, n_streams, T, max_det, Bs, crop_hw, max_crops, max_ended, kw = S.SHOT_CASES[k]
    stk, calls = stack_case(k)
    check_stack_case(k, stk, calls)
    ref = StackLoops(n_streams, T, crop_hw, **STACK_KW[k])
    for c, (inp, (sc, si), state) in enumerate(calls):
        got_c, got_i = ref.update(inp, np.full_like(sc, 0xAB))
        assert np.array_equal(got_i, si) and np.array_equal(got_c, sc), c
        assert ref.frame == state['frame'].tolist()
        for s in range(n_streams):
            for g in range(T):
                en = ref.entry[s][g]
                assert (en['idp1'], en['n']) == (state['idp1'][s, g], state['n'][s, g])
                if en['n']:
                    assert (en['first'], en['last']) == (state['first'][s, g], state['last'][s, g])
                    assert np.array_equal(np.array(en['acc']), state['acc'][s, g])


def test_large_case_exercises_truncation():
    stk, calls = stack_case(3)
    check_stack_case(3, stk, calls)


@pytest.mark.parametrize('R', [0, 1, 2, 3, 4])
def test_stack_candidates(R):
    from yolov6.utils.stack import stack_candidates
    c = stack_candidates(R)
    assert len(c) == (2 * R + 1) ** 2 == len(set(c)) and c[0] == (0, 0)
    assert all(-R <= dy <= R and -R <= dx <= R for dy, dx in c)
    keys = [(dy * dy + dx * dx, dy, dx) for dy, dx in c]
    assert keys == sorted(keys)
    if R >= 1:
        assert c[1:5] == [(-1, 0), (0, -1), (0, 1), (1, 0)]
    assert c == StackLoops(1, 1, (1, 1), search=R).candidates()
    with pytest.raises(ValueError):
        stack_candidates(5)


# ---- one track fed by hand (shared with the GPU tests) ---------------------------------------------------------------------------
def one_track_calls(crops, chunk=None, status=None, rows=None, sharp=None, max_ended=2):
    """The calls that show one track (id 0, slot 0 of one stream) the crops [n, Hc, Wc, 3], ``chunk`` frames per call (default:
    all in one), one row per frame, and then end it: a closing call without frames whose record names id 0.  ``status`` /
    ``sharp`` [n] and ``rows`` [n, 28] default to 1 / 0 / a plate 100 pixels wide of confidence 0.9."""
    crops = np.ascontiguousarray(crops, dtype=np.uint8)
    n = len(crops)
    status = np.ones(n, np.int32) if status is None else np.asarray(status, np.int32)
    sharp = np.zeros(n, np.uint64) if sharp is None else np.asarray(sharp, np.uint64)
    rows = np.stack([C.make_row((10, 10, 110, 40))] * max(n, 1))[:n] if rows is None else np.asarray(rows, f32)
    calls = []
    for a in range(0, n, chunk or max(n, 1)):
        b = min(n, a + (chunk or n))
        B = b - a
        calls.append(dict(det=rows[a:b, None].copy(), count=np.ones(B, np.int32), tid=np.zeros((B, 1), np.int32), slot=np.zeros((B, 1), np.int32),
                          crops=crops[a:b, None].copy(), status=status[a:b, None].copy(), sharp=sharp[a:b, None].copy(), stream_of=[0] * B,
                          ended_i=np.zeros((1, max_ended, 12), np.int32), ended_count=np.zeros(1, np.int32)))
    ei = np.zeros((1, max_ended, 12), np.int32)
    ei[0, 0, 0] = 0
    calls.append(dict(det=np.zeros((0, 1, 28), f32), count=np.zeros(0, np.int32), tid=np.zeros((0, 1), np.int32), slot=np.zeros((0, 1), np.int32),
                      crops=crops[:0, None].copy(), status=status[:0, None].copy(), sharp=sharp[:0, None].copy(), stream_of=[],
                      ended_i=ei, ended_count=np.ones(1, np.int32)))
    return calls


def run_np(stk, calls, poison=0xAB):
    """The calls through ``stk``: [((stack_crops, stack_i), shifts, state)] per call."""
    out = []
    for inp in calls:
        S_, max_ended = stk.n_streams, inp['ended_i'].shape[1]
        buf = np.full((S_, max_ended) + stk.crop_hw + (3,), poison, np.uint8)
        res = stk.update(inp['det'], inp['count'], inp['tid'], inp['slot'], inp['crops'], inp['status'], inp['sharp'], inp['stream_of'],
                         inp['ended_i'], inp['ended_count'], stack_crops=buf)
        out.append((res, list(stk.shifts), snapshot(stk)))
    return out


def stacked(crops, hw=None, **kw):
    """One track through a fresh StackNp: (the picture or None, stack_i line, the shifts of all frames, the StackNp)."""
    from yolov6.utils.stack import StackNp
    call_kw = {k: kw.pop(k) for k in ('chunk', 'status', 'rows', 'sharp') if k in kw}
    crops = np.asarray(crops, np.uint8)
    stk = StackNp(1, 1, hw or crops.shape[1:3], **kw)
    res = run_np(stk, one_track_calls(crops, **call_kw))
    (sc, si), _, _ = res[-1]
    shifts = [(dy, dx) for _, sh, _ in res for _, _, _, dy, dx in sh]
    return (sc[0, 0] if si[0, 0, 3] else None), si[0, 0].tolist(), shifts, stk


# ---- quality: what the feature is there for ---------------------------------------------------------------------------------------
QUALITY = [(64, 192, 2, 16), (24, 48, 2, 16), (16, 24, 2, 8), (64, 192, 3, 32)]


def noisy_track(Hc, Wc, R, n, seed):
    """(clean plate [Hc, Wc, 3], frames [n, Hc, Wc, 3] uint8, jitter [n, 2]): a plate of 8 x 6 blocks at the levels 64 / 192 on a
    canvas R pixels larger on every side; frame k is the canvas cut at jitter[k] (uniform in -R..R; frame 0, the reference of the
    alignment, at (0, 0)) plus Gaussian noise of sigma 16, rounded."""
    rng = np.random.default_rng(seed)
    levels = np.where(rng.integers(0, 2, (6, 8)) > 0, 192, 64)
    levels[0, 0], levels[0, 1] = 64, 192
    H, W = Hc + 2 * R, Wc + 2 * R
    canvas = levels[(np.arange(H) * 6 // H)[:, None], (np.arange(W) * 8 // W)[None, :]].astype(np.float64)
    canvas = np.repeat(canvas[:, :, None], 3, axis=2)
    jitter = rng.integers(-R, R + 1, (n, 2))
    jitter[0] = 0
    frames = np.stack([canvas[R + jy:R + jy + Hc, R + jx:R + jx + Wc] for jy, jx in jitter])
    frames = np.clip(np.rint(frames + rng.normal(0.0, SIGMA, frames.shape)), 0, 255).astype(np.uint8)
    return canvas[R:R + Hc, R:R + Wc], frames, jitter


def interior_mse(img, clean, R):
    d = img[R:img.shape[0] - R, R:img.shape[1] - R].astype(np.float64) - clean[R:clean.shape[0] - R, R:clean.shape[1] - R]
    return float((d * d).mean())


@pytest.mark.parametrize('Hc, Wc, R, n', QUALITY, ids=lambda v: str(v))
def test_the_stack_recovers_every_shift_and_divides_the_noise_by_n(Hc, Wc, R, n):
    """Every recovered shift is the negative of the true jitter, the stack's MSE against the clean plate over the interior is at
    most 1.5 sigma^2 / n + 1 (expected: sigma^2 / n + 1/12), and without the search the same frames miss that bar.  Measured
    maxima over the five seeds, as multiples of sigma^2 / n: DESIGN 3.10b."""
    bar = 1.5 * SIGMA * SIGMA / n + 1.0
    worst = worst_plain = 0.0
    for seed in range(5):
        clean, frames, jitter = noisy_track(Hc, Wc, R, n, 100 * Hc + 10 * R + seed)
        assert np.abs(jitter).max() == R and len({tuple(j) for j in jitter.tolist()}) > 2
        img, si, shifts, _ = stacked(frames, search=R, max_frames=n)
        assert si == [n, 0, n - 1, 1]
        assert shifts == [(-jy, -jx) for jy, jx in jitter.tolist()]
        mse = interior_mse(img, clean, R)
        worst = max(worst, mse)
        assert mse <= bar, (seed, mse, bar)
        plain, si0, shifts0, _ = stacked(frames, search=0, max_frames=n)
        assert si0 == si and set(shifts0) == {(0, 0)}
        mse0 = interior_mse(plain, clean, R)
        worst_plain = max(worst_plain, mse0)
        assert mse0 > bar, (seed, mse0, bar)
        assert interior_mse(frames[0], clean, R) > 0.9 * SIGMA * SIGMA          # one frame: the whole noise
    print('stack %dx%d R=%d n=%d: worst MSE %.2f = %.3f sigma^2/n (bar %.2f), unaligned %.1f' % (Hc, Wc, R, n, worst, worst * n / SIGMA ** 2, bar,
                                                                                              worst_plain))


# ---- the edges of the rule -----------------------------------------------------------------------------------------------------------
def _shifted_pair(hw, dy, dx, seed=3):
    """Two crops of random pixels, the second the first moved by (dy, dx): the search, where it runs, answers (-dy, -dx)."""
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (hw[0] + 8, hw[1] + 8, 3), dtype=np.uint8)
    return np.stack([big[4:4 + hw[0], 4:4 + hw[1]], big[4 + dy:4 + dy + hw[0], 4 + dx:4 + dx + hw[1]]])


def test_a_crop_no_larger_than_the_search_window_is_not_searched():
    for hw in ((4, 9), (9, 4), (3, 200)):
        _, si, shifts, _ = stacked(_shifted_pair(hw, 0, 1) if hw[1] > 4 else _shifted_pair(hw, 1, 0), search=2)
        assert si[0] == 2 and shifts == [(0, 0), (0, 0)], hw
    # one more row or column and it is
    assert stacked(_shifted_pair((5, 9), 0, 1), search=2)[2] == [(0, 0), (0, -1)]
    assert stacked(_shifted_pair((9, 5), 1, 0), search=2)[2] == [(0, 0), (-1, 0)]
    assert stacked(_shifted_pair((3, 200), 0, -1), search=1)[2] == [(0, 0), (0, 1)]
    assert stacked(_shifted_pair((9, 9), 0, 1), search=0)[2] == [(0, 0), (0, 0)]


def flat_crops(hw=(7, 13)):
    return np.stack([np.full(hw + (3,), v, np.uint8) for v in (90, 90, 200)])


def stripe_crops(hw=(7, 13)):
    """Vertical stripes of period 2: dx = -2, 0 and 2 cost nothing."""
    c = np.zeros(hw + (3,), np.uint8)
    c[:, ::2] = 255
    return np.stack([c, c, c])


def tie_crops(hw=(7, 13), col=6):
    """A bright column, then its two neighbours: (0, -1) and (0, 1) tie below (0, 0)."""
    a, b = np.zeros(hw + (3,), np.uint8), np.zeros(hw + (3,), np.uint8)
    a[:, col] = 255
    b[:, col - 1] = b[:, col + 1] = 255
    return np.stack([a, b])


def test_ties_go_to_the_lower_candidate():
    from yolov6.utils.stack import align_costs, stack_candidates
    assert stacked(flat_crops(), search=2)[2] == [(0, 0)] * 3
    crops = stripe_crops()
    cand = stack_candidates(2)
    costs = align_costs(crops[1], crops[0].astype(np.uint16), 1, 2)
    assert [costs[cand.index(d)] for d in ((0, -2), (0, 0), (0, 2))] == [0, 0, 0] and costs[cand.index((0, 1))] > 0
    assert stacked(crops, search=2)[2] == [(0, 0)] * 3
    crops = tie_crops()
    costs = align_costs(crops[1], crops[0].astype(np.uint16), 1, 2)
    assert costs[cand.index((0, -1))] == costs[cand.index((0, 1))] == min(costs) < costs[0]
    assert cand.index((0, -1)) < cand.index((0, 1))
    assert stacked(crops, search=2)[2] == [(0, 0), (0, -1)]


def test_255_white_frames_fill_the_sum_and_the_256th_is_left_out():
    white = np.full((256, 5, 7, 3), 255, np.uint8)
    white[255] = 0                                              # would pull the mean down if it were taken
    img, si, shifts, stk = stacked(white, search=1, max_frames=255, chunk=100)
    assert si == [255, 0, 254, 1] and len(shifts) == 255 and stk.stats['full'] == 1
    assert (stk.acc[0, 0] == 65025).all() and (img == 255).all()
    with pytest.raises(ValueError):
        stacked(white[:1], max_frames=256)


def wide_cost_crops(hw=(24, 40), R=2, n_black=200):
    """``n_black`` black frames, then a white crop whose rows 0..R are black: every cost is 200 * 65280 per white pixel under the
    window, far above 2^32 in all, and the fewest white pixels lie under dy = -R."""
    crops = np.zeros((n_black + 1,) + hw + (3,), np.uint8)
    crops[n_black, R + 1:] = 255
    return crops


def test_a_cost_above_32_bits_decides_the_minimum():
    R, hw = 2, (24, 40)
    crops = wide_cost_crops(hw, R)
    img, si, shifts, stk = stacked(crops, search=R, max_frames=255, chunk=64)
    assert si[0] == 201 and shifts[:200] == [(0, 0)] * 200 and shifts[200] == (-R, 0)
    full = StackLoops(1, 1, hw, search=R)
    acc = [[[0, 0, 0]] * hw[1] for _ in range(hw[0])]
    costs = full.costs(crops[200].tolist(), acc, 200)
    assert min(costs) > 2 ** 32 and full.align(crops[200].tolist(), acc, 200) == (-R, 0)
    cut = StackLoops(1, 1, hw, search=R, cost_bits=32)
    assert cut.align(crops[200].tolist(), acc, 200) != (-R, 0)         # a 32-bit sum picks another candidate


def test_eligibility():
    rng = np.random.default_rng(5)
    crops = rng.integers(0, 256, (9, 5, 7, 3), dtype=np.uint8)
    rows = np.stack([C.make_row((10, 10, 110, 40))] * 9)
    status = np.array([1, 0, 2, 3, 1, 1, 1, 1, 1], np.int32)
    rows[4, 15] = C.NAN                                         # NaN score
    rows[5, 2] = C.NAN                                          # NaN width
    rows[6, 2] = 10 + 99.5                                      # too narrow
    rows[7, 2] = 10 + 100.0                                     # x2 - x1 == min_width joins
    sharp = np.array([7, 7, 7, 7, 7, 7, 7, 7, 6], np.uint64)    # the last: below min_sharp
    img, si, shifts, stk = stacked(crops, search=0, min_width=100.0, min_sharp=7, status=status, rows=rows, sharp=sharp)
    assert si == [2, 0, 7, 1] and stk.stats['summed'] == 2
    assert np.array_equal(img, ((crops[0].astype(np.uint32) + crops[7] + 1) // 2).astype(np.uint8))
    rows[:, 12:20] = 0.25
    assert stacked(crops, search=0, min_score=0.25, rows=rows)[1][0] == 8       # (row 5's NaN width is below every min_width)
    assert stacked(crops, search=0, min_score=0.2500001, rows=rows)[0] is None


@pytest.mark.parametrize('n', [1, 2, 3, 255])
def test_rounding_of_the_mean(n):
    rng = np.random.default_rng(n)
    crops = rng.integers(0, 256, (n, 5, 7, 3), dtype=np.uint8)
    img, si, _, _ = stacked(crops, search=0, max_frames=255)
    total = crops.astype(np.int64).sum(0)
    want = (total + (n >> 1)) // n
    assert si[0] == n and np.array_equal(img, want)
    if n == 2:
        assert (total % 2 == 1).any() and np.array_equal(img[total % 2 == 1], (total[total % 2 == 1] + 1) // 2)      # .5 goes up
    if n == 3:
        assert np.array_equal(img, np.floor(total / 3 + 0.5))     # no .5 at n = 3: round to nearest


def reuse_calls(hw=(5, 7), seed=9):
    """One call in which slot 0 of stream 1 holds track 4, then track 5, then track 6 (records 4 and 5 exist, 5's line first; 6
    stays live), stream 0 has no frame, and max_ended = 2 cuts the record of track 3 in slot 1 off; then a second call that
    ends 6."""
    rng = np.random.default_rng(seed)
    B, md = 6, 3
    crops = rng.integers(0, 256, (B, md) + hw + (3,), dtype=np.uint8)
    det = np.stack([np.stack([C.make_row((10, 10, 110, 40))] * md)] * B)
    tid = np.array([[4, 3, -1], [4, 3, -1], [5, -1, -1], [5, -1, -1], [6, -1, -1], [6, -1, -1]], np.int32)
    slot = np.where(tid >= 0, np.array([0, 1, 0])[None, :], -1).astype(np.int32)
    ei = np.zeros((2, 2, 12), np.int32)
    ei[1, 0, 0], ei[1, 1, 0] = 5, 4                             # (a third record, track 3's, is cut off)
    call0 = dict(det=det, count=np.full(B, 2, np.int32), tid=tid, slot=slot, crops=crops, status=np.ones((B, md), np.int32),
                 sharp=np.zeros((B, md), np.uint64), stream_of=[1, 1, -1, 1, 1, 1], ended_i=ei, ended_count=np.array([0, 3], np.int32))
    ei1 = np.zeros((2, 2, 12), np.int32)
    ei1[1, 0, 0] = 6
    call1 = dict(det=det[:0], count=np.zeros(0, np.int32), tid=tid[:0], slot=slot[:0], crops=crops[:0], status=np.ones((0, md), np.int32),
                 sharp=np.zeros((0, md), np.uint64), stream_of=[], ended_i=ei1, ended_count=np.array([0, 1], np.int32))
    return [call0, call1]


def test_slot_reuse_truncation_and_a_stream_without_frames():
    from yolov6.utils.stack import StackNp
    calls = reuse_calls()
    stk = StackNp(2, 2, (5, 7), search=0)
    (r0, _, st0), (r1, _, _) = run_np(stk, calls)
    crops = calls[0]['crops'].astype(np.uint32)
    sc, si = r0
    # track 4: frames 0 and 1 of the stream (call frames 0, 1); track 5: only stream frame 2 (call frame 3; frame 2 is untracked)
    assert si[1].tolist() == [[1, 2, 2, 1], [2, 0, 1, 1]] and not si[0].any()
    assert np.array_equal(sc[1, 1], (crops[0, 0] + crops[1, 0] + 1) // 2) and np.array_equal(sc[1, 0], crops[3, 0])
    assert (sc[0] == 0xAB).all()                                # the stream without frames: nothing written
    # slot 1's occupant (track 3) was among the ended ones but its record was cut off: dropped at the end of the call
    assert stk.stats['truncated'] == 0 and st0['idp1'][1].tolist() == [7, 4] and st0['frame'].tolist() == [0, 5]
    assert st0['n'][1].tolist() == [2, 2]
    assert r1[1][1, 0].tolist() == [2, 3, 4, 1] and np.array_equal(r1[0][1, 0], (crops[4, 0] + crops[5, 0] + 1) // 2)
    assert stk.stats['reused'] == 2 and stk.stats['closed'] == 1


def test_a_cut_off_record_drops_its_occupant_when_the_slot_is_reused():
    from yolov6.utils.stack import StackNp
    calls = reuse_calls()
    calls[0]['ended_i'][1, 1, 0] = 99                           # track 4's record is not among the two that fit
    stk = StackNp(2, 2, (5, 7), search=0)
    (sc, si), _, _ = run_np(stk, calls)[0]
    assert si[1].tolist() == [[1, 2, 2, 1], [0, 0, 0, 0]] and (sc[1, 1] == 0xAB).all() and stk.stats['truncated'] == 1


def test_reset_empties_one_stream():
    from yolov6.utils.stack import StackNp
    stk = StackNp(2, 2, (5, 7), search=0)
    call = reuse_calls()[0]
    call['stream_of'] = [0, 1, 0, 1, 0, 1]
    run_np(stk, [call])
    assert stk.frame.tolist() == [3, 3] and stk.idp1.all()
    keep = snapshot(stk)
    stk.reset([0])
    assert not stk.idp1[0].any() and not stk.acc[0].any() and stk.frame.tolist() == [0, 3]
    assert all(np.array_equal(getattr(stk, k)[1], keep[k][1]) for k in stk._ARRAYS)
    stk.reset()
    assert not any(getattr(stk, k).any() for k in stk._ARRAYS)


# ---- PlateTrackerNp.enable_stack ---------------------------------------------------------------------------------------------------
def test_enable_stack_changes_nothing_else_on_the_numpy_tracker():
    from yolov6.utils.best_shot import BestShotNp
    from yolov6.utils.stack import StackNp
    from yolov6.utils.track import PlateTrackerNp
    n_streams, max_det, crop_hw, max_crops = 3, 20, (8, 24), 6
    calls = C.random_track_case(21, n_streams=n_streams, max_det=max_det, extent=150, Bs=(4,) * 8)
    kw = dict(max_tracks=8, match_thres=0.3, new_thres=0.2, expand=0.5, max_age=2)
    a, b = PlateTrackerNp(n_streams, **kw), PlateTrackerNp(n_streams, **kw)
    ga, gb = BestShotNp(n_streams, 8, crop_hw, 0.2), BestShotNp(n_streams, 8, crop_hw, 0.2)
    with pytest.raises(RuntimeError):
        b.update_stack([], calls[0][0], calls[0][1])
    b.enable_stack(search=1, max_frames=5, crop_hw=crop_hw, max_crops=max_crops, min_score=0.2)
    ref = StackNp(n_streams, 8, crop_hw, search=1, max_frames=5, min_score=0.2)
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (170, 220, 3), dtype=np.uint8) for _ in range(4)]
    stream_of, n_valid = [0, 1, 2, 1], 0
    for det, count, _, flush in calls:
        oa, ob = a.update(det, count, stream_of, flush), b.update(det, count, stream_of, flush)
        sa = ga.update_from_frames(frames, det, count, oa[1], a.last_slot, stream_of, oa[2], oa[4], max_crops)
        sb = gb.update_from_frames(frames, det, count, ob[1], b.last_slot, stream_of, ob[2], ob[4], max_crops)
        got = b.update_stack(frames, det, count, stream_of)
        assert got is b.last_stack and a.last_stack is None
        for x, y in zip(oa + sa, ob + sb):                      # the nine outputs
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        want = ref.update_from_frames(frames, det, count, ob[1], b.last_slot, stream_of, ob[2], ob[4], max_crops,
                                      stack_crops=np.zeros_like(got[0]))
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0][got[1][..., 3] == 1], want[0][want[1][..., 3] == 1])
        n_valid += int(got[1][..., 3].sum())
    for name in PlateTrackerNp._SLOT_ARRAYS + ('frame', 'next_id', 'dropped'):
        assert np.array_equal(getattr(a, name).view(np.uint8), getattr(b, name).view(np.uint8)), name
    for name in BestShotNp._ARRAYS:
        assert np.array_equal(getattr(ga, name), getattr(gb, name)), name
    assert n_valid > 0 and ref.stats['summed'] > 0
    b.reset([1])
    assert not b._stack['np'].idp1[1].any() and not b._stack['np'].frame[1]
    b.enable_stack(None)
    assert b._stack is None and b.last_stack is None


# ---- C ABI: everything is checked on the host before any launch -------------------------------------------------------------------
def test_stack_state_bytes():
    from yolov6.hip import abi
    sb = abi.load().lp_stack_state_bytes
    one = sb(1, 1, 64, 192)
    assert one >= 4 + 16 + 64 * 192 * 6 and one % 16 == 0
    assert sb(3, 1, 64, 192) == 3 * one and sb(1, 7, 7, 13) % 16 == 0
    assert sb(1, 2, 7, 13) - sb(1, 1, 7, 13) >= 16 + 7 * 13 * 6 and (sb(1, 2, 7, 13) - sb(1, 1, 7, 13)) % 16 == 0
    assert sb(0, 1, 5, 7) == 0 and sb(1, 0, 5, 7) == 0 and sb(1, 129, 5, 7) == 0 and sb(1, 1, 0, 7) == 0 and sb(1, 1, 5, 1025) == 0


def test_stack_update_rejects_bad_arguments_before_launch():
    from yolov6.hip import abi
    lib = abi.load()
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731
    err = lambda: lib.lp_last_error()   # noqa: E731

    def call(stream_of=(0, 1, -1), n_streams=2, max_tracks=8, h=5, w=7, max_det=10, max_crops=4, max_ended=4, B=None, state=0x100000,
             det=0x10000, count=0x2000, tid=0x3000, slot=0x4000, crops=0x20000, status=0x5000, sharp=0x6000, ei=0x7000, ec=0x8000,
             sc=0x30000, si=0x9000, params=True, search=2, max_frames=64, min_score=0.0, min_width=0.0, min_sharp=0):
        so = (ctypes.c_int * max(len(stream_of), 1))(*stream_of) if stream_of is not None else None
        p = abi.StackParams(min_score, min_width, min_sharp, search, max_frames)
        return lib.lp_stack_update(v(state), n_streams, max_tracks, h, w, v(det), v(count), len(stream_of or ()) if B is None else B,
                                   max_det, v(tid), v(slot), v(crops), v(status), v(sharp), max_crops, so, v(ei), v(ec), max_ended,
                                   ctypes.byref(p) if params else None, v(sc), v(si), None)

    for k in ('state', 'det', 'count', 'tid', 'slot', 'crops', 'status', 'sharp', 'ei', 'ec', 'sc', 'si'):
        assert call(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
    assert call(params=False) == LP_ERR_ARG and b'null' in err()
    assert call(stream_of=None, B=3) == LP_ERR_ARG and b'null' in err()
    assert call(state=0x100004) == LP_ERR_ARG and b'aligned' in err()
    assert call(sharp=0x6004) == LP_ERR_ARG and b'aligned' in err()
    assert call(n_streams=0) == LP_ERR_ARG and call(max_tracks=0) == LP_ERR_ARG and call(max_tracks=129) == LP_ERR_ARG and b'128' in err()
    assert call(h=0) == LP_ERR_ARG and call(w=1025) == LP_ERR_ARG and b'1024' in err()
    assert call(B=-1) == LP_ERR_ARG and call(max_det=0) == LP_ERR_ARG and call(max_ended=-1) == LP_ERR_ARG and call(max_crops=-1) == LP_ERR_ARG
    assert call(search=-1) == LP_ERR_ARG and call(search=5) == LP_ERR_ARG and b'search' in err()
    assert call(max_frames=0) == LP_ERR_ARG and call(max_frames=256) == LP_ERR_ARG and b'max_frames' in err()
    assert call(min_score=float('nan')) == LP_ERR_ARG and call(min_score=float('inf')) == LP_ERR_ARG and b'min_score' in err()
    assert call(min_width=float('nan')) == LP_ERR_ARG and call(min_width=-float('inf')) == LP_ERR_ARG and b'min_width' in err()
    assert call(stream_of=(0, 1, 2)) == LP_ERR_ARG and b'frame 2' in err()
    assert call(stream_of=(0, -2, 1)) == LP_ERR_ARG and b'frame 1' in err()
    # an output on top of an input or of another output
    state_bytes = lib.lp_stack_state_bytes(2, 8, 5, 7)
    assert call(sc=0x100000 + state_bytes - 1) == LP_ERR_ARG and b'overlap' in err()
    assert call(si=0x20000) == LP_ERR_ARG and b'overlap' in err()                      # stack_i on the crops
    assert call(sc=0x7000) == LP_ERR_ARG and b'overlap' in err()                       # stack_crops on ended_i
    assert call(si=0x30000) == LP_ERR_ARG and b'overlap' in err()                      # stack_i on stack_crops
    assert call(state=0x10000) == LP_ERR_ARG and b'overlap' in err()                   # the state on det


# ---- tools/infer.py --track --best-shots --stack-shots on the CPU path ---------------------------------------------------------------
def stacks_by_hand(frames, dets, max_det, crop_hw, max_crops=16, stack_kw=None, **kw):
    """PlateTrackerNp + StackNp over the untracked per-frame detections of one stream, one update per frame, then the flush:
    (ended records, stacks) with stacks[k] = (stack_i [4], picture or None) for record k."""
    from yolov6.utils.stack import StackNp
    from yolov6.utils.track import PlateTrackerNp
    trk = PlateTrackerNp(1, **kw)
    stk = StackNp(1, trk.max_tracks, crop_hw, **(stack_kw or {}))
    ended, stacks = [], []

    def collect(ei, ef, ec, out):
        sc, si = out
        for k in range(int(ec[0])):
            ended.append((ei[0, k], ef[0, k]))
            stacks.append((si[0, k], sc[0, k].copy() if si[0, k, 3] else None))

    for frame, d in zip(frames, dets):
        pad = np.zeros((1, max_det, 28), f32)
        pad[0, :len(d)] = d
        _, tid, ei, ef, ec = trk.update(pad, [len(d)], max_ended=2 * trk.max_tracks)
        collect(ei, ef, ec, stk.update_from_frames([frame], pad, [len(d)], tid, trk.last_slot, [0], ei, ec, max_crops))
    _, tid, ei, ef, ec = trk.flush_all()
    collect(ei, ef, ec, stk.update_from_frames([], np.zeros((0, 1, 28), f32), [], tid, trk.last_slot, [], ei, ec, max_crops))
    return ended, stacks


def check_stack_files(out_dir, ended, stacks):
    """stacks.txt is line-parallel to plates.txt and the PNGs decode to the expected pictures (RGB)."""
    from PIL import Image
    assert (out_dir / 'plates.txt').read_text().splitlines() == C.plate_lines(ended)
    lines = (out_dir / 'stacks.txt').read_text().splitlines()
    assert len(lines) == len(ended) == len(stacks)
    n_png = 0
    for k, (line, (ri, _), (ki, crop)) in enumerate(zip(lines, ended, stacks)):
        name = 'stacks/%d_%d.png' % (k, ri[0]) if crop is not None else '-'
        assert line == '%d %d %d %d %s' % (ri[0], ki[0], ki[1], ki[2], name), k
        if crop is not None:
            assert np.array_equal(np.asarray(Image.open(str(out_dir / name))), crop[:, :, ::-1])
            n_png += 1
    assert sorted(os.listdir(str(out_dir / 'stacks'))) == sorted('%d_%d.png' % (k, e[0][0]) for k, (e, s) in enumerate(zip(ended, stacks))
                                                                 if s[1] is not None)
    return n_png


def test_infer_stack_shots_cpu(tmp_path, monkeypatch):
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None, 'epoch': 0}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    frames = C._moving_frames(6)
    for k, f in enumerate(frames):
        Image.fromarray(f).save(str(img_dir / ('f%02d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 160], conf_thres=0.06, iou_thres=0.45, max_det=20,
              device='cpu', not_save_img=True, save_txt=True)
    plain = infer.run(save_dir=str(tmp_path / 'o1'), **kw)
    tkw = dict(track=True, track_max_age=2, track_iou=0.25, track_expand=0.25, best_shots=True, crop_size=(16, 48))
    shot = infer.run(save_dir=str(tmp_path / 'o2'), **tkw, **kw)
    both = infer.run(save_dir=str(tmp_path / 'o3'), stack_shots=True, stack_search=1, stack_max_frames=4, stack_min_width=8.0, **tkw, **kw)
    assert all(torch.equal(a, b) for a, b in zip(shot, both))                   # the flag changes nothing else
    for name in ('plates.txt', 'tracks.txt', 'shots.txt'):
        assert (tmp_path / 'o2' / name).read_text() == (tmp_path / 'o3' / name).read_text()
    assert not (tmp_path / 'o2' / 'stacks.txt').exists() and not (tmp_path / 'o2' / 'stacks').exists()
    bgr = [f[:, :, ::-1] for f in frames]                                       # the PNGs are RGB, the Inferer's frames BGR
    ended, stacks = stacks_by_hand(bgr, [d.numpy() for d in plain], 20, (16, 48), stack_kw=dict(search=1, max_frames=4, min_width=8.0),
                                   max_tracks=64, match_thres=0.25, new_thres=0.0, expand=0.25, max_age=2, ncls=m)
    assert check_stack_files(tmp_path / 'o3', ended, stacks) >= 1
    assert max(s[0][0] for s in stacks) >= 2                                    # some track was averaged over several frames
    with pytest.raises(ValueError):
        infer.run(save_dir=str(tmp_path / 'o4'), stack_shots=True, track=True, **kw)      # needs --best-shots
    with pytest.raises(ValueError):
        infer.run(save_dir=str(tmp_path / 'o5'), stack_shots=True, stack_search=5, **tkw, **kw)
