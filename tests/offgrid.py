"""Inputs off the grid on which fp32 arithmetic is exact, for the tracker, the cross-tile merge and the share quantiser of the
watchlist and the sightings log (tests/test_offgrid_cpu.py, tests/test_offgrid_gpu.py).

The shipped random cases (``test_track_cpu.random_track_case``, ``test_tiles_cpu.random_case``, ``test_watch_cpu.random_reads``) draw
integer boxes and confidences k / 8: every fp32 operation on them is exact, so a kernel that fuses a multiply-add, sums in another
order or divides through a reciprocal produces the same bits.  Here are
  - ``offgrid_rows`` / ``offgrid_twin``: rows with full-mantissa coordinates and confidences, and the off-grid twin of a shipped case;
  - ``offgrid_merge_case``: the same for lp_merge_tiles;
  - constructed DECISION cases: an IoU is no output -- it decides a match -- and random scenes have no pair close enough to the
    threshold, or to another pair, for one ulp to matter.  ``tracker_cases`` / ``merge_cases`` search, with fixed seeds, for inputs on
    which one named wrong computation (``defect``) decides otherwise than the specification: threshold straddles, the IoU that is
    exactly the fp32 nearest to the threshold, and order swaps;
  - ``quantiser_shares``: vote shares at the boundaries k / 255 of ``watch.position_weight``;
  - ``held_calls``: tracks near the origin, missed for two frames (k = 3 in the velocity), then held for three (vel * 3 rounds).
``defect(name)`` runs the numpy specification with ONE computation replaced by its emulation; nothing wrong is ever built for or
run on the device.  Everything is seeded; the searches are vectorised and take a few seconds in all, once per process."""
import contextlib

import numpy as np

import test_track_cpu as C

f32, f64 = np.float32, np.float64
EXPANDS = (0.3, 0.1)
MATCH_THRES = (0.37, 0.3)
NEW_THRES = 0.23
MERGE_THRES = (0.45, 0.3)
HARD_CONF = (f32(1) - f32(2.0 ** -24), f32(2.0 ** -126), f32(2.0 ** -140))     # just below 1, the smallest normal, a subnormal
QUANT_KS = (1, 2, 127, 128, 254, 255)
MIN_INSTANCES = 4                                                               # of every kind of constructed case


# ---- values ---------------------------------------------------------------------------------------------------------------------------
def full_mantissa(rng, shape, lo, hi):
    """fp32 uniform in [lo, hi), none of them a multiple of 2^-9 (so of no 2^-k with k < 10)."""
    v = rng.uniform(lo, hi, shape).astype(f32)
    for _ in range(20):
        bad = (v * f32(512) == np.floor(v * f32(512))) | (v >= f32(hi))
        if not bad.any():
            return v
        v = np.where(bad, rng.uniform(lo, hi, shape).astype(f32), v)
    raise AssertionError('no full-mantissa draw')


def is_off_grid(v):
    v = np.asarray(v, f32)
    return (v * f32(512) != np.floor(v * f32(512)))


def sum_left(c):
    """fp32 c0 + c1 + ... + c7 left to right, over the last axis."""
    c = np.asarray(c, f32)
    s = c[..., 0] + c[..., 1]
    for k in range(2, 8):
        s = s + c[..., k]
    return s


def sum_pairwise(c):
    """fp32 ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7)): the order of ``np.sum`` on eight contiguous floats."""
    c = np.asarray(c, f32)
    return ((c[..., 0] + c[..., 1]) + (c[..., 2] + c[..., 3])) + ((c[..., 4] + c[..., 5]) + (c[..., 6] + c[..., 7]))


def fma(a, b, c):
    """fp32 fused multiply-add, emulated: the product of two fp32 is exact in float64; the sum is rounded to float64, then to fp32."""
    with np.errstate(all='ignore'):
        return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def permuted_confidences(rng, n):
    """(c [n, 8], d [n, 8]) fp32 in (0, 1): d[i] is a permutation of c[i] whose left-to-right fp32 sum differs from c[i]'s, while
    the exact sums are equal."""
    out_c, out_d = [], []
    while len(out_c) < n:
        c = full_mantissa(rng, (4 * n + 8, 8), 0.05, 1.0)
        d = np.stack([row[rng.permutation(8)] for row in c])
        for i in np.nonzero(sum_left(c) != sum_left(d))[0][:n - len(out_c)]:
            out_c.append(c[i])
            out_d.append(d[i])
    return np.array(out_c, f32), np.array(out_d, f32)


def offgrid_rows(rng, n, extent=4000.0, ncls=C.NCLS, hard=0.15):
    """``n`` detection rows in the layout of ``make_row``: box and corner coordinates with full mantissas in [0, extent), confidences
    uniform in (0, 1); a share ``hard`` of the rows holds one of HARD_CONF, and rows 2k, 2k + 1 of the first quarter hold
    permutations of the same eight confidences."""
    w, h = full_mantissa(rng, n, 30, 90), full_mantissa(rng, n, 10, 30)
    x1, y1 = full_mantissa(rng, n, 0, extent - 100), full_mantissa(rng, n, 0, extent - 100)
    rows = np.zeros((n, 28), f32)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = x1, y1, x1 + w, y1 + h
    rows[:, 4:12] = rows[:, [0, 1, 0, 3, 2, 3, 2, 1]] + full_mantissa(rng, (n, 8), -2, 2)
    rows[:, :12] = np.where(is_off_grid(rows[:, :12]), rows[:, :12], rows[:, :12] + f32(2.0 ** -11))
    rows[:, 12:20] = full_mantissa(rng, (n, 8), 0.001, 1.0)
    pairs = n // 8
    if pairs:
        c, d = permuted_confidences(rng, pairs)
        rows[0:2 * pairs:2, 12:20], rows[1:2 * pairs:2, 12:20] = c, d
    for k, r in enumerate(2 * pairs + np.nonzero(rng.random(n - 2 * pairs) < hard)[0]):
        rows[r, 12 + int(rng.integers(0, 8))] = HARD_CONF[k % 3]
    rows[:, 20:28] = np.stack([rng.integers(0, k, n) for k in ncls], 1)
    return rows


def offgrid_twin(calls, seed, jitter=0.5, hard=0.05):
    """The off-grid twin of a list of calls of ``random_track_case`` (4-tuples) or ``lp_testing.all_on_scene`` (5-tuples): the same
    births, deaths, NaNs, counts, stream tables and flushes; every finite box coordinate of a row below the count moves by up to
    ``jitter`` px to a full-mantissa value, the corners follow the box, every confidence that is neither 0 nor NaN becomes a
    full-mantissa value in (0, 1), a share ``hard`` of the rows one of HARD_CONF, and one row in ten takes a permutation of the
    confidences of the row before it.  Rows that are equal in a frame stay equal (their IoUs with every slot tie)."""
    rng = np.random.default_rng(seed)
    out = []
    for call in calls:
        det, count = call[0].copy(), call[1]
        for b in range(len(det)):
            seen, prev = {}, None
            for r in range(min(max(int(count[b]), 0), det.shape[1])):
                key = det[b, r].tobytes()
                if key in seen:
                    det[b, r] = seen[key]
                    continue
                row = det[b, r]
                box = row[0:4] + full_mantissa(rng, 4, -jitter, jitter)
                box = np.where(is_off_grid(box), box, box + f32(2.0 ** -11))
                row[0:4] = np.where(np.isfinite(row[0:4]), box, row[0:4])
                row[4:12] = row[[0, 1, 0, 3, 2, 3, 2, 1]]
                conf = full_mantissa(rng, 8, 0.001, 1.0)
                if prev is not None and rng.random() < 0.1:
                    conf = prev[rng.permutation(8)]
                if rng.random() < hard:
                    conf[int(rng.integers(0, 8))] = HARD_CONF[int(rng.integers(0, 3))]
                prev = conf.copy()
                row[12:20] = np.where((row[12:20] == 0) | np.isnan(row[12:20]), row[12:20], conf)
                seen[key] = row.copy()
        out.append((det,) + tuple(call[1:]))
    return out


# ---- the overlap quotient and the wrong computations --------------------------------------------------------------------------------------
def overlap_quotient(a, b, metric='iou', den_fma=False, min_after=False):
    """fp32 quotient of ``tiles.overlaps`` / ``track.iou_matrix`` for boxes a (i, the kept one) and b (j) [..., 4], elementwise with
    broadcasting, op by op in their order.  ``den_fma``: area_i + area_j - inter as a compiler contracts it, fma(-w, h, fma(jw, jh, area_i)): neither
    area_j nor inter is rounded on its way into the denominator;
    ``min_after`` ('ios'): the minimum of inter / area_i and inter / area_j in place of inter / min(area_i, area_j)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    ix1, iy1, ix2, iy2 = (a[..., k] for k in range(4))
    jx1, jy1, jx2, jy2 = (b[..., k] for k in range(4))
    with np.errstate(all='ignore'):
        xx1 = np.where(ix1 > jx1, ix1, jx1)
        yy1 = np.where(iy1 > jy1, iy1, jy1)
        xx2 = np.where(ix2 < jx2, ix2, jx2)
        yy2 = np.where(iy2 < jy2, iy2, jy2)
        w = xx2 - xx1
        w = np.where(w > 0, w, f32(0))
        h = yy2 - yy1
        h = np.where(h > 0, h, f32(0))
        inter = w * h
        iarea = (ix2 - ix1) * (iy2 - iy1)
        jarea = (jx2 - jx1) * (jy2 - jy1)
        if metric == 'iou':
            ovr = inter / (fma(-w, h, fma(jx2 - jx1, jy2 - jy1, iarea)) if den_fma else iarea + jarea - inter)
        elif min_after:
            qi, qj = inter / iarea, inter / jarea
            ovr = np.where(qi < qj, qi, qj)
        else:
            ovr = inter / np.where(iarea < jarea, iarea, jarea)
    assert ovr.dtype == f32
    return ovr


def _expand_fma(box, e):
    box = np.asarray(box, f32)
    w, h = box[..., 2] - box[..., 0], box[..., 3] - box[..., 1]
    return np.stack([fma(-e, w, box[..., 0]), fma(-e, h, box[..., 1]), fma(e, w, box[..., 2]), fma(e, h, box[..., 3])], -1)


def _iou_matrix_fma(a, b):
    a, b = np.asarray(a, f32).reshape(-1, 4), np.asarray(b, f32).reshape(-1, 4)
    return overlap_quotient(a[:, None, :], b[None, :, :], 'iou', den_fma=True)


def _predict_fma(box, vel, k):
    k = np.asarray(k, f32)
    return np.stack([fma(vel[..., 0], k, box[..., 0]), fma(vel[..., 1], k, box[..., 1]), fma(vel[..., 0], k, box[..., 2]),
                     fma(vel[..., 1], k, box[..., 3])], -1)


def _velocity_rcp(new, old, k):
    with np.errstate(all='ignore'):
        r = f32(1) / np.asarray(k, f32)
        return np.stack([((new[..., 0] + new[..., 2]) * f32(0.5) - (old[..., 0] + old[..., 2]) * f32(0.5)) * r,
                         ((new[..., 1] + new[..., 3]) * f32(0.5) - (old[..., 1] + old[..., 3]) * f32(0.5)) * r], -1)


def _score_pairwise(row):
    with np.errstate(all='ignore'):
        return sum_pairwise(row[12:20]) / f32(8.0)


def _scores_pairwise(rows):
    with np.errstate(all='ignore'):
        return sum_pairwise(rows[:, 12:20]) / f32(8.0)


def _share_rcp(v, tot):
    with np.errstate(all='ignore'):
        return v * (f32(1) / tot)


def _over_f32(iou, thres):
    return iou > f32(thres)


def _add_total64(self, s, t, p, conf):
    """``PlateTrackerNp._add_total`` with the head's total kept in float64 (per track) and rounded to fp32 for the share."""
    tot = self.__dict__.setdefault('_total64', {})
    key = (s, t, int(self.id[s, t]), p)
    tot[key] = (tot.get(key, 0.0) if self.total[s, t, p] != 0 else 0.0) + float(conf)
    self.total[s, t, p] = f32(tot[key])


def _held_fma(box, cor, vel, k):
    """``track.held_geometry`` with every coordinate as one fused multiply-add coord + vel * k."""
    v2, v4 = np.tile(np.asarray(vel, f32), 2), np.tile(np.asarray(vel, f32), 4)
    return fma(v2, k, box), fma(v4, k, cor)


def _overlaps_variant(**kw):
    thr32 = kw.pop('thr32', False)

    def overlaps(kept, box, thres, metric):
        kept = np.asarray(kept, f32).reshape(-1, 4)
        ovr = overlap_quotient(kept, np.asarray(box, f32)[None, :], metric, **kw)     # (each switch acts on its own metric only)
        return ovr > f32(thres) if thr32 else ovr.astype(f64) > float(thres)
    return overlaps


def _weight_f64(share):
    """``watch.position_weight`` with the product share * 255 in float64: floor of the exact product."""
    share = np.asarray(share, f32)
    with np.errstate(all='ignore'):
        t = np.minimum(share.astype(f64) * 255.0, 255.0)
        pos = share > 0
        return np.where(pos, np.where(pos, t, 0.0).astype(np.int32) + 1, 1).astype(np.int32)


def _weight_rint(share):
    """``watch.position_weight`` with the product rounded to the nearest integer in place of truncated."""
    share = np.asarray(share, f32)
    with np.errstate(all='ignore'):
        t = np.minimum(np.rint(share * f32(255.0)), f32(255.0))
        pos = share > 0
        return np.where(pos, np.where(pos, t, f32(0)).astype(np.int32) + 1, 1).astype(np.int32)


# name -> (family, [(module or class, attribute, replacement)])
def _defects():
    from yolov6.utils import tiles, track, watch
    trk = track.PlateTrackerNp
    return {
        'expand_fma': ('track', [(track, 'expand_boxes', _expand_fma)]),
        'den_fma': ('track', [(track, 'iou_matrix', _iou_matrix_fma)]),
        'pred_fma': ('track', [(track, 'predict_boxes', _predict_fma)]),
        'vel_rcp': ('track', [(track, 'centre_velocity', _velocity_rcp)]),
        'score_pairwise': ('track', [(track, 'new_score', _score_pairwise)]),
        'total_f64': ('track', [(trk, '_add_total', _add_total64)]),
        'held_fma': ('track', [(track, 'held_geometry', _held_fma)]),
        'share_rcp': ('track', [(track, 'vote_share', _share_rcp)]),
        'thr_f32': ('track', [(track, 'over_threshold', _over_f32)]),
        'merge_den_fma': ('merge', [(tiles, 'overlaps', _overlaps_variant(den_fma=True))]),
        'merge_score_pairwise': ('merge', [(tiles, 'row_scores', _scores_pairwise)]),
        'merge_thr_f32': ('merge', [(tiles, 'overlaps', _overlaps_variant(thr32=True))]),
        'merge_ios_min_after': ('merge', [(tiles, 'overlaps', _overlaps_variant(min_after=True))]),
        'quant_f64': ('quant', [(watch, 'position_weight', _weight_f64)]),
        'quant_rint': ('quant', [(watch, 'position_weight', _weight_rint)]),
    }


TRACK_DEFECTS = ('expand_fma', 'den_fma', 'pred_fma', 'vel_rcp', 'held_fma', 'score_pairwise', 'total_f64', 'share_rcp', 'thr_f32')
MERGE_DEFECTS = ('merge_den_fma', 'merge_score_pairwise', 'merge_thr_f32', 'merge_ios_min_after')
QUANT_DEFECTS = ('quant_f64', 'quant_rint')


@contextlib.contextmanager
def defect(name):
    """The numpy specifications with the one computation ``name`` replaced by its emulation (None: unchanged)."""
    patches = _defects()[name][1] if name else []
    saved = [(obj, attr, getattr(obj, attr)) for obj, attr, _ in patches]
    try:
        for obj, attr, new in patches:
            setattr(obj, attr, new)
        yield
    finally:
        for obj, attr, old in saved:
            setattr(obj, attr, old)


@contextlib.contextmanager
def count_denominator_changes():
    """While active, every IoU the specifications evaluate ('iou' of ``track.iou_matrix`` and ``tiles.overlaps``) is also evaluated
    with the fused denominator: yields a dict with ``pairs`` (pairs whose boxes intersect) and ``changed`` (of those, the pairs whose
    quotient has other bits)."""
    from yolov6.utils import tiles, track
    stats = dict(pairs=0, changed=0)
    iou_matrix, overlaps = track.iou_matrix, tiles.overlaps

    def note(a, b):
        q, qf = overlap_quotient(a, b), overlap_quotient(a, b, den_fma=True)
        hit = q > 0
        stats['pairs'] += int(hit.sum())
        stats['changed'] += int((hit & (q.view(np.int32) != qf.view(np.int32))).sum())

    def iou_matrix_counted(a, b):
        a, b = np.asarray(a, f32).reshape(-1, 4), np.asarray(b, f32).reshape(-1, 4)
        note(a[:, None, :], b[None, :, :])
        return iou_matrix(a, b)

    def overlaps_counted(kept, box, thres, metric):
        if metric == 'iou':
            note(np.asarray(kept, f32).reshape(-1, 4), np.asarray(box, f32)[None, :])
        return overlaps(kept, box, thres, metric)

    track.iou_matrix, tiles.overlaps = iou_matrix_counted, overlaps_counted
    try:
        yield stats
    finally:
        track.iou_matrix, tiles.overlaps = iou_matrix, overlaps


# ---- searching ---------------------------------------------------------------------------------------------------------------------------
def _bits(v):
    return np.asarray(v, f32).view(np.int32).astype(np.int64)


def _ulp_step(v, n):
    """fp32 ``v`` moved by ``n`` units in the last place (positive finite values)."""
    return (np.asarray(v, f32).view(np.int32) + np.asarray(n, np.int32)).view(f32)


def tune_to_target(evaluate, box, target, rng, rounds=60):
    """Move the four coordinates of ``box`` [4] by units in the last place until ``evaluate(boxes [m, 4]) -> fp32 [m]`` gives exactly
    ``target``: steepest descent over single-coordinate moves of 2^k ulps, then random moves of a few ulps around the best point.
    Returns the box, or None."""
    want = int(_bits(target))
    steps = np.array([s * 2 ** k for k in range(22) for s in (1, -1)], np.int32)
    moves = np.zeros((4 * len(steps), 4), np.int32)
    for c in range(4):
        moves[c * len(steps):(c + 1) * len(steps), c] = steps
    box = np.asarray(box, f32).copy()
    err = abs(int(_bits(evaluate(box[None]))[0]) - want)
    for _ in range(rounds):
        if err == 0:
            return box
        cand = _ulp_step(box[None, :], moves)
        e = np.abs(_bits(evaluate(cand)) - want)
        k = int(np.argmin(e))
        if e[k] >= err:
            break
        box, err = cand[k], int(e[k])
    for _ in range(8):
        if err == 0:
            return box
        cand = _ulp_step(box[None, :], rng.integers(-24, 25, (4096, 4)).astype(np.int32))
        e = np.abs(_bits(evaluate(cand)) - want)
        k = int(np.argmin(e))
        if e[k] < err:
            box, err = cand[k], int(e[k])
    return box if err == 0 else None


def nearest_f32_above(thres):
    """The fp32 nearest to ``thres`` if it lies above it (then ``iou > float32(thres)`` and ``(double)iou > thres`` disagree for
    exactly this IoU), else None."""
    t = f32(thres)
    return t if float(t) > float(thres) else None


def _pair_iou(a, b):
    """fp32 [n]: ``track.iou_matrix`` (as patched at the moment) of a[i] and b[i]."""
    from yolov6.utils import track
    return np.concatenate([np.diagonal(track.iou_matrix(a[i:i + 64], b[i:i + 64])) for i in range(0, len(a), 64)]).astype(f32)


def _final_iou(A0, A1, R, gaps, e):
    """The IoU that decides the match of row R in the scene [A0], gaps[0] empty frames, [A1], gaps[1] empty frames, [R] on one slot,
    by the tracker's own functions (as patched at the moment): velocity of A0 -> A1 over k = gaps[0] + 1, prediction with
    k = gaps[1] + 1, expansion, IoU."""
    from yolov6.utils import track
    vel = track.centre_velocity(A1, A0, f32(gaps[0] + 1))
    pred = track.predict_boxes(A1, vel.astype(f32), f32(gaps[1] + 1))
    return _pair_iou(track.expand_boxes(pred, e), track.expand_boxes(R, e))


def _scene_boxes(rng, n, gaps=(0, 0), lo=100.0, hi=3000.0):
    """A0, A1, R [n, 4] of the scene of ``_final_iou``: an object of full-mantissa position in [lo, hi) and velocity, and a row R
    that overlaps its prediction by an IoU around 0.2 .. 0.6."""
    x, y = full_mantissa(rng, n, lo, hi), full_mantissa(rng, n, lo, hi)
    w, h = full_mantissa(rng, n, 40, 90), full_mantissa(rng, n, 12, 30)
    A0 = np.stack([x, y, x + w, y + h], -1).astype(f32)
    v = np.stack([full_mantissa(rng, n, -2, 2), full_mantissa(rng, n, -0.7, 0.7)], -1)
    A1 = (A0 + np.tile(v * f32(gaps[0] + 1), 2) + full_mantissa(rng, (n, 4), -0.3, 0.3)).astype(f32)
    off = np.stack([full_mantissa(rng, n, 0.2, 0.6) * w * rng.choice([-1, 1], n).astype(f32), full_mantissa(rng, n, -0.2, 0.2) * h], -1)
    R = (A1 + np.tile(v * f32(gaps[1] + 1), 2) + np.tile(off, 2) + full_mantissa(rng, (n, 4), -0.3, 0.3)).astype(f32)
    return A0, A1, R


def _conf(rng, lo=0.3):
    return full_mantissa(rng, 8, lo, 1.0)


def _track_case(kind, aimed_at, frames, max_det=2, **kw):
    det, count = C.frames_of(frames, max_det)
    kw = dict(dict(max_tracks=4, new_thres=0.0, max_age=3), **kw)
    return dict(kind=kind, defect=aimed_at, kw=kw, n_streams=1, max_ended=4, calls=[(det, count, [0] * len(det), [1])])


def _ids(rng):
    return [int(rng.integers(0, n)) for n in C.NCLS]


def tracker_straddles(aimed_at, seed, n=4096, want=6):
    """Scenes [A0], g0 x [], [A1], g1 x [], [R] whose deciding IoU has other bits under the wrong computation ``aimed_at`` than under
    the specification, with match_thres set to the smaller of the two values: the one matches, the other starts a new track.  The
    velocity through a reciprocal needs k = 3 in the velocity (g0 = 2).  The fused prediction needs k = 3 in the velocity AND in the
    prediction (g0 = g1 = 2): vel * k is exact for k = 1 and 2, and also for a velocity that is a plain difference of centres (it
    has few significant bits), so only a velocity divided by 3 gives a product that rounds.  Both show only where a coordinate is
    about as small as the velocity, so those scenes lie near the origin."""
    rng = np.random.default_rng(seed)
    gaps = {'vel_rcp': (2, 0), 'pred_fma': (2, 2)}.get(aimed_at, (0, 0))
    near = gaps != (0, 0)
    out = []
    for e in EXPANDS:
        A0, A1, R = _scene_boxes(rng, 8 * n, gaps, 2.0, 16.0) if near else _scene_boxes(rng, n)
        ef = f32(e)
        with defect(None):
            im, first_m = _final_iou(A0, A1, R, gaps, ef), _pair_iou(_exp(A0, ef), _exp(A1, ef))
        with defect(aimed_at):
            idf, first_d = _final_iou(A0, A1, R, gaps, ef), _pair_iou(_exp(A0, ef), _exp(A1, ef))
        ok = (im != idf) & (np.minimum(im, idf) > 0.2) & (np.maximum(im, idf) < 0.6) & (np.minimum(first_m, first_d) > 0.7)
        picks = list(np.nonzero(ok & (im > idf))[0][:want // 4 + 1]) + list(np.nonzero(ok & (im < idf))[0][:want // 4 + 1])
        for i in picks:
            ids = _ids(rng)
            frames = ([[C.make_row(A0[i], ids, _conf(rng))]] + [[]] * gaps[0] + [[C.make_row(A1[i], ids, _conf(rng))]] + [[]] * gaps[1] +
                      [[C.make_row(R[i], ids, _conf(rng))]])
            out.append(_track_case('straddle', aimed_at, frames, match_thres=float(min(im[i], idf[i])), expand=e))
    return out


def _exp(box, e):
    from yolov6.utils import track
    return track.expand_boxes(box, e)


def tracker_exact_threshold(seed, want=4, tries=60):
    """Scenes [A], [R] whose IoU is exactly the fp32 nearest to match_thres, where that fp32 lies above the threshold: the rule
    (double)iou > match_thres matches; ``iou > (float)match_thres`` does not."""
    rng = np.random.default_rng(seed)
    out = []
    for thres in MATCH_THRES:
        target = nearest_f32_above(thres)
        if target is None:
            continue
        found = 0
        for t in range(tries):
            if found >= want:
                break
            e = f32(EXPANDS[t % 2])
            A0, _, R = _scene_boxes(rng, 1)
            got = tune_to_target(lambda r: _pair_iou(_exp(np.repeat(A0, len(r), 0), e), _exp(r, e)), R[0], target, rng)
            if got is None or not np.isfinite(got).all():
                continue
            ids = _ids(rng)
            out.append(_track_case('exact', 'thr_f32', [[C.make_row(A0[0], ids, _conf(rng))], [C.make_row(got, ids, _conf(rng))]],
                                   match_thres=thres, expand=float(EXPANDS[t % 2])))
            found += 1
    return out


def _tuned_swaps(aimed_at, rng, e, want, tries=40):
    """Two slots of different shapes whose IoUs with the row are a few ulps apart: S1 is tuned until its IoU is S0's, then moved by
    a few ulps until the larger of the two is the other one under ``aimed_at``.  -> [(S0, S1, R)]"""
    ef, out = f32(e), []
    for _ in range(tries):
        if len(out) >= want:
            break
        x, y, w, h = (full_mantissa(rng, 1, lo, hi)[0] for lo, hi in ((200, 3000), (200, 3000), (50, 90), (14, 30)))
        R = np.array([x, y, x + w, y + h], f32)
        S0 = (R + np.tile([rng.uniform(0.15, 0.4) * w, rng.uniform(-0.1, 0.1) * h], 2) + full_mantissa(rng, 4, -1, 1)).astype(f32)
        S1 = (R - np.tile([rng.uniform(0.15, 0.4) * w, rng.uniform(-0.1, 0.1) * h], 2) + full_mantissa(rng, 4, -1, 1)).astype(f32)
        rows = lambda m: _exp(np.repeat(R[None], m, 0), ef)                      # noqa: E731
        with defect(None):
            m0 = _pair_iou(_exp(S0[None], ef), rows(1))[0]
            S1 = tune_to_target(lambda c: _pair_iou(_exp(c, ef), rows(len(c))), S1, m0, rng)
            if S1 is None or not m0 > 0.4:
                continue
            cand = _ulp_step(S1[None, :], rng.integers(-6, 7, (2048, 4)).astype(np.int32))
            m1 = _pair_iou(_exp(cand, ef), rows(len(cand)))
        with defect(aimed_at):
            d0, d1 = _pair_iou(_exp(S0[None], ef), rows(1))[0], _pair_iou(_exp(cand, ef), rows(len(cand)))
        flips = np.nonzero((m0 >= m1) != (d0 >= d1))[0]
        if len(flips):
            out.append((S0, cand[flips[0]], R))
    return out


def tracker_swaps(aimed_at, seed, n=16384, want=6):
    """Two slots and one row: slot boxes S0 and S1 = S0 mirrored about the centre of the row R, every coordinate exact in fp32, so
    that the two IoUs are equal in exact arithmetic; in fp32 they differ in the last bits, and under ``aimed_at`` the other one is
    the larger: the greedy settle gives the row to the other slot.  The fused denominator moves both IoUs of a mirrored pair almost
    alike, so such pairs are rare for it; ``_tuned_swaps`` adds pairs of unlike slots with IoUs a few ulps apart."""
    rng = np.random.default_rng(seed)
    out = []
    for e in EXPANDS:
        ef = f32(e)
        x, y = full_mantissa(rng, n, 640, 800), full_mantissa(rng, n, 300, 400)
        w, h = full_mantissa(rng, n, 50, 90), full_mantissa(rng, n, 14, 30)
        R = np.stack([x, y, x + w, y + h], -1).astype(f32)
        d = np.stack([full_mantissa(rng, n, 0.15, 0.45) * w, full_mantissa(rng, n, -0.15, 0.15) * h], -1).astype(f32)
        S0 = (R + np.tile(d, 2)).astype(f32)
        sx, sy = R[:, 0].astype(f64) + R[:, 2], R[:, 1].astype(f64) + R[:, 3]
        S1_64 = np.stack([sx - S0[:, 2], sy - S0[:, 3], sx - S0[:, 0], sy - S0[:, 1]], -1)
        S1 = S1_64.astype(f32)
        exact = (S1.astype(f64) == S1_64).all(1)
        flip = rng.random(n) < 0.5
        S0, S1 = np.where(flip[:, None], S1, S0), np.where(flip[:, None], S0, S1)
        res = []
        for name in (None, aimed_at):
            with defect(name):
                res.append((_pair_iou(_exp(S0, ef), _exp(R, ef)), _pair_iou(_exp(S1, ef), _exp(R, ef))))
        (m0, m1), (d0, d1) = res
        ok = exact & ((m0 >= m1) != (d0 >= d1)) & (np.minimum(np.minimum(m0, m1), np.minimum(d0, d1)) > 0.4)
        for i in np.nonzero(ok)[0][:want // 2 + 1]:
            frames = [[C.make_row(S0[i], _ids(rng), _conf(rng)), C.make_row(S1[i], _ids(rng), _conf(rng))], [C.make_row(R[i], _ids(rng), _conf(rng))]]
            out.append(_track_case('swap', aimed_at, frames, match_thres=0.3, expand=e))
        for S0, S1, R in _tuned_swaps(aimed_at, rng, e, want // 2):
            frames = [[C.make_row(S0, _ids(rng), _conf(rng)), C.make_row(S1, _ids(rng), _conf(rng))], [C.make_row(R, _ids(rng), _conf(rng))]]
            out.append(_track_case('swap-tuned', aimed_at, frames, match_thres=0.3, expand=e))
    return out


def tracker_score_straddles(seed, want=6):
    """Two rows far apart whose confidences are permutations of each other, new_thres set to the larger of their two left-to-right
    scores: exactly one of them starts a track; with the pairwise sum it is the other one, both or none."""
    rng = np.random.default_rng(seed)
    c, d = permuted_confidences(rng, 4000)
    s1, s2, p1, p2 = (v / f32(8.0) for v in (sum_left(c), sum_left(d), sum_pairwise(c), sum_pairwise(d)))
    thr = np.maximum(s1, s2)
    ok = ((p1 >= thr) != (s1 >= thr)) | ((p2 >= thr) != (s2 >= thr))
    out = []
    for i in np.nonzero(ok)[0][:want]:
        rows = offgrid_rows(rng, 2, hard=0.0)
        rows[0, :12], rows[1, :12] = rows[0, :12] % f32(1000), rows[1, :12] % f32(1000) + f32(2000)
        rows[0, 12:20], rows[1, 12:20] = c[i], d[i]
        out.append(_track_case('score', 'score_pairwise', [[rows[0], rows[1]]], match_thres=0.3, expand=0.3, new_thres=float(thr[i])))
    return out


_cache = {}


def tracker_cases():
    """Every constructed tracker case, by kind: {'straddle:<defect>': [...], 'exact:thr_f32': [...], 'swap:<defect>': [...],
    'score:score_pairwise': [...]}; made once per process."""
    if 'track' not in _cache:
        out = {}
        for k, name in enumerate(('expand_fma', 'den_fma', 'pred_fma', 'vel_rcp')):
            out['straddle:' + name] = tracker_straddles(name, 100 + k)
        out['exact:thr_f32'] = tracker_exact_threshold(200)
        for k, name in enumerate(('expand_fma', 'den_fma')):
            out['swap:' + name] = tracker_swaps(name, 300 + k)
        out['score:score_pairwise'] = tracker_score_straddles(400)
        _cache['track'] = out
    return _cache['track']


# ---- lp_merge_tiles -------------------------------------------------------------------------------------------------------------------------
MERGE_FRAME = (3000, 4000)
MERGE_TILES = [(0, 0, 0, 2200, 2600), (0, 300, 700, 2200, 2600)]              # (frame, y0, x0, th, tw): they share x 700..2600, y 300..2200


def _shifted(loc, tile):
    """Tile-local boxes [n, 4] in frame coordinates, by the fp32 adds of ``merge_tiles_np``."""
    return (np.asarray(loc, f32) + np.array([tile[2], tile[1], tile[2], tile[1]], f32)).astype(f32)


def _merge_case(kind, aimed_at, P, Q, conf_p, conf_q, thres, metric, rng):
    """One frame, two tiles: row P (tile-local, tile 0) and row Q (tile 1)."""
    det_t = np.zeros((2, 16, 28), f32)
    det_t[0, 0], det_t[1, 0] = C.make_row(P, _ids(rng), conf_p), C.make_row(Q, _ids(rng), conf_q)
    return dict(kind=kind, defect=aimed_at, case=(det_t, np.array([1, 1], np.int32), list(MERGE_TILES), [MERGE_FRAME]), thres=float(thres),
                metric=metric, max_det=8)


def _merge_pairs(rng, n):
    """Tile-local P (tile 0) and Q (tile 1) [n, 4] that overlap in the frame, inside the region both tiles see, far from every side."""
    x, y = full_mantissa(rng, n, 900, 2300), full_mantissa(rng, n, 500, 1900)
    w, h = full_mantissa(rng, n, 40, 90), full_mantissa(rng, n, 12, 30)
    Pf = np.stack([x, y, x + w, y + h], -1).astype(f32)
    off = np.stack([full_mantissa(rng, n, -0.5, 0.5) * w, full_mantissa(rng, n, -0.3, 0.3) * h], -1)
    Qf = (Pf + np.tile(off, 2) + full_mantissa(rng, (n, 4), -2, 2)).astype(f32)
    org = np.array([MERGE_TILES[1][2], MERGE_TILES[1][1]] * 2, f32)
    return Pf, (Qf - org).astype(f32)


def merge_cases():
    """Every constructed merge case, by kind; made once per process."""
    if 'merge' in _cache:
        return _cache['merge']
    rng = np.random.default_rng(500)
    out = {'straddle:merge_den_fma': [], 'straddle:merge_ios_min_after': [], 'exact:merge_thr_f32:iou': [], 'exact:merge_thr_f32:ios': [],
           'swap:merge_score_pairwise': []}
    hi, lo = lambda: full_mantissa(rng, 8, 0.7, 1.0), lambda: full_mantissa(rng, 8, 0.2, 0.5)   # noqa: E731
    P, Q = _merge_pairs(rng, 4096)
    a, b = _shifted(P, MERGE_TILES[0]), _shifted(Q, MERGE_TILES[1])
    qm, qd = overlap_quotient(a, b), overlap_quotient(a, b, den_fma=True)
    ok = (qm != qd) & (np.minimum(qm, qd) > 0.1) & (np.maximum(qm, qd) < 0.9)
    for i in list(np.nonzero(ok & (qm > qd))[0][:3]) + list(np.nonzero(ok & (qm < qd))[0][:3]):
        out['straddle:merge_den_fma'].append(_merge_case('straddle', 'merge_den_fma', P[i], Q[i], hi(), lo(), min(qm[i], qd[i]), 'iou', rng))
    qm, qd = overlap_quotient(a, b, 'ios'), overlap_quotient(a, b, 'ios', min_after=True)
    for i in np.nonzero((qd < qm) & (qd > 0.1))[0][:6]:
        out['straddle:merge_ios_min_after'].append(_merge_case('straddle', 'merge_ios_min_after', P[i], Q[i], hi(), lo(), qd[i], 'ios', rng))
    for metric in ('iou', 'ios'):
        for thres in MERGE_THRES:
            target = nearest_f32_above(thres)
            if target is None:
                continue
            near = np.argsort(np.abs(overlap_quotient(a, b, metric) - target))
            for i in near[:40]:
                if len(out['exact:merge_thr_f32:' + metric]) >= MIN_INSTANCES + 1:
                    break
                got = tune_to_target(lambda q: overlap_quotient(a[i][None], _shifted(q, MERGE_TILES[1]), metric), Q[i], target, rng)
                if got is not None:
                    out['exact:merge_thr_f32:' + metric].append(_merge_case('exact', 'merge_thr_f32', P[i], got, hi(), lo(), thres, metric, rng))
    c, d = permuted_confidences(rng, 4000)
    s1, s2, p1, p2 = sum_left(c), sum_left(d), sum_pairwise(c), sum_pairwise(d)
    strong = np.nonzero(overlap_quotient(a, b) > 0.6)[0]
    for k, i in enumerate(np.nonzero((s1 >= s2) != (p1 >= p2))[0][:6]):
        j = strong[k]
        out['swap:merge_score_pairwise'].append(_merge_case('swap', 'merge_score_pairwise', P[j], Q[j], c[i], d[i], 0.45, 'iou', rng))
    _cache['merge'] = out
    return out


def offgrid_merge_case(seed, max_det_t=16):
    """Two frames of five and three tiles (an overview and corner tiles that overlap) with off-grid rows: objects drawn in frame
    coordinates are seen by every tile that holds them, each time with a jitter of its own (cross-tile duplicates of IoU around 0.9),
    beside clutter; full-mantissa confidences, some of them permutations of another tile's; counts below 0 and above ``max_det_t``
    with rows behind the count."""
    rng = np.random.default_rng(seed)
    shapes = [(int(rng.integers(300, 360)), int(rng.integers(400, 480))), (int(rng.integers(200, 260)), int(rng.integers(300, 380)))]
    tiles = []
    for f, (h, w) in enumerate(shapes):
        th, tw = (h * 2) // 3, (w * 2) // 3
        corners = [(0, 0), (0, w - tw), (h - th, 0), (h - th, w - tw)] if f == 0 else [(0, 0), (h - th, w - tw)]
        tiles += [(f, 0, 0, h, w)] + [(f, y0, x0, th, tw) for y0, x0 in corners]
    det_t = np.zeros((len(tiles), max_det_t, 28), f32)
    det_t[:, :, :12] = full_mantissa(rng, (len(tiles), max_det_t, 12), 0, 200)
    det_t[:, :, 12:20] = full_mantissa(rng, (len(tiles), max_det_t, 8), 0.001, 1.0)
    count_t = np.zeros(len(tiles), np.int32)
    fill = [0] * len(tiles)
    for f, (h, w) in enumerate(shapes):
        for _ in range(14):
            bw, bh = float(rng.uniform(20, 60)), float(rng.uniform(8, 24))
            x, y = float(rng.uniform(0, w - bw)), float(rng.uniform(0, h - bh))
            conf, ids = full_mantissa(rng, 8, 0.05, 1.0), _ids(rng)
            for t, (tf, y0, x0, th, tw) in enumerate(tiles):
                if tf != f or fill[t] >= max_det_t or not (x0 <= x and y0 <= y and x + bw <= x0 + tw and y + bh <= y0 + th):
                    continue
                box = np.array([x - x0, y - y0, x + bw - x0, y + bh - y0], f32) + full_mantissa(rng, 4, -1, 1)
                box = np.clip(box, 0, [tw, th, tw, th]).astype(f32)
                c = conf[rng.permutation(8)] if rng.random() < 0.5 else full_mantissa(rng, 8, 0.05, 1.0)
                det_t[t, fill[t]] = C.make_row(box, ids, c)
                fill[t] += 1
    for t in range(len(tiles)):
        mode = int(rng.integers(0, 8))
        count_t[t] = -3 if mode == 0 else (max_det_t + 5 if mode == 1 else fill[t])
    return det_t, count_t, tiles, shapes


# ---- the share quantiser ----------------------------------------------------------------------------------------------------------------------
def quantiser_shares():
    """fp32 [18]: k / 255 rounded to fp32, one ulp below and one ulp above, for k of QUANT_KS.

    The rule truncates the fp32 product share * 255.0f.  A share whose fp32 product rounds UP to an integer k while the exact
    product is below k would be quantised differently by a float64 product -- but no fp32 has that property: with u the ulp of the
    shares around k / 255, the largest share s with 255 s < k has k - 255 s = r u, where r = k 2^p mod 255 is the 8-bit pattern of
    k rotated until its top bit is set, so r >= 128, while half an ulp of the product is at most 128 u; and for r = 128 (k a power of
    two) the product lies in the binade below k, whose half ulp is 64 u.  ``test_offgrid_cpu`` checks this at every k."""
    vals = []
    for k in QUANT_KS:
        s = f32(k) / f32(255)
        vals += [np.nextafter(s, f32(0)), s, np.nextafter(s, f32(2))]
    return np.array(vals, f32)


def edge_reads(shares, rolled=False):
    """(entries, ended_i, ended_f, ended_count): one stream with one ended record per share, every head reading id 0.  Plain: all
    eight heads of line j hold shares[j], and entry p is wildcards with id 9 at position p, so every entry is one mismatch of cost
    16 * q(shares[j]): entry 0 wins with n_hits 8 unless some head quantises otherwise.  ``rolled``: head p of line j holds
    shares[(j + p) % n], for the sightings log, which stores all eight weights."""
    shares = np.asarray(shares, f32)
    M = len(shares)
    ended_i, ended_f = np.zeros((1, M, 12), np.int32), np.zeros((1, M, 12), f32)
    ended_i[0, :, 0], ended_i[0, :, 3] = np.arange(M), 1
    for p in range(8):
        ended_f[0, :, p] = np.roll(shares, -p) if rolled else shares
    entries = np.full((8, 8), 255, np.uint8)
    entries[np.arange(8), np.arange(8)] = 9
    return entries, ended_i, ended_f, np.array([M], np.int32)


def share_votes(target, rng, tries=200):
    """fp32 confidences (a, b, c), a the largest, with fl(a / fl(fl(a + b) + c)) == ``target`` exactly: the share of a head that was
    voted id A with a, then B with b, then C with c.  None if the search finds none (a share above 1 never has one)."""
    target = f32(target)
    if not 1.0 / 3 < float(target) < 1.0:
        return None
    for _ in range(tries):
        a = full_mantissa(rng, 1, 0.5, 0.99)[0]
        rest = float(a) / float(target) - float(a)
        b = f32(rest * rng.uniform(0.35, 0.65))
        c = _ulp_step(f32(rest - float(b)), np.arange(-200, 201, dtype=np.int32))
        ok = ((a / ((a + b) + c)) == target) & (c > 0) & (c < a) & (b < a) & (b > 0)
        if ok.any():
            return a, b, c[np.nonzero(ok)[0][0]]
    return None


def share_scene(seed=7):
    """Three frames of one stream whose tracks end up with the reachable shares of ``quantiser_shares`` in their heads, eight
    targets a track: frame f votes id f + 1 in every head, with the confidences of ``share_votes``.  Returns (frames as rows per
    frame, the targets reached [n_tracks, 8])."""
    rng = np.random.default_rng(seed)
    shares = quantiser_shares()
    votes, reached = [], []
    for s in shares:
        v = share_votes(s, rng)
        if v is not None:
            votes.append(v)
            reached.append(s)
    n = min(len(votes) // 8, 8)
    assert n >= 1, 'too few reachable shares'
    votes, reached = np.array(votes[:8 * n], f32).reshape(n, 8, 3), np.array(reached[:8 * n], f32).reshape(n, 8)
    frames = []
    for f in range(3):
        rows = []
        for t in range(n):
            x, y = f32(100.37 + 200 * t + 1.3 * f), f32(50.71 + 0.4 * f)
            rows.append(C.make_row((x, y, x + f32(60.3), y + f32(20.9)), (f + 1,) * 8, votes[t, :, f]))
        frames.append(rows)
    return frames, reached


# ---- held rows ----------------------------------------------------------------------------------------------------------------------------------
HELD_KW = dict(max_tracks=8, match_thres=0.3, new_thres=NEW_THRES, expand=0.3, max_age=3)
# frames in which the object of a stream is seen.  A gap of two frames makes the next match divide the velocity by k = 3; the three
# misses behind it are held at box + vel * misses, and vel * 3 is the one product of a held row that rounds
HELD_VISIBLE = ((0, 3, 7), (0, 1, 4, 8), (0, 3), (1, 4, 8), (0, 1, 2, 3, 4, 5, 6, 7, 8), (0, 3, 6))
HELD_STREAMS = 2 * len(HELD_VISIBLE)


def held_calls(seed=9, n_frames=9):
    """HELD_STREAMS streams with one object each, seen in the frames HELD_VISIBLE[s % 6]: full-mantissa positions within a few
    pixels of the origin and velocities of up to 2 px a frame, so that a coordinate is about as small as vel * k and one ulp of the
    velocity, or of the product, shows in the held row (an object at x = 1000 hides both).  Ten tracks are held at misses = 3 after a
    velocity that was divided by 3.  Calls of 4, 1 and 4 time steps with one frame per stream each; the last one flushes."""
    rng = np.random.default_rng(seed)
    S = HELD_STREAMS
    p0 = full_mantissa(rng, (S, 2), 2, 16)
    v = np.stack([full_mantissa(rng, S, -2, 2), full_mantissa(rng, S, -0.7, 0.7)], -1)
    wh = np.stack([full_mantissa(rng, S, 40, 90), full_mantissa(rng, S, 12, 30)], -1)
    ids = [_ids(rng) for _ in range(S)]
    frames = []
    for f in range(n_frames):
        for s in range(S):
            rows = []
            if f in HELD_VISIBLE[s % len(HELD_VISIBLE)]:
                c = (p0[s] + v[s] * f32(f) + full_mantissa(rng, 2, -0.3, 0.3)).astype(f32)
                rows.append(C.make_row((c[0], c[1], c[0] + wh[s, 0], c[1] + wh[s, 1]), ids[s], _conf(rng)))
            frames.append(rows)
    det, count = C.frames_of(frames, 2)
    cut = [0, 4 * S, 5 * S, n_frames * S]
    return [(det[a:b], count[a:b], list(range(S)) * ((b - a) // S), [int(b == cut[-1])] * S) for a, b in zip(cut[:-1], cut[1:])]


def held_maps():
    """(lines, zones, planes) per stream for the held scene: sixteen gates across the few pixels the anchors travel, two zones, and
    the first plane of ``test_speed_cpu.speed_planes``.  Zones and speed read the tracker's STORED box (the last detection), never
    the velocity or a held row, so no rounding of the held geometry can reach them: they are run on this scene for its off-grid
    stored boxes."""
    import test_speed_cpu as P
    S = HELD_STREAMS
    lines = [[(float(x), -50.0, float(x), 200.0) for x in range(20, 84, 4)] for _ in range(S)]
    zones = [[([(0, -50), (45, -50), (45, 200), (0, 200)], 1), ([(45, -50), (300, -50), (300, 200), (45, 200)], 2)] for _ in range(S)]
    return lines, zones, [P.speed_planes()[0]] * S


def run_held_addons_np():
    """The held scene through ``PlateTrackerNp`` (as patched at the moment) with hold, zones and speed: per call a dict of det_hold and
    the zone and speed outputs with their memos."""
    from yolov6.utils import track
    from yolov6.utils.speed import GroundPlaneNp
    from yolov6.utils.zones import ZoneMapNp
    lines, zones, planes = held_maps()
    trk = track.PlateTrackerNp(HELD_STREAMS, **HELD_KW)
    trk.enable_hold()
    trk.enable_zones(ZoneMapNp(HELD_STREAMS, lines, zones), min_hits=1)
    trk.enable_speed(GroundPlaneNp(HELD_STREAMS, planes), min_hits=1, confirm=2)
    outs = []
    for det, count, stream_of, flush in held_calls():
        trk.update(det, count, stream_of, flush, 6)
        out = dict(det_hold=trk.last_hold[0], n_held=trk.last_hold[1] - np.clip(count, 0, det.shape[1]), zone_memo=trk.zone_memo, speed_memo=trk.speed_memo())
        out.update(zip(('zone_ev', 'zone_count', 'zone_occ', 'zone_totals'), trk.last_zone))
        out.update(zip(('speed_i', 'speed_ev', 'speed_count'), trk.last_speed))
        outs.append({k: np.array(v, copy=True) for k, v in out.items()})
    return trk, outs


# ---- running the specification ------------------------------------------------------------------------------------------------------------------
def run_tracker_np(calls, n_streams, max_ended, hold=False, **kw):
    """The calls through a fresh ``PlateTrackerNp`` (as patched at the moment): (tracker, [outputs by name per call])."""
    from yolov6.utils import track
    trk = track.PlateTrackerNp(n_streams, **kw)
    if hold:
        trk.enable_hold()
    outs = []
    for det, count, stream_of, flush in (c[:4] for c in calls):
        o = trk.update(det, count, stream_of, flush, max_ended)
        out = dict(zip(('det_out', 'tid', 'ended_i', 'ended_f', 'ended_count'), (np.array(a, copy=True) for a in o)))
        if hold:
            out.update(zip(('det_hold', 'count_hold', 'tid_hold'), (np.array(a, copy=True) for a in trk.last_hold)))
        outs.append(out)
    return trk, outs


def differing(a, b):
    """Sorted names of the outputs in which two runs (lists of dicts of arrays) differ in any bit."""
    names = set()
    for x, y in zip(a, b):
        for k in x:
            if x[k].shape != y[k].shape or not np.array_equal(np.ascontiguousarray(x[k]).view(np.uint8), np.ascontiguousarray(y[k]).view(np.uint8)):
                names.add(k)
    return sorted(names)


# (seed, n_streams, max_tracks, max_det, frames per call, objects per stream, extent, max_age): shipped cases of test_track_gpu.CASES
TWINS = {
    's3-t4-d20': (13, 3, 4, 20, (8, 2, 5, 7, 1, 6, 3, 4), 8, 500, 3),
    's9-t16-d20': (14, 9, 16, 20, (70, 3, 66, 1, 9, 65), 8, 600, 0),
    's3-t128-d128': (15, 3, 128, 128, (3, 2, 3, 1, 2, 3), 190, 2500, 3),
}


def twin_case(name, expand, match_thres):
    """(calls, n_streams, tracker parameters) of the off-grid twin of a shipped case."""
    seed, S, T, max_det, Bs, n_obj, extent, max_age = TWINS[name]
    calls = offgrid_twin(C.random_track_case(seed, n_streams=S, max_det=max_det, n_obj=n_obj, extent=extent, Bs=Bs), 1000 + seed)
    return calls, S, dict(max_tracks=T, match_thres=match_thres, new_thres=NEW_THRES, expand=expand, max_age=max_age)


def full_matrix_calls(seed=3):
    """``test_track_update_full_matrix`` with a fractional jitter and full-mantissa confidences: 128 slots x 128 rows, every pair
    above the threshold, thousands of near-equal IoUs for the sort and the settle."""
    rng = np.random.default_rng(seed)
    rows = [C.make_row((k % 7, k % 5, 1000 + k, 1000 + (k % 11)), ids=rng.integers(0, 24, 8), conf=full_mantissa(rng, 8, 0.05, 1.0)) for k in range(128)]
    frames = []
    for f in range(3):
        cur = [rows[i].copy() for i in rng.permutation(128)]
        for r in cur:
            r[0:4] += full_mantissa(rng, 4, -2, 2)
        frames.append(cur)
    det, count = C.frames_of(frames, 128)
    return [(det[:1], count[:1], [0], [0]), (det[1:], count[1:], [0, 0], [1])]
