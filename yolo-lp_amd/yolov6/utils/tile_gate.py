"""Skipping the unchanged tiles of fixed-camera frames in tiled detection: the rule, on the CPU.

This module is the written-down specification of ``lp_tile_gate_luma_batch`` and ``lp_tile_gate_update`` (include/lp_hip.h,
csrc/lp_tile_gate.hip), which match ``luma_blocks_np`` and ``gate_update_np`` on every integer, and ``TileGateNp`` is the CPU
form of ``yolov6.hip.runtime.TileGate`` and what the CPU path of ``Inferer(tile=..., tile_gate=True)`` runs.  On a fixed camera
nearly every tile of a frame shows the pixels of the frame before; a tile that has not changed yields the same detections again,
so its forward is skipped and its rows come from a cache.  Everything is integer.

Luma.  A BGR frame gives L = (29 B + 150 G + 77 R + 128) >> 8 (255 on white, 0 on black); an NV12 frame gives L = Y, its chroma
plane is never read (a change of chroma alone is invisible there).
Block sums.  S[by, bx] = the sum of L over the frame pixels y in [4 by, min(4 by + 4, h)), x in [4 bx, min(4 bx + 4, w)):
uint16 [ceil(h / 4), ceil(w / 4)], at most 4080.
Tile region.  Tile (y0, x0, th, tw) owns the blocks by in [y0 >> 2, (y0 + th - 1) >> 2], bx likewise: every block it overlaps
(conservative by up to 3 pixels where an origin is no multiple of 4, which can only cause one more forward).  The overview tile
owns the whole grid.
Cells.  Inside a tile's block range cells are 4 x 4 blocks (16 x 16 px) anchored at the tile's first block; the cells at the end
of a range are smaller.  npix(cell) = the frame pixels in its blocks (blocks are clipped by the frame only), A(cell) = the sum
of |S_cur - S_ref| over its blocks in int32; the cell is CHANGED iff 16 A > thres16 * npix, thres16 = floor(thres * 16 + 1/2),
``thres`` in luma levels per pixel, 0..255.
State per (stream, tile): ref uint16 [nby, nbx] and age int32, -1 = never detected.
Per call and tile: ncell = the number of changed cells (0 for a never-detected tile: its ref is not read);
    flag = age < 0  or  ncell >= min_cells  or  (refresh > 0 and age + 1 >= refresh).
Flagged: ref <- S_cur over the whole region; age <- t_local % refresh if age was -1 and refresh > 0 (t_local = the index of the tile
in its stream's plan: the periodic refreshes of a stream's tiles are staggered over the period instead of falling on one call),
else age <- 0.  Not flagged: ref is untouched and age += 1.
So a tile's ref is always the frame its cached detections were computed on: slow drift accumulates against that frame until it
crosses the threshold; it cannot creep past unnoticed the way it would with a running reference.
A frame with stream -1 is not gated: all its tiles are flagged, no state is read or written, nothing is cached.

Defaults thres = 2.0, min_cells = 1, refresh = 50: choices, not measurements -- there is no footage here to tune them on.  What
places them: for Gaussian sensor noise of sigma 2 on both frames the difference of two block sums is the sum of 16 differences of
sigma 2 sqrt(2), sigma_block = 8 sqrt(2) = 11.3; its magnitude has mean 11.3 sqrt(2 / pi) = 9.0 and deviation 11.3 sqrt(1 - 2 / pi) =
6.8, so the A of a full cell (16 blocks) has mean about 144 and deviation about 27, against a bar of thres * 256 = 512: more
than thirteen deviations.  At sigma 5 the mean is 361 and the deviation 68: the bar is only about two deviations away and ``thres``
must be raised.  (The rounding of L is ignored in this arithmetic.)

Illumination (``illum='gain'``, opt-in; ``gate_update_gain_np`` = ``lp_tile_gate_update_gain`` on every integer).  An exposure step, a
cloud or dusk moves every pixel of a tile by a common factor, which the rule above reads as a change of every cell.  In gain mode
a tile's cells are compared after the reference is scaled by ONE gain per tile, estimated robustly.  ONE = 4096 (Q12); every
intermediate fits int32, the one division is of two unsigned 32-bit values.
Range.  hi = floor(max_gain * 4096 + 1/2) with max_gain in [1, 4], so hi <= 16384; lo = ceil(4096 * 4096 / hi) (``check_illum``).
Gain of a cell.  R_c / C_c = the sum of ref / of the current block sums over the cell's blocks, both <= 16 * 4080 = 65280.  A cell
with R_c == 0 has no gain; otherwise g_c = min((C_c * 4096 + (R_c >> 1)) / R_c, 65535) (C_c * 4096 <= 267386880).
Gain of the tile.  m = the cells that have a gain.  m == 0: G_raw = 4096.  Otherwise G_raw = the LOWER MEDIAN, the value of rank
(m - 1) // 2 (0-based) of the sorted g_c: the illumination is the factor most cells agree on, and a car that enters the tile must
neither bias the gain (the mean ratio sum(cur) / sum(ref) is biased by it, enough to mark every cell) nor be hidden by it.
out_of_range = G_raw < lo or G_raw > hi; G = clamp(G_raw, lo, hi).
Changed cell.  A_g(cell) = the sum over its blocks of |S_cur * 4096 - S_ref * G| (a term <= 4080 * 16384 = 66846720, 16 terms
< 2^31); the cell is CHANGED iff A_g > thres16 * npix * 256 (<= 267386880).  With G == 4096 this is 16 A > thres16 * npix exactly.
Per call and tile: flag = age < 0 or out_of_range or ncell >= min_cells or (refresh > 0 and age + 1 >= refresh); ref and age move
as above; gain = G_raw.  A never-detected tile gives (flag, ncell, gain) = (1, 0, 0): its ref is not read.  So the reference is
still the frame the cached rows were computed on, and the gain is always measured against that frame: drift accumulates in G_raw
until it leaves [lo, hi], then the tile is detected again and the gain starts from 4096.
What it does not do: one gain per tile and no offset term (haze, a veiling glare); a shadow EDGE that crosses a tile re-detects it
(a half-tile step of 0.8 changes 128 of 320 cells); the overview tile sees one gain for the whole frame; a uniform object that
fills more than half of a tile on a uniform background reads as illumination, up to max_gain; saturated regions do not follow
the gain and re-detect; the cached confidences are those of the reference frame's exposure.  illum = 'none' and max_gain = 1.5
are choices like the other defaults, not tuned on footage.
"""
import numpy as np

from yolov6.utils.nv12 import Nv12Frame

MAX_THRES16 = 255 * 16
DEFAULTS = dict(thres=2.0, min_cells=1, refresh=50)
ONE = 4096                                              # a gain of 1 in Q12
MAX_CELL_GAIN = 65535                                   # the cap of a cell's gain: 16 bits


def check_params(thres=2.0, min_cells=1, refresh=50):
    """(thres16, min_cells, refresh) of the public parameters, checked: 0 <= thres <= 255, min_cells >= 1, refresh >= 0."""
    t = float(thres)
    if not 0.0 <= t <= 255.0:
        raise ValueError('tile gate: thres must be in [0, 255] luma levels per pixel')
    if int(min_cells) != min_cells or int(min_cells) < 1:
        raise ValueError('tile gate: min_cells must be an integer >= 1')
    if int(refresh) != refresh or int(refresh) < 0:
        raise ValueError('tile gate: refresh must be an integer >= 0 (0: no periodic refresh)')
    return int(np.floor(t * 16.0 + 0.5)), int(min_cells), int(refresh)


def check_illum(illum='none', max_gain=1.5):
    """(lo, hi), the Q12 range of a tile's gain, of the public parameters, checked: ``illum`` 'none' or 'gain', 1 <= max_gain <= 4."""
    if illum not in ('none', 'gain'):
        raise ValueError("tile gate: illum must be 'none' or 'gain'")
    try:
        g = float(max_gain)
    except (TypeError, ValueError):
        raise ValueError('tile gate: max_gain must be a number in [1, 4]')
    if not 1.0 <= g <= 4.0:                             # (false for a NaN too)
        raise ValueError('tile gate: max_gain must be in [1, 4]')
    hi = int(np.floor(g * ONE + 0.5))
    return -(-ONE * ONE // hi), hi


def grid_shape(h, w):
    """(nby, nbx) of the block grid of an h x w frame."""
    return (int(h) + 3) // 4, (int(w) + 3) // 4


def luma_np(frame):
    """L uint8 [h, w] of a host frame: a BGR array [h, w, 3] or an ``Nv12Frame`` with numpy planes."""
    if isinstance(frame, Nv12Frame):
        return np.ascontiguousarray(np.asarray(frame.y)[:frame.h, :frame.w])
    f = np.asarray(frame)
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
        raise ValueError('a BGR frame is a uint8 array [h, w, 3]')
    f = f.astype(np.int32)
    return ((29 * f[:, :, 0] + 150 * f[:, :, 1] + 77 * f[:, :, 2] + 128) >> 8).astype(np.uint8)


def luma_blocks_np(frame):
    """S uint16 [ceil(h / 4), ceil(w / 4)] of a host frame (BGR array or ``Nv12Frame``)."""
    L = luma_np(frame).astype(np.int64)
    h, w = L.shape
    nby, nbx = grid_shape(h, w)
    pad = np.zeros((4 * nby, 4 * nbx), np.int64)
    pad[:h, :w] = L
    return pad.reshape(nby, 4, nbx, 4).sum(axis=(1, 3)).astype(np.uint16)


def tile_blocks(tile):
    """(by0, by1, bx0, bx1), both ends included, of a tile (y0, x0, th, tw)."""
    y0, x0, th, tw = (int(v) for v in tile[-4:])
    return y0 >> 2, (y0 + th - 1) >> 2, x0 >> 2, (x0 + tw - 1) >> 2


def _block_pixels(h, w, by0, by1, bx0, bx1):
    """int64 [nby, nbx]: frame pixels of every block of a range."""
    rows = np.minimum(4 * np.arange(by0, by1 + 1) + 4, h) - 4 * np.arange(by0, by1 + 1)
    cols = np.minimum(4 * np.arange(bx0, bx1 + 1) + 4, w) - 4 * np.arange(bx0, bx1 + 1)
    return rows[:, None].astype(np.int64) * cols[None, :]


def _cells(a):
    """Sums of an int64 [nby, nbx] array over cells of 4 x 4 anchored at (0, 0): [ceil(nby / 4), ceil(nbx / 4)]."""
    ncy, ncx = (a.shape[0] + 3) // 4, (a.shape[1] + 3) // 4
    pad = np.zeros((4 * ncy, 4 * ncx), np.int64)
    pad[:a.shape[0], :a.shape[1]] = a
    return pad.reshape(ncy, 4, ncx, 4).sum(axis=(1, 3))


def changed_cells(cur, ref, frame_hw, tile, thres16):
    """ncell of one tile: ``cur`` = the frame's block grid, ``ref`` = the tile's reference [nby, nbx]."""
    by0, by1, bx0, bx1 = tile_blocks(tile)
    region = cur[by0:by1 + 1, bx0:bx1 + 1].astype(np.int64)
    A = _cells(np.abs(region - ref.astype(np.int64)))
    npix = _cells(_block_pixels(frame_hw[0], frame_hw[1], by0, by1, bx0, bx1))
    return int((16 * A > int(thres16) * npix).sum())


def cell_gains_np(cur, ref, tile):
    """(g, has) of one tile, both [ncy, ncx]: ``has`` = the cell has a gain (R_c > 0), ``g`` int64 = its g_c (0 where it has none)."""
    by0, by1, bx0, bx1 = tile_blocks(tile)
    C = _cells(cur[by0:by1 + 1, bx0:bx1 + 1].astype(np.int64))
    R = _cells(ref.astype(np.int64))
    has = R > 0
    Rs = np.where(has, R, 1)
    g = np.minimum((C * ONE + (Rs >> 1)) // Rs, MAX_CELL_GAIN)
    return np.where(has, g, 0), has


def tile_gain_np(g, has):
    """G_raw of one tile: the lower median of the gains of the cells that have one, 4096 when no cell has."""
    v = np.sort(np.asarray(g)[np.asarray(has)], axis=None)
    return ONE if v.size == 0 else int(v[(v.size - 1) // 2])


def changed_cells_gain(cur, ref, frame_hw, tile, thres16, G):
    """ncell of one tile in gain mode, ``G`` = the tile's clamped gain: the cells with A_g > thres16 * npix * 256."""
    by0, by1, bx0, bx1 = tile_blocks(tile)
    region = cur[by0:by1 + 1, bx0:bx1 + 1].astype(np.int64)
    A = _cells(np.abs(region * ONE - ref.astype(np.int64) * int(G)))
    npix = _cells(_block_pixels(frame_hw[0], frame_hw[1], by0, by1, bx0, bx1))
    return int((A > int(thres16) * npix * 256).sum())


class GateState:
    """The persistent state of a gate: per stream the fixed frame shape and tile plan, per (stream, tile) ``ref`` and ``age``."""

    def __init__(self, frame_shapes, plans):
        self.shapes = [(int(s[0]), int(s[1])) for s in frame_shapes]
        self.plans = [[tuple(int(v) for v in t[-4:]) for t in plan] for plan in plans]
        for (h, w), plan in zip(self.shapes, self.plans):
            for y0, x0, th, tw in plan:
                if y0 < 0 or x0 < 0 or th < 1 or tw < 1 or y0 + th > h or x0 + tw > w:
                    raise ValueError('tile gate: a tile is not inside its %d x %d frame' % (h, w))
        self.ref = [[np.zeros(self._region(t), np.uint16) for t in plan] for plan in self.plans]
        self.age = [np.full(len(plan), -1, np.int32) for plan in self.plans]

    @staticmethod
    def _region(tile):
        by0, by1, bx0, bx1 = tile_blocks(tile)
        return by1 - by0 + 1, bx1 - bx0 + 1

    def reset(self, streams=None):
        for s in (range(len(self.plans)) if streams is None else streams):
            self.age[int(s)][:] = -1


def check_streams(stream_of, n_frames, n_streams):
    """``stream_of`` of a call as a list (default range(n_frames)): -1 or 0..n_streams-1, a stream at most once."""
    so = list(range(n_frames)) if stream_of is None else [int(s) for s in stream_of]
    if len(so) != n_frames:
        raise ValueError('tile gate: %d streams for %d frames' % (len(so), n_frames))
    seen = set()
    for f, s in enumerate(so):
        if s < -1 or s >= n_streams:
            raise ValueError('tile gate: stream %d of frame %d (need -1 or 0..%d)' % (s, f, n_streams - 1))
        if s >= 0 and s in seen:
            raise ValueError('tile gate: stream %d appears twice in one call (at most one frame per stream and call)' % s)
        seen.add(s)
    return so


def gate_update_np(state, grids, stream_of, thres16, min_cells, refresh):
    """One call of the rule on ``state`` (updated in place): ``grids[f]`` = the block grid of frame f (None for stream -1),
    ``stream_of[f]`` its stream.  Returns (flags, ncell), per frame a list over the tiles of its stream; a frame of stream -1
    gets ([], [])."""
    flags, ncells = [], []
    for cur, s in zip(grids, stream_of):
        if s < 0:
            flags.append([])
            ncells.append([])
            continue
        h, w = state.shapes[s]
        if cur.shape != grid_shape(h, w):
            raise ValueError('tile gate: the grid of stream %d must be %s' % (s, grid_shape(h, w)))
        fl, nc = [], []
        for t, tile in enumerate(state.plans[s]):
            age = int(state.age[s][t])
            n = 0 if age < 0 else changed_cells(cur, state.ref[s][t], (h, w), tile, thres16)
            flag = age < 0 or n >= min_cells or (refresh > 0 and age + 1 >= refresh)
            if flag:
                by0, by1, bx0, bx1 = tile_blocks(tile)
                state.ref[s][t] = cur[by0:by1 + 1, bx0:bx1 + 1].astype(np.uint16).copy()
                state.age[s][t] = t % refresh if (age < 0 and refresh > 0) else 0
            else:
                state.age[s][t] = age + 1
            fl.append(1 if flag else 0)
            nc.append(n)
        flags.append(fl)
        ncells.append(nc)
    return flags, ncells


def gate_update_gain_np(state, grids, stream_of, thres16, min_cells, refresh, lo, hi):
    """``gate_update_np`` in gain mode, (lo, hi) from ``check_illum``.  Returns (flags, ncell, gain): gain = G_raw per tile, 0 for
    a never-detected tile; a frame of stream -1 gets ([], [], [])."""
    flags, ncells, gains = [], [], []
    for cur, s in zip(grids, stream_of):
        if s < 0:
            flags.append([])
            ncells.append([])
            gains.append([])
            continue
        h, w = state.shapes[s]
        if cur.shape != grid_shape(h, w):
            raise ValueError('tile gate: the grid of stream %d must be %s' % (s, grid_shape(h, w)))
        fl, nc, gn = [], [], []
        for t, tile in enumerate(state.plans[s]):
            age = int(state.age[s][t])
            n = g_raw = 0
            out_of_range = False
            if age >= 0:
                g_raw = tile_gain_np(*cell_gains_np(cur, state.ref[s][t], tile))
                out_of_range = g_raw < lo or g_raw > hi
                n = changed_cells_gain(cur, state.ref[s][t], (h, w), tile, thres16, min(max(g_raw, lo), hi))
            flag = age < 0 or out_of_range or n >= min_cells or (refresh > 0 and age + 1 >= refresh)
            if flag:
                by0, by1, bx0, bx1 = tile_blocks(tile)
                state.ref[s][t] = cur[by0:by1 + 1, bx0:bx1 + 1].astype(np.uint16).copy()
                state.age[s][t] = t % refresh if (age < 0 and refresh > 0) else 0
            else:
                state.age[s][t] = age + 1
            fl.append(1 if flag else 0)
            nc.append(n)
            gn.append(g_raw)
        flags.append(fl)
        ncells.append(nc)
        gains.append(gn)
    return flags, ncells, gains


def count_out_of_range(gains, lo, hi):
    """The tiles of a call whose gain was estimated (not 0) and lies outside [lo, hi]."""
    return sum(1 for gn in gains for g in gn if g and not lo <= g <= hi)


class TileGateNp:
    """``runtime.TileGate`` on the CPU.  ``detect_tiles(frames, tiles, tile_max_det)`` -> (det_t [>= len(tiles), tile_max_det, 28]
    fp32, count_t [>= len(tiles)]) is the per-tile detector: ``tiles`` is a list of (frame index, y0, x0, th, tw) into ``frames``,
    the rows are in tile-local source pixels, rounded (what ``merge_tiles_np`` takes).  ``frame_shapes[s]`` is the fixed shape of
    stream s; ``tile_hw`` the tile size.  ``detect_padded(frames, stream_of=None)`` returns (det [F, max_det, 28], count [F]) as
    ``merge_tiles_np`` does, running ``detect_tiles`` on the flagged tiles only (not at all when nothing is flagged) and taking
    the rows of the others from the cache.  With ``illum='gain'`` the rule is ``gate_update_gain_np``'s with the range of
    ``max_gain``; ``last_gain`` then holds the G_raw of the last call per frame and tile (0: no estimate; all 0 with 'none') and
    ``stats`` has ``tiles_out_of_range`` (estimated gains outside the range; a tile gone entirely black has G_raw 0 and is not
    counted)."""

    def __init__(self, detect_tiles, frame_shapes, tile_hw, iou_thres, max_det, overlap=0.2, overview=True, metric='iou', border=1,
                 tile_max_det=None, thres=2.0, min_cells=1, refresh=50, illum='none', max_gain=1.5):
        from yolov6.core.tiles import plan_tiles
        from yolov6.utils.tiles import MAX_CANDIDATES, MAX_TILES_PER_FRAME
        self.thres16, self.min_cells, self.refresh = check_params(thres, min_cells, refresh)
        self.gain_lo, self.gain_hi = check_illum(illum, max_gain)
        self.illum = illum
        self.detect_tiles = detect_tiles
        self.tile_hw, self.overlap, self.overview = tile_hw, overlap, overview
        self.iou_thres, self.max_det, self.metric, self.border = float(iou_thres), int(max_det), metric, int(border)
        plans = [plan_tiles(s, tile_hw, overlap, overview) for s in frame_shapes]
        most = max(len(p) for p in plans)
        if most > MAX_TILES_PER_FRAME:
            raise ValueError('%d tiles for one frame (at most %d): use larger tiles or a smaller overlap' % (most, MAX_TILES_PER_FRAME))
        self.tile_max_det = max(1, min(self.max_det, MAX_CANDIDATES // most)) if tile_max_det is None else int(tile_max_det)
        self.state = GateState(frame_shapes, plans)
        self.n_streams = len(plans)
        self.cache_det = [np.zeros((len(p), self.tile_max_det, 28), np.float32) for p in plans]
        self.cache_count = [np.zeros(len(p), np.int32) for p in plans]
        self.last_flags, self.last_ncell, self.last_gain = [], [], []
        self.stats = dict(calls=0, tiles_seen=0, tiles_detected=0, forwards=0)
        if illum == 'gain':
            self.stats['tiles_out_of_range'] = 0

    def reset(self, streams=None):
        """Forget ``streams`` (all for None): their tiles count as never detected, their cached rows are cleared."""
        self.state.reset(streams)
        for s in (range(self.n_streams) if streams is None else streams):
            self.cache_det[int(s)][:] = 0
            self.cache_count[int(s)][:] = 0

    def detect_padded(self, frames, stream_of=None):
        from yolov6.core.tiles import plan_tiles
        from yolov6.utils.tiles import merge_tiles_np
        so = check_streams(stream_of, len(frames), self.n_streams)
        for f, s in zip(frames, so):
            if s >= 0 and tuple(f.shape[:2]) != self.state.shapes[s]:
                raise ValueError('tile gate: a frame of %s on stream %d, whose frames are %s: a stream has one fixed frame size'
                                 % (tuple(f.shape[:2]), s, self.state.shapes[s]))
        grids = [None if s < 0 else luma_blocks_np(f) for f, s in zip(frames, so)]
        if self.illum == 'gain':
            flags, ncell, gain = gate_update_gain_np(self.state, grids, so, self.thres16, self.min_cells, self.refresh, self.gain_lo,
                                                     self.gain_hi)
            self.stats['tiles_out_of_range'] += count_out_of_range(gain, self.gain_lo, self.gain_hi)
        else:
            flags, ncell = gate_update_np(self.state, grids, so, self.thres16, self.min_cells, self.refresh)
            gain = [[0] * len(fl) for fl in flags]
        plans = [self.state.plans[s] if s >= 0 else plan_tiles(f.shape, self.tile_hw, self.overlap, self.overview)
                 for f, s in zip(frames, so)]
        flags = [fl if s >= 0 else [1] * len(p) for fl, s, p in zip(flags, so, plans)]
        ncell = [nc if s >= 0 else [0] * len(p) for nc, s, p in zip(ncell, so, plans)]
        gain = [gn if s >= 0 else [0] * len(p) for gn, s, p in zip(gain, so, plans)]
        todo = [(f, t) for f, fl in enumerate(flags) for t, on in enumerate(fl) if on]
        tmd = self.tile_max_det
        fresh = {}
        if todo:
            det_t, count_t = self.detect_tiles(frames, [(f,) + tuple(plans[f][t]) for f, t in todo], tmd)
            det_t, count_t = np.asarray(det_t, np.float32), np.asarray(count_t)
            for k, (f, t) in enumerate(todo):
                n = min(max(int(count_t[k]), 0), tmd)
                rows = np.zeros((tmd, 28), np.float32)
                rows[:n] = det_t[k, :n]
                if so[f] >= 0:
                    self.cache_det[so[f]][t], self.cache_count[so[f]][t] = rows, n
                else:
                    fresh[(f, t)] = (rows, n)
        tiles = [(f,) + tuple(t) for f, p in enumerate(plans) for t in p]
        rows = [self.cache_det[so[f]][t] if so[f] >= 0 else fresh[(f, t)][0] for f, p in enumerate(plans) for t in range(len(p))]
        counts = [self.cache_count[so[f]][t] if so[f] >= 0 else fresh[(f, t)][1] for f, p in enumerate(plans) for t in range(len(p))]
        det, count, _ = merge_tiles_np(np.stack(rows), np.asarray(counts, np.int32), tiles, [f.shape for f in frames], self.iou_thres,
                                       self.max_det, self.metric, self.border)
        self.last_flags, self.last_ncell, self.last_gain = flags, ncell, gain
        self.stats['calls'] += 1
        self.stats['tiles_seen'] += len(tiles)
        self.stats['tiles_detected'] += len(todo)
        self.stats['forwards'] += 1 if todo else 0
        return det, count

    def detect(self, frames, stream_of=None):
        """Unpadded: a list of [n_f, 28] arrays."""
        det, count = self.detect_padded(frames, stream_of)
        return [det[f, :int(count[f])].copy() for f in range(len(frames))]
