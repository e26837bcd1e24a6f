"""The tile gate on the CPU (yolov6/utils/tile_gate.py, the specification of lp_tile_gate_luma_batch and lp_tile_gate_update):
``luma_blocks_np`` against loops over Python integers, the rule on ``TileGateNp`` with a stub detector that records the tiles it
is given, the cache semantics, the argument checks of the two C entry points (no device needed) and
``tools/infer.py --tile ... --tile-gate`` on the CPU path.  ``blocks_loops``, ``ncell_loops``, ``pitched_nv12`` and ``StubDetector``
are shared with tests/test_tile_gate_gpu.py."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

LP_ERR_ARG = -1
f32 = np.float32
SHAPE, TILE, OVERLAP = (70, 100), (32, 48), 8          # y origins 0, 24, 38 (no multiple of 4), x origins 0, 40, 52; plus the overview


# ---- the rule once more, as loops over Python integers --------------------------------------------------------------------------------
def luma_loops(frame):
    """L as a list of rows of Python integers: a BGR array or an ``Nv12Frame``."""
    from yolov6.utils.nv12 import Nv12Frame
    if isinstance(frame, Nv12Frame):
        return [[int(frame.y[y, x]) for x in range(frame.w)] for y in range(frame.h)]
    return [[(29 * int(p[0]) + 150 * int(p[1]) + 77 * int(p[2]) + 128) >> 8 for p in row] for row in frame]


def blocks_loops(frame):
    L = luma_loops(frame)
    h, w = len(L), len(L[0])
    out = np.zeros(((h + 3) // 4, (w + 3) // 4), np.uint16)
    for by in range(out.shape[0]):
        for bx in range(out.shape[1]):
            out[by, bx] = sum(L[y][x] for y in range(4 * by, min(4 * by + 4, h)) for x in range(4 * bx, min(4 * bx + 4, w)))
    return out


def ncell_loops(cur, ref, hw, tile, thres16):
    """Changed cells of one tile by the words of the rule; ``ref`` is the tile's [nby, nbx] reference."""
    h, w = hw
    y0, x0, th, tw = tile
    by0, by1, bx0, bx1 = y0 >> 2, (y0 + th - 1) >> 2, x0 >> 2, (x0 + tw - 1) >> 2
    n = 0
    for cy in range(by0, by1 + 1, 4):
        for cx in range(bx0, bx1 + 1, 4):
            A = npix = 0
            for by in range(cy, min(cy + 4, by1 + 1)):
                for bx in range(cx, min(cx + 4, bx1 + 1)):
                    A += abs(int(cur[by, bx]) - int(ref[by - by0, bx - bx0]))
                    npix += (min(4 * by + 4, h) - 4 * by) * (min(4 * bx + 4, w) - 4 * bx)
            n += 16 * A > thres16 * npix
    return n


def pitched_nv12(rng, h, w, pitch):
    """A host ``Nv12Frame`` whose luma rows are ``pitch`` bytes apart, the padding filled with other bytes."""
    from yolov6.utils.nv12 import Nv12Frame
    ybuf = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    uv = rng.integers(0, 256, (h // 2, w // 2, 2), dtype=np.uint8)
    return Nv12Frame(ybuf[:, :w], uv)


class StubDetector:
    """One row per tile, its box, scores and ids a function of the tile's pixels; ``calls`` records the tiles of every call."""

    def __init__(self):
        self.calls = []

    def __call__(self, frames, tiles, tmd):
        self.calls.append([tuple(t) for t in tiles])
        det, count = np.zeros((len(tiles), tmd, 28), f32), np.zeros(len(tiles), np.int32)
        for k, (f, y0, x0, th, tw) in enumerate(tiles):
            px = frames[f].y if hasattr(frames[f], 'y') else frames[f]               # (an Nv12Frame: its luma plane)
            v = int(np.asarray(px)[y0:y0 + th, x0:x0 + tw].astype(np.int64).sum())
            x1, y1 = 3 + v % 5, 3 + (v // 5) % 4
            det[k, 0, :4] = [x1, y1, x1 + 14, y1 + 9]
            det[k, 0, 4:12] = [x1, y1, x1 + 14, y1, x1 + 14, y1 + 9, x1, y1 + 9]
            det[k, 0, 12:20] = (v % 89 + 10) / 100.0
            det[k, 0, 20:28] = v % 7
            count[k] = 1
        return det, count


def base_frame(seed=0, shape=SHAPE):
    """A BGR frame with channels in 0..200, so that + 40 on every channel is + 40 of luma exactly."""
    return np.random.default_rng(seed).integers(0, 201, shape + (3,), dtype=np.uint8)


def raised(frame, ys, xs, by):
    out = frame.copy()
    out[ys, xs] = (out[ys, xs].astype(np.int32) + by).astype(np.uint8)
    return out


def make_gate(stub=None, shapes=(SHAPE,), **kw):
    from yolov6.utils.tile_gate import TileGateNp
    return TileGateNp(stub or StubDetector(), list(shapes), TILE, 0.45, 20, overlap=OVERLAP, **kw)


def owners(plan, by, bx):
    """The tiles of a plan whose block range holds block (by, bx)."""
    return [int(y0 >> 2 <= by <= (y0 + th - 1) >> 2 and x0 >> 2 <= bx <= (x0 + tw - 1) >> 2) for y0, x0, th, tw in plan]


# ---- luma_blocks_np ---------------------------------------------------------------------------------------------------------------------
def test_luma_blocks_np_against_the_loops():
    from yolov6.utils.tile_gate import grid_shape, luma_blocks_np, luma_np
    rng = np.random.default_rng(1)
    sizes = [(h, w) for h in (1, 3, 4, 5, 17) for w in (1, 3, 4, 5, 17)] + [SHAPE]
    for h, w in sizes:
        frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        got = luma_blocks_np(frame)
        assert got.dtype == np.uint16 and got.shape == grid_shape(h, w) == ((h + 3) // 4, (w + 3) // 4)
        assert np.array_equal(got, blocks_loops(frame)), (h, w)
    for h, w in [(h, w) for h in (2, 4, 6, 18) for w in (2, 4, 6, 18)] + [SHAPE]:
        frame = pitched_nv12(rng, h, w, w + 13)
        assert frame.pitch_y == w + 13
        got = luma_blocks_np(frame)
        assert got.shape == grid_shape(h, w) and np.array_equal(got, blocks_loops(frame)), (h, w)
        assert np.array_equal(luma_np(frame), np.asarray(frame.y))
    white, black = np.full((8, 8, 3), 255, np.uint8), np.zeros((8, 8, 3), np.uint8)
    assert (luma_np(white) == 255).all() and (luma_np(black) == 0).all()
    assert (luma_blocks_np(white) == 4080).all() and (luma_blocks_np(black) == 0).all()
    for c, wgt in ((0, 29), (1, 150), (2, 77)):
        one = black.copy()
        one[:, :, c] = 255
        assert (luma_np(one) == (wgt * 255 + 128) >> 8).all()


# ---- the rule on TileGateNp ---------------------------------------------------------------------------------------------------------------
def test_first_call_flags_everything_and_a_still_frame_nothing():
    stub = StubDetector()
    gate = make_gate(stub)
    plan = gate.state.plans[0]
    assert len(plan) == 10 and plan[-1] == (0, 0) + SHAPE and (38, 52, 32, 48) in plan
    a = base_frame()
    gate.detect_padded([a])
    assert gate.last_flags == [[1] * 10] and gate.last_ncell == [[0] * 10]         # never detected: ref is not read
    assert stub.calls == [[(0,) + t for t in plan]]
    gate.detect_padded([a.copy()])
    assert gate.last_flags == [[0] * 10] and gate.last_ncell == [[0] * 10] and len(stub.calls) == 1
    assert gate.stats == dict(calls=2, tiles_seen=20, tiles_detected=10, forwards=1)


def test_one_pixel_is_below_the_bar_and_one_block_flags_its_owners():
    stub = StubDetector()
    gate = make_gate(stub)
    plan = gate.state.plans[0]
    a = base_frame()
    a[8, 8] = 0
    gate.detect_padded([a])
    b = a.copy()
    b[8, 8] = 255                                                                    # A = 255: 16 * 255 <= 32 * 256
    gate.detect_padded([b])
    assert gate.last_flags == [[0] * 10] and len(stub.calls) == 1
    # one 4 x 4 block raised by 40: A = 640 > 512 in every tile that owns it
    for by, bx in ((2, 2), (10, 15), (17, 24)):
        c = raised(a, slice(4 * by, 4 * by + 4), slice(4 * bx, 4 * bx + 4), 40)
        gate = make_gate(StubDetector())
        gate.detect_padded([a])
        gate.detect_padded([c])
        want = owners(plan, by, bx)
        assert gate.last_flags == [want] and want[-1] == 1 and 2 <= sum(want) < 10, (by, bx)
        assert gate.detect_tiles.calls[1] == [(0,) + t for t, on in zip(plan, want) if on]
    # a block inside the overlap strip x in [40, 48): both neighbours and the overview
    c = raised(a, slice(8, 12), slice(40, 44), 40)
    gate = make_gate(StubDetector())
    gate.detect_padded([a])
    gate.detect_padded([c])
    flagged = [t for t, on in zip(plan, gate.last_flags[0]) if on]
    assert flagged == [(0, 0, 32, 48), (0, 40, 32, 48), (0, 0) + SHAPE]


def test_threshold_edge_and_partial_cells():
    a = base_frame(3)
    gate = make_gate()
    gate.detect_padded([a])
    b = raised(a, slice(8, 12), slice(8, 12), 32)                                    # A = 512: 16 * 512 == 32 * 256
    gate.detect_padded([b])
    assert gate.last_flags == [[0] * 10]
    c = raised(b, 13, 13, 1)                                                         # the same cell of both owners: A = 513
    gate.detect_padded([c])
    assert gate.last_flags == [[1] + [0] * 8 + [1]] and gate.last_ncell == [[1] + [0] * 8 + [1]]
    # the bottom right pixel: the overview's cell there is 6 x 4 px (bar A > 48), that of the tile at (38, 52) is 2 x 16 px (A > 64)
    gate = make_gate()
    gate.detect_padded([a])
    gate.detect_padded([raised(a, 69, 99, 48)])
    assert gate.last_flags == [[0] * 10]
    gate.detect_padded([raised(a, 69, 99, 49)])
    assert gate.last_flags == [[0] * 9 + [1]]
    gate.detect_padded([raised(a, 69, 99, 49)])                                       # the overview's ref moved: nothing now
    assert gate.last_flags == [[0] * 10]
    gate.detect_padded([raised(a, 69, 99, 65)])                                       # 65 against the tile's old ref, 16 against the overview's new
    assert gate.last_flags == [[0] * 8 + [1, 0]]
    # other thresholds: thres16 is the bar in sixteenths
    from yolov6.utils.tile_gate import check_params
    assert check_params(2.0, 1, 50) == (32, 1, 50) and check_params(0.03, 1, 0)[0] == 0 and check_params(0.04, 1, 0)[0] == 1
    assert check_params(255, 3, 7) == (4080, 3, 7)
    for bad in ((-0.1, 1, 50), (255.5, 1, 50), (2.0, 0, 50), (2.0, 1, -1), (2.0, 1.5, 50)):
        with pytest.raises(ValueError):
            check_params(*bad)


def test_min_cells():
    a = base_frame(4)
    gate = make_gate(min_cells=2)
    gate.detect_padded([a])
    b = raised(a, slice(0, 4), slice(0, 4), 40)                                      # one changed cell
    gate.detect_padded([b])
    assert gate.last_flags == [[0] * 10] and gate.last_ncell == [[1] + [0] * 8 + [1]]
    c = raised(b, slice(16, 20), slice(0, 4), 40)                                     # a second cell of the same tiles
    gate.detect_padded([c])
    assert gate.last_flags == [[1] + [0] * 8 + [1]] and gate.last_ncell == [[2] + [0] * 8 + [2]]


def test_drift_accumulates_against_the_detected_frame():
    from yolov6.utils.tile_gate import luma_blocks_np
    a = base_frame(5)
    gate = make_gate()
    gate.detect_padded([a])
    ref0 = [r.copy() for r in gate.state.ref[0]]
    frames = [raised(a, slice(0, 16), slice(0, 16), k) for k in (1, 2, 3)]             # a full cell, + 1 per pixel per call: A = 256, 512, 768
    for k in (0, 1):
        gate.detect_padded([frames[k]])
        assert gate.last_flags == [[0] * 10]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(gate.state.ref[0], ref0))
    gate.detect_padded([frames[2]])
    assert gate.last_flags == [[1] + [0] * 8 + [1]]
    S = luma_blocks_np(frames[2])
    assert np.array_equal(gate.state.ref[0][0], S[:8, :12]) and np.array_equal(gate.state.ref[0][9], S)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(gate.state.ref[0][1:9], ref0[1:9]))
    assert gate.state.age[0].tolist() == [0] + [t % 50 + 3 for t in range(1, 9)] + [0]      # the stagger of the first call, three calls on


def test_refresh_staggers_and_forces():
    a = base_frame(6)
    gate = make_gate(refresh=4)
    gate.detect_padded([a])
    assert gate.state.age[0].tolist() == [t % 4 for t in range(10)]                  # t_local % refresh after the first detection
    age = [t % 4 for t in range(10)]
    for _ in range(9):
        gate.detect_padded([a])
        want = [int(v + 1 >= 4) for v in age]
        assert gate.last_flags == [want] and gate.last_ncell == [[0] * 10] and 2 <= sum(want) <= 3      # spread over the period
        age = [0 if on else v + 1 for v, on in zip(age, want)]
        assert gate.state.age[0].tolist() == age
    never = make_gate(refresh=0)
    never.detect_padded([a])
    assert never.state.age[0].tolist() == [0] * 10
    for k in range(60):
        never.detect_padded([a])
        assert never.last_flags == [[0] * 10]
    assert never.state.age[0].tolist() == [60] * 10
    default = make_gate()
    default.detect_padded([a])
    for k in range(50):
        default.detect_padded([a])
    assert default.last_flags == [[1] + [0] * 9] and default.stats['tiles_detected'] == 20      # each tile once more in 50 calls, one by one


def test_reset_streams_and_untracked_frames():
    shapes = [SHAPE, (40, 64)]
    stub = StubDetector()
    gate = make_gate(stub, shapes)
    a, b = base_frame(7), base_frame(8, (40, 64))
    assert [len(p) for p in gate.state.plans] == [10, 5]
    gate.detect_padded([a, b])
    gate.detect_padded([b, a], stream_of=[1, 0])
    assert gate.last_flags == [[0] * 5, [0] * 10]
    gate.detect_padded([b], stream_of=[1])                                           # stream 0 is absent: its state stays
    assert gate.last_flags == [[0] * 5] and gate.state.age[0].tolist()[0] == gate.state.age[1].tolist()[0] - 1
    gate.reset([1])
    assert not gate.cache_count[1].any() and not gate.cache_det[1].any() and gate.cache_count[0].any()
    gate.detect_padded([a, b])
    assert gate.last_flags == [[0] * 10, [1] * 5]
    gate.reset()
    gate.detect_padded([a, b])
    assert gate.last_flags == [[1] * 10, [1] * 5]
    # stream -1: not gated, every tile detected, no state read or written, nothing cached
    ages = [x.copy() for x in gate.state.age]
    cache = [x.copy() for x in gate.cache_det]
    other = base_frame(9, (50, 60))
    n = len(stub.calls)
    det, count = gate.detect_padded([other, a], stream_of=[-1, 0])
    assert gate.last_flags[0] == [1] * len(gate.last_flags[0]) and len(gate.last_flags[0]) == 5 and gate.last_flags[1] == [0] * 10
    assert [t[0] for t in stub.calls[n]] == [0] * 5
    assert all(np.array_equal(x, y) for x, y in zip(cache, gate.cache_det)) and gate.state.age[1].tolist() == ages[1].tolist()
    assert gate.state.age[0].tolist() == (ages[0] + 1).tolist()
    alone = make_gate(StubDetector(), [(50, 60)]).detect_padded([other])
    assert np.array_equal(det[0], alone[0][0]) and count[0] == alone[1][0]
    for bad in ([0, 0], [0, 2], [-2, 0], [0]):
        with pytest.raises(ValueError):
            gate.detect_padded([a, b], stream_of=bad)
    with pytest.raises(ValueError, match='fixed frame size'):
        gate.detect_padded([b, a])


def test_random_edits_against_the_loops():
    """Random patch edits over a sequence of calls: flags, ncell, ref and age as the loops give them."""
    from yolov6.utils.tile_gate import check_params, luma_blocks_np
    rng = np.random.default_rng(11)
    gate = make_gate(thres=1.5, min_cells=2, refresh=5)
    thres16, min_cells, refresh = check_params(1.5, 2, 5)
    plan = gate.state.plans[0]
    frame = base_frame(10)
    ref, age = [None] * 10, [-1] * 10
    seen = set()
    for call in range(8):
        for _ in range(int(rng.integers(0, 4))):
            y, x, hh, ww = int(rng.integers(0, 66)), int(rng.integers(0, 96)), int(rng.integers(1, 24)), int(rng.integers(1, 24))
            frame = raised(frame, slice(y, y + hh), slice(x, x + ww), int(rng.integers(1, 30)))
        gate.detect_padded([frame])
        cur = blocks_loops(frame) if call < 2 else luma_blocks_np(frame)
        for t, tile in enumerate(plan):
            by0, by1, bx0, bx1 = tile[0] >> 2, (tile[0] + tile[2] - 1) >> 2, tile[1] >> 2, (tile[1] + tile[3] - 1) >> 2
            n = 0 if age[t] < 0 else ncell_loops(cur, ref[t], SHAPE, tile, thres16)
            on = age[t] < 0 or n >= min_cells or age[t] + 1 >= refresh
            assert (gate.last_flags[0][t], gate.last_ncell[0][t]) == (int(on), n), (call, t)
            if on:
                ref[t], age[t] = cur[by0:by1 + 1, bx0:bx1 + 1].copy(), (t % refresh if age[t] < 0 else 0)
            else:
                age[t] += 1
            assert np.array_equal(gate.state.ref[0][t], ref[t]) and gate.state.age[0][t] == age[t]
            seen.add((int(on), min(n, 2)))
    assert {(0, 0), (0, 1), (1, 0), (1, 2)} <= seen


# ---- the cache ------------------------------------------------------------------------------------------------------------------------------
def test_cache_semantics():
    from yolov6.utils.tiles import merge_tiles_np
    stub = StubDetector()
    gate = make_gate(stub)
    plan = gate.state.plans[0]
    tiles = [(0,) + t for t in plan]
    a = base_frame(12)
    d0, c0 = gate.detect_padded([a])
    rows, counts = stub(None or [a], tiles, gate.tile_max_det)
    stub.calls.pop()
    want = merge_tiles_np(rows, counts, tiles, [SHAPE], 0.45, 20, 'iou', 1)
    assert np.array_equal(d0, want[0]) and np.array_equal(c0, want[1]) and c0[0] > 0 and d0.shape == (1, 20, 28)
    b = raised(a, 8, 8, 3)                                                            # below the bar: the output of the call before
    d1, c1 = gate.detect_padded([b])
    assert gate.last_flags == [[0] * 10] and np.array_equal(d1, d0) and np.array_equal(c1, c0)
    c = raised(a, slice(40, 60), slice(60, 90), 40)                                   # some tiles: fresh rows for them, the old rows for the others
    d2, c2 = gate.detect_padded([c])
    on = gate.last_flags[0]
    assert 0 < sum(on) < 10
    fresh, fcount = stub([c], tiles, gate.tile_max_det)
    stub.calls.pop()
    assert any(not np.array_equal(fresh[t], rows[t]) for t in range(10) if on[t])
    mixed = np.where(np.array(on, bool)[:, None, None], fresh, rows)
    want = merge_tiles_np(mixed, counts, tiles, [SHAPE], 0.45, 20, 'iou', 1)
    assert np.array_equal(d2, want[0]) and np.array_equal(c2, want[1])
    assert not np.array_equal(d2, d0)
    full = merge_tiles_np(fresh, fcount, tiles, [SHAPE], 0.45, 20, 'iou', 1)          # and that is what detecting every tile gives:
    assert np.array_equal(d2, full[0])                                                # the tiles left out show the pixels they showed
    outs = gate.detect([c])
    assert len(outs) == 1 and np.array_equal(outs[0], d2[0, :int(c2[0])])


# ---- C ABI: everything is checked on the host before any launch ----------------------------------------------------------------------------
def _desc(abi, rows):
    d = (abi.TileGateDesc * max(len(rows), 1))()
    for e, (p0, pitch0, h0, w0, fmt, blocks) in zip(d, rows):
        e.p0, e.pitch0, e.h0, e.w0, e.format, e.blocks = p0 or None, pitch0, h0, w0, fmt, blocks or None
    return d


def test_luma_batch_rejects_bad_arguments_before_launch():
    """Fake device addresses: a launch would fault, so LP_ERR_ARG proves the host check came first."""
    from yolov6.hip import abi
    lib = abi.load()
    err = lambda: lib.lp_last_error()   # noqa: E731
    good = [(0x100000, 300, 70, 100, 0, 0x200000), (0x110000, 128, 70, 100, 1, 0x210000)]

    def call(rows=good, n=None):
        return lib.lp_tile_gate_luma_batch(_desc(abi, rows), len(rows) if n is None else n, None)

    def frame(k, **kw):
        f = dict(zip(('p0', 'pitch0', 'h0', 'w0', 'fmt', 'blocks'), good[k]))
        f.update(kw)
        rows = list(good)
        rows[k] = tuple(f[x] for x in ('p0', 'pitch0', 'h0', 'w0', 'fmt', 'blocks'))
        return rows

    assert call(n=-1) == LP_ERR_ARG and b'n_frames' in err()
    assert lib.lp_tile_gate_luma_batch(None, 2, None) == LP_ERR_ARG and b'null desc' in err()
    assert call(rows=[], n=0) == 0                                                     # nothing to do: no launch
    assert call(frame(1, p0=0)) == LP_ERR_ARG and b'frame 1' in err() and b'null plane' in err()
    assert call(frame(0, blocks=0)) == LP_ERR_ARG and b'frame 0' in err() and b'null block grid' in err()
    assert call(frame(1, blocks=0x210001)) == LP_ERR_ARG and b'aligned' in err()
    assert call(frame(0, fmt=2)) == LP_ERR_ARG and b'format' in err() and call(frame(0, fmt=-1)) == LP_ERR_ARG
    assert call(frame(0, h0=0)) == LP_ERR_ARG and b'h0' in err() and call(frame(1, w0=0)) == LP_ERR_ARG
    assert call(frame(0, pitch0=299)) == LP_ERR_ARG and b'pitch0 299' in err() and b'300' in err()
    assert call(frame(1, pitch0=99)) == LP_ERR_ARG and b'frame 1' in err() and b'pitch0' in err()
    grid = 18 * 25 * 2
    for k, at in ((0, 0x100000), (0, 0x100000 + 69 * 300 + 298), (0, 0x110000 + 69 * 128 + 98), (0, 0x210000 + grid - 2), (1, 0x200000 - grid + 2),
                  (1, 0x100000 - grid + 2)):
        assert call(frame(k, blocks=at)) == LP_ERR_ARG and b'overlap' in err(), (k, hex(at))


def test_gate_update_rejects_bad_arguments_before_launch():
    from yolov6.hip import abi
    lib = abi.load()
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731
    err = lambda: lib.lp_last_error()   # noqa: E731
    frames = [(0, 0, 70, 100, 0, 0x200000), (0, 0, 40, 64, 1, 0x210000)]             # the planes are not read here
    S, T = 3, 10

    def call(rows=frames, n=None, so=(2, 0), S=S, tiles=0x300000, nt=(10, 0, 5), T=T, ref=0x400000, ref_elems=5000, age=0x500000, thres16=32,
             min_cells=1, refresh=50, flag=0x600000, ncell=0x700000, desc=True):
        n = len(rows) if n is None else n
        so_c = (ctypes.c_int * max(len(so), 1))(*so) if so is not None else None
        nt_c = (ctypes.c_int * max(len(nt), 1))(*nt) if nt is not None else None
        return lib.lp_tile_gate_update(_desc(abi, rows) if desc else None, n, so_c, S, v(tiles), nt_c, T, v(ref), ref_elems, v(age), thres16,
                                       min_cells, refresh, v(flag), v(ncell), None)

    assert call(n=-1) == LP_ERR_ARG and b'n_frames' in err() and call(S=0) == LP_ERR_ARG and b'n_streams' in err()
    assert call(T=0) == LP_ERR_ARG and b'max_tiles' in err() and call(T=65, nt=(65, 0, 5)) == LP_ERR_ARG and b'1..64' in err()
    for kw in (dict(thres16=-1), dict(thres16=4081), dict(min_cells=0), dict(refresh=-1)):
        assert call(**kw) == LP_ERR_ARG and b'thres16' in err(), kw
    assert call(ref_elems=0) == LP_ERR_ARG and b'ref_elems' in err() and call(ref_elems=1 << 31) == LP_ERR_ARG
    for k in ('tiles', 'ref', 'age', 'flag', 'ncell'):
        assert call(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
    assert call(nt=None) == LP_ERR_ARG and b'null' in err() and call(so=None) == LP_ERR_ARG and call(desc=False) == LP_ERR_ARG and b'null' in err()
    assert call(tiles=0x300002) == LP_ERR_ARG and b'aligned' in err() and call(ref=0x400001) == LP_ERR_ARG and call(age=0x500002) == LP_ERR_ARG
    assert call(ncell=0x700002) == LP_ERR_ARG and b'aligned' in err()
    assert call(nt=(11, 0, 5)) == LP_ERR_ARG and b'stream 0 has 11 tiles' in err() and call(nt=(10, -1, 5)) == LP_ERR_ARG
    assert call(so=(2, 3)) == LP_ERR_ARG and b'stream 3 of frame 1' in err() and call(so=(-2, 0)) == LP_ERR_ARG
    assert call(so=(2, 2)) == LP_ERR_ARG and b'twice' in err() and b'stream 2' in err()
    bad = [frames[0], (0, 0, 40, 64, 1, 0)]
    assert call(rows=bad) == LP_ERR_ARG and b'frame 1' in err() and b'null block grid' in err()
    # (the descriptor of a frame of stream -1 is not read.)  This request passes every host check, so it LAUNCHES: without a device the
    # launch fails with a HIP error, with one the kernel would dereference the fake addresses -- a memory-access fault that takes the
    # whole process down, some tests later.  Only asked for where no device can take it.
    if not torch.cuda.is_available():
        assert call(rows=bad, so=(2, -1)) != LP_ERR_ARG or b'null block grid' not in err()
    assert call(rows=[(0, 0, 0, 100, 0, 0x200000), frames[1]]) == LP_ERR_ARG and b'h0' in err()
    grid0, slots = 18 * 25 * 2, S * T
    for k, at in (('ref', 0x200000 + grid0 - 2), ('ref', 0x210000), ('ref', 0x300000 + slots * 32 - 2), ('age', 0x400000 + 9996), ('age', 0x300000),
                  ('flag', 0x500000 + slots * 4 - 1), ('flag', 0x200000), ('ncell', 0x600000 + 2 * T - 4), ('ncell', 0x400000), ('age', 0x700000 + 8 * T - 4)):
        assert call(**{k: at}) == LP_ERR_ARG and b'overlap' in err(), (k, hex(at))
    assert call(rows=[], n=0, so=(), desc=False, flag=0, ncell=0) == 0              # no frame: nothing to write, no launch


# ---- tools/infer.py --tile --tile-gate on the CPU path ---------------------------------------------------------------------------------------
def repeated_image_dir(tmp_path, shape=(150, 200)):
    """A directory holding one image three times, then another of the same size."""
    from PIL import Image
    rng = np.random.default_rng(12)
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    first, last = (rng.integers(0, 255, shape + (3,), dtype=np.uint8) for _ in range(2))
    for k, img in enumerate((first, first, first, last)):
        Image.fromarray(img).save(str(img_dir / ('f%d.png' % k)))
    return img_dir


def test_infer_tile_gate_cpu(tmp_path, monkeypatch):
    from yolov6.core.inferer import Inferer
    from yolov6.core.tiles import plan_tiles
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(os.path.join(REPO, 'configs', 'yololps.py'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None, 'epoch': 0}, str(ckpt))
    img_dir = repeated_image_dir(tmp_path)
    ran = []
    inner = Inferer._tiles_cpu
    monkeypatch.setattr(Inferer, '_tiles_cpu', lambda self, frames, tiles, *a: (ran.append(len(tiles)), inner(self, frames, tiles, *a))[1])
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[96, 96], conf_thres=0.06, iou_thres=0.45, max_det=30,
              device='cpu', not_save_img=True, save_txt=True, tile=[96, 96], tile_overlap=24)
    plain = infer.run(save_dir=str(tmp_path / 'o0'), **kw)
    n_tiles = len(plan_tiles((150, 200), (96, 96), 24))
    assert ran == [n_tiles] * 4 and n_tiles > 4
    del ran[:]
    gated = infer.run(save_dir=str(tmp_path / 'o1'), tile_gate=True, **kw)
    assert ran == [n_tiles, n_tiles]                                                  # the first and the last image only
    assert len(plain) == len(gated) == 4 and sum(len(d) for d in plain) > 0
    for a, b in zip(plain, gated):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    names = sorted(p.name for p in (tmp_path / 'o0' / 'imgs').iterdir())
    assert names == sorted(p.name for p in (tmp_path / 'o1' / 'imgs').iterdir()) and names
    for name in names:
        assert (tmp_path / 'o0' / 'imgs' / name).read_bytes() == (tmp_path / 'o1' / 'imgs' / name).read_bytes()
    from PIL import Image
    Image.fromarray(np.zeros((100, 200, 3), np.uint8)).save(str(img_dir / 'g9.png'))
    with pytest.raises(ValueError, match='--tile-gate'):
        infer.run(save_dir=str(tmp_path / 'o2'), tile_gate=True, **kw)
    with pytest.raises(ValueError, match='tile_gate needs tile'):
        infer.run(save_dir=str(tmp_path / 'o3'), tile_gate=True, **dict(kw, tile=None))
