"""The gain mode of the tile gate on the CPU (yolov6/utils/tile_gate.py, the specification of lp_tile_gate_update_gain): the gain
of a cell and the median of a tile against loops over Python integers, the arithmetic bounds, the rule with G == 4096 against the
rule without a gain, its behaviour under drift on a synthetic scene, ``TileGateNp(illum='gain')`` with a stub detector, and the
argument checks of the C entry point (no device needed).  ``scene``, ``drifted``, ``SCENE_TILE`` and ``gain_loops`` are shared
with tests/test_tile_gate_gain_gpu.py."""
import ctypes

import numpy as np
import pytest

from test_tile_gate_cpu import OVERLAP, SHAPE, TILE, StubDetector, base_frame, make_gate

LP_ERR_ARG = -1
SCENE_HW, SCENE_TILE = (360, 640), (0, 0, 256, 320)      # the tile: 16 x 20 = 320 full cells
PATCH = (slice(40, 72), slice(100, 196))                 # 32 x 96 px at no multiple of 16: cell rows 2..4, cell columns 6..12 = 21 cells
PATCH_CELLS = 21


# ---- the rule once more, as loops over Python integers --------------------------------------------------------------------------------
def gain_loops(cur, ref, tile):
    """(the g_c of the cells that have one, in cell order; G_raw) of one tile by the words of the rule."""
    y0, x0, th, tw = tile
    by0, by1, bx0, bx1 = y0 >> 2, (y0 + th - 1) >> 2, x0 >> 2, (x0 + tw - 1) >> 2
    gains = []
    for cy in range(by0, by1 + 1, 4):
        for cx in range(bx0, bx1 + 1, 4):
            R = C = 0
            for by in range(cy, min(cy + 4, by1 + 1)):
                for bx in range(cx, min(cx + 4, bx1 + 1)):
                    C += int(cur[by, bx])
                    R += int(ref[by - by0, bx - bx0])
            if R:
                gains.append(min((C * 4096 + (R >> 1)) // R, 65535))
    return gains, (sorted(gains)[(len(gains) - 1) // 2] if gains else 4096)


def ncell_gain_loops(cur, ref, hw, tile, thres16, G):
    h, w = hw
    y0, x0, th, tw = tile
    by0, by1, bx0, bx1 = y0 >> 2, (y0 + th - 1) >> 2, x0 >> 2, (x0 + tw - 1) >> 2
    n = 0
    for cy in range(by0, by1 + 1, 4):
        for cx in range(bx0, bx1 + 1, 4):
            A = npix = 0
            for by in range(cy, min(cy + 4, by1 + 1)):
                for bx in range(cx, min(cx + 4, bx1 + 1)):
                    A += abs(int(cur[by, bx]) * 4096 - int(ref[by - by0, bx - bx0]) * G)
                    npix += (min(4 * by + 4, h) - 4 * by) * (min(4 * bx + 4, w) - 4 * bx)
            n += A > thres16 * npix * 256
    return n


def _gain_of(cur, ref, tile):
    from yolov6.utils.tile_gate import cell_gains_np, tile_gain_np
    g, has = cell_gains_np(cur, ref, tile)
    return g, has, tile_gain_np(g, has)


def _check_against_loops(cur, ref, tile):
    g, has, G = _gain_of(cur, ref, tile)
    want, want_G = gain_loops(cur, ref, tile)
    assert g[has].tolist() == want and int(has.sum()) == len(want) and not g[~has].any()
    assert G == want_G
    return len(want), G


def test_cell_and_tile_gain_against_the_loops():
    rng = np.random.default_rng(30)
    m_seen = set()
    for shape, tile in (((70, 100), (0, 0, 70, 100)), ((70, 100), (38, 52, 32, 48)), ((37, 53), (0, 0, 37, 53)), ((37, 53), (5, 7, 30, 41)),
                        ((16, 16), (0, 0, 16, 16)), ((16, 32), (0, 0, 16, 32)), ((4, 4), (0, 0, 4, 4)), ((48, 16), (0, 0, 48, 16))):
        gy, gx = (shape[0] + 3) // 4, (shape[1] + 3) // 4
        by0, by1, bx0, bx1 = tile[0] >> 2, (tile[0] + tile[2] - 1) >> 2, tile[1] >> 2, (tile[1] + tile[3] - 1) >> 2
        for k in range(4):
            cur = rng.integers(0, 4081, (gy, gx)).astype(np.uint16)
            ref = rng.integers(1, 4081, (by1 - by0 + 1, bx1 - bx0 + 1)).astype(np.uint16)
            if k == 1:
                ref[:4, :4] = 0                                                       # a cell with R_c == 0 has no gain
            if k == 2:
                ref[:] = (cur[by0:by1 + 1, bx0:bx1 + 1].astype(np.int64) * 2 // 3).astype(np.uint16)   # many tied ratios
                ref[ref == 0] = 1
            m, _ = _check_against_loops(cur, ref, tile)
            m_seen.add(min(m, 4) if m < 4 else 4 + m % 2)
            if k == 1:
                assert m == ((by1 - by0 + 4) // 4) * ((bx1 - bx0 + 4) // 4) - 1
    assert {1, 2, 3, 4, 5} <= m_seen                                                   # m = 1, 2, 3 and larger even and odd counts


def test_gain_edge_cases():
    from yolov6.utils.tile_gate import check_illum
    lo, hi = check_illum('gain', 1.5)
    tile = (0, 0, 16, 48)                                                              # three cells
    cur = np.full((4, 12), 100, np.uint16)
    # an all-zero ref: m = 0 gives 4096, which is never out of range
    assert _check_against_loops(cur, np.zeros((4, 12), np.uint16), tile) == (0, 4096) and lo <= 4096 <= hi
    # m = 1
    ref = np.zeros((4, 12), np.uint16)
    ref[:, 4:8] = 50
    assert _check_against_loops(cur, ref, tile) == (1, 8192)
    # m = 2: the LOWER median
    ref[:, 8:] = 200
    assert _check_against_loops(cur, ref, tile) == (2, 2048)
    # m = 3: the middle one
    ref[:, :4] = 100
    assert _check_against_loops(cur, ref, tile) == (3, 4096)
    # the cap: R_c = 1, C_c = 65280
    one = np.zeros((4, 4), np.uint16)
    one[0, 0] = 1
    g, has, G = _gain_of(np.full((4, 4), 4080, np.uint16), one, (0, 0, 16, 16))
    assert (65280 * 4096 + 0) // 1 > 65535 and g.tolist() == [[65535]] and G == 65535
    assert _check_against_loops(np.full((4, 4), 4080, np.uint16), one, (0, 0, 16, 16)) == (1, 65535)
    # rounding to nearest: 3 / 2 and 1 / 3
    two = np.zeros((4, 4), np.uint16)
    two[0, 0], cur3 = 3, np.zeros((4, 4), np.uint16)
    cur3[0, 0] = 1
    assert _gain_of(cur3, two, (0, 0, 16, 16))[2] == (4096 + 1) // 3 == 1365
    # ties: 7 cells of one ratio, 2 above, 2 below
    cur = np.full((4, 44), 300, np.uint16)
    ref = np.full((4, 44), 200, np.uint16)
    ref[:, :8], ref[:, 8:16] = 100, 400
    assert _check_against_loops(cur, ref, (0, 0, 16, 176)) == (11, 6144)


def test_arithmetic_stays_inside_int32():
    """Block sums of 0 and 4080 and G in {lo, 4096, 16384}: every intermediate of the rule, computed in int64, is below 2^31."""
    from yolov6.utils.tile_gate import MAX_THRES16, check_illum
    lo, hi = check_illum('gain', 4.0)
    assert (lo, hi) == (1024, 16384)
    top = 0
    for s_cur in (0, 4080):
        for s_ref in (0, 4080):
            C, R = np.int64(16 * s_cur), np.int64(16 * s_ref)
            top = max(top, int(C * 4096 + (R >> 1)))                                 # the numerator of g_c
            for G in (lo, 4096, 16384):
                term = abs(np.int64(s_cur) * 4096 - np.int64(s_ref) * G)
                top = max(top, int(np.int64(s_cur) * 4096), int(np.int64(s_ref) * G), int(term), int(16 * term))
    top = max(top, MAX_THRES16 * 256 * 256)                                           # thres16 * npix * 256 of a full cell
    assert top == 16 * 4080 * 16384 < 2 ** 31
    assert 16 * 4080 * 4096 + (16 * 4080 >> 1) < 2 ** 32                              # (the division is unsigned 32-bit)
    # and the specification computes what the loops compute at those extremes
    from yolov6.utils.tile_gate import changed_cells_gain
    cur, ref = np.full((4, 4), 4080, np.uint16), np.zeros((4, 4), np.uint16)
    for G in (lo, 4096, 16384):
        for a, b in ((cur, ref), (ref, cur), (cur, cur)):
            for t16 in (0, 4080):
                assert changed_cells_gain(a, b, (16, 16), (0, 0, 16, 16), t16, G) == ncell_gain_loops(a, b, (16, 16), (0, 0, 16, 16), t16, G)


def test_unit_gain_is_the_rule_without_a_gain():
    """More than half of the cells equal to ref: G_raw == 4096, and the changed cells are those of ``changed_cells``."""
    from yolov6.utils.tile_gate import changed_cells, changed_cells_gain, luma_blocks_np
    rng = np.random.default_rng(31)
    counts = set()
    for tile in ((0, 0) + SHAPE, (38, 52, 32, 48), (0, 40, 32, 48)):
        by0, by1, bx0, bx1 = tile[0] >> 2, (tile[0] + tile[2] - 1) >> 2, tile[1] >> 2, (tile[1] + tile[3] - 1) >> 2
        a = base_frame(31)
        a[a == 0] = 1
        ref = luma_blocks_np(a)[by0:by1 + 1, bx0:bx1 + 1]
        b = a.copy()
        ys, xs = slice(tile[0], tile[0] + tile[2] // 3), slice(tile[1], tile[1] + tile[3] // 2)  # a sixth of the tile is raised
        amp = np.repeat(rng.integers(0, 50, (tile[3] + 15) // 16), 16)[:tile[3] // 2]   # by another amount per 16 columns: 0..49 levels
        b[ys, xs] = (b[ys, xs].astype(np.int32) + amp[None, :, None]).clip(0, 255).astype(np.uint8)
        cur = luma_blocks_np(b)
        g, has, G = _gain_of(cur, ref, tile)
        assert has.all() and 2 * int((g == 4096).sum()) > g.size and G == 4096
        seen = set()
        for t16 in (0, 1, 32, 500, 4080):
            n = changed_cells(cur, ref, SHAPE, tile, t16)
            assert changed_cells_gain(cur, ref, SHAPE, tile, t16, 4096) == n == ncell_gain_loops(cur, ref, SHAPE, tile, t16, 4096)
            seen.add(n)
        assert 0 in seen and max(seen) > 0
        counts |= seen
    assert len(counts) >= 4


# ---- behaviour on a synthetic scene -----------------------------------------------------------------------------------------------------
def scene(top=200, seed=0, hw=SCENE_HW):
    """8 x 8 px patches of luma 20..top, float64 [h, w]."""
    rng = np.random.default_rng(seed)
    return np.kron(rng.integers(20, top + 1, (hw[0] // 8, hw[1] // 8)), np.ones((8, 8)))


def drifted(base, gain, seed, patch=None, sigma=2.0):
    """The scene at ``gain`` with Gaussian noise of ``sigma`` (truncated at two sigma, so that top * gain + 2 sigma is the largest
    pixel and nothing saturates), a patch of luma 230 on top where given, as a grey BGR frame (its luma is the value itself)."""
    noise = np.clip(np.random.default_rng(seed).normal(0.0, sigma, base.shape), -2 * sigma, 2 * sigma)
    v = base * gain + noise
    if patch is not None:
        v[patch] = 230.0 + noise[patch]
    v = np.floor(v + 0.5)
    assert v.max() < 255 and v.min() > 0, 'the scene must not saturate'
    return np.repeat(v.astype(np.uint8)[:, :, None], 3, axis=2)


def _one_tile_state(first):
    from yolov6.utils.tile_gate import GateState, check_illum, gate_update_gain_np, luma_blocks_np
    state = GateState([SCENE_HW], [[SCENE_TILE]])
    lo, hi = check_illum('gain', 1.5)
    assert gate_update_gain_np(state, [luma_blocks_np(first)], [0], 32, 1, 0, lo, hi) == ([[1]], [[0]], [[0]])     # never detected
    return state, lo, hi


@pytest.mark.parametrize('gain', [0.8, 0.9, 1.05, 1.2, 1.25])
def test_a_drift_changes_every_cell_today_and_none_with_the_gain(gain):
    from yolov6.utils.tile_gate import changed_cells, gate_update_gain_np, luma_blocks_np
    base = scene()
    state, lo, hi = _one_tile_state(drifted(base, 1.0, 41))
    ref = state.ref[0][0].copy()
    cur = luma_blocks_np(drifted(base, gain, 42))
    assert changed_cells(cur, ref, SCENE_HW, SCENE_TILE, 32) == 320
    fl, nc, gn = gate_update_gain_np(state, [cur], [0], 32, 1, 0, lo, hi)
    assert (fl, nc) == ([[0]], [[0]]) and abs(gn[0][0] - int(np.floor(4096 * gain + 0.5))) <= 4
    assert np.array_equal(state.ref[0][0], ref) and state.age[0][0] == 1

    # a bright patch on top of the drift: flagged, by no more cells than the patch overlaps, and the gain is not biased
    state, lo, hi = _one_tile_state(drifted(base, 1.0, 41))
    cur = luma_blocks_np(drifted(base, gain, 42, PATCH))
    fl, nc, gn = gate_update_gain_np(state, [cur], [0], 32, 1, 0, lo, hi)
    assert fl == [[1]] and 1 <= nc[0][0] <= PATCH_CELLS and abs(gn[0][0] - int(np.floor(4096 * gain + 0.5))) <= 4
    assert np.array_equal(state.ref[0][0], cur[:64, :80]) and state.age[0][0] == 0


def test_a_gain_out_of_range_flags_the_tile():
    from yolov6.utils.tile_gate import gate_update_gain_np, luma_blocks_np
    base = scene(top=150)                                                              # 150 * 1.6 + 4 < 255
    for gain, out in ((1.6, True), (1.45, False), (0.6, True), (0.7, False)):
        state, lo, hi = _one_tile_state(drifted(base, 1.0, 43))
        fl, nc, gn = gate_update_gain_np(state, [luma_blocks_np(drifted(base, gain, 44))], [0], 32, 1, 0, lo, hi)
        assert abs(gn[0][0] - int(np.floor(4096 * gain + 0.5))) <= 4 and (nc == [[0]]) == (not out)     # (clamped to the range, G fits no cell)
        assert fl == [[int(out)]] and (gn[0][0] < lo or gn[0][0] > hi) == out, gain


# ---- TileGateNp ---------------------------------------------------------------------------------------------------------------------------
def _scaled(frame, gain):
    return np.floor(frame.astype(np.float64) * gain + 0.5).astype(np.uint8)           # channels 0..200: no saturation up to 1.27


DRIFT = [1.0, 1.02, 1.05, 1.1, 1.2, 1.15, 1.0, 0.9, 0.8, 0.85]


def test_gain_mode_runs_the_detector_at_the_first_call_and_at_refreshes_only():
    a = base_frame(45)
    # no refresh: one forward, the rows of the first call ever after; today's rule detects every tile of every call
    stub, plain = StubDetector(), StubDetector()
    gate, old = make_gate(stub, refresh=0, illum='gain'), make_gate(plain, refresh=0)
    first = None
    for k, g in enumerate(DRIFT):
        det, count = gate.detect_padded([_scaled(a, g)])
        old.detect_padded([_scaled(a, g)])
        first = (det.copy(), count.copy()) if k == 0 else first
        assert np.array_equal(det, first[0]) and np.array_equal(count, first[1])
        assert gate.last_flags == [[int(k == 0)] * 10] and gate.last_ncell == [[0] * 10]
        want = 0 if k == 0 else int(np.floor(4096 * g + 0.5))
        assert all(abs(v - want) <= (8 if k else 0) for v in gate.last_gain[0]), (k, gate.last_gain)
        if g not in (1.0, 1.02):                                                       # 200 * 0.02 = 4 levels: past the bar of 2 on most cells
            assert old.last_flags == [[1] * 10], k
    assert len(stub.calls) == 1 and len(plain.calls) >= 8
    assert gate.stats == dict(calls=10, tiles_seen=100, tiles_detected=10, forwards=1, tiles_out_of_range=0)
    # refresh 4: the flags are those of the stagger alone
    stub = StubDetector()
    gate = make_gate(stub, refresh=4, illum='gain', max_gain=2.0)                      # (a refreshed tile's gain is against its new reference)
    plan = gate.state.plans[0]
    age = None
    for k, g in enumerate(DRIFT):
        gate.detect_padded([_scaled(a, g)])
        want = [1] * 10 if k == 0 else [int(v + 1 >= 4) for v in age]
        age = [t % 4 for t in range(10)] if k == 0 else [0 if on else v + 1 for v, on in zip(age, want)]
        assert gate.last_flags == [want] and gate.last_ncell == [[0] * 10] and gate.state.age[0].tolist() == age, k
        assert stub.calls[-1] == [(0,) + t for t, on in zip(plan, want) if on]
    assert gate.stats['tiles_out_of_range'] == 0
    # out of range: detected again, counted, and the gain starts from the new reference
    gate = make_gate(StubDetector(), refresh=0, illum='gain', max_gain=1.1)
    for g, on in ((1.0, 1), (1.05, 0), (1.2, 1), (1.25, 0)):
        gate.detect_padded([_scaled(a, g)])
        assert gate.last_flags == [[on] * 10], g
    assert gate.stats['tiles_out_of_range'] == 10 and all(abs(v - 4267) <= 8 for v in gate.last_gain[0])      # 1.25 / 1.2


def test_illum_none_is_the_gate_without_the_new_arguments():
    rng = np.random.default_rng(46)
    a = base_frame(46)
    gates = [make_gate(StubDetector(), refresh=3), make_gate(StubDetector(), refresh=3, illum='none', max_gain=2.0)]
    for k, g in enumerate(DRIFT):
        frame = _scaled(a, g if k % 3 == 0 else 1.0)
        if k % 2:
            y, x = int(rng.integers(0, 50)), int(rng.integers(0, 80))
            frame[y:y + 12, x:x + 12] //= 2
        outs = [gt.detect_padded([frame]) for gt in gates]
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        p, q = gates
        assert p.last_flags == q.last_flags and p.last_ncell == q.last_ncell and p.stats == q.stats and 'tiles_out_of_range' not in q.stats
        assert q.last_gain == [[0] * 10] == p.last_gain
        assert all(np.array_equal(x, y) for x, y in zip(p.state.ref[0], q.state.ref[0])) and np.array_equal(p.state.age[0], q.state.age[0])
        assert p.detect_tiles.calls == q.detect_tiles.calls
    assert 10 < gates[0].stats['tiles_detected'] < 100


def test_check_illum():
    from yolov6.utils.tile_gate import TileGateNp, check_illum
    assert check_illum() == check_illum('none', 1.5) == check_illum('gain', 1.5) == (2731, 6144)
    assert check_illum('gain', 1) == (4096, 4096) and check_illum('gain', 4.0) == (1024, 16384) and check_illum('gain', 1.25) == (3277, 5120)
    for lo, hi in (check_illum('gain', g) for g in (1.0, 1.0001, 1.1, 1.3333, 2.0, 3.999)):
        assert 1 <= lo <= 4096 <= hi <= 16384 and lo * hi >= 4096 * 4096 > (lo - 1) * hi
    for bad in (('on', 1.5), ('GAIN', 1.5), (None, 1.5), ('gain', 0.99), ('gain', 4.01), ('gain', float('nan')), ('gain', 'x'), ('gain', None)):
        with pytest.raises(ValueError):
            check_illum(*bad)
    with pytest.raises(ValueError):
        TileGateNp(StubDetector(), [SHAPE], TILE, 0.45, 20, overlap=OVERLAP, illum='gain', max_gain=5)
    with pytest.raises(ValueError):
        make_gate(illum='offset')


# ---- C ABI: everything is checked on the host before any launch ----------------------------------------------------------------------------
def test_gate_update_gain_rejects_bad_arguments_before_launch():
    """Fake device addresses: a launch would fault, so LP_ERR_ARG proves the host check came first."""
    from yolov6.hip import abi
    from test_tile_gate_cpu import _desc
    lib = abi.load()
    v = lambda p: ctypes.c_void_p(p) if p else None   # noqa: E731
    err = lambda: lib.lp_last_error()   # noqa: E731
    frames = [(0, 0, 70, 100, 0, 0x200000), (0, 0, 40, 64, 1, 0x210000)]             # the planes are not read here
    S, T = 3, 10

    def call(rows=frames, n=None, so=(2, 0), S=S, tiles=0x300000, nt=(10, 0, 5), T=T, ref=0x400000, ref_elems=5000, age=0x500000, thres16=32,
             min_cells=1, refresh=50, lo=2731, hi=6144, flag=0x600000, ncell=0x700000, gain=0x800000, desc=True):
        n = len(rows) if n is None else n
        so_c = (ctypes.c_int * max(len(so), 1))(*so) if so is not None else None
        nt_c = (ctypes.c_int * max(len(nt), 1))(*nt) if nt is not None else None
        return lib.lp_tile_gate_update_gain(_desc(abi, rows) if desc else None, n, so_c, S, v(tiles), nt_c, T, v(ref), ref_elems, v(age), thres16,
                                            min_cells, refresh, lo, hi, v(flag), v(ncell), v(gain), None)

    assert call(n=-1) == LP_ERR_ARG and b'lp_tile_gate_update_gain' in err() and b'n_frames' in err()
    assert call(S=0) == LP_ERR_ARG and b'n_streams' in err()
    assert call(T=0) == LP_ERR_ARG and b'max_tiles' in err() and call(T=65, nt=(65, 0, 5)) == LP_ERR_ARG and b'1..64' in err()
    for kw in (dict(thres16=-1), dict(thres16=4081), dict(min_cells=0), dict(refresh=-1)):
        assert call(**kw) == LP_ERR_ARG and b'thres16' in err(), kw
    for kw in (dict(lo=0), dict(lo=-5), dict(lo=4097), dict(hi=4095), dict(hi=16385), dict(lo=6144, hi=2731)):
        assert call(**kw) == LP_ERR_ARG and b'gain_lo' in err() and b'16384' in err(), kw
    assert call(ref_elems=0) == LP_ERR_ARG and b'ref_elems' in err() and call(ref_elems=1 << 31) == LP_ERR_ARG
    for k in ('tiles', 'ref', 'age', 'flag', 'ncell', 'gain'):
        assert call(**{k: 0}) == LP_ERR_ARG and b'null' in err(), k
    assert call(nt=None) == LP_ERR_ARG and b'null' in err() and call(so=None) == LP_ERR_ARG and call(desc=False) == LP_ERR_ARG and b'null' in err()
    for kw in (dict(tiles=0x300002), dict(ref=0x400001), dict(age=0x500002), dict(ncell=0x700002), dict(gain=0x800002), dict(gain=0x800001)):
        assert call(**kw) == LP_ERR_ARG and b'aligned' in err(), kw
    assert call(nt=(11, 0, 5)) == LP_ERR_ARG and b'stream 0 has 11 tiles' in err() and call(nt=(10, -1, 5)) == LP_ERR_ARG
    assert call(so=(2, 3)) == LP_ERR_ARG and b'stream 3 of frame 1' in err() and call(so=(-2, 0)) == LP_ERR_ARG
    assert call(so=(2, 2)) == LP_ERR_ARG and b'twice' in err() and b'stream 2' in err()
    assert call(rows=[frames[0], (0, 0, 40, 64, 1, 0)]) == LP_ERR_ARG and b'frame 1' in err() and b'null block grid' in err()
    grid0, slots, outs = 18 * 25 * 2, S * T, 2 * T
    for k, at in (('gain', 0x700000 + 4 * outs - 4), ('gain', 0x600000 + outs - 4), ('gain', 0x200000 + grid0 - 4), ('gain', 0x300000),
                  ('gain', 0x400000 + 9996), ('gain', 0x500000 + slots * 4 - 4), ('ncell', 0x800000 + 4 * outs - 4), ('flag', 0x800000 + 4 * outs - 1),
                  ('age', 0x800000 - slots * 4 + 4), ('ref', 0x800000 - 9996), ('ref', 0x200000 + grid0 - 2), ('flag', 0x500000 + slots * 4 - 1)):
        assert call(**{k: at}) == LP_ERR_ARG and b'overlap' in err(), (k, hex(at))
    assert call(rows=[], n=0, so=(), desc=False, flag=0, ncell=0, gain=0) == 0       # no frame: nothing to write, no launch
