"""The gain mode of the tile gate on the GPU, bit for bit: lp_tile_gate_update_gain against ``gate_update_gain_np`` over sequences
of calls and on grids built for the selection of the median, every output and the state between guards; against
lp_tile_gate_update where the gain is 1; ``runtime.TileGate(illum='gain')`` against ``TileGateNp(illum='gain')``; and
``tools/infer.py --tile-gate --tile-gate-illum gain``.  The kernel keeps no per-cell gains in LDS, so there is no capacity whose two
sides would need a shape of their own."""
import ctypes
import importlib
import logging
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_tile_gate_cpu import StubDetector
from test_tile_gate_gpu import CFG, POISON, _DeviceGate, _edit, _same, _stream, _tiny

pytestmark = pytest.mark.gpu

GUARD = 64                                               # guard elements on both sides of ref, age, flag, ncell and gain
AGE_GUARD, FLAG_FILL, WORD_FILL = 0x5a5a5a5a, 9, -9
LO, HI = 2731, 6144                                      # check_illum('gain', 1.5)


class _GainGate(_DeviceGate):
    """``_DeviceGate`` with ref and age between guards, and one call of lp_tile_gate_update_gain whose three outputs lie between
    guards too: every output entry must be written and no guard element may change."""

    def __init__(self, shapes, plans):
        super().__init__(shapes, plans)
        self.ref_buf = torch.full((self.ref_elems + 2 * GUARD,), POISON, dtype=torch.int16, device='cuda')
        self.ref = self.ref_buf[GUARD:GUARD + self.ref_elems]
        self.age_buf = torch.full((self.S * self.T + 2 * GUARD,), AGE_GUARD, dtype=torch.int32, device='cuda')
        self.age = self.age_buf[GUARD:GUARD + self.S * self.T].view(self.S, self.T)
        self.age.fill_(-1)

    def update_gain(self, grids, stream_of, thres16, min_cells, refresh, lo=LO, hi=HI):
        abi, F, T = self.abi, len(stream_of), self.T
        desc = (abi.TileGateDesc * F)()
        for d, g, s in zip(desc, grids, stream_of):
            if s >= 0:
                self.grids[s].copy_(torch.from_numpy(np.ascontiguousarray(g).view(np.int16)))
                d.h0, d.w0, d.blocks = self.shapes[s][0], self.shapes[s][1], self.grids[s].data_ptr()
        flag = torch.full((F * T + 2 * GUARD,), FLAG_FILL, dtype=torch.uint8, device='cuda')
        ncell = torch.full((F * T + 2 * GUARD,), WORD_FILL, dtype=torch.int32, device='cuda')
        gain = torch.full((F * T + 2 * GUARD,), WORD_FILL, dtype=torch.int32, device='cuda')
        p = lambda t, size: ctypes.c_void_p(t.data_ptr() + GUARD * size)   # noqa: E731
        rc = abi.load().lp_tile_gate_update_gain(desc, F, (ctypes.c_int * F)(*stream_of), self.S, ctypes.c_void_p(self.table.data_ptr()),
                                                 self.n_tiles, T, ctypes.c_void_p(self.ref.data_ptr()), self.ref_elems,
                                                 ctypes.c_void_p(self.age.data_ptr()), thres16, min_cells, refresh, lo, hi, p(flag, 1), p(ncell, 4),
                                                 p(gain, 4), _stream())
        abi.check(rc, 'lp_tile_gate_update_gain')
        torch.cuda.synchronize()
        outs = []
        for t, fill in ((flag, FLAG_FILL), (ncell, WORD_FILL), (gain, WORD_FILL)):
            host = t.cpu().numpy()
            assert (host[:GUARD] == fill).all() and (host[GUARD + F * T:] == fill).all(), 'a guard element of an output was written'
            assert (host[GUARD:GUARD + F * T] != fill).all(), 'an output entry was not written'
            outs.append(host[GUARD:GUARD + F * T].reshape(F, T))
        self.assert_guards()
        return outs

    def assert_guards(self):
        ref, age = self.ref_buf.cpu().numpy().view(np.uint16), self.age_buf.cpu().numpy()
        assert (ref[:GUARD] == POISON).all() and (ref[GUARD + self.ref_elems:] == POISON).all(), 'a guard element of ref was written'
        assert (age[:GUARD] == AGE_GUARD).all() and (age[GUARD + self.S * self.T:] == AGE_GUARD).all(), 'a guard element of age was written'


def _step(dev, state, grids, so, thres16, min_cells, refresh, lo=LO, hi=HI, what=''):
    """One call on the device and in the specification: flag, ncell, gain, ref and age must agree on every integer.  Returns the
    specification's (flags, ncell, gain)."""
    from yolov6.utils.tile_gate import gate_update_gain_np
    flag, ncell, gain = dev.update_gain(grids, so, thres16, min_cells, refresh, lo, hi)
    want = gate_update_gain_np(state, grids, so, thres16, min_cells, refresh, lo, hi)
    for f, s in enumerate(so):
        if s < 0:                                            # not gated: (1, 0, 0) for every t
            assert (flag[f] == 1).all() and not ncell[f].any() and not gain[f].any(), (what, f)
            continue
        nt = len(dev.plans[s])
        got = (flag[f, :nt].tolist(), ncell[f, :nt].tolist(), gain[f, :nt].tolist())
        assert got == (want[0][f], want[1][f], want[2][f]), (what, f)
        assert not flag[f, nt:].any() and not ncell[f, nt:].any() and not gain[f, nt:].any(), (what, f)      # t >= n_tiles: (0, 0, 0)
    dev.assert_state(state, what)
    return want


def _noisy(rng, base, gain):
    """``base`` (float) at ``gain`` with noise of sigma 2, as uint8 of the same shape; nothing saturates for base <= 120, gain <= 1.9."""
    v = np.floor(base * gain + rng.normal(0.0, 2.0, base.shape) + 0.5)
    assert v.max() < 255
    return v.clip(0, 255).astype(np.uint8)


def _grid(frame, nv12):
    from yolov6.utils.nv12 import Nv12Frame
    from yolov6.utils.tile_gate import luma_blocks_np
    if nv12:                                                 # the frame's first channel as a luma plane
        y = np.ascontiguousarray(frame[:, :, 0])
        return luma_blocks_np(Nv12Frame(y, np.zeros((y.shape[0] // 2, y.shape[1] // 2, 2), np.uint8)))
    return luma_blocks_np(frame)


@pytest.mark.parametrize('nv12', [False, True])
def test_update_gain_equals_the_specification_over_a_drifting_sequence(nv12):
    """Partial blocks and cells, a tile origin that is no multiple of 4, tiles of one block and of one cell, 289 cells (more than the
    lanes), age < 0, drift inside the range, a patch on top, drift above and below the range, a refresh that falls due, a frame of
    stream -1, a stream with fewer tiles than max_tiles, a stream absent from a call."""
    from yolov6.utils.tile_gate import GateState
    rng = np.random.default_rng(50)
    small = (38, 54) if nv12 else (37, 53)                   # (an NV12 frame has even sizes)
    shapes = [small, (272, 272), (64, 64)]
    plans = [[(0, 0) + small, (5, 7, 30, 41), (0, 0, 4, 4), (16, 16, 16, 16), (1, 2, 3, 3), (20, 35, 17, 18)],
             [(0, 0, 272, 272), (130, 141, 142, 131)], [(0, 0, 64, 64)]]
    dev, state = _GainGate(shapes, plans), GateState(shapes, plans)
    base = [rng.integers(10, 121, s + (3,)).astype(np.float64) for s in shapes]
    thres16, min_cells, refresh = 32, 1, 5
    #        gain per stream, stream_of
    calls = [((1.0, 1.0, 1.0), [0, 1, 2]), ((1.1, 0.9, 1.2), [1, 0, 2]), ((1.3, 0.8, 1.3), [2, -1, 0, 1]), ((1.3, 0.8, 1.3), [0, 1]),
             ((1.7, 0.5, 1.45), [1, 2, 0]), ((1.75, 0.52, 1.0), [-1]), ((1.75, 0.52, 1.0), [0, 1, 2]), ((1.75, 0.52, 1.0), [2, 1, 0]),
             ((1.8, 0.55, 1.05), [0, 1, 2])]
    seen, ranged = set(), set()
    for k, (gains, so) in enumerate(calls):
        frames = [_noisy(rng, b, g) for b, g in zip(base, gains)]
        if k == 3:                                           # a patch on top of the drift: some cells, not all
            frames[0][8:24, 20:40] = 200
            frames[1][100:140, 60:200] = 200
        grids = [_grid(frames[s], nv12) if s >= 0 else None for s in so]
        fl, nc, gn = _step(dev, state, grids, so, thres16, min_cells, refresh, what='call %d' % k)
        for f, s in enumerate(so):
            seen |= set(zip(fl[f], [min(n, 2) for n in nc[f]]))
            ranged |= {'below' if 0 < g < LO else 'above' if g > HI else 'in' if g else 'none' for g in gn[f]}
    assert {(1, 0), (0, 0), (1, 2)} <= seen and ranged == {'below', 'above', 'in', 'none'}
    assert max(state.age[0]) < refresh and state.age[2][0] < refresh


def _exact(gains):
    """(ref grid, cur grid) [4, 4 n] of a 16 x 16 n px frame whose cell c has exactly the gain ``gains[c]`` (None: no gain): its
    ref blocks are 256 each, R_c = 4096, and its cur blocks sum to the gain, so g_c = (C_c * 4096 + 2048) / 4096 = C_c."""
    n = len(gains)
    ref, cur = np.zeros((4, 4 * n), np.uint16), np.zeros((4, 4 * n), np.uint16)
    for c, g in enumerate(gains):
        if g is None:
            cur[:, 4 * c:4 * c + 4] = 77
            continue
        ref[:, 4 * c:4 * c + 4] = 256
        q, r = divmod(int(g), 16)
        blocks = np.full(16, q, np.uint16)
        blocks[:r] += 1
        assert blocks.max() <= 4080
        cur[:, 4 * c:4 * c + 4] = blocks.reshape(4, 4)
    return ref, cur


def test_the_median_is_selected_exactly():
    """Grids with chosen gains, one case per stream, all in one call after the call that sets ref: m in {0, 1, even, odd}, gains that
    differ only in the low byte or only in the high byte, all equal, ties around the median's rank, the cap, a median below lo and
    above hi, and gains spread over the 16 bits."""
    from yolov6.utils.tile_gate import GateState
    rng = np.random.default_rng(51)
    cases = [
        ('m = 0', [None] * 5, 4096),
        ('m = 1', [None, 5000, None], 5000),
        ('m = 2: the lower one', [4100, None, 4000], 4000),
        ('m = 4', [4100, 4000, 4200, 4300], 4100),
        ('m = 5', [4100, 4000, 4200, 4300, 3900], 4100),
        ('the low byte alone', [0x1000 + int(v) for v in rng.permutation(256)[:41]], None),
        ('the high byte alone', [(int(v) << 8) | 0x37 for v in rng.permutation(np.arange(1, 255))[:40]], None),
        ('all equal', [4321] * 33, 4321),
        ('ties at the rank', [4096] * 10 + [4095] * 9 + [4097] * 9, 4096),
        ('one high byte holds the rank, many low bytes', [0x1200 + int(v) for v in rng.integers(0, 256, 300)] + [100, 200, 60000, 65000], None),
        ('below lo', [2000] * 6 + [4096] * 5, 2000),
        ('above hi', [7000] * 6 + [4096] * 5, 7000),
        ('zero', [0] * 3 + [4096] * 2, 0),
        ('spread', [int(v) for v in rng.integers(0, 65281, 777)], None),
    ]
    shapes = [(16, 16 * len(g)) for _, g, _ in cases]
    plans = [[(0, 0) + s] for s in shapes]
    dev, state = _GainGate(shapes, plans), GateState(shapes, plans)
    so = list(range(len(cases)))
    pairs = [_exact(g) for _, g, _ in cases]
    _step(dev, state, [p[0] for p in pairs], so, 32, 1, 0, what='ref')
    fl, nc, gn = _step(dev, state, [p[1] for p in pairs], so, 32, 1, 0, what='cur')
    for k, (name, gains, want) in enumerate(cases):
        have = sorted(g for g in gains if g is not None)
        want = (have[(len(have) - 1) // 2] if have else 4096) if want is None else want
        assert gn[k] == [want], name
        assert fl[k] == [1] or LO <= want <= HI, name
    # the cap: R_c = 1 and C_c = 65280 in most cells
    ref, cur = np.zeros((4, 12), np.uint16), np.full((4, 12), 4080, np.uint16)
    ref[0, 0] = ref[0, 4] = 1
    ref[:, 8:] = 4080
    dev, state = _GainGate([(16, 48)], [[(0, 0, 16, 48)]]), GateState([(16, 48)], [[(0, 0, 16, 48)]])
    _step(dev, state, [ref], [0], 32, 1, 0, what='cap ref')
    assert _step(dev, state, [cur], [0], 32, 1, 0, hi=16384, what='cap')[2] == [[65535]]


def test_update_gain_flags_a_damaged_table_entry_and_touches_nothing():
    from yolov6.utils.tile_gate import luma_blocks_np
    shapes, plans = [(40, 64)], [[(0, 0, 32, 48), (8, 16, 32, 48), (0, 0, 40, 64)]]
    dev = _GainGate(shapes, plans)
    table = dev.table_np.copy()
    table[0, 0, :4] = (16, 0, 32, 48)                        # y0 + th > h0
    table[0, 1, 4] = dev.ref_elems - 10                      # its region would leave ref
    dev.table.copy_(torch.from_numpy(table))
    rng = np.random.default_rng(52)
    frame = rng.integers(0, 256, (40, 64, 3), dtype=np.uint8)
    for k in range(2):                                       # with age -1 and, for the good tile, with age 0
        grid = luma_blocks_np(frame if k == 0 else _edit(rng, frame, 3))
        flag, ncell, gain = dev.update_gain([grid], [0], 32, 1, 50)
        assert flag[0].tolist()[:2] == [1, 1] and ncell[0].tolist()[:2] == [-1, -1] and gain[0].tolist()[:2] == [0, 0]
        age, ref = dev.age.cpu().numpy(), dev.ref.cpu().numpy().view(np.uint16)
        assert age[0].tolist()[:2] == [-1, -1]
        o = int(table[0, 2, 4])
        assert (ref[:o] == POISON).all() and (ref[o + grid.size:] == POISON).all()          # no state byte of the damaged entries
    assert flag[0, 2] == 1 and ncell[0, 2] > 0 and np.array_equal(ref[o:o + grid.size], grid.reshape(-1))


def test_update_gain_with_a_unit_gain_is_lp_tile_gate_update():
    """More than half of the cells of every tile equal to ref: flag, ncell, ref and age are those of lp_tile_gate_update on a copy of
    the state, and every estimated gain is 4096."""
    from yolov6.core.tiles import plan_tiles
    from yolov6.utils.tile_gate import luma_blocks_np
    rng = np.random.default_rng(53)
    shapes = [(96, 160), (282, 277)]
    plans = [plan_tiles(shapes[0], (64, 64), 16), [(0, 0, 282, 277), (130, 141, 152, 136)]]
    a, b = _GainGate(shapes, plans), _DeviceGate(shapes, plans)
    frames = [rng.integers(1, 201, s + (3,), dtype=np.uint8) for s in shapes]
    changed = 0
    for k in range(4):
        if k:
            frames = [_edit(rng, f, 1) for f in frames]      # one patch of at most 19 x 19 px: at most 4 cells of a tile's 16 or more
        grids = [luma_blocks_np(f) for f in frames]
        for thres16, min_cells, refresh in ((32, 1, 3),):
            flag, ncell, gain = a.update_gain(grids, [0, 1], thres16, min_cells, refresh)
            want_f, want_n = b.update(grids, [0, 1], thres16, min_cells, refresh)
        assert np.array_equal(flag, want_f) and np.array_equal(ncell, want_n), k
        assert torch.equal(a.age, b.age) and torch.equal(a.ref, b.ref), k
        for f in range(2):
            assert set(gain[f, :len(plans[f])].tolist()) == ({0} if k == 0 else {4096}), k
        changed += int(ncell.sum())
    assert changed > 0


# ---- runtime.TileGate(illum='gain') ---------------------------------------------------------------------------------------------------
def _scaled(a, gain):
    v = np.floor(a.astype(np.float64) * gain + 0.5)
    assert v.max() < 255
    return v.astype(np.uint8)


@pytest.mark.parametrize('nv12', [False, True])
def test_tile_gate_gain_end_to_end(nv12):
    """First frame, drift, drift with a moved patch, drift out of range: flags, changed cells, gains and stats are ``TileGateNp``'s;
    the rows are ``detect_tiled_padded``'s bit for bit where every tile is detected, and the first call's where none is."""
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import Nv12Frame, bgr_to_nv12_np
    from yolov6.utils.tile_gate import TileGateNp
    m = _tiny(torch.float16)
    size, conf, iou, max_det, kw = [64, 64], 0.06, 0.45, 40, dict(overlap=16, batch=8)
    shapes = [(96, 160), (80, 120)]
    rng = np.random.default_rng(54)
    bgr = [rng.integers(10, 141, s + (3,), dtype=np.uint8) for s in shapes]
    host = [bgr_to_nv12_np(f, 'bt601') for f in bgr] if nv12 else bgr

    def drift(frames, gain, patch=None):
        """The frames at ``gain`` (an NV12 frame: its luma plane), stream 0 with a 16 x 16 patch of other pixels where given."""
        out = []
        for k, f in enumerate(frames):
            px = _scaled(np.asarray(f.y) if nv12 else f, gain)
            if patch is not None and k == 0:
                px[patch] = rng.integers(150, 250, px[patch].shape, dtype=np.uint8)
            out.append(Nv12Frame(px, np.asarray(f.uv)) if nv12 else px)
        return out

    with torch.no_grad():
        gate = runtime.TileGate(m, shapes, size, conf, iou, max_det, illum='gain', max_gain=1.5, **kw)
        spec = TileGateNp(StubDetector(), shapes, (64, 64), iou, max_det, overlap=16, illum='gain', max_gain=1.5)
        n_tiles = [len(p) for p in gate.plans]
        assert n_tiles == [len(p) for p in spec.state.plans] and min(n_tiles) >= 5 and gate.plans[0][-1] == (0, 0) + shapes[0]

        def full(frames):
            det, count = runtime.detect_tiled_padded(m, frames, size, conf, iou, max_det, **kw)
            return det.clone(), count.clone()

        def step(frames_host):
            frames = [f.to('cuda') if nv12 else torch.from_numpy(f).cuda() for f in frames_host]
            det, count = gate.detect_padded(frames)
            spec.detect_padded(frames_host)
            assert gate.last_flags == spec.last_flags and gate.last_ncell == spec.last_ncell and gate.last_gain == spec.last_gain
            assert {k: v for k, v in gate.stats.items() if k != 'forwards'} == {k: v for k, v in spec.stats.items() if k != 'forwards'}
            return frames, det.clone(), count.clone()

        # the first frame: everything is detected
        frames, det_a, count_a = step(host)
        want = full(frames)
        assert gate.last_flags == [[1] * n for n in n_tiles] and gate.last_gain == [[0] * n for n in n_tiles]
        assert _same(det_a, want[0]) and _same(count_a, want[1])
        forwards = gate.stats['forwards']
        # drift alone: no forward, the same bytes, one gain everywhere
        _, det_b, count_b = step(drift(host, 1.1))
        assert gate.last_flags == [[0] * n for n in n_tiles] and gate.stats['forwards'] == forwards
        assert all(abs(g - 4506) <= 40 for gn in gate.last_gain for g in gn), gate.last_gain
        assert _same(det_b, det_a) and _same(count_b, count_a)
        # more drift and a patch: the tiles that own it, the overview among them, and no tile of the other stream
        step(drift(host, 1.2, (slice(30, 46), slice(60, 76))))
        on = gate.last_flags
        assert 0 < sum(on[0]) < n_tiles[0] and on[0][-1] == 1 and not any(on[1]) and gate.stats['forwards'] == forwards + 1
        # drift out of the range: everything is detected again (the tiles of the patch are at 1.7 / 1.2, in range, but the patch is
        # gone), and the result is a full detection's
        frames, det_d, count_d = step(drift(host, 1.7))
        assert gate.last_flags == [[1] * n for n in n_tiles]
        assert gate.stats['tiles_out_of_range'] == n_tiles[0] - sum(on[0]) + n_tiles[1]
        want = full(frames)
        assert _same(det_d, want[0]) and _same(count_d, want[1])
        # the same frame again: a gain of exactly 1
        det_1, count_1 = gate.detect_padded([frames[1]], stream_of=[1])
        assert _same(det_1, det_d[1:]) and _same(count_1, count_d[1:])
        assert gate.last_flags == [[0] * n_tiles[1]] and set(gate.last_gain[0]) == {4096} and gate.stats['calls'] == 5


def test_infer_tile_gate_gain_gpu(tmp_path, monkeypatch, caplog):
    from PIL import Image
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    first = np.random.default_rng(55).integers(10, 141, (150, 200, 3), dtype=np.uint8)
    for k, g in enumerate((1.0, 1.1, 1.2, 0.9)):
        Image.fromarray(_scaled(first, g)).save(str(img_dir / ('f%d.png' % k)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[96, 96], conf_thres=0.06, iou_thres=0.45, max_det=30, device='0',
              save_txt=True, not_save_img=True, half=True, tile=[96, 96], tile_overlap=24, batch_size=8, tile_gate=True)
    with caplog.at_level(logging.INFO):
        gated = infer.run(save_dir=str(tmp_path / 'o1'), tile_gate_illum='gain', tile_gate_max_gain=1.5, **kw)
    line = [r.getMessage() for r in caplog.records if r.getMessage().startswith('Tile gate:')]
    assert len(line) == 1 and '; gain ' in line[0] and line[0].endswith(', 0 tiles out of range'), line
    low, high = (float(v) for v in line[0].split('; gain ')[1].split(',')[0].split('..'))
    assert abs(low - 0.9) <= 0.01 and abs(high - 1.2) <= 0.01, line
    n = int(line[0].split()[4])
    assert line[0].startswith('Tile gate: %d of %d tiles detected (4 calls, ' % (n // 4, n)) and n >= 16, line
    assert len(gated) == 4 and all(torch.equal(d, gated[0]) for d in gated)               # the rows of the first frame throughout
    caplog.clear()
    with caplog.at_level(logging.INFO):
        infer.run(save_dir=str(tmp_path / 'o0'), **kw)                                     # without the gain every frame is detected whole
    line = [r.getMessage() for r in caplog.records if r.getMessage().startswith('Tile gate:')]
    assert len(line) == 1 and line[0].startswith('Tile gate: %d of %d tiles detected (4 calls, ' % (n, n)) and 'gain' not in line[0], line
