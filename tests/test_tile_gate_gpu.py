"""The tile gate on the GPU, bit for bit: lp_tile_gate_luma_batch against ``luma_blocks_np`` at the edges of its loads,
lp_tile_gate_update against ``gate_update_np`` over a sequence of calls, ``runtime.TileGate`` against ``detect_tiled_padded`` and
``TileGateNp``, and ``Inferer(tile=..., tile_gate=True)`` against the run without the gate."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_tile_gate_cpu import StubDetector, repeated_image_dir

pytestmark = pytest.mark.gpu

CFG = lambda n: os.path.join(REPO, 'configs', n + '.py')   # noqa: E731
POISON = 0x7777


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- lp_tile_gate_luma_batch == luma_blocks_np ---------------------------------------------------------------------------------------
def _luma_gpu(planes, fmt):
    """lp_tile_gate_luma_batch on ``planes`` = [(device tensor of the plane's bytes, pitch, h, w)] of one format, every grid between
    guards in one poisoned buffer: the grids as numpy arrays.  The guards must come back untouched."""
    from yolov6.hip import abi
    from yolov6.utils.tile_gate import grid_shape
    G = 24                                                   # guard elements on both sides of every grid
    sizes = [grid_shape(h, w) for _, _, h, w in planes]
    offs, n = [], G
    for a, b in sizes:
        offs.append(n)
        n += a * b + G
    out = torch.full((n,), POISON, dtype=torch.int16, device='cuda')
    desc = (abi.TileGateDesc * len(planes))()
    for d, (t, pitch, h, w), o in zip(desc, planes, offs):
        d.p0, d.pitch0, d.h0, d.w0, d.format, d.blocks = t.data_ptr(), pitch, h, w, fmt, out.data_ptr() + 2 * o
    abi.check(abi.load().lp_tile_gate_luma_batch(desc, len(planes), _stream()), 'lp_tile_gate_luma_batch')
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint16)
    keep = np.ones(n, bool)
    grids = []
    for (a, b), o in zip(sizes, offs):
        grids.append(host[o:o + a * b].reshape(a, b))
        keep[o:o + a * b] = False
    assert (host[keep] == POISON).all(), 'a guard element was written'
    return grids


def test_luma_bgr_edges_in_one_call():
    """Widths around the 16-pixel unit, heights around the 4-row band, all frames in one call and back to back in one allocation
    that ends at the last pixel of the last frame (its guard is another tensor): a frame starts wherever the one before ended, so
    the loads are at every alignment, and a tail read past a row would pick up the next frame's (or the guard's) bytes."""
    from yolov6.utils.tile_gate import luma_blocks_np
    rng = np.random.default_rng(20)
    shapes = [(h, w) for w in (15, 16, 17, 63, 64, 65) for h in (1, 4, 5, 9)] + [(70, 100), (3, 1), (1, 1)]
    host = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    buf = torch.from_numpy(np.concatenate([f.reshape(-1) for f in host])).cuda()
    guard = torch.full((4096,), 255, dtype=torch.uint8, device='cuda')
    assert buf.numel() == sum(h * w * 3 for h, w in shapes)
    planes, off = [], 0
    for h, w in shapes:
        planes.append((buf[off:off + h * w * 3], 3 * w, h, w))
        off += h * w * 3
    assert len({p[0].data_ptr() % 16 for p in planes}) > 4
    for got, f, s in zip(_luma_gpu(planes, 0), host, shapes):
        assert np.array_equal(got, luma_blocks_np(f)), s
    assert bool((guard == 255).all())


def test_luma_nv12_edges_and_pitches():
    from yolov6.utils.nv12 import Nv12Frame
    from yolov6.utils.tile_gate import luma_blocks_np
    rng = np.random.default_rng(21)
    shapes = [(h, w) for w in (16, 18, 62, 64, 66) for h in (2, 4, 6, 10)] + [(70, 100)]
    for pitched in (False, True):
        host, planes = [], []
        for h, w in shapes:
            pitch = (w + 63) // 64 * 64 + 64 if pitched else w
            raw = rng.integers(0, 256, (h - 1) * pitch + w, dtype=np.uint8)           # ends at the last pixel of the last row
            y = np.lib.stride_tricks.as_strided(raw, (h, w), (pitch, 1))
            host.append(Nv12Frame(y, np.zeros((h // 2, w // 2, 2), np.uint8)))
            planes.append((torch.from_numpy(raw).cuda(), pitch, h, w))
        for got, f, s in zip(_luma_gpu(planes, 1), host, shapes):
            assert np.array_equal(got, luma_blocks_np(f)), (pitched, s)


# ---- lp_tile_gate_update == gate_update_np -------------------------------------------------------------------------------------------
class _DeviceGate:
    """The device state of lp_tile_gate_update for ``plans`` (built here, not by the runtime) and one call through the ABI."""

    def __init__(self, shapes, plans):
        from yolov6.hip import abi
        from yolov6.utils.tile_gate import grid_shape, tile_blocks
        self.abi, self.shapes, self.plans = abi, shapes, plans
        self.S, self.T = len(plans), max(len(p) for p in plans)
        table = np.zeros((self.S, self.T, 8), np.int32)
        off = 5                                              # ref does not begin at a region
        for s, plan in enumerate(plans):
            for t, tile in enumerate(plan):
                by0, by1, bx0, bx1 = tile_blocks(tile)
                table[s, t, :5] = tuple(tile) + (off,)
                off += (by1 - by0 + 1) * (bx1 - bx0 + 1) + 3   # and the regions have gaps between them
        self.table_np, self.ref_elems = table, off
        self.table = torch.from_numpy(table).cuda()
        self.ref = torch.full((off,), POISON, dtype=torch.int16, device='cuda')
        self.age = torch.full((self.S, self.T), -1, dtype=torch.int32, device='cuda')
        self.grids = [torch.zeros(grid_shape(h, w), dtype=torch.int16, device='cuda') for h, w in shapes]
        self.n_tiles = (ctypes.c_int * self.S)(*[len(p) for p in plans])

    def update(self, grids, stream_of, thres16, min_cells, refresh):
        abi, F = self.abi, len(stream_of)
        desc = (abi.TileGateDesc * F)()
        for d, g, s in zip(desc, grids, stream_of):
            if s >= 0:
                self.grids[s].copy_(torch.from_numpy(g.view(np.int16)))
                d.h0, d.w0, d.blocks = self.shapes[s][0], self.shapes[s][1], self.grids[s].data_ptr()
        flag = torch.full((F, self.T), 9, dtype=torch.uint8, device='cuda')
        ncell = torch.full((F, self.T), -9, dtype=torch.int32, device='cuda')
        rc = abi.load().lp_tile_gate_update(desc, F, (ctypes.c_int * F)(*stream_of), self.S, ctypes.c_void_p(self.table.data_ptr()), self.n_tiles,
                                            self.T, ctypes.c_void_p(self.ref.data_ptr()), self.ref_elems, ctypes.c_void_p(self.age.data_ptr()),
                                            thres16, min_cells, refresh, ctypes.c_void_p(flag.data_ptr()), ctypes.c_void_p(ncell.data_ptr()),
                                            _stream())
        abi.check(rc, 'lp_tile_gate_update')
        torch.cuda.synchronize()
        return flag.cpu().numpy(), ncell.cpu().numpy()

    def assert_state(self, state, what):
        """ref and age against the specification's: the regions of detected tiles bit for bit, everything else as it was filled."""
        ref, age = self.ref.cpu().numpy().view(np.uint16), self.age.cpu().numpy()
        want_ref = np.full(self.ref_elems, POISON, np.uint16)
        want_age = np.full((self.S, self.T), -1, np.int32)
        for s, plan in enumerate(self.plans):
            for t in range(len(plan)):
                want_age[s, t] = state.age[s][t]
                if state.age[s][t] >= 0:
                    r = state.ref[s][t].reshape(-1)
                    o = self.table_np[s, t, 4]
                    want_ref[o:o + r.size] = r
        assert np.array_equal(age, want_age), what
        assert np.array_equal(ref, want_ref), what


def _edit(rng, frame, n):
    out = frame.copy()
    h, w = frame.shape[:2]
    for _ in range(n):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        hh, ww = int(rng.integers(1, 20)), int(rng.integers(1, 20))
        out[y:y + hh, x:x + ww] = (out[y:y + hh, x:x + ww].astype(np.int32) + int(rng.integers(1, 40))).clip(0, 255).astype(np.uint8)
    return out


def test_update_equals_the_specification_over_six_calls():
    from yolov6.core.tiles import plan_tiles
    from yolov6.utils.tile_gate import GateState, gate_update_np, luma_blocks_np
    rng = np.random.default_rng(22)
    shapes = [(70, 100), (96, 160), (64, 64)]
    plans = [plan_tiles(shapes[0], (32, 48), 8), plan_tiles(shapes[1], (32, 48), 8), [(0, 0, 64, 64)]]
    assert [len(p) for p in plans] == [10, 17, 1]
    dev, state = _DeviceGate(shapes, plans), GateState(shapes, plans)
    frames = [rng.integers(0, 201, s + (3,), dtype=np.uint8) for s in shapes]
    thres16, min_cells, refresh = 24, 2, 4
    calls = [[0, 1, 2], [1, 0, 2], [2, -1, 0], [0, 1], [-1], [1, 2, 0]]               # stream 1 absent from call 2, stream 2 from call 3; two -1 frames
    seen = set()
    for k, so in enumerate(calls):
        for s in set(so) - {-1}:
            frames[s] = _edit(rng, frames[s], int(rng.integers(0, 4)) if k else 0)
        grids = [luma_blocks_np(frames[s]) if s >= 0 else None for s in so]
        flag, ncell = dev.update(grids, so, thres16, min_cells, refresh)
        want_f, want_n = gate_update_np(state, grids, so, thres16, min_cells, refresh)
        for f, s in enumerate(so):
            nt = len(plans[s]) if s >= 0 else 0
            if s < 0:
                assert (flag[f] == 1).all() and (ncell[f] == 0).all(), (k, f)
                continue
            assert flag[f, :nt].tolist() == want_f[f] and ncell[f, :nt].tolist() == want_n[f], (k, f)
            assert not flag[f, nt:].any() and not ncell[f, nt:].any(), (k, f)
            seen |= set(zip(want_f[f], [min(n, 2) for n in want_n[f]]))
        dev.assert_state(state, 'call %d' % k)
    assert {(1, 0), (0, 0), (0, 1), (1, 2)} <= seen


def test_update_with_more_cells_than_lanes_and_with_one_cell():
    from yolov6.utils.tile_gate import GateState, gate_update_np, luma_blocks_np
    rng = np.random.default_rng(23)
    shapes = [(282, 277), (16, 16), (9, 13)]
    plans = [[(0, 0, 282, 277), (130, 141, 152, 136)], [(0, 0, 16, 16)], [(0, 0, 9, 13), (3, 5, 6, 8)]]
    dev, state = _DeviceGate(shapes, plans), GateState(shapes, plans)
    assert ((282 + 15) // 16) * ((277 + 15) // 16) > 256                              # cells of the first tile: more than a workgroup's lanes
    frames = [rng.integers(0, 201, s + (3,), dtype=np.uint8) for s in shapes]
    big = 0
    for k in range(4):
        if k:
            frames[0] = _edit(rng, frames[0], 60)
            frames[1] = _edit(rng, frames[1], k - 1)
            frames[2] = _edit(rng, frames[2], 1)
        grids = [luma_blocks_np(f) for f in frames]
        flag, ncell = dev.update(grids, [0, 1, 2], 32, 1, 0)
        want_f, want_n = gate_update_np(state, grids, [0, 1, 2], 32, 1, 0)
        for f in range(3):
            nt = len(plans[f])
            assert flag[f, :nt].tolist() == want_f[f] and ncell[f, :nt].tolist() == want_n[f], (k, f)
        dev.assert_state(state, 'call %d' % k)
        big = max(big, want_n[0][0])
        assert want_n[1][0] <= 1
    assert big > 20


def test_update_flags_a_damaged_table_entry_and_touches_nothing():
    """The host cannot see the device table: an entry outside its frame, or whose region leaves ref, is flagged with ncell -1."""
    from yolov6.utils.tile_gate import luma_blocks_np
    shapes, plans = [(40, 64)], [[(0, 0, 32, 48), (8, 16, 32, 48), (0, 0, 40, 64)]]
    dev = _DeviceGate(shapes, plans)
    table = dev.table_np.copy()
    table[0, 0, :4] = (16, 0, 32, 48)                        # y0 + th > h0
    table[0, 1, 4] = dev.ref_elems - 10                      # its region would leave ref
    dev.table.copy_(torch.from_numpy(table))
    grid = luma_blocks_np(np.random.default_rng(24).integers(0, 256, (40, 64, 3), dtype=np.uint8))
    flag, ncell = dev.update([grid], [0], 32, 1, 50)
    assert flag[0].tolist() == [1, 1, 1] and ncell[0].tolist() == [-1, -1, 0]
    age, ref = dev.age.cpu().numpy(), dev.ref.cpu().numpy().view(np.uint16)
    assert age[0].tolist() == [-1, -1, 2]
    o = int(table[0, 2, 4])
    assert np.array_equal(ref[o:o + grid.size], grid.reshape(-1)) and (ref[:o] == POISON).all() and (ref[o + grid.size:] == POISON).all()


# ---- runtime.TileGate -----------------------------------------------------------------------------------------------------------------
def _tiny(dtype):
    from yolov6.utils.synth import build_synthetic
    return build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5).cuda().to(dtype)


def _upload(host, nv12):
    from yolov6.utils.nv12 import bgr_to_nv12_np
    if nv12:
        return [bgr_to_nv12_np(f, 'bt601').to('cuda') for f in host]
    return [torch.from_numpy(f).cuda() for f in host]


def _host_view(host, nv12):
    """The frames as the CPU form of the gate sees them."""
    from yolov6.utils.nv12 import bgr_to_nv12_np
    return [bgr_to_nv12_np(f, 'bt601') for f in host] if nv12 else host


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('dtype,nv12', [(torch.float32, False), (torch.float16, False), (torch.float16, True), (torch.float32, True)])
def test_tile_gate_end_to_end(dtype, nv12):
    from yolov6.hip import runtime
    from yolov6.utils.tile_gate import TileGateNp
    m = _tiny(dtype)
    size, conf, iou, max_det, kw = [64, 64], 0.06, 0.45, 40, dict(overlap=16, batch=8)
    shapes = [(96, 160), (80, 120)]
    rng = np.random.default_rng(25)
    host = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    with torch.no_grad():
        gate = runtime.TileGate(m, shapes, size, conf, iou, max_det, **kw)
        spec = TileGateNp(StubDetector(), shapes, (64, 64), iou, max_det, overlap=16)
        n_tiles = [len(p) for p in gate.plans]
        assert n_tiles == [len(p) for p in spec.state.plans] and min(n_tiles) >= 5 and sum(n_tiles) > 8

        def full(frames):
            det, count = runtime.detect_tiled_padded(m, frames, size, conf, iou, max_det, **kw)
            return det.clone(), count.clone()

        def step(frames_host):
            frames = _upload(frames_host, nv12)
            det, count = gate.detect_padded(frames)
            spec.detect_padded(_host_view(frames_host, nv12))
            assert gate.last_flags == spec.last_flags and gate.last_ncell == spec.last_ncell
            return frames, det.clone(), count.clone()

        # (a) the first call: everything is flagged, the result is detect_tiled_padded's
        frames, det_a, count_a = step(host)
        assert gate.last_flags == [[1] * n for n in n_tiles]
        want = full(frames)
        assert _same(det_a, want[0]) and _same(count_a, want[1]) and int(count_a.sum()) > 0
        forwards = gate.stats['forwards']
        assert gate.stats['tiles_detected'] == sum(n_tiles) and forwards == -(-sum(n_tiles) // 8)
        # (b) the same frames again: no forward, the same bytes
        _, det_b, count_b = step(host)
        assert gate.last_flags == [[0] * n for n in n_tiles] and gate.stats['forwards'] == forwards
        assert _same(det_b, det_a) and _same(count_b, count_a)
        # (d) a change below the bar: the output of (b)
        low = [f.copy() for f in host]
        low[0][40, 70] ^= 3
        _, det_d, count_d = step(low)
        assert gate.stats['forwards'] == forwards and _same(det_d, det_b) and _same(count_d, count_b)
        # (c) a 16 x 16 patch overwritten (the small change undone): the flags of the CPU form, the result of a full detection
        new = [f.copy() for f in host]
        new[0][30:46, 60:76] = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
        frames, det_c, count_c = step(new)
        on = gate.last_flags
        assert 0 < sum(on[0]) < n_tiles[0] and on[0][-1] == 1 and not any(on[1])
        assert gate.stats['forwards'] == forwards + 1 and gate.stats['tiles_detected'] == sum(n_tiles) + sum(on[0])
        want = full(frames)
        assert _same(det_c, want[0]) and _same(count_c, want[1])
        # a call with one stream, in another order of streams, and unpadded
        det_1, count_1 = gate.detect_padded([frames[1]], stream_of=[1])
        spec.detect_padded([_host_view(new, nv12)[1]], stream_of=[1])
        assert gate.last_flags == [[0] * n_tiles[1]] and _same(det_1, det_c[1:]) and _same(count_1, count_c[1:])
        outs = gate.detect([frames[1], frames[0]], stream_of=[1, 0])
        spec.detect_padded(_host_view(new, nv12)[::-1], stream_of=[1, 0])
        counts = count_c.tolist()
        assert [len(o) for o in outs] == counts[::-1] and torch.equal(outs[1], det_c[0, :counts[0]]) and torch.equal(outs[0], det_c[1, :counts[1]])
        # (f) steady calls allocate nothing on the device
        torch.cuda.synchronize()
        for _ in range(10):
            before = torch.cuda.memory_stats()['allocation.all.allocated']
            det, count = gate.detect_padded(frames)
            assert torch.cuda.memory_stats()['allocation.all.allocated'] == before
        assert _same(det, det_c) and _same(count, count_c) and gate.stats['forwards'] == forwards + 1
        # (e) reset: everything is flagged again
        gate.reset([0])
        assert not bool(gate.cache_count[0].any()) and bool(gate.cache_count[1].any())
        gate.detect_padded(frames)
        assert gate.last_flags == [[1] * n_tiles[0], [0] * n_tiles[1]]
        gate.reset()
        det, count = gate.detect_padded(frames)
        assert gate.last_flags == [[1] * n for n in n_tiles] and _same(det, det_c) and _same(count, count_c)
        # a frame of stream -1 goes through detect_tiled_padded and leaves no trace
        ages = gate.age.clone()
        det, count = gate.detect_padded([frames[0], frames[1]], stream_of=[-1, 1])
        assert gate.last_flags == [[1] * n_tiles[0], [0] * n_tiles[1]] and _same(det, det_c) and _same(count, count_c)
        assert torch.equal(gate.age[0], ages[0]) and torch.equal(gate.age[1], ages[1] + 1)
        with pytest.raises(ValueError, match='fixed frame size'):
            gate.detect_padded(frames[::-1])
        with pytest.raises(ValueError, match='twice'):
            gate.detect_padded(frames, stream_of=[1, 1])


def test_infer_tile_gate_gpu(tmp_path, monkeypatch):
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': m.half(), 'ema': None}, str(ckpt))
    img_dir = repeated_image_dir(tmp_path)
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[96, 96], conf_thres=0.06, iou_thres=0.45, max_det=30, device='0',
              save_txt=True, not_save_img=True, half=True, tile=[96, 96], tile_overlap=24, batch_size=8, save_crops=True, crop_size=(16, 48))
    plain = infer.run(save_dir=str(tmp_path / 'o0'), **kw)
    gated = infer.run(save_dir=str(tmp_path / 'o1'), tile_gate=True, **kw)
    assert len(plain) == len(gated) == 4 and sum(len(d) for d in plain) > 0
    for a, b in zip(plain, gated):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    files = sorted(str(p.relative_to(tmp_path / 'o0')) for p in (tmp_path / 'o0').rglob('*') if p.is_file())
    assert files == sorted(str(p.relative_to(tmp_path / 'o1')) for p in (tmp_path / 'o1').rglob('*') if p.is_file()) and len(files) > 4
    for name in files:
        assert (tmp_path / 'o0' / name).read_bytes() == (tmp_path / 'o1' / name).read_bytes(), name
