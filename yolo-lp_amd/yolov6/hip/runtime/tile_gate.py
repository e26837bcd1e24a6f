"""Tiled detection of fixed-camera streams that runs the network only on the tiles that changed (lp_tile_gate_luma_batch,
lp_tile_gate_update*; yolov6/utils/tile_gate.py states the rule)."""
import ctypes

import numpy as np
import torch

from yolov6.hip import abi

from ._base import _dptr, _frames_on, _persistent, _stream_ptr, _unpad
from .tiles import _METRICS, detect_tiled_padded, detect_tiles_padded, merge_tiles, merge_tiles_buffers, plan_tiled


class TileGate:
    """Tiled detection of fixed-camera streams that runs the network only on the tiles that changed (lp_tile_gate_luma_batch,
    lp_tile_gate_update; ``yolov6.utils.tile_gate`` states the rule and ``TileGateNp`` there is the same class on the CPU).
    ``frame_shapes[s]`` is the fixed (h, w) of camera stream s; the tile plan of every stream is ``plan_tiled``'s, made once; the
    other arguments are ``detect_tiled``'s, plus the rule's ``thres`` (luma levels per pixel a 16 x 16 cell must change by),
    ``min_cells`` (changed cells that flag a tile) and ``refresh`` (calls after which a tile is detected again anyway, 0: never).
    The object owns the device tile table, the per-tile reference block sums and ages, the block grids of the current frames, the
    flags, and a detection cache per stream -- ``cache_det`` [S,Tmax,tile_max_det,28] fp32 and ``cache_count`` [S,Tmax] int32,
    tile-local rounded rows as ``detect_tiles_padded`` returns them.

    ``detect_padded(frames, stream_of=None)`` -> (det [F,max_det,28], count [F] int32) on the device, in frame pixels, with the
    shape and meaning of ``detect_tiled_padded``'s: what ``PlateTracker.update``, ``plate_crops``, ``redact_plates`` and
    ``LookbackRedactor`` take.  ``frames``: BGR device tensors or ``Nv12Frame``s (one kind), frame f of stream ``stream_of[f]``
    (default f); every stream at most once per call, every frame of its stream's shape.  A frame of stream -1 is not gated: it
    goes through ``detect_tiled_padded`` as it is and nothing of it is kept.  Per call: the luma kernel, the update kernel, ONE
    HOST READ of the flags and changed-cell counts (5 bytes per tile slot; the host builds the tile batches, so it must know),
    ``detect_tiles_padded`` on the flagged tiles only (no forward when nothing is flagged), their rows into the cache, the
    call's tiles gathered from the cache, ``merge_tiles`` over the full tile table.  With every tile flagged the result is
    ``detect_tiled_padded``'s bit for bit (with ``tile_max_det`` derived from the streams' plans; the engine computes a tile's rows
    independently of its batch slot).  A steady call allocates nothing on the device; the returned tensors are persistent per
    combination of streams: a later call with the same ``stream_of`` overwrites them.
    ``last_flags`` / ``last_ncell``: per frame of the last call the host lists over its tiles (a frame of stream -1: all 1 / 0);
    ``stats``: calls, tiles_seen, tiles_detected, forwards, summed since construction.
    ``illum='gain'`` (lp_tile_gate_update_gain) tolerates exposure and daylight drift: the cells of a tile are compared after the
    reference is scaled by the tile's gain, the median of its cells' gains, within [1 / ``max_gain``, ``max_gain``]; outside that
    range the tile is detected again.  The one host read then carries 9 bytes per slot; ``last_gain`` holds the Q12 gains of
    the last call (4096 = 1; 0: no estimate -- a never-detected tile, a frame of stream -1, and always with ``illum='none'``), and
    ``stats`` has ``tiles_out_of_range`` as well."""

    def __init__(self, model, frame_shapes, img_size, conf_thres, iou_thres, max_det, tile_hw=None, overlap=0.2, overview=True,
                 metric='iou', border=1, batch=32, tile_max_det=None, thres=2.0, min_cells=1, refresh=50, illum='none', max_gain=1.5):
        from yolov6.utils import tile_gate as tg
        self.thres16, self.min_cells, self.refresh = tg.check_params(thres, min_cells, refresh)
        self.gain_lo, self.gain_hi = tg.check_illum(illum, max_gain)
        self.illum = illum
        if metric not in _METRICS:
            raise ValueError('metric must be one of %s' % sorted(_METRICS))
        self.model, self.img_size = model, img_size
        self.conf_thres, self.iou_thres, self.max_det = conf_thres, iou_thres, int(max_det)
        self.tile_hw, self.overlap, self.overview, self.metric, self.border, self.batch = tile_hw, overlap, overview, metric, border, int(batch)
        self.shapes = [(int(s[0]), int(s[1])) for s in frame_shapes]
        if not self.shapes:
            raise ValueError('TileGate needs at least one stream')
        tiles, self.tile_max_det = plan_tiled(self.shapes, img_size, max_det, tile_hw, overlap, overview, tile_max_det)
        self._arg_tile_max_det = tile_max_det
        S = self.n_streams = len(self.shapes)
        self.plans = [[t[1:] for t in tiles if t[0] == s] for s in range(S)]
        Tmax = self.max_tiles = max(len(p) for p in self.plans)
        dev = next(model.parameters()).device
        if dev.type != 'cuda':
            raise ValueError('TileGate runs on a GPU (TileGateNp is the CPU form)')
        self.device = dev
        W = abi.LP_TILE_GATE_TILE_WORDS
        table = np.zeros((S, Tmax, W), np.int32)
        off = 0
        for s, plan in enumerate(self.plans):
            for t, tile in enumerate(plan):
                by0, by1, bx0, bx1 = tg.tile_blocks(tile)
                table[s, t, :5] = tile + (off,)
                off += (by1 - by0 + 1) * (bx1 - bx0 + 1)
        if off >= 1 << 31:
            raise ValueError('TileGate: the reference block sums of these streams exceed 2^31 entries')
        self._ref_elems = off
        self._n_tiles = (ctypes.c_int * S)(*[len(p) for p in self.plans])
        with torch.cuda.device(dev):
            self._table = torch.from_numpy(table).to(dev)
            self.ref = torch.zeros(off, dtype=torch.int16, device=dev)           # uint16 bit patterns
            self.age = torch.full((S, Tmax), -1, dtype=torch.int32, device=dev)
            cells = [tg.grid_shape(h, w) for h, w in self.shapes]
            starts = np.cumsum([0] + [(a * b + 7) // 8 * 8 for a, b in cells])
            self._grids = torch.zeros(int(starts[-1]), dtype=torch.int16, device=dev)
            self._grid_ptr = [self._grids.data_ptr() + 2 * int(o) for o in starts[:-1]]
            # ncell int32 [S*Tmax], in gain mode gain int32 [S*Tmax], then flag uint8 [S*Tmax]: one read
            self._out_words = 2 if illum == 'gain' else 1
            nb = (4 * self._out_words + 1) * S * Tmax
            self._out = torch.zeros(nb, dtype=torch.uint8, device=dev)
            self._out_host = torch.zeros(nb, dtype=torch.uint8).pin_memory()
            self.cache_det = torch.zeros(S, Tmax, self.tile_max_det, abi.LP_DET_COLS, dtype=torch.float32, device=dev)
            self.cache_count = torch.zeros(S, Tmax, dtype=torch.int32, device=dev)
        self._calls = {}
        self.last_flags, self.last_ncell, self.last_gain = [], [], []
        self.stats = dict(calls=0, tiles_seen=0, tiles_detected=0, forwards=0)
        if illum == 'gain':
            self.stats['tiles_out_of_range'] = 0

    def reset(self, streams=None):
        """Forget ``streams`` (all for None): their tiles count as never detected and their cached rows are cleared."""
        for s in (range(self.n_streams) if streams is None else streams):
            self.age[int(s)].fill_(-1)
            self.cache_det[int(s)].zero_()
            self.cache_count[int(s)].zero_()

    def _call_buffers(self, streams):
        """The persistent buffers of the calls whose gated frames are of ``streams``, in that order."""
        def make():
            idx = [s * self.max_tiles + t for s in streams for t in range(len(self.plans[s]))]
            tiles = [(k,) + tuple(tile) for k, s in enumerate(streams) for tile in self.plans[s]]
            dev = self.device
            return dict(idx=torch.tensor(idx, dtype=torch.int64, device=dev), tiles=tiles, shapes=[self.shapes[s] for s in streams],
                        det_t=torch.empty(len(idx), self.tile_max_det, abi.LP_DET_COLS, dtype=torch.float32, device=dev),
                        count_t=torch.empty(len(idx), dtype=torch.int32, device=dev),
                        merge=merge_tiles_buffers(len(streams), self.max_det, dev))
        return _persistent(self._calls, tuple(streams), make)

    def _describe(self, frames, streams, nv12):
        """The lp_tile_gate_desc array of ``frames`` (of ``streams``, one kind): planes, sizes and each stream's block grid."""
        desc = (abi.TileGateDesc * len(frames))()
        for d, fr, s in zip(desc, frames, streams):
            if nv12:
                d.p0, d.pitch0, d.format = fr.y.data_ptr(), fr.pitch_y, 1
            else:
                d.p0, d.pitch0, d.format = fr.data_ptr(), 3 * fr.shape[1], 0
            d.h0, d.w0, d.blocks = fr.shape[0], fr.shape[1], self._grid_ptr[s]
        return desc

    def _luma(self, desc):
        """lp_tile_gate_luma_batch on the current stream: the block sums of the described frames into their streams' grids."""
        abi.check(abi.load().lp_tile_gate_luma_batch(desc, len(desc), _stream_ptr(self.device)), 'lp_tile_gate_luma_batch')

    def _update(self, desc, streams):
        """lp_tile_gate_update on the current stream: flags and changed-cell counts of the call into ``_out``, ref and age moved on."""
        S, Tmax, n = self.n_streams, self.max_tiles, len(streams)
        head = (desc, n, (ctypes.c_int * n)(*streams), S, _dptr(self._table), self._n_tiles, Tmax, _dptr(self.ref), self._ref_elems,
                _dptr(self.age), self.thres16, self.min_cells, self.refresh)
        flag = ctypes.c_void_p(self._out.data_ptr() + 4 * self._out_words * S * Tmax)
        if self.illum == 'gain':
            gain = ctypes.c_void_p(self._out.data_ptr() + 4 * S * Tmax)
            abi.check(abi.load().lp_tile_gate_update_gain(*head, self.gain_lo, self.gain_hi, flag, _dptr(self._out), gain,
                                                          _stream_ptr(self.device)), 'lp_tile_gate_update_gain')
        else:
            abi.check(abi.load().lp_tile_gate_update(*head, flag, _dptr(self._out), _stream_ptr(self.device)), 'lp_tile_gate_update')

    def detect_padded(self, frames, stream_of=None):
        from yolov6.utils import tile_gate as tg
        if not frames:
            raise ValueError('TileGate.detect_padded needs at least one frame')
        frames = list(frames)
        dev, nv12 = _frames_on(frames, 'TileGate')
        if dev != self.device:
            raise ValueError('TileGate: the frames must be on the model\'s device %s' % self.device)
        so = tg.check_streams(stream_of, len(frames), self.n_streams)
        gated = [f for f, s in enumerate(so) if s >= 0]
        for f in gated:
            if tuple(frames[f].shape[:2]) != self.shapes[so[f]]:
                raise ValueError('TileGate: a frame of %s on stream %d, whose frames are %s: a stream has one fixed frame size'
                                 % (tuple(frames[f].shape[:2]), so[f], self.shapes[so[f]]))
        S, Tmax, n = self.n_streams, self.max_tiles, len(gated)
        flags, ncell, gains = [None] * len(frames), [None] * len(frames), [None] * len(frames)
        det_g = count_g = None
        todo = []
        with torch.cuda.device(dev):
            if gated:
                streams = [so[f] for f in gated]
                desc = self._describe([frames[f] for f in gated], streams, nv12)
                self._luma(desc)
                self._update(desc, streams)
                self._out_host.copy_(self._out, non_blocking=True)
                torch.cuda.current_stream(dev).synchronize()          # the one host read of a call: the host builds the tile batches
                host = self._out_host.numpy()
                words = host[:4 * self._out_words * S * Tmax].view(np.int32).reshape(self._out_words, S, Tmax)
                nc_all, fl_all = words[0], host[4 * self._out_words * S * Tmax:].reshape(S, Tmax)
                for k, f in enumerate(gated):
                    nt = len(self.plans[so[f]])
                    flags[f], ncell[f] = fl_all[k, :nt].tolist(), nc_all[k, :nt].tolist()
                    gains[f] = words[1][k, :nt].tolist() if self.illum == 'gain' else [0] * nt
                    if min(ncell[f]) < 0:
                        raise RuntimeError('TileGate: the device tile table of stream %d is damaged' % so[f])
                    todo += [(f, t) for t in range(nt) if flags[f][t]]
                if todo:
                    tiles = [(f,) + tuple(self.plans[so[f]][t]) for f, t in todo]
                    det_t, count_t = detect_tiles_padded(self.model, frames, tiles, self.img_size, self.conf_thres, self.iou_thres,
                                                         self.tile_max_det, self.batch)
                    dst = torch.tensor([so[f] * Tmax + t for f, t in todo], dtype=torch.int64, device=dev)
                    self.cache_det.view(S * Tmax, self.tile_max_det, abi.LP_DET_COLS).index_copy_(0, dst, det_t[:len(todo)])
                    self.cache_count.view(-1).index_copy_(0, dst, count_t[:len(todo)])
                buf = self._call_buffers(streams)
                torch.index_select(self.cache_det.view(S * Tmax, self.tile_max_det, abi.LP_DET_COLS), 0, buf['idx'], out=buf['det_t'])
                torch.index_select(self.cache_count.view(-1), 0, buf['idx'], out=buf['count_t'])
                det_g, count_g, _ = merge_tiles(buf['det_t'], buf['count_t'], buf['tiles'], buf['shapes'], self.iou_thres, self.max_det,
                                                self.metric, self.border, out=buf['merge'])
            self.stats['calls'] += 1
            self.stats['tiles_seen'] += sum(len(self.plans[so[f]]) for f in gated)
            self.stats['tiles_detected'] += len(todo)
            self.stats['forwards'] += -(-len(todo) // self.batch)
            if self.illum == 'gain':
                self.stats['tiles_out_of_range'] += tg.count_out_of_range([gains[f] for f in gated], self.gain_lo, self.gain_hi)
            if n == len(frames):
                self.last_flags, self.last_ncell, self.last_gain = flags, ncell, gains
                return det_g, count_g
            # frames of stream -1: not gated, nothing kept
            loose = [f for f, s in enumerate(so) if s < 0]
            lf = [frames[f] for f in loose]
            det_u, count_u = detect_tiled_padded(self.model, lf, self.img_size, self.conf_thres, self.iou_thres, self.max_det, self.tile_hw,
                                                 self.overlap, self.overview, self.metric, self.border, self.batch, self._arg_tile_max_det)
            for f, fr in zip(loose, lf):
                nt = len(plan_tiled([tuple(fr.shape[:2])], self.img_size, self.max_det, self.tile_hw, self.overlap, self.overview)[0])
                flags[f], ncell[f], gains[f] = [1] * nt, [0] * nt, [0] * nt
                self.stats['tiles_seen'] += nt
                self.stats['tiles_detected'] += nt
                self.stats['forwards'] += -(-nt // self.batch)
            det = torch.zeros(len(frames), self.max_det, abi.LP_DET_COLS, dtype=torch.float32, device=dev)
            count = torch.zeros(len(frames), dtype=torch.int32, device=dev)
            if gated:
                g = torch.tensor(gated, dtype=torch.int64, device=dev)
                det[g], count[g] = det_g, count_g
            u = torch.tensor(loose, dtype=torch.int64, device=dev)
            det[u], count[u] = det_u, count_u
        self.last_flags, self.last_ncell, self.last_gain = flags, ncell, gains
        return det, count

    def detect(self, frames, stream_of=None):
        """``detect_padded`` unpadded: a list of [n_f, 28] tensors (copies), with one more host read, of the counts, as
        ``detect_tiled`` has."""
        det, count = self.detect_padded(frames, stream_of)
        return [d.clone() for d in _unpad(det, count.cpu().tolist())]
