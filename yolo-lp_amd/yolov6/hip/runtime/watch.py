"""The ended plate reads looked up on the device: in a watchlist (lp_watch_match; yolov6/utils/watch.py states the rule) and in
the log of earlier reads (lp_sight_update; yolov6/utils/sight.py states the rule)."""
import torch

from yolov6.hip import abi

from ._base import _aligned_span, _check_ended, _cuda_device, _dptr, _persistent, _stream_ptr


class Watchlist:
    """A watchlist on the device (lp_watch_match; ``yolov6.utils.watch`` states the rule and ``watch_match_np`` there is the
    same computation on the CPU, on every int32): ``entries`` [N,8] ids (0..63, 255 = wildcard; ``watch.parse_watchlist`` reads
    a file), ``confuse`` [3,64,64] sixteenths or None (``watch.confuse_table``).  Validated and uploaded once; a changed list is
    a new object.  ``n``: its length; ``entries_np`` / ``confuse_np``: the checked host copies."""

    def __init__(self, entries, confuse=None, device='cuda'):
        from yolov6.utils import watch
        self.entries_np = watch.check_entries(entries)
        self.confuse_np = None if confuse is None else watch.check_confuse(confuse)
        self.n = len(self.entries_np)
        self.device = _cuda_device(device, 'Watchlist lives on a GPU (watch_match_np is the CPU form)')
        self.entries = torch.from_numpy(self.entries_np).to(self.device)
        self.confuse = None if self.confuse_np is None else torch.from_numpy(self.confuse_np).to(self.device)
        self._out = {}
        self._align = {}
        #: match_align [S,max_ended] int32 of the last ``match`` with ``indel=1``, else None
        self.last_align = None

    def align_buffer(self, S, max_ended):
        """The persistent match_align [S,max_ended] int32 of a ``match(..., indel=1)`` of that shape."""
        key = (int(S), int(max_ended))
        return _persistent(self._align, key, lambda: torch.empty(key[0], key[1], dtype=torch.int32, device=self.device))

    def buffers(self, S, max_ended):
        """The persistent (match_i [S,max_ended,4] int32, workspace) of a ``match`` of that shape."""
        key = (int(S), int(max_ended))
        need = abi.load().lp_watch_workspace_bytes(*key)
        return _persistent(self._out, key, lambda: (torch.empty(key[0], key[1], 4, dtype=torch.int32, device=self.device),
                                                    torch.empty(need + 256, dtype=torch.uint8, device=self.device)))

    def match(self, ended_i, ended_f, ended_count, max_mismatch=1, max_cost=None, indel=0, gap_cost=None):
        """match_i [S,max_ended,4] int32 = (entry, mismatches, cost, n_hits) per line of the ended records of a
        ``PlateTracker.update`` (device tensors), enqueued on the current stream with no host read: the accepted entry of the
        smallest (cost, index), -1 for none, and how many were accepted.  ``max_mismatch`` 0..8; ``max_cost``: a float in fully
        confident mismatches (``watch.cost_units`` makes it the integer of the rule; None: no limit).  Persistent buffers per
        (S, max_ended): a later call of the same shape overwrites what the earlier one returned.  ``indel=1``
        (lp_watch_match_indel): one lost or gained character in heads 2..7 is tolerated at ``gap_cost`` fully confident mismatches
        (``watch.gap_units``; None: 1); the alignment codes, match_align [S,max_ended] int32, are left in ``last_align`` (None
        without it; ``watch.align_text`` names a code)."""
        from yolov6.utils import watch
        return self._match(ended_i, ended_f, ended_count, *watch.check_params(max_mismatch, watch.cost_units(max_cost)),
                           *watch.check_indel(indel, watch.gap_units(gap_cost)))

    def _match(self, ended_i, ended_f, ended_count, mm, mc, indel=0, gap=0):
        """``match`` with the limits, ``indel`` and ``gap_cost`` as the checked integers of the rule."""
        _check_ended(ended_i, ended_f, ended_count, self.device, 'the ended records must be contiguous tensors on the watchlist\'s device')
        S, max_ended = ended_i.shape[:2]
        match_i, ws = self.buffers(S, max_ended)
        self.last_align = None
        if indel:
            self.last_align = self.align_buffer(S, max_ended)
            with torch.cuda.device(self.device):
                abi.check(abi.load().lp_watch_match_indel(_dptr(self.entries), self.n, _dptr(self.confuse), _dptr(ended_i), _dptr(ended_f),
                                                          _dptr(ended_count), S, max_ended, mm, mc, indel, gap, _dptr(match_i),
                                                          _dptr(self.last_align), *_aligned_span(ws), _stream_ptr(self.device)),
                          'lp_watch_match_indel')
            return match_i
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_watch_match(_dptr(self.entries), self.n, _dptr(self.confuse), _dptr(ended_i), _dptr(ended_f),
                                                _dptr(ended_count), S, max_ended, mm, mc, _dptr(match_i), *_aligned_span(ws),
                                                _stream_ptr(self.device)), 'lp_watch_match')
        return match_i


class SightLog:
    """A log of sightings on the device (lp_sight_update; ``yolov6.utils.sight`` states the rule and ``sight_update_np`` there is
    the same computation on the CPU, on every int32): a ring of ``capacity`` reads of ``n_streams`` streams that one call scans
    for the earlier sightings of the reads that end and then appends them to.  ``confuse`` [3,64,64] sixteenths or None
    (``watch.confuse_table``); ``pair`` uint8 [S,S] or None: pair[s_read][s_entry] != 0 lets entries of stream s_entry match reads
    of stream s_read.  The object owns the zeroed state (int32 [1 + capacity, 8]) and persistent output buffers per
    (S, max_ended)."""

    def __init__(self, capacity, n_streams, confuse=None, pair=None, device='cuda'):
        from yolov6.utils import sight, watch
        self.capacity, self.n_streams = sight.check_log(capacity, n_streams)
        self.confuse_np = None if confuse is None else watch.check_confuse(confuse)
        self.pair_np = sight.check_pair(pair, self.n_streams)
        self.device = _cuda_device(device, 'SightLog lives on a GPU (SightLogNp is the CPU form)')
        self.confuse = None if self.confuse_np is None else torch.from_numpy(self.confuse_np).to(self.device)
        self.pair = None if self.pair_np is None else torch.from_numpy(self.pair_np).to(self.device)
        nbytes = abi.load().lp_sight_state_bytes(self.capacity)
        #: int32 [1 + capacity, 8] on the device: the header row and one row per slot
        self.state = torch.zeros(nbytes // 4, dtype=torch.int32, device=self.device).view(1 + self.capacity, 8)
        self._now = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._bound = 0          # no fewer than the appends since the last clear: every call adds its lines
        self._out = {}

    @property
    def total(self):
        """The reads appended since the last ``clear`` (a host read, outside the hot path)."""
        return int(self.state[0, 0].item())

    def clear(self):
        """Empty the log."""
        self.state.zero_()
        self._bound = 0

    def buffers(self, S, max_ended):
        """The persistent (sight_i [S,max_ended,8] int32, workspace) of an ``update`` of that shape."""
        key = (int(S), int(max_ended))
        need = abi.load().lp_sight_workspace_bytes(*key)
        return _persistent(self._out, key, lambda: (torch.empty(key[0], key[1], 8, dtype=torch.int32, device=self.device),
                                                    torch.empty(need + 256, dtype=torch.uint8, device=self.device)))

    def update(self, ended_i, ended_f, ended_count, now, window, min_hits=1, max_mismatch=1, max_cost=None):
        """sight_i [S,max_ended,8] int32 = (slot, mismatches, cost, n_hits, prev_stream, prev_id, prev_stamp, prev_seq) per line of
        the ended records of a ``PlateTracker.update`` (device tensors): the best earlier sighting within ``window`` of ``now`` of
        every read of at least ``min_hits`` hits, (-1, 0, 0, 0, -1, -1, 0, 0) for none; then the reads are appended.  Enqueued on the
        current stream with no host read.  ``now``: an int (copied into a buffer of the log's with one enqueued copy) or a device
        int32 [1] that the call reads in place; ``max_cost``: a float in fully confident mismatches (None: no limit).  Persistent
        buffers per (S, max_ended): a later call of the same shape overwrites what the earlier one returned."""
        from yolov6.utils import sight, watch
        mm, mc = watch.check_params(max_mismatch, watch.cost_units(max_cost))
        if torch.is_tensor(now):
            _, window, min_hits = sight.check_call(0, window, min_hits)
        else:
            now, window, min_hits = sight.check_call(now, window, min_hits)
            self._now.fill_(now)
            now = self._now
        return self._update(ended_i, ended_f, ended_count, now, window, min_hits, mm, mc)

    def _update(self, ended_i, ended_f, ended_count, now, window, min_hits, mm, mc):
        """``update`` with ``now`` on the device and the parameters as the checked integers of the rule."""
        if now.dtype != torch.int32 or now.numel() != 1:
            raise ValueError('now must be an int or a device int32 [1]')
        _check_ended(ended_i, ended_f, ended_count, self.device,
                     'the ended records and now must be contiguous tensors on the log\'s device', also=(now,))
        S, max_ended = ended_i.shape[:2]
        if S != self.n_streams:
            raise ValueError('the ended records must have the log\'s %d streams' % self.n_streams)
        from yolov6.utils.sight import MAX_APPENDS
        if self._bound + S * max_ended > MAX_APPENDS:
            raise RuntimeError('the log takes fewer than 2^31 appends between clears: clear() it')
        self._bound += S * max_ended
        sight_i, ws = self.buffers(S, max_ended)
        with torch.cuda.device(self.device):
            abi.check(abi.load().lp_sight_update(_dptr(self.state), self.capacity, _dptr(self.confuse), _dptr(self.pair), _dptr(ended_i),
                                                 _dptr(ended_f), _dptr(ended_count), S, max_ended, _dptr(now), window, min_hits, mm, mc,
                                                 _dptr(sight_i), *_aligned_span(ws), _stream_ptr(self.device)), 'lp_sight_update')
        return sight_i
