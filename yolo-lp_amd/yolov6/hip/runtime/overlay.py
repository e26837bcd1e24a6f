"""Annotation overlay drawn on the device (yolov6/utils/overlay.py is the specification; lp_overlay_draw_batch) and the scene overlay
before it: lines, zones, their counts and the speed tags (yolov6/utils/scene.py is the specification; lp_overlay_scene_batch)."""
import ctypes

import numpy as np
import torch

from yolov6.hip import abi

from ._base import (_aligned, _buffer, _check_det_count, _cuda_device, _desc_run, _dptr, _frames_on, _plane_descs, _runs_by_key,
                    _stream_ptr, _stream_workspace)

_overlay_ws = {}
_overlay_params_memo = {}


class OverlayFont:
    """The glyph atlas of ``draw_plates`` on a device, uploaded once: ``atlas`` uint8 [G, gh, gw] coverage and ``glyph_of`` uint16
    [8, 64] as ``yolov6.utils.overlay.build_atlas`` makes them (or any caller's data with the thirteen fixed glyphs)."""

    def __init__(self, atlas, glyph_of, device='cuda'):
        from yolov6.utils.overlay import check_font
        self.atlas_np, self.glyph_of_np = check_font(atlas, glyph_of)
        self.device = _cuda_device(device, 'OverlayFont lives on a GPU; the CPU path takes the arrays themselves (draw_plates_np)')
        self.atlas = torch.from_numpy(self.atlas_np).to(self.device)
        self.glyph_of = torch.from_numpy(self.glyph_of_np.view(np.int16)).to(self.device)      # the bits of the uint16 table
        self.n_glyphs, self.gh, self.gw = self.atlas_np.shape


def _overlay_params(font, styles, palette, matrix, show_id, label, draw_box):
    """lp_overlay_params of checked styles and palette, the colours in the bytes of a frame of ``matrix`` (None: BGR)."""
    from yolov6.utils.redact import fill_bytes
    key = (font.n_glyphs, font.gh, font.gw, tuple(styles), None if palette is None else palette.tobytes(), matrix, bool(show_id),
           bool(label), bool(draw_box))
    p = _overlay_params_memo.get(key)       # the colour conversion of an NV12 matrix is not free: once per distinct call
    if p is not None:
        return p
    if len(_overlay_params_memo) >= 64:
        _overlay_params_memo.clear()
    p = _overlay_params_memo[key] = abi.OverlayParams()
    p.n_styles = len(styles)
    for d, s in zip(p.styles, styles):
        for name in ('box', 'quad', 'plate', 'text'):
            getattr(d, name)[:] = fill_bytes(getattr(s, name), matrix)
        d.t, d.a_line, d.a_plate, d.a_text, d.pad = s.t, s.a_line, s.a_plate, s.a_text, s.pad
    p.n_palette = 0 if palette is None else len(palette)
    for k in range(p.n_palette):
        p.palette[k][:] = fill_bytes(tuple(int(v) for v in palette[k]), matrix)
    p.n_glyphs, p.gh, p.gw = font.n_glyphs, font.gh, font.gw
    p.show_id, p.label, p.draw_box = int(bool(show_id)), int(bool(label)), int(bool(draw_box))
    return p


def draw_plates(frames, det, count, atlas, glyph_of=None, tid=None, style=None, styles=None, palette=None, show_id=True, label=True,
                draw_box=True, status=None):
    """Draw the detections of B device frames onto them IN PLACE (lp_overlay_draw_batch, two launches per 64 frames on the current
    stream, no host read): box outline, corner-quad outline and a label with the track id and the eight heads' characters.
    ``frames`` is a list of contiguous uint8 CUDA [h,w,3] BGR tensors or of ``Nv12Frame`` with CUDA planes (one kind; NV12 is drawn
    in its own planes, no BGR copy exists); ``det`` [>= B,max_det,28] + ``count`` int32 on the device exactly as
    ``detect_frames_padded``, ``detect_tiled_padded``, ``TileGate.detect_padded``, ``PlateTracker.update`` (det_out) or the
    tracker's ``last_hold`` leave them; ``tid`` int32 [>= B,max_det] as ``PlateTracker.update`` returns it, or None; ``style`` int32
    [>= B,max_det] picks one of ``styles`` (a list of up to 8 ``yolov6.utils.overlay.Style``, colours (B, G, R), converted with
    the frame's matrix for NV12) per row, < 0 skips the row; ``palette`` uint8 [P <= 64, 3] colours the quad and the label plate
    by ``tid % P``.  ``atlas`` is an ``OverlayFont`` (uploaded once, reused), or the two arrays of one.  Writes into the caller's
    tensors and returns status [B,max_det] int32: 1 = corners, 2 = box, 3 = nothing drawable, 0 = no such row or a skipped one.
    ``yolov6.utils.overlay.draw_plates_np`` is the same computation on the CPU, byte for byte.

    THE OVERLAY GOES LAST on a stream: crops and best shots read the frames first, ``redact_plates`` comes next, then ``draw_scene``
    (if used: zone fills lie under the plate outlines), then this call, so outlines sit on top of a mosaic.  Draw on a clone when
    other consumers need the clean frame."""
    from yolov6.utils.overlay import check_palette, check_styles
    if not frames:
        raise ValueError('draw_plates needs at least one frame')
    dev, nv12 = _frames_on(frames, 'draw_plates')
    _check_det_count(det, count, min_batch=len(frames))
    if det.device != dev or det.shape[1] < 1:
        raise ValueError('det must be on the frames\' device with max_det >= 1')
    font = atlas if isinstance(atlas, OverlayFont) else OverlayFont(atlas, glyph_of, dev)
    if font.device != dev:
        raise ValueError('the OverlayFont is on %s, the frames on %s' % (font.device, dev))
    styles, palette = check_styles(styles), check_palette(palette)
    n, max_det = len(frames), det.shape[1]
    for name, a in (('tid', tid), ('style', style)):
        if a is not None and not (a.is_cuda and a.device == dev and a.dtype == torch.int32 and a.dim() == 2 and a.shape[0] >= n
                                  and a.shape[1] == max_det and a.is_contiguous()):
            raise ValueError('%s must be a contiguous CUDA int32 [>= %d, %d] tensor on the frames\' device' % (name, n, max_det))
    status = _buffer(status, (n, max_det), torch.int32, dev, 'status')
    desc = _plane_descs(abi.RedactDesc, frames, nv12)
    # one call per run of frames that share the colours' bytes: a BGR list is one run, an NV12 list one per matrix
    key = [f.matrix if nv12 else None for f in frames]
    lib = abi.load()
    with torch.cuda.device(dev):
        for b0, b1 in _runs_by_key(key):
            params = _overlay_params(font, styles, palette, key[b0], show_id, label, draw_box)
            run = _desc_run(desc, b0)
            need = lib.lp_overlay_workspace_bytes(b1 - b0, max_det)
            ws = _stream_workspace(_overlay_ws, dev, need)
            abi.check(lib.lp_overlay_draw_batch(run, b1 - b0, _dptr(det[b0:b1]), _dptr(count[b0:b1]), max_det,
                                                None if tid is None else _dptr(tid[b0:b1]), None if style is None else _dptr(style[b0:b1]),
                                                ctypes.byref(params), _dptr(font.atlas), _dptr(font.glyph_of), _dptr(status[b0:b1]),
                                                _aligned(ws), need, _stream_ptr(dev)), 'lp_overlay_draw_batch')
    return status


_scene_ws = {}
_scene_style_memo = {}


class SceneFont:
    """The glyph atlas of ``draw_scene`` on a device, uploaded once: a ``yolov6.utils.scene.SceneAtlas`` (``build_scene_atlas``) or
    any uint8 [G, gh, gw] coverage array with the seventeen fixed glyphs (digits, '#', ' ', '?', '+', '-', '.', ':')."""

    def __init__(self, atlas, device='cuda'):
        from yolov6.utils.scene import check_scene_font
        self.source = atlas
        self.atlas_np = check_scene_font(atlas)
        self.device = _cuda_device(device, 'SceneFont lives on a GPU; the CPU path takes the atlas itself (draw_scene_np)')
        self.atlas = torch.from_numpy(self.atlas_np).to(self.device)
        self.n_glyphs, self.gh, self.gw = self.atlas_np.shape


def _scene_style(font, style, matrix):
    """lp_scene_style of a checked style, the colours in the bytes of a frame of ``matrix`` (None: BGR)."""
    from yolov6.utils.redact import fill_bytes
    key = (font.n_glyphs, font.gh, font.gw, style, matrix)
    p = _scene_style_memo.get(key)
    if p is not None:
        return p
    if len(_scene_style_memo) >= 64:
        _scene_style_memo.clear()
    p = _scene_style_memo[key] = abi.SceneStyle()
    for name in ('zone', 'alert', 'line', 'mark', 'plate', 'text', 'tag'):
        getattr(p, name)[:] = fill_bytes(getattr(style, name), matrix)
    for name in ('t', 'marker', 'a_fill', 'a_fill_busy', 'a_line', 'a_plate', 'a_text', 'pad'):
        setattr(p, name, getattr(style, name))
    p.n_glyphs, p.gh, p.gw = font.n_glyphs, font.gh, font.gw
    return p


def _i32_on(t, shape, dev, what):
    """``t`` checked as a contiguous CUDA int32 tensor on ``dev`` whose shape matches ``shape`` (None: any size, a leading '>=' by a
    negative number)."""
    ok = torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == torch.int32 and t.is_contiguous() and t.dim() == len(shape)
    for have, want in zip(t.shape if ok else (), shape):
        ok = ok and (want is None or (have >= -want if want < 0 else have == want))
    if not ok:
        raise ValueError('%s must be a contiguous CUDA int32 tensor on the frames\' device of shape %s' % (
            what, [('>= %d' % -w if w is not None and w < 0 else w) for w in shape]))
    return t


def draw_scene(frames, zone_map, font, names=None, stream_of=None, zone=None, speed=None, det=None, count=None, tid=None, style=None,
               status=None):
    """Draw the scene of B device frames onto them IN PLACE (lp_overlay_scene_batch, two launches per 64 frames on the current
    stream, no host read): the zones of ``zone_map`` (a ``runtime.ZoneMap``) as a translucent fill plus an outline, its directed
    lines with a marker on their +1 side, a label per line with its running +/- totals and per zone with its occupancy -- in the
    alert colour while a dwell alert fires -- and a km/h tag beside every plate whose track has a speed estimate.  ``frames`` as
    ``draw_plates`` takes them (NV12 lists are split into runs per matrix); ``font`` a ``SceneFont``; ``names`` uint16
    [S,24,12] glyph indices (``yolov6.utils.scene.names_of``; a CUDA int16 tensor of those bits, a host array, or None);
    ``stream_of`` host ints, the stream of each frame (None: frame b is stream b; an entry outside [0, S) skips the frame);
    ``zone`` = ``tracker.last_zone`` or None (no labels, no busy or alert look); ``speed`` = ``tracker.last_speed`` or None, with
    ``det``, ``count`` and ``tid`` as ``PlateTracker.update`` returns them (all four or no tags); ``style`` a
    ``yolov6.utils.scene.SceneStyle``.  Returns the tag status int32 [B,max_det] (1: the row got a tag), or None without ``det``.
    ``yolov6.utils.scene.draw_scene_np`` is the same computation on the CPU, byte for byte.

    ORDER on a stream: crops and best shots read the frames first, ``redact_plates`` comes next, then ``draw_scene``, then
    ``draw_plates``: zone fills lie under the plate outlines.

    What it does not do: one style per call; labels do not avoid each other or the plate labels; no anti-aliasing; names are cut
    to 12 glyphs of the atlas; the geometry is in pixels, there is no ground-plane grid; the tag shows the estimate at the end of
    the call; it is not combined with the look-back redaction."""
    from yolov6.utils.scene import N_NAMES, MAX_NAME, check_names, check_scene_style
    if not frames:
        raise ValueError('draw_scene needs at least one frame')
    dev, nv12 = _frames_on(frames, 'draw_scene')
    if not (hasattr(zone_map, 'packed') and torch.is_tensor(zone_map.packed) and zone_map.packed.device == dev):
        raise ValueError('draw_scene needs a runtime.ZoneMap on the frames\' device %s' % dev)
    if not isinstance(font, SceneFont) or font.device != dev:
        raise ValueError('draw_scene needs a SceneFont on the frames\' device %s' % dev)
    style = check_scene_style(style)
    n, S = len(frames), zone_map.n_streams
    so = None
    if stream_of is not None:
        stream_of = [int(s) for s in stream_of]
        if len(stream_of) != n:
            raise ValueError('stream_of must name the stream of each of the %d frames' % n)
        so = (ctypes.c_int32 * n)(*stream_of)
    if names is not None and not torch.is_tensor(names):
        names = torch.from_numpy(check_names(names, S).view(np.int16)).to(dev)
    if names is not None and not (names.is_cuda and names.device == dev and names.dtype == torch.int16 and names.is_contiguous()
                                  and tuple(names.shape) == (S, N_NAMES, MAX_NAME)):
        raise ValueError('names must be a contiguous CUDA int16 [%d, %d, %d] tensor (the bits of the uint16 table)' % (S, N_NAMES, MAX_NAME))
    ev = cnt = occ = totals = None
    max_events = 0
    if zone is not None:
        ev, cnt, occ, totals = zone
        _i32_on(cnt, (S,), dev, 'zone_count'), _i32_on(occ, (S, 8), dev, 'zone_occ'), _i32_on(totals, (S, 2, 16), dev, 'zone_totals')
        max_events = _i32_on(ev, (S, None, 12), dev, 'zone_ev').shape[1]
        if max_events < 1:                        # no room for an event: no alert can be seen
            ev = cnt = None
    tagged = (speed is not None, det is not None, count is not None, tid is not None)
    if any(tagged) and not all(tagged):
        raise ValueError('speed, det, count and tid come together')
    rows = speed_i = None
    max_det = T = 0
    if all(tagged):
        _check_det_count(det, count, min_batch=n)
        max_det = det.shape[1]
        if det.device != dev or max_det < 1:
            raise ValueError('det must be on the frames\' device with max_det >= 1')
        _i32_on(tid, (-n, max_det), dev, 'tid')
        speed_i = _i32_on(speed[0], (S, None, 8), dev, 'speed_i')
        T = speed_i.shape[1]
        status = _buffer(status, (n, max_det), torch.int32, dev, 'status')
        rows = max_det
    else:
        status = None
    desc = _plane_descs(abi.RedactDesc, frames, nv12)
    key = [f.matrix if nv12 else None for f in frames]
    lib = abi.load()
    with torch.cuda.device(dev):
        for b0, b1 in _runs_by_key(key):
            p = _scene_style(font, style, key[b0])
            need = lib.lp_overlay_scene_workspace_bytes(b1 - b0, rows or 0)
            ws = _stream_workspace(_scene_ws, dev, need)
            run_so = None if so is None else ctypes.cast(ctypes.byref(so, 4 * b0), ctypes.POINTER(ctypes.c_int32))
            if so is None and b0:                 # frame b is stream b: say so for a run that does not start at frame 0
                run_so = (ctypes.c_int32 * (b1 - b0))(*range(b0, b1))
            abi.check(lib.lp_overlay_scene_batch(
                _desc_run(desc, b0), b1 - b0, run_so, S, _dptr(zone_map.packed), _dptr(totals), _dptr(occ), _dptr(ev), _dptr(cnt), max_events,
                _dptr(speed_i), T, None if rows is None else _dptr(det[b0:b1]), None if rows is None else _dptr(count[b0:b1]),
                None if rows is None else _dptr(tid[b0:b1]), max_det, ctypes.byref(p), _dptr(font.atlas), _dptr(names),
                None if rows is None else _dptr(status[b0:b1]), _aligned(ws), need, _stream_ptr(dev)), 'lp_overlay_scene_batch')
    return status
