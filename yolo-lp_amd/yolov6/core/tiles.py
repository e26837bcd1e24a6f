"""Host side of tiled detection of large frames: which regions of a frame go through the network.

A frame much larger than the network input loses its small plates when it is shrunk to one input (a 3840x2160 frame at
640x640 is shrunk 6x).  ``plan_tiles`` slices it into overlapping tiles of the network's size instead, plus the whole
frame as an overview tile for plates larger than the overlap; ``yolov6.hip.runtime.detect_tiled`` runs the tiles of many
frames through the engine in batches and merges the per-tile detections per frame on the device
(``lp_merge_tiles``; on the CPU ``yolov6.utils.tiles.merge_tiles_np``).
"""


def hw_pair(v):
    """(h, w) of a size given as one number, [n] or [h, w] (``img_size`` / ``tile_hw``)."""
    if isinstance(v, (list, tuple)):
        return (int(v[0]), int(v[0])) if len(v) == 1 else (int(v[0]), int(v[1]))
    return int(v), int(v)


def _axis(n, t, overlap):
    """Tile origins and length along one axis of ``n`` pixels: [(origin, length)]."""
    ov = int(t * overlap) if isinstance(overlap, float) and overlap < 1 else int(overlap)
    if not 0 <= ov < t:
        raise ValueError('overlap %r of a %d px tile: need 0 <= overlap < tile' % (overlap, t))
    if n <= t:
        return [(0, n)]
    out, o = [], 0
    while o + t < n:
        out.append((o, t))
        o += t - ov
    out.append((n - t, t))          # the last tile is shifted back inside the frame, never padded
    return out


def plan_tiles(shape, tile_hw, overlap=0.2, overview=True):
    """Tiles of a frame of ``shape`` (h, w[, c]) as a list of (y0, x0, th, tw), row-major.

    Per axis of length n with tile length t and overlap ov pixels (a float < 1: that fraction of t, rounded down): n <= t
    gives one tile [0, n); else origins 0, t-ov, 2(t-ov), ... while origin + t < n, then a last origin n - t.  With
    ``overview`` and more than one tile the whole frame (0, 0, h, w) is appended as the last tile."""
    h, w = int(shape[0]), int(shape[1])
    th, tw = hw_pair(tile_hw)
    if h < 1 or w < 1 or th < 1 or tw < 1:
        raise ValueError('frame %dx%d, tile %dx%d: sizes must be >= 1' % (h, w, th, tw))
    tiles = [(y0, x0, lh, lw) for y0, lh in _axis(h, th, overlap) for x0, lw in _axis(w, tw, overlap)]
    if overview and len(tiles) > 1:
        tiles.append((0, 0, h, w))
    return tiles


def plan_frames(shapes, tile_hw, overlap=0.2, overview=True):
    """The tiles of several frames as one flat list of (frame, y0, x0, th, tw) -- frames ascending, a frame's tiles
    contiguous: the table ``runtime.preprocess_tiles`` and ``runtime.merge_tiles`` take."""
    return [(f,) + t for f, s in enumerate(shapes) for t in plan_tiles(s, tile_hw, overlap, overview)]


def tiles_per_frame(tiles, n_frames):
    n = [0] * n_frames
    for t in tiles:
        n[t[0]] += 1
    return n
