"""Cross-tile merge of tiled detection, on the CPU: ``merge_tiles_np`` is the written-down specification of
``lp_merge_tiles`` (include/lp_hip.h, csrc/lp_tiles.hip), which matches it bit for bit, and the CPU path of
``Inferer(tile=...)``.  Everything is fp32, evaluated op by op in the kernel's order.
"""
import numpy as np

DET_COLS = 28
MAX_TILES_PER_FRAME = 64        # lp_merge_tiles: the tile table travels as kernel arguments
MAX_CANDIDATES = 16384          # ... and a frame's candidate slots (tiles_of_frame * max_det_t) are sorted in LDS
METRICS = {'iou': 0, 'ios': 1}


def _sort_keys(score, slot):
    """The 64-bit keys lp_nms and lp_merge_tiles sort ascending: descending score (as ordered fp32 bits), then slot."""
    score = np.where(score == 0, np.float32(0), score).astype(np.float32)        # -0 ties with +0
    bits = score.view(np.uint32)
    u = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000))
    return ((~u).astype(np.uint64) << np.uint64(32)) | slot.astype(np.uint64)


def row_scores(rows):
    """fp32 [n]: (c12 + ... + c19) / 8 of rows [n, 28], summed left to right."""
    with np.errstate(all='ignore'):
        score = rows[:, 12] + rows[:, 13]
        for c in range(14, 20):
            score = score + rows[:, c]
        return score / np.float32(8.0)


def overlaps(kept, box, thres, metric):
    """bool [K]: which of the earlier boxes ``kept`` [K,4] overlap ``box`` [4] by more than ``thres`` (fp32 xyxy).
    'iou': torchvision's ``inter / (area_i + area_j - inter) > thres``; 'ios': ``inter / min(area_i, area_j) > thres``;
    fp32 op by op, the quotient compared in double."""
    kept = np.asarray(kept, np.float32).reshape(-1, 4)
    box = np.asarray(box, np.float32)
    ix1, iy1, ix2, iy2 = (kept[:, k] for k in range(4))
    jx1, jy1, jx2, jy2 = (np.full(len(kept), box[k], np.float32) for k in range(4))
    with np.errstate(all='ignore'):
        xx1 = np.where(ix1 > jx1, ix1, jx1)
        yy1 = np.where(iy1 > jy1, iy1, jy1)
        xx2 = np.where(ix2 < jx2, ix2, jx2)
        yy2 = np.where(iy2 < jy2, iy2, jy2)
        w = xx2 - xx1
        w = np.where(w > 0, w, np.float32(0))
        h = yy2 - yy1
        h = np.where(h > 0, h, np.float32(0))
        inter = w * h
        iarea = (ix2 - ix1) * (iy2 - iy1)
        jarea = (jx2 - jx1) * (jy2 - jy1)
        if METRICS[metric] == 0:
            den = iarea + jarea - inter
        else:
            den = np.where(iarea < jarea, iarea, jarea)
        ovr = inter / den
        assert ovr.dtype == np.float32
        return ovr.astype(np.float64) > float(thres)


def merge_tiles_np(det_t, count_t, tiles, frame_shapes, thres, max_det, metric='iou', border=1):
    """Per-frame merge of per-tile detections.

    ``det_t`` [T, max_det_t, 28] fp32 and ``count_t`` [T]: the tiles' detections in tile-local source pixels, rounded (after
    the rescale with each tile's (th, tw) as its source image).  ``tiles[t]`` = (frame, y0, x0, th, tw), the tiles of a frame
    contiguous and frames ascending; ``frame_shapes[f]`` = (h, w[, c]).  Returns (det [F,max_det,28] fp32, count [F] int32,
    src [F,max_det] int32 = tile * max_det_t + row of every kept row, -1 past the count); rows past the count are zero.

    Per frame: (1) candidates = rows r < min(max(count_t[t], 0), max_det_t) of its tiles in (tile, row) order; (2) with
    ``border >= 0`` a row whose tile-local box touches (within ``border`` px) a tile side that is not a frame side is
    dropped: a plate cut by the slicing, which the neighbouring tile sees whole; (3) columns 0..11 are shifted by the tile's
    origin; (4) score = (c12 + ... + c19) / 8 summed left to right in fp32, order = descending score, ties in candidate
    order; (5) greedy: a candidate is kept unless an already kept candidate OF ANOTHER TILE overlaps it by more than
    ``thres`` (``overlaps``); (6) the first ``max_det`` kept rows."""
    det_t = np.ascontiguousarray(det_t, dtype=np.float32)
    count_t = np.asarray(count_t).astype(np.int64)
    if det_t.ndim != 3 or det_t.shape[2] != DET_COLS or det_t.shape[1] < 1:
        raise ValueError('det_t must be [T, max_det_t >= 1, 28]')
    if metric not in METRICS:
        raise ValueError('metric must be one of %s' % sorted(METRICS))
    if not 0.0 <= thres <= 1.0:
        raise ValueError('thres must be in [0, 1]')
    F, max_det, border = len(frame_shapes), int(max_det), int(border)
    if max_det < 1:
        raise ValueError('max_det must be >= 1')
    max_det_t = det_t.shape[1]
    if len(tiles) > det_t.shape[0] or len(tiles) > len(count_t):
        raise ValueError('%d tiles for %d detection lists' % (len(tiles), det_t.shape[0]))
    per_frame = [[] for _ in range(F)]
    prev = 0
    for t, (f, y0, x0, th, tw) in enumerate(tiles):
        if not prev <= f < F:
            raise ValueError('frame of tile %d: tiles of a frame must be contiguous, frames ascending' % t)
        h, w = frame_shapes[f][:2]
        if y0 < 0 or x0 < 0 or th < 1 or tw < 1 or y0 + th > h or x0 + tw > w:
            raise ValueError('region of tile %d is not inside its frame' % t)
        per_frame[f].append(t)
        prev = f
    for f, ts in enumerate(per_frame):
        if len(ts) > MAX_TILES_PER_FRAME:
            raise ValueError('frame %d has %d tiles (at most %d)' % (f, len(ts), MAX_TILES_PER_FRAME))
        if len(ts) * max_det_t > MAX_CANDIDATES:
            raise ValueError('frame %d: %d tiles x max_det_t %d = %d candidates (at most %d)'
                             % (f, len(ts), max_det_t, len(ts) * max_det_t, MAX_CANDIDATES))
    det = np.zeros((F, max_det, DET_COLS), np.float32)
    count = np.zeros(F, np.int32)
    src = np.full((F, max_det), -1, np.int32)
    for f, ts in enumerate(per_frame):
        h, w = frame_shapes[f][:2]
        rows, tile_of, src_of, slots = [], [], [], []
        for lt, t in enumerate(ts):
            _, y0, x0, th, tw = tiles[t]
            n = min(max(int(count_t[t]), 0), max_det_t)
            r = det_t[t, :n]
            keep = np.ones(n, bool)
            if border >= 0:
                x1, y1, x2, y2 = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
                b = np.float32(border)
                if x0 > 0:
                    keep &= ~(x1 <= b)
                if y0 > 0:
                    keep &= ~(y1 <= b)
                if x0 + tw < w:
                    keep &= ~(x2 >= np.float32(tw - border))
                if y0 + th < h:
                    keep &= ~(y2 >= np.float32(th - border))
            idx = np.nonzero(keep)[0]
            r = r[idx].copy()
            r[:, 0:12:2] = r[:, 0:12:2] + np.float32(x0)
            r[:, 1:12:2] = r[:, 1:12:2] + np.float32(y0)
            rows.append(r)
            tile_of.append(np.full(len(idx), t, np.int64))
            src_of.append(t * max_det_t + idx)
            slots.append(lt * max_det_t + idx)
        if not rows:
            continue
        rows, tile_of = np.concatenate(rows), np.concatenate(tile_of)
        src_of, slots = np.concatenate(src_of), np.concatenate(slots)
        score = row_scores(rows)
        order = np.argsort(_sort_keys(score, slots), kind='stable')
        kept = []
        for i in order:
            if len(kept) >= max_det:
                break
            other = [k for k in kept if tile_of[k] != tile_of[i]]
            if other and overlaps(rows[other, :4], rows[i, :4], thres, metric).any():
                continue
            kept.append(i)
        n = len(kept)
        det[f, :n], count[f], src[f, :n] = rows[kept], n, src_of[kept]
    return det, count, src
