#!/usr/bin/env python3
"""Frames benchmark: rescaled detections from host frames, end to end, per frame and batched.

    python tools/frames_bench.py [--model yololps] [--size 640] [--dtype f16] [--frame 1080 1920] [--batches 8 32 64]
                                 [--crops N] [--redact [--redact-cell 16] [--redact-sigma 8]]
    python tools/frames_bench.py --tile [--tile-baseline] [--tile-frame 2160 3840] [--tile-size 640] [--tile-overlap 128]
                                 [--tile-frames 4] [--tile-batch 32] [--runs 3]
    python tools/frames_bench.py --tile --gate [--gate-moving K] [--gate-thres F] [--gate-refresh N] [--nv12 [bt709]] [--tile-frame 2160 3840] [--runs 3]
    python tools/frames_bench.py --tile --gate --gate-illum gain --gate-drift A [--gate-drift-period 8] [--gate-moving K] [--nv12 [bt709]] [--runs 3]
    python tools/frames_bench.py --track [--track-batch 32] [--runs 3] [--best-shot [--stack]] [--redact [--hold [--lookback D]]] [--nv12]
                                 [--watch N [--watch-mismatch 1] [--watch-indel] [--watch-live [--watch-live-min-hits 1]]] [--sightings C] [--zones L Z] [--speed]
    python tools/frames_bench.py --nv12 [bt709] [--batches 32] [--crops N] [--runs 3]          (also with --tile)
    python tools/frames_bench.py --jpeg Q [--jpeg-frames 4] [--jpeg-restart 16] [--tile-frame 2160 3840] [--nv12 [bt601f]] [--redact]
    python tools/frames_bench.py --annotate [--annotate-plates N] [--jpeg-frames 4] [--tile-frame 2160 3840] [--nv12 [bt601f]]
    python tools/frames_bench.py --annotate --scene L Z [--scene-cover] [--speed] [--jpeg-frames 4] [--tile-frame 2160 3840] [--nv12 [bt709]]

Input is seeded synthetic host frames (uint8 BGR numpy arrays, 1920x1080 by default).  Prints one JSON line with
  - frames/s of the per-frame path (upload, lp_preprocess_letterbox, detect at B=1 with hipGraph replay, lp_rescale_round,
    host read: what Inferer.infer does per frame) and of FrameBatcher + detect_frames at each batch size;
  - the device time of each stage of one batch from events (H2D from pinned memory, letterbox, detect, rescale) and the
    stage that bounds the batched path;
  - the letterbox kernel's GB/s over the bytes it must move: the source rows it samples plus its output;
  - with ``--crops N``, the device time of the plate-crop stage (runtime.plate_crops, 64x192 crops) on N seeded synthetic
    quads per frame (rotated and perspective plates, and one in four with unusable corners that falls back to its box),
    timed in the same event chain right behind rescale, and its share of the detect stage.
With ``--tile`` the tool measures tiled detection of large frames instead (its other modes are unchanged): seeded frames
of ``--tile-frame`` (3840x2160 by default) already on the device, ``runtime.detect_tiled_with_crops`` on ``--tile-frames`` of
them per call -- frames/s over ``--runs`` timed runs, and the device time of each stage from events: tile letterbox
(lp_preprocess_tiles_batch), detect, rescale, merge (lp_merge_tiles), crops.  ``--tile-baseline`` also times, in the same
run, the same job done with the entry points that existed before tiling: region copies made contiguous on the device,
``detect_frames(auto=False)`` per ``--tile-batch`` tiles, the detections read to the host and merged there by
``merge_tiles_np``.
With ``--track`` the tool measures plate tracking instead: ``--track-batch`` camera streams, one frame each per step --
frames/s of FrameBatcher + ``detect_frames`` alone and of ``detect_frames_padded`` + ``PlateTracker.update`` + the host read
of the voted rows and track ids, ``--runs`` timed runs each in the same process, alternating; the device time of the update
from events (median of ``--reps``) next to the detect stage of the same chain, at the bench's own detection density; and the
update alone on a full frame per stream (128 live tracks x 128 rows, every pair above the threshold: 16384 sorted keys).
``--stack`` (with ``--best-shot``) adds lp_stack_update behind the gallery: its device time from events (median of ``--reps``) with 1, 8
and 32 constant rectified rows per stream, every one searched over 25 candidates and summed in every call.
``--best-shot`` adds the best-shot stages of ``PlateTracker.update_with_shots`` to that event chain, right behind the update:
plate crops (16 slots of 64x192 per frame), lp_crop_sharpness and lp_best_shot_update, each from events, at the bench's own
detection density; and a worst case on 16 constant rows per stream whose sharpness is made to grow with every call, so that
every row of every frame replaces its shot (16 x 36 KB copied per stream by one workgroup).
With ``--nv12 [MATRIX]`` the same seeded frames are sent as BGR and as NV12 (encoded on the host before any clock starts, as a
decoder would deliver them), alternating, ``--runs`` timed runs each: frames/s of FrameBatcher + ``detect_frames``; the stages of
one batch from events for both kinds (H2D, letterbox -- lp_preprocess_tiles_batch on the BGR frames against
lp_preprocess_nv12_batch on the NV12 frames, in the same run --, detect, rescale), the NV12 convert stage (lp_nv12_to_bgr_batch,
with its GB/s over 1.5 B read + 3 B written per pixel) and, with ``--crops N``, the crop stage behind it.  With ``--tile`` the
same for tiled detection: frames/s of ``detect_tiled_with_crops`` for both kinds and the stage times of each.
With ``--redact`` (also with ``--nv12``) the plate-redaction stage (runtime.redact_plates, in place on the device frames) is timed
at the end of the same event chain, on the ``--crops`` quads of each frame (4 when ``--crops`` is not given): ``redact`` = the mosaic
(lp_redact_plates_batch's two kernels, cell means + write), ``redact_fill`` = the fill (the write kernel alone), so their
difference is what the cell means cost, ``redact_gauss`` = the Gaussian blur of ``--redact-sigma`` (lp_redact_gauss_batch: the tile
blur + the same write kernel); and the mosaic's and the blur's share of the detect stage.  With ``--nv12`` the NV12 planes themselves
are redacted.
With ``--track --redact [--hold]`` (also with ``--nv12``: the streams' frames are then NV12) the update and the mosaic behind it
are timed from events on the tracker's own rows, every stream seeing another frame in every step so that tracks are missed;
``--hold`` runs a second tracker with ``enable_hold`` on the same frames, alternating, and redacts along its ``last_hold``:
``update_ms`` / ``update_hold_ms``, ``redact_ms`` / ``redact_hold_ms``, ``redact_gauss_ms`` / ``redact_gauss_hold_ms`` (the blur along
the same rows) and the rows per frame each covered.
``--lookback D`` adds a third tracker with the hold and a ``LookbackRedactor`` of that depth behind it: ``update_lookback_ms`` (the
same update), ``lookback_ms`` (lp_lookback_update) and ``redact_lookback_ms`` (the mosaic on the frames that leave the delay, along
the rows released for them).
The model is the synthetic recipe of bench.py (same weights scale), prepared as Inferer prepares it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIGMA = {'yololps': 0.25, 'yololpn': 0.6}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='yololps', choices=list(SIGMA))
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--dtype', default='f16', choices=['f16', 'f32'])
    ap.add_argument('--frame', nargs=2, type=int, default=[1080, 1920], metavar=('H', 'W'))
    ap.add_argument('--batches', nargs='+', type=int, default=[8, 32, 64])
    ap.add_argument('--frames', type=int, default=256, help='frames per timed run of the batched path')
    ap.add_argument('--single-frames', type=int, default=128, help='frames per timed run of the per-frame path')
    ap.add_argument('--distinct', type=int, default=16, help='distinct seeded frames, cycled')
    ap.add_argument('--reps', type=int, default=5, help='event-timed repetitions of each stage')
    ap.add_argument('--conf', type=float, default=0.4)
    ap.add_argument('--iou', type=float, default=0.45)
    ap.add_argument('--max-det', type=int, default=1000)
    ap.add_argument('--crops', type=int, default=0, help='plate crops per frame to time (0: no crop stage)')
    ap.add_argument('--redact', action='store_true', help='also time the plate-redaction stage (mosaic, and fill) on the quads of --crops (4 without it)')
    ap.add_argument('--redact-cell', type=int, default=16, help='with --redact: side of a mosaic cell')
    ap.add_argument('--redact-sigma', type=float, default=8.0, help='with --redact: sigma of the Gaussian blur (0.5..16)')
    ap.add_argument('--tile', action='store_true', help='measure tiled detection of large frames (detect_tiled) instead')
    ap.add_argument('--tile-baseline', action='store_true', help='with --tile: also time region copies + detect_frames + host merge')
    ap.add_argument('--tile-frame', nargs=2, type=int, default=[2160, 3840], metavar=('H', 'W'))
    ap.add_argument('--tile-size', type=int, default=None, help='tile side (default: --size)')
    ap.add_argument('--tile-overlap', type=int, default=128, help='tile overlap in pixels')
    ap.add_argument('--tile-frames', type=int, default=4, help='frames per detect_tiled call')
    ap.add_argument('--tile-batch', type=int, default=32, help='tiles per forward')
    ap.add_argument('--gate', action='store_true', help='with --tile: measure the tile gate (runtime.TileGate) on fixed-camera frames -- the seeded '
                                                        'frames held still per stream -- against detect_tiled_padded on the same frames')
    ap.add_argument('--gate-moving', type=int, default=0, metavar='K', help='with --gate: patches of 96 x 32 px per frame that move a few pixels per step')
    ap.add_argument('--gate-thres', type=float, default=2.0, metavar='F', help='with --gate: the gate\'s thres (luma levels per pixel)')
    ap.add_argument('--gate-refresh', type=int, default=50, metavar='N', help='with --gate: the gate\'s refresh (calls after which a tile is detected again anyway; 0: never)')
    ap.add_argument('--gate-illum', default='none', choices=['none', 'gain'], help='with --gate: also measure the gate with this illum on frames '
                    'whose brightness drifts (--gate-drift), beside illum none and the plain path')
    ap.add_argument('--gate-drift', type=float, default=0.0, metavar='A', help='with --gate: the frames of step k are multiplied by '
                    '1 + A sin(2 pi k / P) on the device (0 <= A < 1); their base is scaled so that nothing saturates at 1 + A')
    ap.add_argument('--gate-drift-period', type=int, default=8, metavar='P', help='with --gate-drift: steps per period (a multiple of 8 with --gate-moving)')
    ap.add_argument('--track', action='store_true', help='measure plate tracking (PlateTracker.update behind detect_frames) instead')
    ap.add_argument('--track-batch', type=int, default=32, help='with --track: camera streams = frames per step')
    ap.add_argument('--best-shot', action='store_true', help='with --track: also time crops + sharpness + gallery behind the update')
    ap.add_argument('--stack', action='store_true', help='with --track --best-shot: also time lp_stack_update (PlateTracker.enable_stack) behind '
                                                         'the gallery, at 1, 8 and 32 live tracks per stream')
    ap.add_argument('--hold', action='store_true', help='with --track --redact: also time the update with the redaction hold (enable_hold) '
                                                        'and the redaction along its rows')
    ap.add_argument('--lookback', type=int, default=0, metavar='D', help='with --track --redact --hold: also time the look-back delay of '
                                                                         'that depth (LookbackRedactor) behind the update with the hold')
    ap.add_argument('--watch', type=int, default=0, metavar='N', help='with --track: also time the lookup of the ended reads in a seeded '
                                                                      'random watchlist of N entries (lp_watch_match); every stream is '
                                                                      'flushed once per step so that there are reads')
    ap.add_argument('--sightings', type=int, default=0, metavar='C', help='with --track: also time the update of a full, seeded log of '
                                                                          'sightings of C slots on the ended reads (lp_sight_update), '
                                                                          'and lp_watch_match on a list of C entries and the same reads')
    ap.add_argument('--watch-mismatch', type=int, default=1, help='with --watch: positions that may differ')
    ap.add_argument('--watch-indel', action='store_true', help='with --watch: also time the lookup that tolerates one lost or gained character '
                                                               '(lp_watch_match_indel) on the same list, reads and limits')
    ap.add_argument('--watch-live', action='store_true', help='with --watch: also time the lookup of the live tracks (lp_watch_live), on a '
                                                              'step with fresh reads and on one without')
    ap.add_argument('--watch-live-min-hits', type=int, default=1, help='with --watch-live: detections a track needs before it is looked up')
    ap.add_argument('--speed', action='store_true', help='with --track: also time lp_speed_update (PlateTracker.enable_speed) behind the update, '
                    'with one oblique calibrated plane per stream')
    ap.add_argument('--zones', nargs=2, type=int, default=None, metavar=('L', 'Z'), help='with --track: also time lp_zone_update '
                    '(PlateTracker.enable_zones) behind the update, with L seeded lines (0..16) and Z seeded zones of 16 vertices (0..8) per stream')
    ap.add_argument('--nv12', nargs='?', const='bt709', default=None, choices=['bt601', 'bt709', 'bt601f', 'bt709f'], metavar='MATRIX',
                    help='also send the same seeded frames as NV12 with this matrix and compare (default matrix: bt709)')
    ap.add_argument('--jpeg', type=int, default=None, metavar='Q', help='measure the JPEG stage instead (also with --nv12 and --redact): '
                    'runtime.encode_jpeg at quality Q with its reads against D2H + PIL on one thread, on --jpeg-frames frames of --tile-frame '
                    'and on a batch of 64 crops of 64 x 192')
    ap.add_argument('--jpeg-frames', type=int, default=4, help='with --jpeg or --annotate: frames per call')
    ap.add_argument('--annotate', action='store_true', help='measure the overlay stage instead (also with --nv12): runtime.draw_plates on '
                    '--jpeg-frames frames of --tile-frame with 0, 4 and 64 plates per frame, against D2H + PIL drawing on one thread and '
                    'against the JPEG encode of the same frames')
    ap.add_argument('--scene', nargs=2, type=int, default=None, metavar=('L', 'Z'),
                    help='with --annotate: measure the scene overlay instead: runtime.draw_scene of L lines and Z zones of 16 vertices '
                         '(with --speed: and a km/h tag on 16 plates per frame) beside runtime.draw_plates and D2H + PIL polygon / line')
    ap.add_argument('--scene-cover', action='store_true', help='with --scene: zone 0 covers the whole frame')
    ap.add_argument('--annotate-plates', type=int, default=None, metavar='N', help='with --annotate: only N plates per frame')
    ap.add_argument('--jpeg-restart', type=int, default=16, help='with --jpeg: MCUs per restart interval (1..32)')
    ap.add_argument('--runs', type=int, default=3, help='timed runs of the frames/s figures (the spread is reported)')
    return ap.parse_args()


def tile_mode(args, model, dev, tdt):
    """--tile: frames/s of detect_tiled_with_crops (and of the baseline) and the device time of every stage."""
    import torch
    from yolov6.hip import runtime
    from yolov6.utils.tiles import merge_tiles_np
    size, stride = [args.size, args.size], int(model.stride.max())
    h0, w0 = args.tile_frame
    tile = args.tile_size or args.size
    F, B = args.tile_frames, args.tile_batch
    conf, iou, max_det = args.conf, args.iou, args.max_det
    rng = np.random.default_rng(0)
    host_frames = [rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8) for _ in range(F)]
    frames = [torch.from_numpy(f).to(dev) for f in host_frames]
    nv_frames = None
    if args.nv12:
        from yolov6.utils.nv12 import bgr_to_nv12_np
        nv_frames = [bgr_to_nv12_np(f, args.nv12).to(dev) for f in host_frames]
    shapes = [(h0, w0)] * F
    tiles, tmd = runtime.plan_tiled(shapes, size, max_det, (tile, tile), args.tile_overlap, True)
    kw = dict(tile_hw=(tile, tile), overlap=args.tile_overlap, batch=B)
    sync = torch.cuda.synchronize
    out = dict(metric='frames/s of tiled detection (device frames in, merged detections + crops out)', model=args.model,
               dtype=args.dtype, frame=[h0, w0], tile=tile, overlap=args.tile_overlap, tiles_per_frame=len(tiles) // F,
               frames_per_call=F, tiles_per_forward=B, tile_max_det=tmd, runs=args.runs)

    def timed(fn, calls):
        fn()
        sync()
        fps = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            fps.append(round(calls * F / (time.perf_counter() - t0), 2))
        return fps

    def tiled(fr=None):
        return runtime.detect_tiled_with_crops(model, frames if fr is None else fr, size, conf, iou, max_det, **kw)

    def baseline():         # what the entry points before tiling can do for the same job
        dets, counts = [], []
        for c0 in range(0, len(tiles), B):
            copies = [frames[f][y0:y0 + th, x0:x0 + tw].contiguous() for f, y0, x0, th, tw in tiles[c0:c0 + B]]
            det, count = runtime.detect_frames_padded(model, copies, size, conf, iou, tmd, auto=False, batch=B)
            dets.append(det[:len(copies)].cpu().numpy())
            counts.append(count[:len(copies)].cpu().numpy())
        det, count, _ = merge_tiles_np(np.concatenate(dets), np.concatenate(counts), tiles, shapes, iou, max_det)
        d_det, d_count = torch.from_numpy(det).to(dev), torch.from_numpy(count).to(dev)
        ns = [int(c) for c in count]
        return det, runtime.plate_crops(frames, d_det, d_count, max_crops=max(ns + [1]))

    with torch.no_grad():
        runtime.prepare_for(model, (B, 3, *size), tdt)
        dets, _, _ = tiled()
        out['detections_per_frame'] = [len(d) for d in dets]
        calls = max(2, args.frames // (F * 8))
        if nv_frames is None:
            out['tiled_fps_runs'] = timed(tiled, calls)
        else:                              # BGR and NV12 device frames, alternating
            tiled(nv_frames)
            sync()
            both = dict(bgr=[], nv12=[])
            for _ in range(args.runs):
                for kind, fr in (('bgr', frames), ('nv12', nv_frames)):
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        tiled(fr)
                    sync()
                    both[kind].append(round(calls * F / (time.perf_counter() - t0), 2))
            out['tiled_fps_runs'] = both['bgr']
            out['nv12'] = dict(matrix=args.nv12, tiled_fps_runs=both['nv12'], tiled_fps=float(np.median(both['nv12'])))
        out['tiled_fps'] = float(np.median(out['tiled_fps_runs']))
        if args.tile_baseline:
            bdet, _ = baseline()
            out['baseline_equal'] = all(np.array_equal(bdet[f, :len(dets[f])], dets[f].cpu().numpy()) for f in range(F))
            out['baseline_fps_runs'] = timed(baseline, calls)
            out['baseline_fps'] = float(np.median(out['baseline_fps_runs']))
            out['tiled_over_baseline'] = round(out['tiled_fps'] / out['baseline_fps'], 3)

        # device time per stage of one call, from events on one stream
        x = torch.empty(B, 3, *size, dtype=tdt, device=dev)
        names = ('tile_letterbox', 'detect', 'rescale', 'merge', 'crops')
        if nv_frames is not None:          # the NV12 chain first: tile letterbox from the planes, one conversion before the crops
            bgr_out = [torch.empty(h0, w0, 3, dtype=torch.uint8, device=dev) for _ in range(F)]
            nv_names = ('tile_letterbox', 'detect', 'rescale', 'merge', 'convert', 'crops')
            nv_times = {k: [] for k in nv_names}
            for _ in range(args.reps + 1):
                acc = dict.fromkeys(nv_names, 0.0)
                pairs = []

                def mark(name, fn):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    r = fn()
                    b.record()
                    pairs.append((name, a, b))
                    return r

                dl, cl = [], []
                for c0 in range(0, len(tiles), B):
                    mark('tile_letterbox', lambda: runtime.preprocess_tiles(nv_frames, tiles[c0:c0 + B], size, stride, tdt, batch=B, out=x))
                    det, count, _ = mark('detect', lambda: runtime.detect_padded(model, x, conf, iou, tmd))
                    dl.append(det)
                    cl.append(count)
                det_t, count_t = torch.cat(dl), torch.cat(cl)
                mark('rescale', lambda: runtime.rescale_round_batch(det_t, count_t, size, [(t[3], t[4]) for t in tiles]))
                det, count, _ = mark('merge', lambda: runtime.merge_tiles(det_t, count_t, tiles, shapes, iou, max_det))
                conv = mark('convert', lambda: runtime.nv12_to_bgr(nv_frames, out=bgr_out))
                mark('crops', lambda: runtime.plate_crops(conv, det, count, max_crops=16))
                sync()
                for name, a, b in pairs:
                    acc[name] += a.elapsed_time(b)
                for k in nv_names:
                    nv_times[k].append(acc[k])
            out['nv12']['stage_ms_per_call'] = {k: round(float(np.median(v[1:])), 4) for k, v in nv_times.items()}
            out['nv12']['tile_letterbox_runs'] = [round(v, 4) for v in nv_times['tile_letterbox'][1:]]
        times = {k: [] for k in names}
        for _ in range(args.reps + 1):
            acc = dict.fromkeys(names, 0.0)
            pairs = []

            def mark(name, fn):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                r = fn()
                b.record()
                pairs.append((name, a, b))
                return r

            dl, cl = [], []
            for c0 in range(0, len(tiles), B):
                mark('tile_letterbox', lambda: runtime.preprocess_tiles(frames, tiles[c0:c0 + B], size, stride, tdt, batch=B, out=x))
                det, count, _ = mark('detect', lambda: runtime.detect_padded(model, x, conf, iou, tmd))
                dl.append(det)
                cl.append(count)
            det_t, count_t = torch.cat(dl), torch.cat(cl)
            mark('rescale', lambda: runtime.rescale_round_batch(det_t, count_t, size, [(t[3], t[4]) for t in tiles]))
            det, count, _ = mark('merge', lambda: runtime.merge_tiles(det_t, count_t, tiles, shapes, iou, max_det))
            mark('crops', lambda: runtime.plate_crops(frames, det, count, max_crops=16))
            sync()
            for name, a, b in pairs:
                acc[name] += a.elapsed_time(b)
            for k in names:
                times[k].append(acc[k])
        med = {k: float(np.median(v[1:])) for k, v in times.items()}
        out['stage_ms_per_call'] = {k: round(v, 4) for k, v in med.items()}
        out['tile_letterbox_runs'] = [round(v, 4) for v in times['tile_letterbox'][1:]]
        out['stage_pct_of_detect'] = {k: round(100.0 * med[k] / med['detect'], 2) for k in names if k != 'detect'}
        out['merged_counts'] = count.cpu().tolist()
        out['candidates_per_frame'] = [int(count_t[f * (len(tiles) // F):(f + 1) * (len(tiles) // F)].clamp(0, tmd).sum()) for f in range(F)]
    print(json.dumps(out))


def gate_host_steps(args, top=256):
    """host[k][f]: the seeded still frames of the gate modes, pixels below ``top``, with ``--gate-moving`` patches of 96 x 32 px that
    move 3 px down and 5 px right per step (8 steps; one step without patches)."""
    h0, w0 = args.tile_frame
    F, K = args.tile_frames, args.gate_moving
    rng = np.random.default_rng(0)
    still = [rng.integers(0, top, (h0, w0, 3), dtype=np.uint8) for _ in range(F)]
    STEPS, PH, PW = 8, 32, 96
    patches = rng.integers(0, top, (F, max(K, 1), PH, PW, 3), dtype=np.uint8)
    origin = np.stack([rng.integers(0, h0 - PH - 4 * STEPS, (F, max(K, 1))), rng.integers(0, w0 - PW - 6 * STEPS, (F, max(K, 1)))], -1)
    host = []
    for k in range(STEPS if K else 1):
        step = []
        for f in range(F):
            img = still[f].copy()
            for j in range(K):
                y, x = int(origin[f, j, 0]) + 3 * k, int(origin[f, j, 1]) + 5 * k
                img[y:y + PH, x:x + PW] = patches[f, j]
            step.append(img)
        host.append(step)
    return host


def gate_mode(args, model, dev, tdt):
    """--tile --gate: the tile gate on still frames with ``--gate-moving`` moving patches.  Reports under ``gate``: the active tiles
    per frame and the forwards per call of the gated path, frames/s with and without the gate (alternating in the same run, on the
    same frames), the device time by events of each of the gate's two kernels, and the luma kernel's read rate."""
    import torch
    from yolov6.hip import runtime
    size = [args.size, args.size]
    h0, w0 = args.tile_frame
    tile = args.tile_size or args.size
    F, B, K = args.tile_frames, args.tile_batch, args.gate_moving
    conf, iou, max_det = args.conf, args.iou, args.max_det
    host = gate_host_steps(args)
    if args.nv12:
        from yolov6.utils.nv12 import bgr_to_nv12_np
        steps = [[bgr_to_nv12_np(f, args.nv12).to(dev) for f in st] for st in host]
    else:
        steps = [[torch.from_numpy(f).to(dev) for f in st] for st in host]
    kw = dict(tile_hw=(tile, tile), overlap=args.tile_overlap, batch=B)
    sync = torch.cuda.synchronize
    with torch.no_grad():
        runtime.prepare_for(model, (B, 3, *size), tdt)
        gate = runtime.TileGate(model, [(h0, w0)] * F, size, conf, iou, max_det, thres=args.gate_thres, refresh=args.gate_refresh, **kw)
        n_tiles = len(gate.plans[0])

        def gated(k):
            return gate.detect_padded(steps[k % len(steps)])

        def plain(k):
            return runtime.detect_tiled_padded(model, steps[k % len(steps)], size, conf, iou, max_det, **kw)

        calls = max(len(steps), args.frames // (F * 8))
        for k in range(len(steps)):         # warm-up: both paths over every step once
            gated(k)
            plain(k)
        sync()
        fps = dict(gated=[], plain=[])
        before = dict(gate.stats)
        for _ in range(args.runs):
            for name, fn in (('gated', gated), ('plain', plain)):
                t0 = time.perf_counter()
                for k in range(calls):
                    fn(k)
                sync()
                fps[name].append(round(calls * F / (time.perf_counter() - t0), 2))
        n_calls = gate.stats['calls'] - before['calls']
        out = dict(metric='frames/s of tiled detection of fixed-camera frames with and without the tile gate', model=args.model,
                   dtype=args.dtype, frame=[h0, w0], tile=tile, overlap=args.tile_overlap, tiles_per_frame=n_tiles, frames_per_call=F,
                   tiles_per_forward=B, runs=args.runs, nv12=args.nv12)
        g = out['gate'] = dict(moving=K, thres=args.gate_thres, refresh=args.gate_refresh, steps=len(steps), calls_per_run=calls)
        g['active_tiles_per_frame'] = round((gate.stats['tiles_detected'] - before['tiles_detected']) / (n_calls * F), 3)
        g['forwards_per_call'] = round((gate.stats['forwards'] - before['forwards']) / n_calls, 3)
        g['gated_fps_runs'], g['plain_fps_runs'] = fps['gated'], fps['plain']
        g['gated_fps'], g['plain_fps'] = float(np.median(fps['gated'])), float(np.median(fps['plain']))
        g['gated_over_plain'] = round(g['gated_fps'] / g['plain_fps'], 3)
        # the device time of the two kernels, by events
        frames = steps[0]
        desc = gate._describe(frames, list(range(F)), bool(args.nv12))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        luma_ms, update_ms = [], []
        for _ in range(args.reps + 1):
            ev[0].record()
            gate._luma(desc)
            ev[1].record()
            gate._update(desc, list(range(F)))
            ev[2].record()
            sync()
            luma_ms.append(ev[0].elapsed_time(ev[1]))
            update_ms.append(ev[1].elapsed_time(ev[2]))
        read = F * h0 * w0 * (1 if args.nv12 else 3)
        g['luma_ms_runs'], g['update_ms_runs'] = [round(v, 4) for v in luma_ms[1:]], [round(v, 4) for v in update_ms[1:]]
        g['luma_ms'], g['update_ms'] = float(np.median(luma_ms[1:])), float(np.median(update_ms[1:]))
        g['luma_bytes_read'] = read
        g['luma_read_bytes_per_s'] = round(read / (g['luma_ms'] * 1e-3), 1)
    print(json.dumps(out))


def gate_drift_mode(args, model, dev, tdt):
    """--tile --gate --gate-illum gain --gate-drift A [--gate-drift-period P]: the gate under a drift of the brightness.  The still
    frames of the gate mode (their base scaled so that no pixel reaches 255 at 1 + A) are multiplied on the device by
    1 + A sin(2 pi k / P) for step k (an NV12 frame: its luma plane).  Four paths alternate in every run over the same number of
    calls: the gate with illum none on the frames WITHOUT drift (what the gate was built for), the gate with illum none and with
    illum gain on the drifting frames, and ``detect_tiled_padded`` on the drifting frames.  Reports under ``gate``: per path the
    active tiles per frame and frames/s, and the device time by events of lp_tile_gate_update and lp_tile_gate_update_gain on
    the same descriptors (a steady frame: the cell passes, no copy of ref)."""
    import torch
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import Nv12Frame, bgr_to_nv12_np
    A, P = float(args.gate_drift), int(args.gate_drift_period)
    if not 0.0 <= A < 1.0 or P < 1 or (args.gate_moving and P % 8):
        raise SystemExit('--gate-drift needs 0 <= A < 1 and a period >= 1 (a multiple of 8 with --gate-moving)')
    size = [args.size, args.size]
    h0, w0 = args.tile_frame
    tile = args.tile_size or args.size
    F, B, K = args.tile_frames, args.tile_batch, args.gate_moving
    conf, iou, max_det = args.conf, args.iou, args.max_det
    host = gate_host_steps(args, top=int(254.0 / (1.0 + A)) + 1)        # pixel * (1 + A) + 1/2 < 255
    gains = [1.0 + A * float(np.sin(2.0 * np.pi * k / P)) for k in range(P)]

    def device_frames(step, g):
        out = []
        for f in step:
            if args.nv12:
                f = bgr_to_nv12_np(f, args.nv12).to(dev)
                px = f.y
            else:
                px = torch.from_numpy(f).to(dev)
            if g != 1.0:
                px = (px.to(torch.float32) * g + 0.5).to(torch.uint8)     # on the device
            out.append(Nv12Frame(px, f.uv, args.nv12) if args.nv12 else px)
        return out

    still = [device_frames(st, 1.0) for st in host]
    drift = [device_frames(host[k % len(host)], g) for k, g in enumerate(gains)]
    assert max(int((f.y if args.nv12 else f).max()) for st in drift for f in st) < 255
    kw = dict(tile_hw=(tile, tile), overlap=args.tile_overlap, batch=B)
    sync = torch.cuda.synchronize
    with torch.no_grad():
        runtime.prepare_for(model, (B, 3, *size), tdt)
        mk = lambda illum: runtime.TileGate(model, [(h0, w0)] * F, size, conf, iou, max_det, thres=args.gate_thres,   # noqa: E731
                                            refresh=args.gate_refresh, illum=illum, **kw)
        gates = dict(still_none=mk('none'), drift_none=mk('none'), drift_gain=mk('gain'))
        n_tiles = len(gates['drift_gain'].plans[0])
        paths = dict(still_none=lambda k: gates['still_none'].detect_padded(still[k % len(still)]),
                     drift_none=lambda k: gates['drift_none'].detect_padded(drift[k % P]),
                     drift_gain=lambda k: gates['drift_gain'].detect_padded(drift[k % P]),
                     plain=lambda k: runtime.detect_tiled_padded(model, drift[k % P], size, conf, iou, max_det, **kw))
        calls = max(P, args.frames // (F * 8))
        for k in range(P):                  # warm-up: every path over a period once
            for fn in paths.values():
                fn(k)
        sync()
        fps = {name: [] for name in paths}
        before = {name: dict(gt.stats) for name, gt in gates.items()}
        for _ in range(args.runs):
            for name, fn in paths.items():
                t0 = time.perf_counter()
                for k in range(calls):
                    fn(k)
                sync()
                fps[name].append(round(calls * F / (time.perf_counter() - t0), 2))
        out = dict(metric='frames/s of tiled detection of fixed-camera frames under a drift of the brightness, with and without the gain of the tile gate',
                   model=args.model, dtype=args.dtype, frame=[h0, w0], tile=tile, overlap=args.tile_overlap, tiles_per_frame=n_tiles,
                   frames_per_call=F, tiles_per_forward=B, runs=args.runs, nv12=args.nv12)
        g = out['gate'] = dict(moving=K, thres=args.gate_thres, refresh=args.gate_refresh, illum=args.gate_illum, drift=A, drift_period=P,
                               gain_min=round(min(gains), 4), gain_max=round(max(gains), 4), calls_per_run=calls)
        for name, gt in gates.items():
            n_calls = gt.stats['calls'] - before[name]['calls']
            g[name + '_active_tiles_per_frame'] = round((gt.stats['tiles_detected'] - before[name]['tiles_detected']) / (n_calls * F), 3)
            g[name + '_tiles_detected'] = gt.stats['tiles_detected'] - before[name]['tiles_detected']
        g['drift_gain_tiles_out_of_range'] = gates['drift_gain'].stats['tiles_out_of_range'] - before['drift_gain']['tiles_out_of_range']
        for name in paths:
            g[name + '_fps_runs'], g[name + '_fps'] = fps[name], float(np.median(fps[name]))
        g['gain_over_none_under_drift'] = round(g['drift_gain_fps'] / g['drift_none_fps'], 3)
        g['gain_under_drift_over_none_on_still'] = round(g['drift_gain_fps'] / g['still_none_fps'], 3)
        g['gain_over_plain'] = round(g['drift_gain_fps'] / g['plain_fps'], 3)
        # the device time of the kernels, by events, on the same descriptors: every cell of every tile is walked, no tile is flagged
        frames = drift[P // 4]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ms = dict(luma=[], update=[], update_gain=[])
        d_none = gates['drift_none']._describe(frames, list(range(F)), bool(args.nv12))
        d_gain = gates['drift_gain']._describe(frames, list(range(F)), bool(args.nv12))
        for _ in range(args.reps + 2):      # two are dropped: with illum none the first flags every tile and moves ref to these frames
            ev[0].record()
            gates['drift_gain']._luma(d_gain)
            ev[1].record()
            gates['drift_gain']._update(d_gain, list(range(F)))
            ev[2].record()
            gates['drift_none']._luma(d_none)
            ev[3].record()
            gates['drift_none']._update(d_none, list(range(F)))
            ev[4].record()
            sync()
            ms['luma'].append(ev[0].elapsed_time(ev[1]))
            ms['update_gain'].append(ev[1].elapsed_time(ev[2]))
            ms['update'].append(ev[3].elapsed_time(ev[4]))
        for name, v in ms.items():
            g[name + '_ms_runs'], g[name + '_ms'] = [round(x, 4) for x in v[2:]], float(np.median(v[2:]))
        g['update_gain_over_update'] = round(g['update_gain_ms'] / g['update_ms'], 3)
    print(json.dumps(out))


def track_mode(args, model, dev, tdt):
    """--track: frames/s with and without PlateTracker.update behind detect_frames, and the device time of the update."""
    import torch
    from yolov6.hip import runtime
    from yolov6.core.frames import FrameBatcher, letterbox_hw
    size, stride = [args.size, args.size], int(model.stride.max())
    h0, w0 = args.frame
    B, conf, iou, max_det = args.track_batch, args.conf, args.iou, args.max_det
    rng = np.random.default_rng(0)
    pool = [rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8) for _ in range(args.distinct)]
    if args.nv12:
        from yolov6.utils.nv12 import bgr_to_nv12_np
        pool = [bgr_to_nv12_np(f, args.nv12) for f in pool]         # what a decoder delivers: encoded before any clock starts
    if args.hold and not args.redact:
        raise SystemExit('--hold needs --track --redact')
    if args.lookback and not args.hold:
        raise SystemExit('--lookback needs --track --redact --hold')
    H, W = letterbox_hw((h0, w0), size, stride)
    sync = torch.cuda.synchronize
    out = dict(metric='frames/s end to end with and without plate tracking (host frames in, rows out)', model=args.model,
               dtype=args.dtype, frame=[h0, w0], net=[H, W], streams=B, runs=args.runs, conf=conf, matrix=args.nv12)
    with torch.no_grad():
        runtime.prepare_for(model, (B, 3, H, W), tdt)
        batcher = FrameBatcher(dev)
        x = torch.empty(B, 3, H, W, dtype=tdt, device=dev)
        trk = runtime.PlateTracker(B, max_tracks=128, ncls=model, device=dev)
        batch_of = lambda k: batcher.put([pool[(k * B + j) % len(pool)] for j in range(B)])   # noqa: E731

        def plain(k):
            return runtime.detect_frames(model, batch_of(k), size, conf, iou, max_det, batch=B, out=x)

        def tracked(k):
            det, count = runtime.detect_frames_padded(model, batch_of(k), size, conf, iou, max_det, batch=B, out=x)
            det_out, tid = trk.update(det, count)[:2]
            return runtime._unpad(det_out, count.cpu().tolist()), tid.cpu()

        nb = max(2, args.frames // B)
        fps = dict(plain=[], tracked=[])
        for fn in (plain, tracked):
            for k in range(2):
                fn(k)
        sync()
        for _ in range(args.runs):
            for name, fn in (('plain', plain), ('tracked', tracked)):
                t0 = time.perf_counter()
                for k in range(nb):
                    fn(k)
                sync()
                fps[name].append(round(nb * B / (time.perf_counter() - t0), 1))
        out['fps_runs'] = fps
        out['fps'] = {k: float(np.median(v)) for k, v in fps.items()}
        out['tracked_over_plain'] = round(out['fps']['tracked'] / out['fps']['plain'], 4)

        # device time of detect and of the update behind it, from events on one stream
        frames = batch_of(0)
        times = dict(detect=[], track=[])
        for _ in range(args.reps + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            xx, _ = runtime.preprocess_frames(frames, size, stride, tdt, batch=B, out=x)
            ev[0].record()
            det, count, _ = runtime.detect_padded(model, xx, conf, iou, max_det)
            runtime.rescale_round_batch(det, count, (H, W), [f.shape for f in frames])
            ev[1].record()
            trk.update(det, count)
            ev[2].record()
            sync()
            times['detect'].append(ev[0].elapsed_time(ev[1]))
            times['track'].append(ev[1].elapsed_time(ev[2]))
        med = {k: float(np.median(v[1:])) for k, v in times.items()}
        out['stage_ms'] = {k: round(v, 4) for k, v in med.items()}
        out['track_pct_of_detect'] = round(100.0 * med['track'] / med['detect'], 2)
        out['detections_per_frame'] = count.clamp(0, max_det).cpu().tolist()
        out['live_tracks_per_stream'] = (trk.state.view(B, -1)[:, 16:].view(B, 128, -1)[:, :, 3] > 0).sum(1).cpu().tolist()

        if args.best_shot:
            out['best_shot'] = best_shot_stages(args, model, dev, tdt, frames, x, (H, W))
            if args.stack:
                out['stack'] = stack_stages(args, model, dev, frames)
        if args.redact:
            out['redact'] = redact_stages(args, model, dev, tdt, batcher, pool, x, (H, W))
        if args.watch:
            out['watch'] = watch_stages(args, model, dev, tdt, batcher, pool, x, (H, W))
            if args.watch_live:
                out['watch_live'] = watch_live_stages(args, model, dev, tdt, batcher, pool, x, (H, W))
        if args.sightings:
            out['sightings'] = sight_stages(args, model, dev, tdt, batcher, pool, x, (H, W))
        if args.zones:
            out['zones'] = zone_stages(args, model, dev, tdt, batcher, pool, x, (H, W))
        if args.speed:
            out['speed'] = speed_stages(args, model, dev, tdt, batcher, pool, x, (H, W))

        # the full case: 128 live tracks x 128 rows per stream, every pair above the threshold
        full = runtime.PlateTracker(B, max_tracks=128, max_age=0, ncls=model, device=dev)
        rows = np.zeros((B, 128, 28), np.float32)
        for k in range(128):
            rows[:, k, 0:4] = (k % 7, k % 5, 1000 + k, 1000 + k % 11)
        rows[:, :, 12:20] = 0.5
        rows[:, :, 20:28] = rng.integers(0, 24, (B, 128, 8))
        fdet = torch.from_numpy(rows).to(dev)
        fcount = torch.full((B,), 128, dtype=torch.int32, device=dev)
        full.update(fdet, fcount)                 # 128 new tracks per stream
        ms = []
        for _ in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tid = full.update(fdet, fcount)[1]
            b.record()
            sync()
            ms.append(a.elapsed_time(b))
        out['full_128x128_ms'] = round(float(np.median(ms[1:])), 4)
        out['full_128x128_matched'] = int((tid >= 0).sum())
    print(json.dumps(out))


def watch_stages(args, model, dev, tdt, batcher, pool, x, net_hw):
    """--track --watch N: device time of lp_watch_match behind the update, from events on one stream.  The list is seeded and
    random (ids within the model's head widths); every step flushes every stream, so the tracks the step began end in it and
    their reads are looked up (``reads_per_step``).  ``block_ms`` is the same call on exactly one query block of synthetic reads:
    the scan's cost per pass over the list, whatever the detector finds.  ``--watch-indel``: lp_watch_match_indel (indel = 1, the
    default gap cost) right behind each of the two calls, on the same list, reads and limits: ``indel_ms`` / ``indel_block_ms``."""
    import torch
    from yolov6.hip import abi, runtime
    from yolov6.utils.track import ncls_of
    size, stride = [args.size, args.size], int(model.stride.max())
    B, conf, iou, max_det = args.track_batch, args.conf, args.iou, args.max_det
    N, QB = args.watch, abi.LP_WATCH_QUERY_BLOCK
    rng = np.random.default_rng(1)
    ncls = ncls_of(model)
    wl = runtime.Watchlist(np.stack([rng.integers(0, n, N, dtype=np.uint8) for n in ncls], 1), device=dev)
    trk = runtime.PlateTracker(B, max_tracks=128, ncls=model, device=dev)
    # one query block of synthetic reads on one stream
    bi, bf = np.zeros((1, QB, 12), np.int32), np.zeros((1, QB, 12), np.float32)
    bi[0, :, 4:], bf[0, :, :8] = np.stack([rng.integers(0, n, QB) for n in ncls], 1), rng.random((QB, 8))
    block = [torch.from_numpy(a).to(dev) for a in (bi, bf, np.array([QB], np.int32))]
    ms, block_ms, reads, indel_ms, indel_block_ms = [], [], [], [], []
    for k in range(args.reps + 2):
        frames = batcher.put([pool[(j + k) % len(pool)] for j in range(B)])
        xx, _ = runtime.preprocess_frames(frames, size, stride, tdt, batch=B, out=x)
        det, count, _ = runtime.detect_padded(model, xx, conf, iou, max_det)
        runtime.rescale_round_batch(det, count, net_hw, [f.shape for f in frames])
        ended_i, ended_f, ended_count = trk.update(det, count, flush=[1] * B)[2:]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        wl.match(ended_i, ended_f, ended_count, args.watch_mismatch)
        ev[1].record()
        ev[2].record()
        wl.match(*block, args.watch_mismatch)
        ev[3].record()
        if args.watch_indel:
            xe = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            xe[0].record()
            wl.match(ended_i, ended_f, ended_count, args.watch_mismatch, indel=1)
            xe[1].record()
            xe[2].record()
            wl.match(*block, args.watch_mismatch, indel=1)
            xe[3].record()
        torch.cuda.synchronize()
        if k >= 2:
            ms.append(ev[0].elapsed_time(ev[1]))
            block_ms.append(ev[2].elapsed_time(ev[3]))
            reads.append(int(ended_count.clamp(0, ended_i.shape[1]).sum()))
            if args.watch_indel:
                indel_ms.append(xe[0].elapsed_time(xe[1]))
                indel_block_ms.append(xe[2].elapsed_time(xe[3]))
    med, bmed, nreads = float(np.median(ms)), float(np.median(block_ms)), float(np.mean(reads))
    extra = {}
    if args.watch_indel:
        imed, ibmed = float(np.median(indel_ms)), float(np.median(indel_block_ms))
        extra = dict(indel_ms=round(imed, 4), indel_over_watch=round(imed / med, 3), indel_block_reads=QB, indel_block_ms=round(ibmed, 4),
                     indel_block_over_block=round(ibmed / bmed, 3), indel_block_pairs_per_s=round(N * QB / (ibmed * 1e-3), 1),
                     watch_runs_ms=[round(v, 4) for v in ms], block_runs_ms=[round(v, 4) for v in block_ms],
                     indel_runs_ms=[round(v, 4) for v in indel_ms], indel_block_runs_ms=[round(v, 4) for v in indel_block_ms])
    return dict(extra, entries=N, max_mismatch=args.watch_mismatch, reps=args.reps, watch_ms=round(med, 4), reads_per_step=round(nreads, 1),
                pairs_per_s=round(N * nreads / (med * 1e-3), 1), block_reads=QB, block_ms=round(bmed, 4),
                block_pairs_per_s=round(N * QB / (bmed * 1e-3), 1), block_list_bytes_per_s=round(N * 8 / (bmed * 1e-3), 1))


def sight_stages(args, model, dev, tdt, batcher, pool, x, net_hw):
    """--track --sightings C: device time of lp_sight_update behind the update, from events on one stream, on a log of C slots that
    is full of seeded random reads (ids within the model's head widths, every slot inside the window: the scan's worst case), and of
    lp_watch_match on a seeded list of C entries with the same reads and limits, as the reference point.  Every step flushes every
    stream, so the tracks the step began end in it (``reads_per_step``).  ``block_ms`` / ``watch_block_ms``: the two calls on exactly
    one query block of synthetic reads."""
    import torch
    from yolov6.hip import abi, runtime
    from yolov6.utils.track import ncls_of
    size, stride = [args.size, args.size], int(model.stride.max())
    B, conf, iou, max_det = args.track_batch, args.conf, args.iou, args.max_det
    N, QB, mm = args.sightings, abi.LP_SIGHT_QUERY_BLOCK, args.watch_mismatch
    rng = np.random.default_rng(1)
    ncls = ncls_of(model)
    ids = np.stack([rng.integers(0, n, N, dtype=np.uint8) for n in ncls], 1)
    wl = runtime.Watchlist(ids, device=dev)
    rows = np.zeros((1 + N, 8), np.int32)
    rows[0, 0] = N
    rows[1:, 0:2] = ids.view(np.int32)
    rows[1:, 2:4] = rng.integers(0, 256, (N, 8), dtype=np.uint8).view(np.int32)
    rows[1:, 4], rows[1:, 5], rows[1:, 7] = rng.integers(0, B, N), np.arange(N) % 1000, np.arange(N)
    logs = [runtime.SightLog(N, n_streams, device=dev) for n_streams in (B, 1)]
    for log in logs:
        log.state.copy_(torch.from_numpy(rows))
    trk = runtime.PlateTracker(B, max_tracks=128, ncls=model, device=dev)
    bi, bf = np.zeros((1, QB, 12), np.int32), np.zeros((1, QB, 12), np.float32)
    bi[0, :, 3], bi[0, :, 4:], bf[0, :, :8] = 1, np.stack([rng.integers(0, n, QB) for n in ncls], 1), rng.random((QB, 8))
    block = [torch.from_numpy(a).to(dev) for a in (bi, bf, np.array([QB], np.int32))]
    now = torch.ones(1, dtype=torch.int32, device=dev)
    times, reads = dict(sight=[], watch=[], sight_block=[], watch_block=[]), []
    for k in range(args.reps + 2):
        frames = batcher.put([pool[(j + k) % len(pool)] for j in range(B)])
        xx, _ = runtime.preprocess_frames(frames, size, stride, tdt, batch=B, out=x)
        det, count, _ = runtime.detect_padded(model, xx, conf, iou, max_det)
        runtime.rescale_round_batch(det, count, net_hw, [f.shape for f in frames])
        ended = trk.update(det, count, flush=[1] * B)[2:]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        ev[0].record()
        logs[0].update(*ended, now, window=1 << 30, max_mismatch=mm)
        ev[1].record()
        ev[2].record()
        wl.match(*ended, mm)
        ev[3].record()
        ev[4].record()
        logs[1].update(*block, now, window=1 << 30, max_mismatch=mm)
        ev[5].record()
        ev[6].record()
        wl.match(*block, mm)
        ev[7].record()
        torch.cuda.synchronize()
        if k >= 2:
            for j, name in enumerate(('sight', 'watch', 'sight_block', 'watch_block')):
                times[name].append(ev[2 * j].elapsed_time(ev[2 * j + 1]))
            reads.append(int(ended[2].clamp(0, ended[0].shape[1]).sum()))
    med = {k: float(np.median(v)) for k, v in times.items()}
    nreads = float(np.mean(reads))
    return dict(capacity=N, max_mismatch=mm, reps=args.reps, sight_ms=round(med['sight'], 4), reads_per_step=round(nreads, 1),
                watch_ms=round(med['watch'], 4), sight_over_watch=round(med['sight'] / med['watch'], 3),
                pairs_per_s=round(N * nreads / (med['sight'] * 1e-3), 1), block_reads=QB, block_ms=round(med['sight_block'], 4),
                watch_block_ms=round(med['watch_block'], 4), block_over_watch_block=round(med['sight_block'] / med['watch_block'], 3),
                block_log_bytes_per_s=round(N * 32 / (med['sight_block'] * 1e-3), 1))


def watch_live_stages(args, model, dev, tdt, batcher, pool, x, net_hw):
    """--track --watch N --watch-live: device time of lp_watch_live behind the update, from events on one stream, on the seeded list
    of ``watch_stages``.  Every step detects another batch of frames and updates the tracker with the lookup held back, then
    enqueues the lookup three times: the first call sees the step's fresh reads (``fresh_reads_per_step`` of the
    ``candidate_slots_per_step`` slots with enough hits; ``fresh_reads_runs`` lists them, since the seeded frames repeat and most
    steps bring few); the second sees the same state again and so has no fresh read: the steady state a deployment pays in every
    frame in which no track is new and no vote flips; the third follows a zeroed memo, so every candidate is fresh (``cold_ms``,
    ``cold_reads``): the worst case.  ``track_ms`` is lp_track_update of the same step, for the ratio."""
    import torch
    from yolov6.hip import runtime
    from yolov6.utils.track import ncls_of
    size, stride = [args.size, args.size], int(model.stride.max())
    B, conf, iou, max_det = args.track_batch, args.conf, args.iou, args.max_det
    N, min_hits = args.watch, args.watch_live_min_hits
    rng = np.random.default_rng(1)
    wl = runtime.Watchlist(np.stack([rng.integers(0, n, N, dtype=np.uint8) for n in ncls_of(model)], 1), device=dev)
    trk = runtime.PlateTracker(B, max_tracks=128, ncls=model, device=dev)
    trk.enable_live_watch(wl, min_hits, args.watch_mismatch)
    times = dict(track=[], fresh=[], steady=[], cold=[])
    fresh, steady_fresh, cand, cold = [], [], [], []
    for k in range(args.reps + 2):
        frames = batcher.put([pool[(j + k) % len(pool)] for j in range(B)])
        xx, _ = runtime.preprocess_frames(frames, size, stride, tdt, batch=B, out=x)
        det, count, _ = runtime.detect_padded(model, xx, conf, iou, max_det)
        runtime.rescale_round_batch(det, count, net_hw, [f.shape for f in frames])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        held, trk._live = trk._live, None          # the update alone; the lookup it would enqueue at its end follows by hand
        ev[0].record()
        trk.update(det, count)
        ev[1].record()
        trk._live = held
        trk._live_watch()
        ev[2].record()
        n_fresh = trk.last_live_reads[3].sum()
        n_fresh = int(n_fresh)                     # (a host read: between the two timed calls, not inside one)
        mid = torch.cuda.Event(enable_timing=True)
        mid.record()
        trk._live_watch()
        ev[3].record()
        n_steady = int(trk.last_live_reads[3].sum())
        trk.live_memo.zero_()
        ev += [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[4].record()
        trk._live_watch()
        ev[5].record()
        torch.cuda.synchronize()
        if k >= 2:
            times['track'].append(ev[0].elapsed_time(ev[1]))
            times['fresh'].append(ev[1].elapsed_time(ev[2]))
            times['steady'].append(mid.elapsed_time(ev[3]))
            fresh.append(n_fresh)
            times['cold'].append(ev[4].elapsed_time(ev[5]))
            steady_fresh.append(n_steady)
            cold.append(int(trk.last_live_reads[3].sum()))
            cand.append(int((trk.state.view(B, -1)[:, 16:].view(B, 128, -1)[:, :, 3] >= min_hits).sum()))
    med = {k: float(np.median(v)) for k, v in times.items()}
    return dict(entries=N, max_mismatch=args.watch_mismatch, min_hits=min_hits, reps=args.reps, watch_live_ms=round(med['fresh'], 4),
                fresh_reads_per_step=round(float(np.mean(fresh)), 1), fresh_reads_runs=fresh, watch_live_runs_ms=[round(v, 4) for v in times['fresh']],
                cold_ms=round(med['cold'], 4), cold_reads=round(float(np.mean(cold)), 1), candidate_slots_per_step=round(float(np.mean(cand)), 1),
                steady_ms=round(med['steady'], 4), steady_fresh_reads=int(max(steady_fresh)), track_ms=round(med['track'], 4),
                steady_over_track=round(med['steady'] / med['track'], 4))


def zone_stages(args, model, dev, tdt, batcher, pool, x, net_hw):
    """--track --zones L Z: device time of lp_zone_update behind the update, from events on one stream, with L seeded lines and Z
    seeded 16-vertex zones (min_dwell 1) per stream, spread over the frame.  Every step detects another batch of frames and updates
    the tracker with the zone stage held back (``track_ms``: lp_track_update_hold of the same call), then enqueues the stage twice:
    the first call sees the step's moves (``zones_ms``, ``events_per_step``, ``eligible_slots_per_step``), the second the same state
    again, where nothing moves: the cost of a frame without events (``steady_ms``)."""
    import torch
    from yolov6.hip import runtime
    size, stride = [args.size, args.size], int(model.stride.max())
    B, conf, iou, max_det = args.track_batch, args.conf, args.iou, args.max_det
    (L, Z), (h0, w0) = args.zones, args.frame
    rng = np.random.default_rng(2)
    lines = [[tuple(rng.uniform(0, (w0, h0, w0, h0))) for _ in range(L)] for _ in range(B)]

    def star():
        ang = np.linspace(0, 2 * np.pi, 16, endpoint=False)
        rad = np.where(np.arange(16) % 2 == 0, 0.45, 0.2) * min(h0, w0) * rng.uniform(0.5, 1.0)
        return np.stack([rng.uniform(0.3, 0.7) * w0 + rad * np.cos(ang), rng.uniform(0.3, 0.7) * h0 + rad * np.sin(ang)], 1), 1
    zones = [[star() for _ in range(Z)] for _ in range(B)]
    trk = runtime.PlateTracker(B, max_tracks=128, ncls=model, device=dev)
    trk.enable_zones(runtime.ZoneMap(B, lines, zones, device=dev))
    times, events, eligible = dict(track=[], zones=[], steady=[]), [], []
    for k in range(args.reps + 2):
        frames = batcher.put([pool[(j + k) % len(pool)] for j in range(B)])
        xx, _ = runtime.preprocess_frames(frames, size, stride, tdt, batch=B, out=x)
        det, count, _ = runtime.detect_padded(model, xx, conf, iou, max_det)
        runtime.rescale_round_batch(det, count, net_hw, [f.shape for f in frames])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        held, trk._zones = trk._zones, None        # the update alone; the stage it would enqueue at its end follows by hand
        ev[0].record()
        trk.update(det, count)
        ev[1].record()
        trk._zones = held
        trk._zone_update()
        ev[2].record()
        n_events = int(trk.last_zone[1].sum())     # (a host read: between the two timed calls, not inside one)
        ev[3].record()
        trk._zone_update()
        ev[4].record()
        torch.cuda.synchronize()
        if k >= 2:
            times['track'].append(ev[0].elapsed_time(ev[1]))
            times['zones'].append(ev[1].elapsed_time(ev[2]))
            times['steady'].append(ev[3].elapsed_time(ev[4]))
            events.append(n_events)
            eligible.append(int((trk.state.view(B, -1)[:, 16:].view(B, 128, -1)[:, :, 3] > 0).sum()))
    med = {k: float(np.median(v)) for k, v in times.items()}
    return dict(lines=L, zones=Z, verts=16, streams=B, reps=args.reps, zones_ms=round(med['zones'], 4), steady_ms=round(med['steady'], 4),
                track_ms=round(med['track'], 4), zones_over_track=round(med['zones'] / med['track'], 4),
                zones_runs_ms=[round(v, 4) for v in times['zones']], track_runs_ms=[round(v, 4) for v in times['track']],
                events_per_step=round(float(np.mean(events)), 1), eligible_slots_per_step=round(float(np.mean(eligible)), 1))


def speed_stages(args, model, dev, tdt, batcher, pool, x, net_hw):
    """--track --speed: device time of lp_speed_update behind the update, from events on one stream, with one oblique plane per stream
    (a limit that about half of the estimates pass, min_span of two frames).  Every step detects another batch of frames and updates
    the tracker with the speed stage held back (``track_ms``: lp_track_update_hold of the same call), then enqueues the stage twice:
    the first call sees the step's detections (``speed_ms``, ``fresh_slots_per_step``, ``events_per_step``), the second the same state
    again, where no slot has a new detection: the cost of a frame without samples (``steady_ms``)."""
    import torch
    from yolov6.hip import runtime
    size, stride = [args.size, args.size], int(model.stride.max())
    B, conf, iou, max_det = args.track_batch, args.conf, args.iou, args.max_det
    h0, w0 = args.frame
    plane = dict(H=(20.0 / w0, 0.0, -10.0, 0.0, -30.0 / h0, 40.0, 0.0, -0.7 / h0, 1.0), period_us=40000, limit_mm_s=3000, min_gap_us=0,
                 min_span_us=80000)
    trk = runtime.PlateTracker(B, max_tracks=128, ncls=model, device=dev)
    trk.enable_speed(runtime.GroundPlane(B, [plane] * B, device=dev))
    times, events, fresh, eligible = dict(track=[], speed=[], steady=[]), [], [], []
    for k in range(args.reps + 2):
        frames = batcher.put([pool[(j + k) % len(pool)] for j in range(B)])
        xx, _ = runtime.preprocess_frames(frames, size, stride, tdt, batch=B, out=x)
        det, count, _ = runtime.detect_padded(model, xx, conf, iou, max_det)
        runtime.rescale_round_batch(det, count, net_hw, [f.shape for f in frames])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        held, trk._speed = trk._speed, None        # the update alone; the stage it would enqueue at its end follows by hand
        ev[0].record()
        trk.update(det, count)
        ev[1].record()
        trk._speed = held
        trk._speed_update()
        ev[2].record()
        n_events = int(trk.last_speed[2].sum())    # (host reads: between the two timed calls, not inside one)
        n_fresh = int((trk.last_speed[0][:, :, 7] >> 8 & 1).sum())
        ev[3].record()
        trk._speed_update()
        ev[4].record()
        torch.cuda.synchronize()
        if k >= 2:
            times['track'].append(ev[0].elapsed_time(ev[1]))
            times['speed'].append(ev[1].elapsed_time(ev[2]))
            times['steady'].append(ev[3].elapsed_time(ev[4]))
            events.append(n_events)
            fresh.append(n_fresh)
            eligible.append(int((trk.last_speed[0][:, :, 0] >= 0).sum()))
    med = {k: float(np.median(v)) for k, v in times.items()}
    return dict(streams=B, reps=args.reps, speed_ms=round(med['speed'], 4), steady_ms=round(med['steady'], 4), track_ms=round(med['track'], 4),
                speed_over_track=round(med['speed'] / med['track'], 4), speed_runs_ms=[round(v, 4) for v in times['speed']],
                track_runs_ms=[round(v, 4) for v in times['track']], events_per_step=round(float(np.mean(events)), 1),
                fresh_slots_per_step=round(float(np.mean(fresh)), 1), eligible_slots_per_step=round(float(np.mean(eligible)), 1))


def redact_stages(args, model, dev, tdt, batcher, pool, x, net_hw):
    """--track --redact [--hold]: device time of the update and of the mosaic behind it, from events on one stream; with --hold a
    second tracker with ``enable_hold`` takes the same frames, alternating, and the mosaic runs along its ``last_hold``.  Every
    stream sees another frame of the pool in every step, so tracks are missed (and end) all the time."""
    import torch
    from yolov6.hip import runtime
    size, stride = [args.size, args.size], int(model.stride.max())
    B, conf, iou, max_det = args.track_batch, args.conf, args.iou, args.max_det
    trackers = dict(plain=runtime.PlateTracker(B, max_tracks=128, ncls=model, device=dev))
    if args.hold:
        trackers['hold'] = runtime.PlateTracker(B, max_tracks=128, ncls=model, device=dev)
        trackers['hold'].enable_hold()
    lb, mid = None, [None]
    if args.lookback:
        from yolov6.utils.nv12 import Nv12Frame
        trackers['lookback'] = runtime.PlateTracker(B, max_tracks=128, ncls=model, device=dev)
        trackers['lookback'].enable_hold()
        lb = runtime.LookbackRedactor(trackers['lookback'], args.lookback, mode='mosaic', cell=args.redact_cell)

        def mark():      # the event between lp_lookback_update and the mosaic of one push
            mid[0] = torch.cuda.Event(enable_timing=True)
            mid[0].record()
    times = {name: dict(update=[], redact=[], redact_gauss=[], lookback=[]) for name in trackers}
    rows = {name: [] for name in trackers}
    warm = max(3, args.lookback + 1)
    for k in range(warm + args.reps + 1):
        for name, trk in trackers.items():
            frames = batcher.put([pool[(j + k) % len(pool)] for j in range(B)])      # (the put restores what the last mosaic wrote)
            xx, _ = runtime.preprocess_frames(frames, size, stride, tdt, batch=B, out=x)
            det, count, _ = runtime.detect_padded(model, xx, conf, iou, max_det)
            runtime.rescale_round_batch(det, count, net_hw, [f.shape for f in frames])
            if name == 'lookback':      # the delay keeps references and the uploader reuses its buffer: copies, before the clock
                frames = [Nv12Frame(f.y.clone(), f.uv.clone(), f.matrix) if isinstance(f, Nv12Frame) else f.clone() for f in frames]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            det_out = trk.update(det, count)[0]
            ev[1].record()
            if name == 'lookback':
                lb.push(frames, between=mark)
                rdet, rcount = lb.buffers(B, lb.entry_rows)[:2]
            else:
                rdet, rcount = (det_out, count) if name == 'plain' else trk.last_hold[:2]
                runtime.redact_plates(frames, rdet, rcount, 'mosaic', args.redact_cell)
            ev[2].record()
            if name != 'lookback':      # the blur along the same rows, behind the mosaic (its time does not depend on the bytes)
                runtime.redact_plates(frames, rdet, rcount, 'gauss', sigma=args.redact_sigma)
                ev[3].record()
            torch.cuda.synchronize()
            if k > warm:
                times[name]['update'].append(ev[0].elapsed_time(ev[1]))
                if name == 'lookback':
                    times[name]['lookback'].append(ev[1].elapsed_time(mid[0]))
                    times[name]['redact'].append(mid[0].elapsed_time(ev[2]))
                else:
                    times[name]['redact'].append(ev[1].elapsed_time(ev[2]))
                    times[name]['redact_gauss'].append(ev[2].elapsed_time(ev[3]))
                rows[name].append(float(rcount.clamp(0, rdet.shape[1]).float().mean()))
    r = dict(redact_cell=args.redact_cell, redact_sigma=args.redact_sigma, reps=args.reps)
    for name in trackers:
        sfx = '' if name == 'plain' else '_' + name
        if name == 'lookback':
            r['lookback_depth'] = args.lookback
            r['lookback_ms'] = round(float(np.median(times[name]['lookback'])), 4)
            r['lookback_state_mib'] = round(lb.state.numel() * 4 / 2 ** 20, 2)
        r['update%s_ms' % sfx] = round(float(np.median(times[name]['update'])), 4)
        r['redact%s_ms' % sfx] = round(float(np.median(times[name]['redact'])), 4)
        if name != 'lookback':
            r['redact_gauss%s_ms' % sfx] = round(float(np.median(times[name]['redact_gauss'])), 4)
        r['redact%s_rows_per_frame' % sfx] = round(float(np.mean(rows[name])), 2)
    return r


def best_shot_stages(args, model, dev, tdt, frames, x, net_hw):
    """--track --best-shot: device time of tracker, crops, sharpness and gallery behind detect, from events on one stream."""
    import torch
    from yolov6.hip import runtime
    size, stride = [args.size, args.size], int(model.stride.max())
    B, conf, iou, max_det = args.track_batch, args.conf, args.iou, args.max_det
    h0, w0 = args.frame
    so = list(range(B))
    names = ('detect', 'track', 'crops', 'sharpness', 'gallery')

    def chain(trk, det_count=None, grow=None):
        """One pass; ``det_count``: fixed rows instead of the detector's; ``grow``: overwrite the sharpness by this value."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        xx, _ = runtime.preprocess_frames(frames, size, stride, tdt, batch=B, out=x)
        ev[0].record()
        det, count, _ = runtime.detect_padded(model, xx, conf, iou, max_det)
        runtime.rescale_round_batch(det, count, net_hw, [f.shape for f in frames])
        ev[1].record()
        if det_count is not None:
            det, count = det_count
        trk.update(det, count)
        ev[2].record()
        crops, status, sharp = trk._shot_crops(frames, det, count, so, trk.max_tracks)
        ev[3].record()
        runtime.crop_sharpness(crops, status, out=sharp)
        if grow is not None:
            sharp.fill_(grow)
        ev[4].record()
        shot_i = trk._shot_gallery(det, count, so, trk.max_tracks)[1]
        ev[5].record()
        torch.cuda.synchronize()
        return [ev[k].elapsed_time(ev[k + 1]) for k in range(5)], count

    def summary(runs):
        a = np.array(runs[1:])
        return {n: dict(median=round(float(np.median(a[:, k])), 4), min=round(float(a[:, k].min()), 4), max=round(float(a[:, k].max()), 4))
                for k, n in enumerate(names)}

    res = {}
    trk = runtime.PlateTracker(B, max_tracks=128, ncls=model, device=dev)
    trk.enable_best_shot((64, 192), max_crops=16)
    runs = []
    for _ in range(args.reps + 1):
        ms, count = chain(trk)
        runs.append(ms)
    res['stage_ms'] = summary(runs)
    res['rows_cropped_per_frame'] = count.clamp(0, 16).cpu().tolist()
    med = {n: v['median'] for n, v in res['stage_ms'].items()}
    res['shot_stages_pct_of_detect'] = round(100.0 * (med['crops'] + med['sharpness'] + med['gallery']) / med['detect'], 2)
    # worst case: 16 constant rows per stream (tracks 0..15 matched in every call), every one replaces its shot in every call
    worst = runtime.PlateTracker(B, max_tracks=128, ncls=model, device=dev)
    worst.enable_best_shot((64, 192), max_crops=16)
    rows = synthetic_quads(B, 16, h0, w0, seed=1)
    rows[:, :, 12:20] = 0.5
    wdet = torch.from_numpy(rows).to(dev)
    wcount = torch.full((B,), 16, dtype=torch.int32, device=dev)
    runs = []
    for k in range(args.reps + 1):
        ms, _ = chain(worst, (wdet, wcount), grow=k + 1)
        runs.append(ms)
    res['worst_stage_ms'] = summary(runs)
    res['worst_bytes_copied_per_stream'] = 16 * 64 * 192 * 3
    state = worst._shots['state'].view(B, -1)[:, 16:].view(B, 128, -1)[:, :16, :32].contiguous().view(torch.int32)
    res['worst_shots_replaced_last_call'] = int((state[:, :, 4] == args.reps).sum())      # frame index of the shot = the last call
    return res


def stack_stages(args, model, dev, frames, live=(1, 8, 32)):
    """--track --best-shot --stack: device time of lp_stack_update behind the gallery, from events on one stream, with L constant
    rectified rows per stream (L live tracks, each searched over 25 candidates and summed in every call after the first)."""
    import torch
    from yolov6.hip import runtime
    B, (h0, w0) = args.track_batch, args.frame
    so = list(range(B))
    res = {}
    for L in live:
        trk = runtime.PlateTracker(B, max_tracks=128, ncls=model, device=dev)
        trk.enable_best_shot((64, 192), max_crops=L)
        trk.enable_stack()
        rows = synthetic_quads(B, 4 * L, h0, w0, seed=2)[:, ::4].copy()       # the rows with four proper corners: status 1
        rows[:, :, 12:20] = 0.5
        det, count = torch.from_numpy(rows).to(dev), torch.full((B,), L, dtype=torch.int32, device=dev)
        ms = []
        for _ in range(args.reps + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            trk.update(det, count)
            crops, status, sharp = trk._shot_crops(frames, det, count, so, trk.max_tracks)
            runtime.crop_sharpness(crops, status, out=sharp)
            trk._shot_gallery(det, count, so, trk.max_tracks)
            ev[0].record()
            trk._stack_update(det, count, so, trk.max_tracks)
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        a = np.array(ms[1:])        # (the first call sums without a search: its entries are empty)
        n = trk._stack['state'].view(B, -1)[:, 16:].view(B, 128, -1)[:, :, :16].contiguous().view(torch.int32)[:, :, 1]
        res['live_%d' % L] = dict(stack_ms=dict(median=round(float(np.median(a)), 4), min=round(float(a.min()), 4), max=round(float(a.max()), 4)),
                                  crops_summed_per_call=int((n == args.reps + 1).sum()), tracks=B * L,
                                  sad_terms_per_call=B * L * 25 * 60 * 188, sum_bytes_per_call=B * L * 64 * 192 * 6 * 2)
    return res


def nv12_mode(args, model, dev, tdt):
    """--nv12: the same seeded frames as BGR and as NV12, alternating -- frames/s, and the stages of one batch of each kind."""
    import torch
    from yolov6.hip import runtime
    from yolov6.core.frames import FrameBatcher, letterbox_hw
    from yolov6.utils.nv12 import Nv12Frame, bgr_to_nv12_np
    size, stride = [args.size, args.size], int(model.stride.max())
    h0, w0 = args.frame
    conf, iou, max_det = args.conf, args.iou, args.max_det
    rng = np.random.default_rng(0)
    pool = [rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8) for _ in range(args.distinct)]
    nv_pool = [bgr_to_nv12_np(f, args.nv12) for f in pool]          # what a decoder delivers: encoded before any clock starts
    H, W = letterbox_hw((h0, w0), size, stride)
    sync = torch.cuda.synchronize
    out = dict(metric='frames/s end to end, the same frames as BGR and as NV12 (host frames in, rescaled detections out)',
               model=args.model, dtype=args.dtype, frame=[h0, w0], net=[H, W], matrix=args.nv12, runs=args.runs)
    res = {}
    with torch.no_grad():
        for B in args.batches:
            runtime.prepare_for(model, (B, 3, H, W), tdt)
            batchers = dict(bgr=FrameBatcher(dev), nv12=FrameBatcher(dev))
            pools = dict(bgr=pool, nv12=nv_pool)
            x = torch.empty(B, 3, H, W, dtype=tdt, device=dev)

            def run(kind, k):
                fr = [pools[kind][(k * B + j) % len(pool)] for j in range(B)]
                return runtime.detect_frames(model, batchers[kind].put(fr), size, conf, iou, max_det, batch=B, out=x)

            for kind in pools:
                for k in range(2):
                    run(kind, k)
            sync()
            nb = max(2, args.frames // B)
            fps = dict(bgr=[], nv12=[])
            for _ in range(args.runs):
                for kind in pools:
                    t0 = time.perf_counter()
                    for k in range(nb):
                        run(kind, k)
                    sync()
                    fps[kind].append(round(nb * B / (time.perf_counter() - t0), 1))
            r = dict(fps_runs=fps, fps={k: float(np.median(v)) for k, v in fps.items()})
            r['nv12_over_bgr'] = round(r['fps']['nv12'] / r['fps']['bgr'], 4)

            # device time per stage of one batch of each kind, from events on one stream, alternating
            n_bgr, n_nv = h0 * w0 * 3, h0 * w0 * 3 // 2
            host = dict(bgr=torch.empty(B * n_bgr, dtype=torch.uint8, pin_memory=True), nv12=torch.empty(B * n_nv, dtype=torch.uint8, pin_memory=True))
            for j in range(B):
                host['bgr'].numpy()[j * n_bgr:(j + 1) * n_bgr] = pool[j % len(pool)].reshape(-1)
                host['nv12'].numpy()[j * n_nv:(j + 1) * n_nv] = nv_pool[j % len(pool)].packed().reshape(-1)
            dbuf = {k: torch.empty(v.numel(), dtype=torch.uint8, device=dev) for k, v in host.items()}
            views = dict(bgr=[dbuf['bgr'][j * n_bgr:(j + 1) * n_bgr].view(h0, w0, 3) for j in range(B)],
                         nv12=[Nv12Frame.from_packed(dbuf['nv12'][j * n_nv:(j + 1) * n_nv], h0, w0, args.nv12) for j in range(B)])
            conv_out = [torch.empty(h0, w0, 3, dtype=torch.uint8, device=dev) for _ in range(B)]
            names = dict(bgr=['h2d', 'letterbox', 'detect', 'rescale'], nv12=['h2d', 'letterbox', 'detect', 'rescale', 'convert'])
            if args.crops:
                crop_hw = (64, 192)
                cdet = torch.from_numpy(synthetic_quads(B, args.crops, h0, w0, seed=B)).to(dev)
                ccount = torch.full((B,), args.crops, dtype=torch.int32, device=dev)
                cout = torch.empty(B, args.crops, *crop_hw, 3, dtype=torch.uint8, device=dev)
                cst = torch.empty(B, args.crops, dtype=torch.int32, device=dev)
                for v in names.values():
                    v.append('crops')
            if args.redact:
                rn = args.crops or 4
                rdet = torch.from_numpy(synthetic_quads(B, rn, h0, w0, seed=B)).to(dev)
                rcount = torch.full((B,), rn, dtype=torch.int32, device=dev)
                rst = torch.empty(B, rn, dtype=torch.int32, device=dev)
                for v in names.values():
                    v.extend(['redact', 'redact_fill', 'redact_gauss'])
            times = {kind: {k: [] for k in v} for kind, v in names.items()}
            for _ in range(args.reps + 1):
                for kind in ('bgr', 'nv12'):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names[kind]) + 1)]
                    ev[0].record()
                    dbuf[kind].copy_(host[kind], non_blocking=True)
                    ev[1].record()
                    xx, _ = runtime.preprocess_frames(views[kind], size, stride, tdt, batch=B, out=x)
                    ev[2].record()
                    det, count, _ = runtime.detect_padded(model, xx, conf, iou, max_det)
                    ev[3].record()
                    runtime.rescale_round_batch(det, count, (H, W), [(h0, w0)] * B)
                    ev[4].record()
                    i, fr = 4, views[kind]
                    if kind == 'nv12':
                        fr = runtime.nv12_to_bgr(views['nv12'], out=conv_out)
                        i += 1
                        ev[i].record()
                    if args.crops:
                        runtime.plate_crops(fr, cdet, ccount, crop_hw, max_crops=args.crops, out=cout, status=cst)
                        i += 1
                        ev[i].record()
                    if args.redact:     # last: it writes the frames (the next repetition's copy restores them)
                        runtime.redact_plates(views[kind], rdet, rcount, 'mosaic', args.redact_cell, status=rst)
                        ev[i + 1].record()
                        runtime.redact_plates(views[kind], rdet, rcount, 'fill', status=rst)
                        ev[i + 2].record()
                        runtime.redact_plates(views[kind], rdet, rcount, 'gauss', status=rst, sigma=args.redact_sigma)
                        ev[i + 3].record()
                    sync()
                    for i, k in enumerate(names[kind]):
                        times[kind][k].append(ev[i].elapsed_time(ev[i + 1]))
            for kind in ('bgr', 'nv12'):
                med = {k: float(np.median(v[1:])) for k, v in times[kind].items()}
                st = {k: round(v, 4) for k, v in med.items()}
                st['letterbox_runs'] = [round(v, 4) for v in times[kind]['letterbox'][1:]]
                st['h2d_MB'] = round(host[kind].numel() / 1e6, 2)
                st['host_other'] = round(max(0.0, B * 1000.0 / r['fps'][kind] - sum(med[k] for k in ('h2d', 'letterbox', 'detect', 'rescale'))), 4)
                if kind == 'nv12':
                    moved = B * h0 * w0 * 4.5
                    st['convert_runs'] = [round(v, 4) for v in times[kind]['convert'][1:]]
                    st['convert_MB'] = round(moved / 1e6, 2)
                    st['convert_GBps'] = round(moved / (med['convert'] * 1e-3) / 1e9, 1)
                    if args.crops:
                        st['convert_pct_of_detect'] = round(100.0 * med['convert'] / med['detect'], 2)
                if args.redact:
                    st['redact_rows_per_frame'], st['redact_cell'], st['redact_sigma'] = rn, args.redact_cell, args.redact_sigma
                    st['redact_pct_of_detect'] = round(100.0 * med['redact'] / med['detect'], 2)
                    st['redact_gauss_pct_of_detect'] = round(100.0 * med['redact_gauss'] / med['detect'], 2)
                r['stage_ms_' + kind] = st
            sp = times['bgr']['letterbox'][1:]
            r['letterbox_nv12_over_bgr'] = round(r['stage_ms_nv12']['letterbox'] / r['stage_ms_bgr']['letterbox'], 4)
            r['bgr_letterbox_spread_ms'] = round(max(sp) - min(sp), 4)
            res[str(B)] = r
            del host, dbuf, views, conv_out
    out['batches'] = res
    print(json.dumps(out))


def synthetic_quads(n_frames, n, h0, w0, seed=0):
    """[n_frames, n, 28] fp32 detection rows: plates of 120..400 px x 1/3.1 of that, turned by up to 30 degrees; row r % 4 == 1
    also has each corner moved by up to 10 % (perspective), r % 4 == 3 has its BL and TR swapped (a bow-tie: the box is used)."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n_frames, n, 28), np.float32)
    for b in range(n_frames):
        for r in range(n):
            w = rng.uniform(120, 400)
            h = w / 3.1
            cx, cy = rng.uniform(w / 2, w0 - w / 2), rng.uniform(h / 2, h0 - h / 2)
            t = np.radians(rng.uniform(-30, 30))
            c, s = np.cos(t), np.sin(t)
            pts = []
            for px, py in ((-w / 2, -h / 2), (-w / 2, h / 2), (w / 2, h / 2), (w / 2, -h / 2)):    # TL, BL, BR, TR
                if r % 4 == 1:
                    px, py = px + rng.uniform(-0.1, 0.1) * w, py + rng.uniform(-0.1, 0.1) * h
                pts.append((cx + c * px - s * py, cy + s * px + c * py))
            xs, ys = [p[0] for p in pts], [p[1] for p in pts]
            rows[b, r, :4] = [min(xs), min(ys), max(xs), max(ys)]
            if r % 4 == 3:
                pts = [pts[0], pts[3], pts[2], pts[1]]
            rows[b, r, 4:12] = [v for p in pts for v in p]
    return rows


def scene_frames(n, h0, w0, seed=0, sigma=6.0):
    """n seeded BGR frames with the statistics of footage rather than of noise (a JPEG of uniform noise measures nothing): a few
    low-frequency sinusoids per channel, 40 flat rectangles, and Gaussian sensor noise of ``sigma`` levels."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h0, :w0].astype(np.float32)
    out = []
    for _ in range(n):
        img = np.empty((h0, w0, 3), np.float32)
        for c in range(3):
            fx, fy, p = rng.uniform(1 / 900, 1 / 90, 3), rng.uniform(1 / 900, 1 / 90, 3), rng.uniform(0, 6.28, 3)
            img[..., c] = 128 + sum(28 * np.sin(xx * a + yy * b + q) for a, b, q in zip(fx, fy, p))
        for _ in range(40):
            y, x = int(rng.integers(0, h0)), int(rng.integers(0, w0))
            img[y:y + int(rng.integers(8, h0 // 4 + 9)), x:x + int(rng.integers(8, w0 // 4 + 9))] = rng.uniform(0, 255, 3)
        img += rng.normal(0, sigma, img.shape).astype(np.float32)
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out


def jpeg_mode(args, dev):
    """--jpeg Q: stage ``jpeg`` = runtime.encode_jpeg with its two host reads, wall time with a sync either side; stage
    ``jpeg_host`` = what a caller has without it, less the PNG's deflate: D2H of the frame, BGR -> RGB, PIL's JPEG at the same
    quality and subsampling on one thread; both on the same device frames, alternating, the median of --reps, with the bytes per
    frame of each.  ``device_ms`` = the four launches of encode_jpeg_padded alone from events.  Two workloads: --jpeg-frames frames
    of --tile-frame (with --nv12 as NV12 planes of that matrix, with --redact after a mosaic on 4 quads per frame), and one
    [64, 64, 192, 3] crop tensor."""
    import io
    import torch
    from PIL import Image
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import bgr_to_nv12_np, nv12_to_bgr_np
    q, restart, sync = args.jpeg, args.jpeg_restart, torch.cuda.synchronize
    h0, w0 = args.tile_frame
    host = scene_frames(args.jpeg_frames, h0, w0)
    if args.nv12:
        host_nv = [bgr_to_nv12_np(f[:h0 & ~1, :w0 & ~1], args.nv12) for f in host]
        frames = [f.to(dev) for f in host_nv]
    else:
        frames = [torch.from_numpy(f).to(dev) for f in host]
    if args.redact:
        rdet = torch.from_numpy(synthetic_quads(len(frames), 4, h0, w0)).to(dev)
        runtime.redact_plates(frames, rdet, torch.full((len(frames),), 4, dtype=torch.int32, device=dev), 'mosaic', args.redact_cell)
    crops = torch.from_numpy(np.stack([f[y:y + 64, x:x + 192] for f in scene_frames(2, 512, 1536, seed=1)
                                       for y in range(0, 256, 64) for x in range(0, 1536, 192)])).to(dev)
    assert crops.shape == (64, 64, 192, 3)

    def host_path(fr):
        sizes = []
        for f in fr:
            if args.nv12 and not torch.is_tensor(f):
                from yolov6.utils.nv12 import Nv12Frame
                bgr = nv12_to_bgr_np(Nv12Frame(f.y.cpu().numpy(), f.uv.cpu().numpy(), f.matrix))
            else:
                bgr = f.cpu().numpy()
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, format='JPEG', quality=q, subsampling=2)
            sizes.append(buf.tell())
        return sizes

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        return (time.perf_counter() - t0) * 1e3, r

    out = dict(metric='JPEG stage: frames/s of runtime.encode_jpeg (reads included) against D2H + PIL on one thread', quality=q,
               restart=restart, reps=args.reps, nv12=args.nv12, redact=bool(args.redact))
    for name, work, n, hw in (('frames', frames, len(frames), (h0, w0)), ('crops', [crops], 64, (64, 192))):
        units = list(crops) if name == 'crops' else work
        t = dict(jpeg=[], jpeg_host=[], device=[])
        retries0 = runtime.jpeg_stats['retries']
        for rep in range(args.reps + 1):        # the first repetition warms up both paths and is dropped
            ms, files = timed(lambda: runtime.encode_jpeg(work, q, restart))
            t['jpeg'].append(ms)
            ms, sizes = timed(lambda: host_path(units))
            t['jpeg_host'].append(ms)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            sync()
            ev[0].record()
            runtime.encode_jpeg_padded(work, q, restart)
            ev[1].record()
            sync()
            t['device'].append(ev[0].elapsed_time(ev[1]))
        med = {k: float(np.median(v[1:])) for k, v in t.items()}
        src_bytes = hw[0] * hw[1] * (1.5 if args.nv12 and name == 'frames' else 3.0)
        out[name] = dict(n=n, size=list(hw), jpeg_ms=round(med['jpeg'], 3), jpeg_host_ms=round(med['jpeg_host'], 3),
                         device_ms=round(med['device'], 3), jpeg_fps=round(n / med['jpeg'] * 1e3, 1),
                         jpeg_host_fps=round(n / med['jpeg_host'] * 1e3, 1), speedup=round(med['jpeg_host'] / med['jpeg'], 2),
                         bytes_per_frame=round(float(np.mean([len(f) for f in files])), 1),
                         bytes_per_frame_host=round(float(np.mean(sizes)), 1), source_MB_per_frame=round(src_bytes / 1e6, 3),
                         retries=runtime.jpeg_stats['retries'] - retries0)
    print(json.dumps(out))
    return out


def annotate_mode(args, dev):
    """--annotate: stage ``overlay`` = runtime.draw_plates on --jpeg-frames frames of --tile-frame (with --nv12 as NV12 planes) with
    0, 4 and 64 plates per frame (--annotate-plates N: that many), from device events, the frames restored outside the window; beside
    it, on the same frames in the same run and alternating with it: ``host`` = what a caller has without it, D2H of the frame plus
    the PIL drawing of ``Inferer.save_annotated`` on one thread, no file write (wall clock); and ``jpeg`` = the launches of
    ``runtime.encode_jpeg_padded`` of the annotated frames (events).  The median of --reps after one dropped warm-up repetition.
    ``overlay_device`` = the two launches alone: the call captured in a graph, 50 replays between two events (from the second
    replay on the frames are drawn on already; the work is the same), so the wrapper's host time is out."""
    import torch
    from PIL import Image, ImageDraw
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import Nv12Frame, bgr_to_nv12_np, nv12_to_bgr_np
    from yolov6.utils.overlay import Style, build_atlas
    sync = torch.cuda.synchronize
    h0, w0 = args.tile_frame
    nf = args.jpeg_frames
    host = scene_frames(nf, h0, w0)
    if args.nv12:
        clean = [bgr_to_nv12_np(f[:h0 & ~1, :w0 & ~1], args.nv12).to(dev) for f in host]
        work = [Nv12Frame(f.y.clone(), f.uv.clone(), f.matrix) for f in clean]
    else:
        clean = [torch.from_numpy(f).to(dev) for f in host]
        work = [f.clone() for f in clean]
    names = [chr(65 + k) for k in range(26)] + [str(k) for k in range(10)]
    font = runtime.OverlayFont(*build_atlas(names[:31], names[:24], names, size=24), device=dev)
    styles = [Style(t=2, a_line=256, a_plate=160, a_text=256, pad=3)]
    palette = np.array([[40, 40, 200], [40, 140, 40], [200, 80, 40], [20, 140, 200]], np.uint8)

    def restore():
        for w, c in zip(work, clean):
            if args.nv12:
                w.y.copy_(c.y)
                w.uv.copy_(c.uv)
            else:
                w.copy_(c)

    def events(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        sync()
        ev[0].record()
        fn()
        ev[1].record()
        sync()
        return ev[0].elapsed_time(ev[1])

    def host_path(rows):
        for f, rr in zip(work, rows):
            if args.nv12:
                bgr = nv12_to_bgr_np(Nv12Frame(f.y.cpu().numpy(), f.uv.cpu().numpy(), f.matrix))
            else:
                bgr = f.cpu().numpy()
            im = Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1]))
            draw = ImageDraw.Draw(im)
            for r in rr:                                            # Inferer.save_annotated, less the file
                draw.rectangle([float(v) for v in r[:4]], outline=(255, 64, 64), width=2)
                draw.polygon([float(v) for v in r[4:12]], outline=(64, 255, 64))

    out = dict(metric='overlay stage: ms per frame of runtime.draw_plates against D2H + PIL drawing on one thread, and the JPEG encode behind it',
               frame=[h0, w0], frames=nf, reps=args.reps, nv12=args.nv12, glyph=[font.gh, font.gw])
    plates = [args.annotate_plates] if args.annotate_plates is not None else [0, 4, 64]
    rng = np.random.default_rng(7)
    for P in plates:
        rows = synthetic_quads(nf, max(P, 1), h0, w0, seed=P)
        rows[:, :, 20:28] = rng.integers(0, 24, rows[:, :, 20:28].shape)
        det = torch.from_numpy(rows).to(dev)
        count = torch.full((nf,), P, dtype=torch.int32, device=dev)
        tid = torch.arange(nf * max(P, 1), dtype=torch.int32, device=dev).view(nf, -1).contiguous()
        t = dict(overlay=[], host=[], jpeg=[])
        for rep in range(args.reps + 1):                            # the first repetition warms up every path and is dropped
            restore()
            t['overlay'].append(events(lambda: runtime.draw_plates(work, det, count, font, tid=tid, styles=styles, palette=palette)))
            t['jpeg'].append(events(lambda: runtime.encode_jpeg_padded(work, 90, 16)))
            restore()
            sync()
            t0 = time.perf_counter()
            host_path(rows[:, :P])
            t['host'].append((time.perf_counter() - t0) * 1e3)
        # the two launches alone: the call captured in a graph, 50 replays between two events (the wrapper's host time is out)
        draw = lambda: runtime.draw_plates(work, det, count, font, tid=tid, styles=styles, palette=palette)      # noqa: E731
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            draw()
        dev_ms = []
        for rep in range(4):
            restore()
            dev_ms.append(events(lambda: [g.replay() for _ in range(50)]) / 50)
        med = {k: float(np.median(v[1:])) / nf for k, v in t.items()}
        out['plates_%d' % P] = dict(overlay_ms_per_frame=round(med['overlay'], 4), host_ms_per_frame=round(med['host'], 3),
                                    jpeg_ms_per_frame=round(med['jpeg'], 4),
                                    overlay_device_ms_per_frame=round(float(np.median(dev_ms[1:])) / nf, 5),
                                    overlay_runs_ms=[round(v / nf, 4) for v in t['overlay'][1:]],
                                    overlay_over_jpeg=round(med['overlay'] / med['jpeg'], 4),
                                    host_over_overlay=round(med['host'] / med['overlay'], 1))
    print(json.dumps(out))
    return out


def scene_mode(args, dev):
    """--annotate --scene L Z: stage ``scene`` = runtime.draw_scene on --jpeg-frames frames of --tile-frame (with --nv12 as NV12 planes):
    Z zones of 16 vertices (--scene-cover: zone 0 is the whole frame) and L lines with names, totals and occupancies, one dwell
    alert, and with --speed a km/h tag on each of 16 plates per frame; from device events, the frames restored outside the window.
    Beside it on the same frames, alternating: ``plates`` = runtime.draw_plates of those 16 plates, and ``host`` = what a caller has
    without the stage: D2H of the frame plus PIL ``polygon`` / ``line`` / ``text`` on one thread, no file write (wall clock).  The median
    of --reps after one dropped warm-up repetition.  ``scene_device`` = the two launches alone: the call captured in a graph, 50
    replays between two events."""
    import torch
    from PIL import Image, ImageDraw
    from yolov6.hip import runtime
    from yolov6.utils.nv12 import Nv12Frame, bgr_to_nv12_np, nv12_to_bgr_np
    from yolov6.utils.overlay import Style, build_atlas
    from yolov6.utils.scene import SceneStyle, build_scene_atlas, names_of
    sync = torch.cuda.synchronize
    h0, w0 = args.tile_frame
    nf, (L, Z), P = args.jpeg_frames, args.scene, 16
    host = scene_frames(nf, h0, w0)
    if args.nv12:
        clean = [bgr_to_nv12_np(f[:h0 & ~1, :w0 & ~1], args.nv12).to(dev) for f in host]
        work = [Nv12Frame(f.y.clone(), f.uv.clone(), f.matrix) for f in clean]
    else:
        clean = [torch.from_numpy(f).to(dev) for f in host]
        work = [f.clone() for f in clean]
    rng = np.random.default_rng(11)
    zones, lines = [], []
    for z in range(Z):                                                  # 16-vertex stars on a 4 x 2 grid, a sixth of the height across
        cx, cy, r = w0 * (2 * (z % 4) + 1) / 8, h0 * (2 * (z // 4) + 1) / 4, h0 / 6
        v = [(cx + (r if k % 2 == 0 else 0.6 * r) * np.cos(k * np.pi / 8), cy + (r if k % 2 == 0 else 0.6 * r) * np.sin(k * np.pi / 8)) for k in range(16)]
        if z == 0 and args.scene_cover:
            v = [(-1.0, -1.0)] + [(w0 * k / 7, -1.0 - k % 2) for k in range(1, 7)] + [(w0 + 1.0, -1.0), (w0 + 1.0, h0 + 1.0)] + \
                [(w0 * k / 7, h0 + 1.0 + k % 2) for k in range(6, 0, -1)] + [(-1.0, h0 + 1.0)]
        zones.append((v, 10))
    for l in range(L):
        lines.append(tuple(float(v) for v in (rng.uniform(0, w0), rng.uniform(0, h0), rng.uniform(0, w0), rng.uniform(0, h0))))
    S = nf
    zm = runtime.ZoneMap(S, [lines] * S, [zones] * S, device=dev)
    atlas = build_scene_atlas(24)
    font = runtime.SceneFont(atlas, device=dev)
    names = names_of((None, None, [['line%02d' % l for l in range(L)]] * S, [['zone%d' % z for z in range(Z)]] * S), atlas)
    names = torch.from_numpy(names.view(np.int16)).to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    ev = torch.zeros(S, 8, 12, **i32)
    ev[:, 0, 0], ev[:, 0, 1] = 4, min(1, max(Z - 1, 0))
    zone = (ev, torch.ones(S, **i32), torch.from_numpy(rng.integers(0, 5, (S, 8)).astype(np.int32)).to(dev),
            torch.from_numpy(rng.integers(0, 5000, (S, 2, 16)).astype(np.int32)).to(dev))
    rows = synthetic_quads(nf, P, h0, w0, seed=P)
    rows[:, :, 20:28] = rng.integers(0, 24, rows[:, :, 20:28].shape)
    det = torch.from_numpy(rows).to(dev)
    count = torch.full((nf,), P, **i32)
    tid = torch.arange(P, **i32).repeat(nf, 1).contiguous()
    speed_i = torch.zeros(S, 64, 8, **i32)
    speed_i[:, :, 0] = -1
    speed_i[:, :P, 0] = torch.arange(P, **i32)
    speed_i[:, :P, 1] = torch.from_numpy(rng.integers(2000, 40000, (S, P)).astype(np.int32)).to(dev)
    tags = dict(speed=(speed_i,), det=det, count=count, tid=tid) if args.speed else {}
    style = SceneStyle()
    pnames = [chr(65 + k) for k in range(26)] + [str(k) for k in range(10)]
    pfont = runtime.OverlayFont(*build_atlas(pnames[:31], pnames[:24], pnames, size=24), device=dev)
    pstyles = [Style(t=2, a_line=256, a_plate=160, a_text=256, pad=3)]

    def restore():
        for w, c in zip(work, clean):
            if args.nv12:
                w.y.copy_(c.y)
                w.uv.copy_(c.uv)
            else:
                w.copy_(c)

    def events(fn):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        sync()
        e[0].record()
        fn()
        e[1].record()
        sync()
        return e[0].elapsed_time(e[1])

    occ_h, tot_h = zone[2].cpu().numpy(), zone[3].cpu().numpy()

    def host_path():
        for b, f in enumerate(work):
            if args.nv12:
                bgr = nv12_to_bgr_np(Nv12Frame(f.y.cpu().numpy(), f.uv.cpu().numpy(), f.matrix))
            else:
                bgr = f.cpu().numpy()
            im = Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1]))
            draw = ImageDraw.Draw(im, 'RGBA')                           # a fill with an alpha blends
            for z, (v, _) in enumerate(zones):
                draw.polygon([(float(x), float(y)) for x, y in v], fill=(0, 160, 200, 48), outline=(0, 160, 200, 255))
                draw.text((float(v[0][0]), float(v[0][1])), 'zone%d %d' % (z, occ_h[b, z]), fill=(255, 255, 255, 255))
            for l, a in enumerate(lines):
                draw.line([a[0], a[1], a[2], a[3]], fill=(255, 255, 0, 255), width=2)
                draw.text((a[2], a[3]), 'line%02d +%d -%d' % (l, tot_h[b, 0, l], tot_h[b, 1, l]), fill=(255, 255, 255, 255))
            if args.speed:
                for r in rows[b]:
                    draw.text((float(r[2]), float(r[1])), '88', fill=(255, 255, 255, 255))

    draw_scene = lambda: runtime.draw_scene(work, zm, font, names=names, zone=zone, style=style, **tags)      # noqa: E731
    t = dict(scene=[], plates=[], host=[])
    for rep_ in range(args.reps + 1):                                   # the first repetition warms up every path and is dropped
        restore()
        t['scene'].append(events(draw_scene))
        t['plates'].append(events(lambda: runtime.draw_plates(work, det, count, pfont, tid=tid, styles=pstyles)))
        restore()
        sync()
        t0 = time.perf_counter()
        host_path()
        t['host'].append((time.perf_counter() - t0) * 1e3)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        draw_scene()
    dev_ms = []
    for rep_ in range(4):
        restore()
        dev_ms.append(events(lambda: [g.replay() for _ in range(50)]) / 50)
    med = {k: float(np.median(v[1:])) / nf for k, v in t.items()}
    device = float(np.median(dev_ms[1:])) / nf
    out = dict(metric='scene overlay stage: ms per frame of runtime.draw_scene against runtime.draw_plates of 16 plates and against D2H + PIL '
                      'polygon / line / text on one thread',
               frame=[h0, w0], frames=nf, reps=args.reps, nv12=args.nv12, lines=L, zones=Z, cover=bool(args.scene_cover), tags=P if args.speed else 0,
               glyph=[font.gh, font.gw], scene_ms_per_frame=round(med['scene'], 4), scene_device_ms_per_frame=round(device, 5),
               plates_ms_per_frame=round(med['plates'], 4), host_ms_per_frame=round(med['host'], 3),
               scene_runs_ms=[round(v / nf, 4) for v in t['scene'][1:]], host_over_scene_device=round(med['host'] / max(device, 1e-9), 1))
    print(json.dumps(out))
    return out


def sampled_rows(h0, rh):
    """Distinct source rows the bilinear resize reads for rh output rows (the y0 / y1 of resize_coef, lp_internal.h)."""
    if rh == h0:
        return h0
    d = np.arange(rh, dtype=np.float64)
    f = ((d + 0.5) * (h0 / rh) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    s = np.clip(s, 0, h0 - 1)
    return len(np.union1d(s, np.minimum(s + 1, h0 - 1)))


def main():
    args = parse()
    import torch
    from yolov6.utils.synth import build_synthetic
    from yolov6.utils.torch_utils import fuse_model
    from yolov6.layers.common import RepVGGBlock
    from yolov6.hip import runtime
    from yolov6.core.frames import FrameBatcher, letterbox_hw
    from yolov6.data.data_augment import letterbox_geometry
    if not torch.cuda.is_available():
        raise SystemExit('frames_bench.py measures the GPU path: no GPU')
    dev = torch.device('cuda', 0)
    tdt = {'f16': torch.float16, 'f32': torch.float32}[args.dtype]
    if args.jpeg is not None:
        return jpeg_mode(args, dev)
    if args.annotate and args.scene is not None:
        return scene_mode(args, dev)
    if args.annotate:
        return annotate_mode(args, dev)
    model = fuse_model(build_synthetic(os.path.join(ROOT, 'configs', args.model + '.py'), sigma=SIGMA[args.model])).eval()
    for layer in model.modules():
        if isinstance(layer, RepVGGBlock):
            layer.switch_to_deploy()
    model = model.to(dev).to(tdt)
    model.lp_graph = True                   # as Inferer sets it
    if args.tile and args.gate:
        if args.gate_illum == 'gain' or args.gate_drift:
            return gate_drift_mode(args, model, dev, tdt)
        return gate_mode(args, model, dev, tdt)
    if args.tile:
        return tile_mode(args, model, dev, tdt)
    if args.track:
        return track_mode(args, model, dev, tdt)
    if args.nv12:
        return nv12_mode(args, model, dev, tdt)
    size, stride = [args.size, args.size], int(model.stride.max())
    h0, w0 = args.frame
    rng = np.random.default_rng(0)
    pool = [rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8) for _ in range(args.distinct)]
    H, W = letterbox_hw((h0, w0), size, stride)
    conf, iou, max_det = args.conf, args.iou, args.max_det
    sync = torch.cuda.synchronize
    out = dict(metric='frames/s end to end (host frames in, rescaled detections out)', model=args.model, dtype=args.dtype,
               frame=[h0, w0], net=[H, W])

    # ---- per-frame path (Inferer.infer at batch_size 1) --------------------------------------------------------------
    def one(f):
        frame = torch.from_numpy(f).to(dev)
        img = runtime.preprocess_letterbox(frame, size, stride, tdt)
        det = runtime.detect(model, img[None], conf, iou, max_det)[0]
        if len(det):
            runtime.rescale_round(img.shape[1:], det, f.shape)
        return det.cpu()

    with torch.no_grad():
        runtime.prepare_for(model, (1, 3, H, W), tdt)
        for i in range(8):
            one(pool[i % len(pool)])
        sync()
        t0 = time.perf_counter()
        for i in range(args.single_frames):
            one(pool[i % len(pool)])
        sync()
        out['per_frame_fps'] = round(args.single_frames / (time.perf_counter() - t0), 1)

        # ---- batched path: FrameBatcher + detect_frames ---------------------------------------------------------------
        batched, stages = {}, {}
        for B in args.batches:
            runtime.prepare_for(model, (B, 3, H, W), tdt)
            batcher = FrameBatcher(dev)
            x = torch.empty(B, 3, H, W, dtype=tdt, device=dev)
            def run(k):
                fr = [pool[(k * B + j) % len(pool)] for j in range(B)]
                return runtime.detect_frames(model, batcher.put(fr), size, conf, iou, max_det, batch=B, out=x)
            for k in range(2):
                run(k)
            sync()
            nb = max(2, args.frames // B)
            t0 = time.perf_counter()
            for k in range(nb):
                run(k)
            sync()
            batched[str(B)] = round(nb * B / (time.perf_counter() - t0), 1)

            # device time per stage of one batch, from events on one stream
            fr = [pool[j % len(pool)] for j in range(B)]
            nbytes = sum(f.nbytes for f in fr)
            host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            hv = host.numpy()
            for j, f in enumerate(fr):
                hv[j * f.nbytes:(j + 1) * f.nbytes] = f.reshape(-1)
            dbuf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            views = [dbuf[j * f.nbytes:(j + 1) * f.nbytes].view(f.shape) for j, f in enumerate(fr)]
            times = {k: [] for k in ('h2d', 'letterbox', 'detect', 'rescale') + (('crops',) if args.crops else ())
                     + (('redact', 'redact_fill', 'redact_gauss') if args.redact else ())}
            if args.redact:
                rn = args.crops or 4
                rdet = torch.from_numpy(synthetic_quads(B, rn, h0, w0, seed=B)).to(dev)
                rcount = torch.full((B,), rn, dtype=torch.int32, device=dev)
                rst = torch.empty(B, rn, dtype=torch.int32, device=dev)
            if args.crops:
                crop_hw = (64, 192)
                cdet = torch.from_numpy(synthetic_quads(B, args.crops, h0, w0, seed=B)).to(dev)
                ccount = torch.full((B,), args.crops, dtype=torch.int32, device=dev)
                cout = torch.empty(B, args.crops, *crop_hw, 3, dtype=torch.uint8, device=dev)
                cst = torch.empty(B, args.crops, dtype=torch.int32, device=dev)
            for _ in range(args.reps + 1):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(times) + 1)]
                ev[0].record()
                dbuf.copy_(host, non_blocking=True)
                ev[1].record()
                xx, _ = runtime.preprocess_frames(views, size, stride, tdt, batch=B, out=x)
                ev[2].record()
                det, count, _ = runtime.detect_padded(model, xx, conf, iou, max_det)
                ev[3].record()
                runtime.rescale_round_batch(det, count, (H, W), [f.shape for f in fr])
                ev[4].record()
                if args.crops:      # enqueued while detect still runs: the event pair brackets the kernel alone
                    runtime.plate_crops(views, cdet, ccount, crop_hw, max_crops=args.crops, out=cout, status=cst)
                    ev[5].record()
                if args.redact:         # last: it writes the frames (the next repetition's copy restores them)
                    i = 5 if args.crops else 4
                    runtime.redact_plates(views, rdet, rcount, 'mosaic', args.redact_cell, status=rst)
                    ev[i + 1].record()
                    runtime.redact_plates(views, rdet, rcount, 'fill', status=rst)
                    ev[i + 2].record()
                    runtime.redact_plates(views, rdet, rcount, 'gauss', status=rst, sigma=args.redact_sigma)
                    ev[i + 3].record()
                sync()
                for i, k in enumerate(times):
                    times[k].append(ev[i].elapsed_time(ev[i + 1]))
            med = {k: float(np.median(v[1:])) for k, v in times.items()}
            stages[str(B)] = {k: round(v, 4) for k, v in med.items()}
            e2e_ms = B * 1000.0 / batched[str(B)]
            stages[str(B)]['host_other'] = round(max(0.0, e2e_ms - sum(med[k] for k in ('h2d', 'letterbox', 'detect', 'rescale'))), 4)
            stages[str(B)]['bound_by'] = max(('h2d', 'letterbox', 'detect', 'rescale', 'host_other'), key=lambda k: stages[str(B)][k])
            _, (rw, rh), _, _ = letterbox_geometry((h0, w0), size, stride=stride)
            moved = B * (sampled_rows(h0, rh) * w0 * 3 + 3 * H * W * x.element_size())
            stages[str(B)]['letterbox_MB'] = round(moved / 1e6, 2)
            stages[str(B)]['letterbox_GBps'] = round(moved / (med['letterbox'] * 1e-3) / 1e9, 1)
            if args.crops:
                stages[str(B)]['crops_per_frame'] = args.crops
                stages[str(B)]['crops_status_counts'] = np.bincount(cst.cpu().numpy().reshape(-1), minlength=4).tolist()
                stages[str(B)]['crops_out_MB'] = round(cout.numel() / 1e6, 2)
                stages[str(B)]['crops_pct_of_detect'] = round(100.0 * med['crops'] / med['detect'], 2)
                del cdet, ccount, cout, cst
            if args.redact:
                stages[str(B)]['redact_rows_per_frame'], stages[str(B)]['redact_cell'] = rn, args.redact_cell
                stages[str(B)]['redact_sigma'] = args.redact_sigma
                stages[str(B)]['redact_pct_of_detect'] = round(100.0 * med['redact'] / med['detect'], 2)
                stages[str(B)]['redact_gauss_pct_of_detect'] = round(100.0 * med['redact_gauss'] / med['detect'], 2)
            del host, dbuf, views
    out['batched_fps'] = batched
    out['stage_ms'] = stages
    out['speedup_vs_per_frame'] = {b: round(v / out['per_frame_fps'], 1) for b, v in batched.items()}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
