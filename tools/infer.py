#!/usr/bin/env python3
"""Inference entry point: the flags and the ``run`` keyword arguments of reference tools/infer.py:19-107.

    python tools/infer.py --weights weights/yololps.pt --source data/images --yaml data/dataset.yaml [--half]
                          [--batch-size 32] [--fixed-shape] [--save-crops [--crop-size 64 192]]
                          [--tile 640 640 [--tile-overlap 0.2] [--no-tile-overview] [--merge-metric iou|ios]]
                          [--track [--track-max-age 5] [--track-iou 0.3] [--track-expand 0.5] [--best-shots [--crop-size 64 192]
                           [--stack-shots [--stack-search 2] [--stack-max-frames 64] [--stack-min-width 0]]]]
                          [--nv12 bt601|bt709|bt601f|bt709f [--nv12-size W H]]
                          [--redact mosaic|fill|gauss [--redact-cell 16] [--redact-sigma 8] [--redact-margin 0.1]
                           [--redact-hold [--redact-hold-min-hits 1] [--redact-lookback D [--redact-lookback-max-back N]]]]
                          [--track --watchlist FILE [--watch-mismatch 1] [--watch-cost F]
                           [--watch-confusable "0D 0Q 8B 2Z 5S" [--watch-confusable-weight 4]]
                           [--watch-live [--watch-live-min-hits 3]] [--watch-indel [--watch-gap-cost 1.0]]]
                          [--track --sightings C [--sight-window N] [--sight-min-hits 1] [--sight-mismatch 1] [--sight-cost F]]
                          [--track --zones FILE [--zones-min-hits 1]]
                          [--track --speed FILE [--speed-min-hits 1] [--speed-confirm 2]]
                          [--save-jpeg Q]
                          [--overlay [--overlay-font TTF] [--overlay-size 24] [--overlay-thickness 2] [--overlay-alpha 256 160 256]
                           [--overlay-scene (with --zones and/or --speed)]]
                          [--tile H W --tile-gate [--tile-gate-thres 2.0] [--tile-gate-min-cells 1] [--tile-gate-refresh 50]
                           [--tile-gate-illum none|gain] [--tile-gate-max-gain 1.5]]
"""
import argparse
import os
import os.path as osp
import sys

import torch

ROOT = os.getcwd()
if str(ROOT) not in sys.path:
    sys.path.append(str(ROOT))

from yolov6.utils.events import LOGGER      # noqa: E402
from yolov6.core.inferer import Inferer      # noqa: E402

# (flag, argparse keywords): the reference's flag set, defaults included
_FLAGS = [
    ('--weights', dict(type=str, default='weights/yolov6s.pt', help='checkpoint (.pt) to run')),
    ('--source', dict(type=str, default='data/images', help='image file or directory of images / videos')),
    ('--yaml', dict(type=str, default='data/dataset.yaml', help='dataset yaml (class names)')),
    ('--img-size', dict(nargs='+', type=int, default=[640, 640], help='network input size, h w')),
    ('--conf-thres', dict(type=float, default=0.4, help='score threshold of the NMS')),
    ('--iou-thres', dict(type=float, default=0.45, help='IoU threshold of the NMS')),
    ('--max-det', dict(type=int, default=1000, help='detections kept per image')),
    ('--device', dict(default='0', help='GPU index (0, or 0,1,2,3) or cpu')),
    ('--save-txt', dict(action='store_true', help='write one label file per image')),
    ('--not-save-img', dict(action='store_true', help='do not write the annotated images')),
    ('--save-dir', dict(type=str, help='output directory (default: project/name)')),
    ('--view-img', dict(action='store_true', help='show the annotated frames')),
    ('--classes', dict(nargs='+', type=int, help='keep these class ids only')),
    ('--agnostic-nms', dict(action='store_true', help='class-agnostic NMS')),
    ('--project', dict(default='runs/inference', help='parent of the default output directory')),
    ('--name', dict(default='exp', help='name of the default output directory')),
    ('--hide-labels', dict(default=False, action='store_true', help='draw boxes without text')),
    ('--hide-conf', dict(default=False, action='store_true', help='draw labels without scores')),
    ('--half', dict(action='store_true', help='fp16 engine')),
    ('--batch-size', dict(type=int, default=1, help='frames per forward on a GPU (consecutive frames of one letterboxed shape)')),
    ('--fixed-shape', dict(action='store_true', help='letterbox every frame to exactly --img-size (no stride-multiple trim)')),
    ('--save-crops', dict(action='store_true', help='write every plate, rectified along its four corners, as crops/<stem>_<k>.png')),
    ('--crop-size', dict(nargs=2, type=int, default=[64, 192], metavar=('H', 'W'), help='size of the plate crops, h w')),
    ('--tile', dict(nargs=2, type=int, default=None, metavar=('H', 'W'),
                    help='detect large frames by overlapping tiles of this size (plus the whole frame), merged per frame; '
                         '--batch-size is then tiles per forward')),
    ('--tile-overlap', dict(type=float, default=0.2, help='overlap of neighbouring tiles: pixels, or a fraction of the tile below 1')),
    ('--no-tile-overview', dict(action='store_true', help='do not add the whole frame as one more tile')),
    ('--merge-metric', dict(default='iou', choices=['iou', 'ios'], help='overlap measure of the cross-tile merge')),
    ('--track', dict(action='store_true', help='track plates across the frames of a video (or of the image files, in order) and vote '
                                               'their characters per track: saves the voted rows, tracks.txt and plates.txt')),
    ('--track-max-age', dict(type=int, default=5, help='frames a track survives unseen')),
    ('--track-iou', dict(type=float, default=0.3, help='IoU (of the expanded boxes) above which a detection continues a track')),
    ('--track-expand', dict(type=float, default=0.5, help='boxes are grown by this fraction of their size on every side before the IoU')),
    ('--best-shots', dict(action='store_true', help='with --track: keep the sharpest rectified crop (--crop-size) of every track and write '
                                                    'shots/<line>_<id>.png and shots.txt, line-parallel to plates.txt')),
    ('--stack-shots', dict(action='store_true', help='with --best-shots: also average the rectified crops of every track, each aligned by '
                                                     'a small integer shift, into one denoised picture and write stacks/<line>_<id>.png and '
                                                     'stacks.txt, line-parallel to plates.txt')),
    ('--stack-search', dict(type=int, default=2, metavar='N', help='with --stack-shots: largest shift of the alignment in pixels (0..4)')),
    ('--stack-max-frames', dict(type=int, default=64, metavar='N', help='with --stack-shots: crops averaged per track at most (1..255)')),
    ('--stack-min-width', dict(type=float, default=0.0, metavar='F',
                               help='with --stack-shots: only plates at least this wide in frame pixels are averaged')),
    ('--nv12', dict(default=None, choices=['bt601', 'bt709', 'bt601f', 'bt709f'], metavar='MATRIX',
                    help='send frames as NV12 with this matrix (bt601, bt709: limited range; bt601f, bt709f: full range): decoded images '
                         'are encoded on the host as a stand-in for a decoder; a source ending in .nv12 is a raw stream of packed frames')),
    ('--nv12-size', dict(nargs=2, type=int, default=None, metavar=('W', 'H'), help='frame size of .nv12 sources')),
    ('--redact', dict(default=None, choices=['mosaic', 'fill', 'gauss'], metavar='MODE',
                      help='also write every frame with its detected plates made unreadable (mosaic, a black fill, or a Gaussian '
                           'blur) to redacted/')),
    ('--redact-cell', dict(type=int, default=16, help='with --redact mosaic: side of a mosaic cell in pixels (even, 2..64)')),
    ('--redact-sigma', dict(type=float, default=8.0, help='with --redact gauss: sigma of the blur in pixels (0.5..16)')),
    ('--redact-margin', dict(type=float, default=0.1, help='with --redact: grow every plate by this fraction of its size (0..4)')),
    ('--redact-hold', dict(action='store_true', help='with --track and --redact: keep a tracked plate redacted, where its track predicts '
                                                     'it, in the frames in which the detector misses it (until the track ends)')),
    ('--redact-hold-min-hits', dict(type=int, default=1, help='with --redact-hold: detections a track needs before it is held')),
    ('--redact-lookback', dict(type=int, default=None, metavar='D',
                               help='with --redact-hold: redact every frame D frames late (1..32), so that the frames before a '
                                    'plate\'s first detection are covered too, where its first two detections extrapolate it')),
    ('--redact-lookback-max-back', dict(type=int, default=None, metavar='N',
                                        help='with --redact-lookback: frames before the first detection that are covered (default D)')),
    ('--watchlist', dict(type=str, default=None, metavar='FILE',
                         help='with --track: look the read of every ended track up in this list (one plate per line: the plate text with * '
                              'or ? for any character, or eight ids with * for any) and write hits.txt beside plates.txt')),
    ('--watch-mismatch', dict(type=int, default=1, help='with --watchlist: positions that may differ (0..8)')),
    ('--watch-cost', dict(type=float, default=None, metavar='F',
                          help='with --watchlist: largest total cost of the differing positions, in fully confident mismatches (a position '
                               'the vote was unsure about costs less; default: no limit)')),
    ('--watch-confusable', dict(type=str, default=None, metavar='PAIRS',
                                help='with --watchlist: pairs of characters that are misread for each other, e.g. "0D 0Q 8B 2Z 5S"')),
    ('--watch-confusable-weight', dict(type=int, default=4, help='with --watch-confusable: what such a pair costs, in sixteenths of a mismatch (0..16)')),
    ('--watch-live', dict(action='store_true', help='with --watchlist: also look a track up while it is still live, once it has enough '
                                                    'detections and again when its voted read changes, and write alerts.txt')),
    ('--watch-live-min-hits', dict(type=int, default=3, metavar='N', help='with --watch-live: detections a track needs before it is looked up')),
    ('--watch-indel', dict(action='store_true', help='with --watchlist: also accept a read that lost or gained one character in heads 2..7 '
                                                     '(counted as one mismatch); hits.txt and alerts.txt gain an alignment column')),
    ('--watch-gap-cost', dict(type=float, default=1.0, metavar='F', help='with --watch-indel: what the lost or gained character costs, in fully '
                                                                         'confident mismatches (0..1)')),
    ('--sightings', dict(type=int, default=None, metavar='C',
                         help='with --track: keep a log of the last C reads of all streams, match the read of every ended track against the '
                              'earlier ones (a broken track, the same vehicle on another video) and write resightings.txt beside plates.txt; '
                              '--watch-confusable applies')),
    ('--sight-window', dict(type=int, default=None, metavar='N', help='with --sightings: frames of the source a sighting stays a candidate (default: no limit)')),
    ('--sight-min-hits', dict(type=int, default=1, metavar='N', help='with --sightings: detections a track needs to be matched and logged')),
    ('--sight-mismatch', dict(type=int, default=1, help='with --sightings: positions that may differ (0..8)')),
    ('--sight-cost', dict(type=float, default=None, metavar='F',
                          help='with --sightings: largest total cost of the differing positions, in fully confident mismatches (default: no limit)')),
    ('--zones', dict(type=str, default=None, metavar='FILE',
                     help='with --track: a file of directed lines (`line NAME x1 y1 x2 y2`) and polygon zones (`zone NAME [dwell=N] x1 y1 x2 y2 '
                          'x3 y3 ...`, an optional `S:` stream prefix) in frame pixels; write the crossings of the live tracks to '
                          'crossings.txt and zone entries, exits, dwell alerts and tracks that ended inside to zones.txt')),
    ('--zones-min-hits', dict(type=int, default=1, metavar='N', help='with --zones: detections a track needs before it is tested')),
    ('--speed', dict(type=str, default=None, metavar='FILE',
                     help='with --track: a calibration file (`plane h0 .. h8` or `points x y X Y ...`: frame pixels to metres on the plane '
                          'the plates move in; `fps F` or `period_us N`; `limit KMH`; `gap_ms N`; `span_ms N`; an optional `S:` stream '
                          'prefix); write peak and chord speed of every ended track to speeds.txt and the tracks over the limit, while '
                          'they are still live, to speeding.txt')),
    ('--speed-min-hits', dict(type=int, default=1, metavar='N', help='with --speed: detections a track needs before it is measured')),
    ('--speed-confirm', dict(type=int, default=2, metavar='N', help='with --speed: estimates in a row over the limit that make an alert')),
    ('--tile-gate', dict(action='store_true', help='with --tile: the source is one fixed camera (frames of one size); run the network only on '
                                                   'the tiles whose pixels changed since they were last detected, keep the rows of the others')),
    ('--tile-gate-thres', dict(type=float, default=2.0, metavar='F',
                               help='with --tile-gate: luma levels per pixel a 16 x 16 cell must change by (0..255)')),
    ('--tile-gate-min-cells', dict(type=int, default=1, metavar='N', help='with --tile-gate: changed cells that make a tile run again')),
    ('--tile-gate-refresh', dict(type=int, default=50, metavar='N', help='with --tile-gate: frames after which a tile runs again anyway (0: never)')),
    ('--tile-gate-illum', dict(choices=('none', 'gain'), default='none',
                               help='with --tile-gate: gain = compare a tile after scaling its reference by one estimated gain per tile, so that '
                                    'an exposure step or a cloud does not run every tile again')),
    ('--tile-gate-max-gain', dict(type=float, default=1.5, metavar='F',
                                  help='with --tile-gate-illum gain: a tile whose gain leaves [1 / F, F] runs again (1..4)')),
    ('--save-jpeg', dict(type=int, default=None, metavar='Q',
                         help='write the redacted frames, the crops, the shots and the stacks as baseline JPEG (.jpg) of quality Q '
                              '(1..100), encoded on the GPU, instead of PNG')),
    ('--overlay', dict(action='store_true', help='also write every frame with box, corner quad and a label (track id with --track, '
                                                 'the eight characters) drawn on it, on the GPU, to annotated/ (.jpg with --save-jpeg)')),
    ('--overlay-font', dict(type=str, default=None, metavar='TTF',
                            help='with --overlay: TrueType file of the label glyphs (default: PIL\'s built-in font, without CJK: the '
                                 'province then shows ?)')),
    ('--overlay-size', dict(type=int, default=24, metavar='PX', help='with --overlay: glyph size in pixels (4..60)')),
    ('--overlay-thickness', dict(type=int, default=2, metavar='N', help='with --overlay: outline thickness in pixels (0..16)')),
    ('--overlay-alpha', dict(nargs=3, type=int, default=[256, 160, 256], metavar=('L', 'P', 'T'),
                             help='with --overlay: opacity 0..256 of the outlines, the label plate and the text')),
    ('--overlay-scene', dict(action='store_true', help='with --overlay and --zones and/or --speed: also draw the zones, the lines with '
                                                       'their direction marker, their names and counts, and a km/h tag per plate')),
]


def get_args_parser(add_help=True):
    parser = argparse.ArgumentParser(description='YOLO-LP inference on MI355X (HIP engine) or CPU.', add_help=add_help)
    for flag, kw in _FLAGS:
        parser.add_argument(flag, **kw)
    args = parser.parse_args()
    LOGGER.info(args)
    return args


@torch.no_grad()
def run(weights=osp.join(ROOT, 'yolov6s.pt'), source=osp.join(ROOT, 'data/images'), yaml=None, img_size=640,
        conf_thres=0.4, iou_thres=0.45, max_det=1000, device='', save_txt=False, not_save_img=False, save_dir=None,
        view_img=True, classes=None, agnostic_nms=False, project=osp.join(ROOT, 'runs/inference'), name='exp',
        hide_labels=False, hide_conf=False, half=False, batch_size=1, fixed_shape=False, save_crops=False, crop_size=(64, 192),
        tile=None, tile_overlap=0.2, no_tile_overview=False, merge_metric='iou', track=False, track_max_age=5, track_iou=0.3,
        track_expand=0.5, best_shots=False, stack_shots=False, stack_search=2, stack_max_frames=64, stack_min_width=0.0, nv12=None, nv12_size=None, redact=None, redact_cell=16,
        redact_margin=0.1, redact_hold=False, redact_hold_min_hits=1, redact_lookback=None, redact_lookback_max_back=None,
        redact_sigma=8.0, watchlist=None, watch_mismatch=1, watch_cost=None, watch_confusable=None, watch_confusable_weight=4,
        watch_live=False, watch_live_min_hits=3, tile_gate=False, tile_gate_thres=2.0, tile_gate_min_cells=1, tile_gate_refresh=50,
        tile_gate_illum='none', tile_gate_max_gain=1.5, sightings=None, sight_window=None, sight_min_hits=1, sight_mismatch=1, sight_cost=None,
        save_jpeg=None, overlay=False, overlay_font=None, overlay_size=24, overlay_thickness=2, overlay_alpha=(256, 160, 256),
        zones=None, zones_min_hits=1, speed=None, speed_min_hits=1, speed_confirm=2, overlay_scene=False,
        watch_indel=False, watch_gap_cost=1.0):
    save_img = not not_save_img
    out_dir = save_dir if save_dir is not None else osp.join(project, name)
    if (save_img or save_txt or save_crops or track or redact or overlay) and not osp.exists(out_dir):
        os.makedirs(out_dir)
    else:
        LOGGER.warning('Save directory already existed')
    if save_txt:
        os.makedirs(osp.join(out_dir, 'labels'), exist_ok=True)
    if tile is not None and tile_overlap >= 1:
        tile_overlap = int(tile_overlap)        # pixels
    results = Inferer(source, weights, device, yaml, img_size, half, batch_size=batch_size, auto=not fixed_shape, tile=tile,
                      tile_overlap=tile_overlap, tile_overview=not no_tile_overview, merge_metric=merge_metric, track=track, track_max_age=track_max_age,
                      track_iou=track_iou, track_expand=track_expand, best_shots=best_shots, stack_shots=stack_shots, stack_search=stack_search,
                      stack_max_frames=stack_max_frames, stack_min_width=stack_min_width, nv12=nv12, nv12_size=nv12_size,
                      redact=redact, redact_cell=redact_cell, redact_margin=redact_margin, redact_hold=redact_hold,
                      redact_hold_min_hits=redact_hold_min_hits, redact_lookback=redact_lookback,
                      redact_lookback_max_back=redact_lookback_max_back, redact_sigma=redact_sigma, watchlist=watchlist,
                      watch_mismatch=watch_mismatch, watch_cost=watch_cost, watch_confusable=watch_confusable,
                      watch_confusable_weight=watch_confusable_weight, watch_live=watch_live, watch_live_min_hits=watch_live_min_hits,
                      tile_gate=tile_gate, tile_gate_thres=tile_gate_thres,
                      tile_gate_min_cells=tile_gate_min_cells, tile_gate_refresh=tile_gate_refresh,
                      tile_gate_illum=tile_gate_illum, tile_gate_max_gain=tile_gate_max_gain, sightings=sightings, sight_window=sight_window,
                      sight_min_hits=sight_min_hits, sight_mismatch=sight_mismatch, sight_cost=sight_cost,
                      save_jpeg=save_jpeg, overlay=overlay, overlay_font=overlay_font, overlay_size=overlay_size,
                      overlay_thickness=overlay_thickness, overlay_alpha=tuple(overlay_alpha), zones=zones,
                      zones_min_hits=zones_min_hits, speed=speed, speed_min_hits=speed_min_hits, speed_confirm=speed_confirm,
                      overlay_scene=overlay_scene, watch_indel=watch_indel, watch_gap_cost=watch_gap_cost).infer(
        conf_thres, iou_thres, classes, agnostic_nms, max_det, out_dir, save_txt, save_img, hide_labels, hide_conf, view_img,
        save_crops=save_crops, crop_size=tuple(crop_size))
    if save_txt or save_img or save_crops:
        LOGGER.info(f"Results saved to {out_dir}")
    return results


def main(args):
    run(**vars(args))


if __name__ == "__main__":
    main(get_args_parser())
