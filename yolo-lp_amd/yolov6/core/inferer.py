"""``Inferer``: the per-image inference driver (host-side mirror of reference
yolov6/core/inferer.py:25-245).

The hot core -- ``model(img)`` then ``non_max_suppression`` (reference :80-83) --
runs on the HIP engine when the device is a GPU.  Weight preparation keeps the
reference's order: checkpoint -> float -> fuse_model -> eval -> switch_to_deploy
-> half.  Detections are rescaled to the source image, rounded, and written as
label lines ``cls*8 xywh(normalised) corners(normalised)`` (reference :100-120).
Drawing / video writing are cv2 GUI plumbing outside the hot-path scope: boxes and
corner polygons are drawn with PIL when images are saved, labels are not rendered.
With ``save_crops`` every detection's plate is also cut out along its four corners as
an upright image (``runtime.plate_crops`` on a GPU, ``plate_crops_np`` on the CPU).
With ``tile`` every frame is detected by overlapping tiles of that size plus an overview of the whole frame, merged per
frame (``runtime.detect_tiled`` on a GPU; per-tile inference and ``merge_tiles_np`` on the CPU): for frames much larger
than the network input, whose plates a single letterbox would shrink away.
With ``track`` the detections of consecutive frames are associated into plate tracks and every track votes its eight
characters over its frames (``runtime.PlateTracker`` on a GPU, ``PlateTrackerNp`` on the CPU): ``infer`` returns and saves the
voted rows and writes ``tracks.txt`` (one line per frame row) and ``plates.txt`` (one line per track).
With ``best_shots`` every track also keeps the sharpest rectified crop it has shown (``PlateTracker.update_with_shots`` on a GPU,
``BestShotNp`` on the CPU): ``shots/<line>_<id>.png`` and ``shots.txt``, line-parallel to ``plates.txt``.
With ``stack_shots`` every track's rectified crops are also aligned and averaged into one denoised picture
(``PlateTracker.enable_stack`` on a GPU, ``StackNp`` on the CPU): ``stacks/<line>_<id>.png`` and ``stacks.txt``.
With ``nv12`` the frames travel as NV12 (``yolov6.utils.nv12``): decoded images are encoded on the host as a stand-in for a
video decoder, ``.nv12`` sources are raw streams of packed frames; on a GPU the planes are uploaded (half the bytes of BGR) and
read by the fused letterbox, a BGR frame exists on the device only where crops are cut; on the CPU every frame goes through
``nv12_to_bgr_np`` into the existing path.
With ``redact`` every detection's plate is made unreadable in the frame itself, by a mosaic, a fill or a Gaussian blur (``runtime.redact_plates`` on a
GPU, in place on the device frames and behind everything that reads them; ``redact_plates_np`` on the CPU), and the frame is
written to ``<save_dir>/redacted/``.  NV12 frames are redacted as NV12 and converted only to be saved.
With ``redact_lookback`` = D every frame is redacted D frames late, so that the frames before a plate's first detection are
covered too (``runtime.LookbackRedactor`` on a GPU, ``LookbackNp`` on the CPU; ``yolov6.utils.lookback`` states the rule).
With ``tile`` and ``tile_gate`` the source is taken as one fixed camera: a tile whose pixels have not changed since it was last
detected is not run through the network again, its rows come from a cache (``runtime.TileGate`` on a GPU, ``TileGateNp`` on the
CPU; ``yolov6.utils.tile_gate`` states the rule).
With ``overlay`` every frame is also written with its rows drawn on it -- box, corner quad, a label with the track id and the eight
characters -- to ``<save_dir>/annotated/`` (``runtime.draw_plates`` on a clone of the device frame on a GPU, ``draw_plates_np`` on
the CPU; ``yolov6.utils.overlay`` states the rule); ``save_annotated`` and the images of ``save_img`` are what they are without it.
"""
import math
import os
import os.path as osp
import time
from collections import deque

import numpy as np
import torch

from yolov6.utils.events import LOGGER, load_yaml
from yolov6.layers.common import DetectBackend
from yolov6.data.data_augment import letterbox
from yolov6.data.datasets import LoadData
from yolov6.utils.nms import non_max_suppression
from yolov6.utils.nv12 import MATRICES, Nv12Frame, bgr_to_nv12_np, nv12_to_bgr_np


class Inferer:
    JPEG_RESTART = 16       # MCUs per restart interval of the files ``save_jpeg`` writes

    def __init__(self, source, weights, device, yaml, img_size, half, batch_size=1, auto=True, tile=None, tile_overlap=0.2,
                 tile_overview=True, merge_metric='iou', track=False, track_max_age=5, track_iou=0.3, track_expand=0.5, best_shots=False,
                 nv12=None, nv12_size=None, redact=None, redact_cell=16, redact_margin=0.1, redact_hold=False, redact_hold_min_hits=1,
                 redact_lookback=None, redact_lookback_max_back=None, redact_sigma=8.0, watchlist=None, watch_mismatch=1, watch_cost=None,
                 watch_confusable=None, watch_confusable_weight=4, watch_live=False, watch_live_min_hits=3, tile_gate=False, tile_gate_thres=2.0,
                 tile_gate_min_cells=1, tile_gate_refresh=50, tile_gate_illum='none', tile_gate_max_gain=1.5, stack_shots=False,
                 stack_search=2, stack_max_frames=64, stack_min_width=0.0, sightings=None, sight_window=None, sight_min_hits=1,
                 sight_mismatch=1, sight_cost=None, save_jpeg=None, overlay=False, overlay_font=None, overlay_size=24, overlay_thickness=2,
                 overlay_alpha=(256, 160, 256), zones=None, zones_min_hits=1, speed=None, speed_min_hits=1, speed_confirm=2, overlay_scene=False,
                 watch_indel=False, watch_gap_cost=1.0):
        """``batch_size > 1`` on a GPU runs consecutive frames of one letterboxed shape as one batch (``_gpu_groups``);
        ``auto=False`` letterboxes every frame to exactly ``img_size`` (the reference pads to the next stride multiple).
        ``tile`` = (h, w): tiled detection (``_gpu_groups``; ``tiled_rows_cpu`` on the CPU) with ``tile_overlap`` (pixels, or a fraction < 1 of the tile),
        the whole frame as one more tile with ``tile_overview``, and the cross-tile merge by ``merge_metric`` ('iou' / 'ios');
        ``batch_size`` is then the number of tiles per forward.
        ``track``: plate tracking with a per-track character vote (``yolov6.utils.track`` states the rules): every video file is
        one stream, all image files of the source, in ``LoadData``'s order, are one more; a row continues the track whose
        predicted box (grown by ``track_expand`` of its size) it overlaps by more than ``track_iou``, a track unseen for more
        than ``track_max_age`` frames ends.
        ``best_shots`` (with ``track``): every track keeps the sharpest plate crop among the first ``SHOT_ROWS`` rows of its
        frames (``yolov6.utils.best_shot`` states the rules); ``infer`` writes one image per ended track that has one.
        ``stack_shots`` (with ``best_shots``): the rectified crops of a track, at most ``stack_max_frames`` of them, each from a
        plate at least ``stack_min_width`` frame pixels wide, are aligned by an integer shift of at most ``stack_search`` pixels and
        averaged (``yolov6.utils.stack`` states the rule and what it does not do); ``infer`` writes one more image per ended track.
        ``nv12`` = 'bt601' | 'bt709' | 'bt601f' | 'bt709f': send every frame as NV12 with that matrix (decoded images are encoded
        with ``bgr_to_nv12_np``, an odd last row or column cut off as a decoder would never deliver one); ``nv12_size`` = (w, h)
        of the frames of ``.nv12`` sources, which need ``nv12``.
        ``redact`` = 'mosaic' | 'fill' (black) | 'gauss': ``infer`` also writes every frame with the plates of its detections made
        unreadable (``yolov6.utils.redact`` states the rules): the quad of every row, grown by ``redact_margin`` of its size about
        its centre, in cells of ``redact_cell`` pixels (mosaic) or under a Gaussian of ``redact_sigma`` pixels, 0.5..16 (gauss).
        ``redact_hold`` (with ``track`` and ``redact``): a plate that is being tracked stays redacted in the frames in which
        the detector misses it, at the box and corners its track predicts, until the track ends (rule 11 of
        ``yolov6.utils.track``); a track needs ``redact_hold_min_hits`` detections before it is held.  The rows returned and
        saved, the crops, ``tracks.txt`` and ``plates.txt`` are what they are without it.
        ``redact_lookback`` = D in 1..32 (with ``track``, ``redact`` and ``redact_hold``): redaction is delayed by D frames per
        stream, and once a new track's second detection has fixed its velocity the frames still inside the delay also get a row
        for it, at most ``redact_lookback_max_back`` (default D) frames before its first detection (``yolov6.utils.lookback``).
        ``redacted/<image name>`` is written when the frame leaves the delay, the rest at the end of the source; every other
        output is what it is without it.
        ``watchlist`` = the path of a watchlist file (with ``track``; ``yolov6.utils.watch`` states the rule and
        ``parse_watchlist`` the format): the read of every ended track is looked up in it, tolerating ``watch_mismatch`` misread
        positions of a total cost of at most ``watch_cost`` fully confident mismatches (None: no limit); ``watch_confusable`` =
        pairs of characters of the ``ads`` names (``'0D 0Q 8B 2Z 5S'``) that cost only ``watch_confusable_weight`` sixteenths of a
        mismatch.  ``infer`` writes ``hits.txt`` beside ``plates.txt``; every other output is what it is without it.
        ``watch_live`` (with ``watchlist``): a track is also looked up while it is still live, as soon as it has
        ``watch_live_min_hits`` detections and again whenever its voted read changes (``yolov6.utils.watch_live`` states the rule;
        the limits are those of ``watchlist``); ``infer`` writes ``alerts.txt``.
        ``watch_indel`` (with ``watchlist``): both lookups also tolerate one lost or gained character in heads 2..7, charged
        ``watch_gap_cost`` fully confident mismatches and counted as one mismatch; ``hits.txt`` and ``alerts.txt`` then end in one
        more column, the alignment: ``-``, ``del@k``, ``ins@k`` or ``end`` (``watch.align_text``).
        ``sightings`` = C (with ``track``; ``yolov6.utils.sight`` states the rule): a log of the last C reads of all streams; the
        read of every ended track of at least ``sight_min_hits`` detections is matched against the reads logged at most
        ``sight_window`` frames of the source earlier (None: no limit), tolerating ``sight_mismatch`` misread positions of a total
        cost of at most ``sight_cost`` fully confident mismatches (None: no limit; ``watch_confusable`` is shared), and is then
        logged itself: a track broken by an occlusion names its first part, a vehicle on a second video its pass on the first.
        ``infer`` writes ``resightings.txt``; every other output is what it is without it.
        ``tile_gate`` (with ``tile``): the whole source is ONE fixed-camera stream, every frame of the size of the first (another
        size raises); a tile is run through the network only when a 16 x 16 cell of it has changed by more than ``tile_gate_thres``
        luma levels per pixel (in at least ``tile_gate_min_cells`` cells) since the tile was last detected, or every
        ``tile_gate_refresh`` frames (0: never); the other tiles keep their rows.  Tile groups are then one frame per call.
        ``tile_gate_illum='gain'`` compares the cells after the tile's reference is scaled by one gain per tile (the median of its
        cells' gains), so an exposure step or a cloud does not re-detect everything; a gain outside
        [1 / ``tile_gate_max_gain``, ``tile_gate_max_gain``] does.
        ``save_jpeg`` = Q in 1..100: the redacted frames, the crops of ``save_crops``, the shots and the stacks are written as
        baseline JPEG files ``.jpg`` of that quality instead of PNG (``yolov6.utils.jpeg`` states the format): on a GPU by
        ``runtime.encode_jpeg``, from the device frames where they are there, on the CPU by ``encode_jpeg_np``, the same bytes.
        ``shots.txt`` and ``stacks.txt`` name the ``.jpg`` files; everything else is what it is without it.
        ``overlay``: ``infer`` also writes every frame with its detections drawn on it -- box, corner quad and a label with the
        track id (with ``track``) and the eight characters (the voted read with ``track``) -- as ``annotated/<image name>``
        (``annotated/<stem>.jpg`` with ``save_jpeg``; ``yolov6.utils.overlay`` states the rules).  On a GPU the drawing is
        ``runtime.draw_plates`` on a clone of the device frame, behind the redaction where that is on, so outlines sit on a
        mosaic and the group's other consumers see the frame without them; on the CPU ``draw_plates_np``, the same bytes.  The glyphs are
        rendered once on the host from the yaml's names at ``overlay_size`` pixels with the TrueType file ``overlay_font`` (None:
        PIL's default font, which has no CJK glyphs: the province then shows '?'); ``overlay_thickness`` is the outlines' width
        (0..16), ``overlay_alpha`` the opacities 0..256 of outlines, label plate and text.  With ``redact_hold`` the predicted rows
        of missed tracks are drawn in a second style.  Not with ``redact_lookback`` (the frame drawn on would not be redacted yet).
        ``zones`` = the path of a file of lines and zones (with ``track``; ``yolov6.utils.zones`` states the rule and ``parse_zones``
        the format; a stream prefix names the tracker's stream: 0 = the image files, 1 + k = the k-th video): the live tracks of at
        least ``zones_min_hits`` detections are tested against them after every tracker call; ``infer`` writes ``crossings.txt`` and
        ``zones.txt`` and logs the totals per line; every other output is what it is without it.
        ``speed`` = the path of a calibration file (with ``track``; ``yolov6.utils.speed`` states the rule and ``parse_ground`` the
        format, stream prefixes as for ``zones``): a homography from frame pixels to metres on the plane the plates move in, the frame
        rate and a limit per stream.  The live tracks of at least ``speed_min_hits`` detections are measured after every tracker call;
        ``infer`` writes ``speeds.txt`` (``id text peak_kmh chord_kmh`` per ended track with at least two samples) and
        ``speeding.txt`` (``frame id text kmh limit_kmh`` for a track over the limit for ``speed_confirm`` estimates in a row, at the
        frame it fired); every other output is what it is without it.
        ``overlay_scene`` (with ``overlay`` and ``zones`` and/or ``speed``): the scene is drawn onto the annotated frames before the
        plates -- zones as a translucent fill plus an outline, lines with a marker on their +1 side, their names with the running
        totals and occupancies, the alert colour while a dwell alert fires, a km/h tag beside every plate with a speed estimate
        (``runtime.draw_scene`` on a GPU, ``draw_scene_np`` on the CPU; ``yolov6.utils.scene`` states the rule and what it does not
        do).  Without it every output file is what it is today."""
        self.__dict__.update(locals())
        self._overlay = None
        if overlay:
            if redact_lookback is not None:
                raise ValueError('overlay does not go with redact_lookback: the frame is redacted frames later')
            self._overlay_styles = self.make_overlay_styles(overlay_size, overlay_thickness, overlay_alpha)
        if overlay_scene and not (overlay and (zones is not None or speed is not None)):
            raise ValueError('overlay_scene needs overlay=True and zones=FILE and/or speed=FILE')
        if save_jpeg is not None:
            from yolov6.utils.jpeg import check_params as check_jpeg
            self.save_jpeg = check_jpeg(save_jpeg, self.JPEG_RESTART, device=True)[0]
        if tile_gate:
            from yolov6.utils.tile_gate import check_illum, check_params as check_gate
            if tile is None:
                raise ValueError('tile_gate needs tile=(H, W)')
            check_gate(tile_gate_thres, tile_gate_min_cells, tile_gate_refresh)
            check_illum(tile_gate_illum, tile_gate_max_gain)
        self._gate = None
        if watchlist is not None:
            from yolov6.utils.watch import check_params, cost_units
            if not track:
                raise ValueError('watchlist needs track=True')
            check_params(watch_mismatch, cost_units(watch_cost))
        if watch_indel:
            from yolov6.utils.watch import gap_units
            if watchlist is None:
                raise ValueError('watch_indel needs watchlist=FILE')
            gap_units(watch_gap_cost)
        if sightings is not None:
            from yolov6.utils.sight import check_call, check_log
            from yolov6.utils.watch import check_params, cost_units
            if not track:
                raise ValueError('sightings needs track=True')
            check_log(sightings, 1)
            check_call(0, 0 if sight_window is None else sight_window, sight_min_hits)
            check_params(sight_mismatch, cost_units(sight_cost))
        if zones is not None:
            from yolov6.utils.watch_live import check_min_hits
            if not track:
                raise ValueError('zones needs track=True')
            check_min_hits(zones_min_hits)
        if speed is not None:
            from yolov6.utils.speed import check_confirm
            from yolov6.utils.watch_live import check_min_hits
            if not track:
                raise ValueError('speed needs track=True')
            check_min_hits(speed_min_hits)
            check_confirm(speed_confirm)
        if watch_live:
            from yolov6.utils.watch_live import check_min_hits
            if watchlist is None:
                raise ValueError('watch_live needs watchlist=FILE')
            check_min_hits(watch_live_min_hits)
        if redact is not None:
            from yolov6.utils.redact import check_params, check_sigma
            if check_params(redact, redact_cell, redact_margin)[0] == 2:
                self.redact_sigma = check_sigma(redact_sigma)
        if redact_hold and not (track and redact is not None):
            raise ValueError('redact_hold needs track=True and redact=MODE')
        if redact_lookback is not None:
            from yolov6.utils.lookback import check_lookback
            if not (track and redact is not None and redact_hold):
                raise ValueError('redact_lookback needs track=True, redact=MODE and redact_hold=True')
            check_lookback(self.TRACK_SLOTS, redact_lookback, redact_lookback_max_back, None)
        if redact_hold and int(redact_hold_min_hits) < 1:
            raise ValueError('redact_hold_min_hits must be >= 1')
        if best_shots and not track:
            raise ValueError('best_shots needs track=True')
        if stack_shots:
            from yolov6.utils.stack import check_params as check_stack
            if not best_shots:
                raise ValueError('stack_shots needs best_shots=True')
            check_stack(stack_search, stack_max_frames, stack_min_width)
        if merge_metric not in ('iou', 'ios'):
            raise ValueError("merge_metric must be 'iou' or 'ios'")
        if nv12 is not None and nv12 not in MATRICES:
            raise ValueError('nv12 must be one of %s' % ', '.join(sorted(MATRICES)))
        self.nv12_size = None if nv12_size is None else (int(nv12_size[0]), int(nv12_size[1]))
        self.tile = None if tile is None else ((int(tile), int(tile)) if isinstance(tile, int) else (int(tile[0]), int(tile[-1])))
        if int(batch_size) < 1:
            raise ValueError('batch_size must be >= 1')
        self.batch_size = int(batch_size)
        self.device = device
        self.img_size = img_size
        cuda = self.device != 'cpu' and torch.cuda.is_available()
        self.device = torch.device(f'cuda:{device}' if cuda else 'cpu')
        self.model = DetectBackend(weights, device=self.device)
        self.stride = self.model.stride
        names = load_yaml(yaml) if yaml else {}
        self.pro_names = names.get('names')
        self.alp_names = names.get('alps')
        self.ads_names = names.get('ads')
        if overlay:
            from yolov6.utils.overlay import build_atlas
            self._overlay = build_atlas(self.pro_names or [], self.alp_names or [], self.ads_names or [], overlay_size, overlay_font)
            self._overlay_dev = None        # runtime.OverlayFont: uploaded with the first group
        self._scene = None
        if overlay_scene:
            from yolov6.utils.scene import build_scene_atlas
            self._scene = build_scene_atlas(overlay_size, overlay_font)
            self._scene_style = self.make_scene_style(overlay_size, overlay_thickness, overlay_alpha)
            self._scene_dev = None          # (runtime.SceneFont, names on the device): uploaded with the first group
        self.img_size = self.check_img_size(self.img_size, s=self.stride)
        self.half = half

        self.model_switch(self.model.model, self.img_size)
        if self.half & (self.device.type != 'cpu'):
            self.model.model.half()
        else:
            self.model.model.float()
            self.half = False
        if self.device.type != 'cpu':   # warm-up: builds the engine and tunes it for this shape
            self.model.model.lp_graph = True      # per-image loop = launch-bound: replay the forward as one hipGraph
            self.model(torch.zeros(1, 3, *self.img_size).to(self.device).type_as(next(self.model.model.parameters())))
        self.files = LoadData(source, nv12_size=self.nv12_size, nv12_matrix=nv12, nv12_chunk=self.batch_size)
        if nv12 is None and any(p.lower().endswith('.nv12') for p in self.files.files):
            raise ValueError('.nv12 sources need nv12=MATRIX (--nv12 MATRIX) and their frame size')
        self.source = source

    def model_switch(self, model, img_size):
        """Collapse every RepVGGBlock to its single 3x3 conv."""
        from yolov6.layers.common import RepVGGBlock
        for layer in model.modules():
            if isinstance(layer, RepVGGBlock):
                layer.switch_to_deploy()
        LOGGER.info("Switch model to deploy modality.")

    def infer(self, conf_thres, iou_thres, classes, agnostic_nms, max_det, save_dir, save_txt, save_img, hide_labels,
              hide_conf, view_img=True, save_crops=False, crop_size=(64, 192)):
        """Run every source image through model + NMS; returns the list of rescaled ``[n, 28]`` detections.  ``save_crops``:
        also write the plate crop (``crop_size`` = (h, w)) of detection k of an image as ``<save_dir>/<rel>/crops/<stem>_<k>.png``
        (RGB; k is the line of the detection in ``<stem>.txt``).

        The frames come in groups of ``(items, dets, crops or None, seconds)`` -- ``items`` = [(frame, path)], ``seconds`` the
        timed model + NMS window of the group -- from ``_per_image`` (groups of one) or, on a GPU with ``tile`` or
        ``batch_size > 1``, from ``_gpu_groups``; every path writes and returns per frame, in source order, the same things.

        With ``track`` the rows returned and saved are the voted ones (the class columns of a tracked row replaced by its
        track's read: columns 12..19 the vote shares, 20..27 the voted ids; the geometry is unchanged), and two files are
        written: ``<save_dir>/tracks.txt``, one line ``path row track_id`` per frame row (-1: untracked), and
        ``<save_dir>/plates.txt``, one line ``id first last hits text share_0..7`` per ended track (all streams are flushed
        at the end; ids count per stream).

        With ``best_shots`` the sharpest crop (``crop_size``) of line k of ``plates.txt`` is written as
        ``<save_dir>/shots/<k>_<id>.png`` (RGB), and ``<save_dir>/shots.txt`` has one line ``id frame row status sharpness file``
        per line of ``plates.txt``: the stream's frame index and the row the shot was cut from, the crop's status (1 corners,
        2 box) and its Laplacian energy; a track without a shot has ``id 0 0 0 0 -``.

        With ``stack_shots`` the average of the aligned rectified crops of line k is written as ``<save_dir>/stacks/<k>_<id>.png``
        (RGB), and ``<save_dir>/stacks.txt`` has one line ``id n first last file`` per line of ``plates.txt``: the crops averaged
        and the stream's frame index of the first and the last of them; a track without a stack has ``id 0 0 0 -``.

        With ``watchlist`` ``<save_dir>/hits.txt`` has one line ``id first last text entry entry_text mismatches cost n_hits`` per
        ended track whose read an entry of the list accepts: the line of ``plates.txt`` up to the text, the index and text of the
        accepted entry of the smallest (cost, index), its two sums, and the number of accepted entries (above 1: ambiguous).
        With ``watch_live`` ``<save_dir>/alerts.txt`` has one line ``frame id text entry entry_text mismatches cost n_hits hits``
        per alert, in the order they fired: the stream frame of the detection that caused the lookup, the track's id and read at
        that moment, the accepted entry as in ``hits.txt``, and the detections the track had.

        With ``sightings`` ``<save_dir>/resightings.txt`` has one line ``id first last text prev_stream prev_id prev_stamp now
        mismatches cost n_hits`` per ended track with an earlier sighting: the line of ``plates.txt`` up to the text, the stream,
        track id and stamp of the best earlier sighting (the smallest (cost, age)), the stamp of this one, the two sums and the
        number of earlier sightings accepted.  A stamp is the number of the source's frame whose update ended the track (of the
        last frame of a batch; the number of frames for the final flush), counted over the whole source.

        With ``redact`` every frame is also written, its plates redacted along the rows returned, as
        ``<save_dir>/redacted/<image name>`` (``.png`` for a frame of a video or a raw stream).

        With ``save_jpeg`` the redacted frames (``redacted/<stem>.jpg``), the crops, the shots and the stacks are ``.jpg`` files of
        the same stems, and ``shots.txt`` / ``stacks.txt`` name those.

        With ``overlay`` every frame is also written with its rows drawn on it as ``<save_dir>/annotated/<image name>``
        (``annotated/<stem>.jpg`` with ``save_jpeg``)."""
        self._redacted = deque()
        self._annotated = deque()
        self._gate = None       # with tile_gate: made at the first frame
        self._gate_gains = []   # with tile_gate_illum='gain': the smallest and largest estimated gain so far (Q12)
        if self.track:
            self._track_begin(crop_size)
        if self.device.type != 'cpu' and (self.tile is not None or self.batch_size > 1 or self.nv12 is not None):
            groups = self._gpu_groups(conf_thres, iou_thres, max_det, save_crops, crop_size)
        else:
            groups = self._per_image(conf_thres, iou_thres, classes, agnostic_nms, max_det, save_crops, crop_size)
        fps = CalcFPS()
        results = []
        for items, dets, crops, seconds in groups:
            for _ in items:     # the FPS figure is per frame (group time / frames in the group)
                fps.update(len(items) / max(seconds, 1e-9))
            for k, ((img_src, img_path), det) in enumerate(zip(items, dets)):
                self.save_outputs(img_src, img_path, det, save_dir, save_txt, save_img)
                if save_crops and len(det):
                    self.write_crops(img_path, crops[k], save_dir)
                results.append(det)
                if self.redact is not None and self.redact_lookback is None:
                    self.write_redacted(img_path, self._redacted.popleft(), save_dir)
                if self._overlay is not None:
                    self.write_redacted(img_path, self._annotated.popleft(), save_dir, 'annotated')
                if self.track:
                    self._track_lines += ['%s %d %d' % (img_path, r, t) for r, t in enumerate(self._track_tids.popleft().tolist())]
            self._write_delayed(save_dir)
        if self.track:
            self._track_finish(save_dir)
            if self.redact_lookback is not None:        # right behind the tracker's flush: the frames still inside the delay
                self._lookback_collect(self._lookback.flush_all())
                self._write_delayed(save_dir)
        if self._gate is not None:
            st = self._gate.stats
            gains = ''
            if self.tile_gate_illum == 'gain':
                gains = '; no gain estimated' if not self._gate_gains else '; gain %.3f..%.3f, %d tiles out of range' % (
                    self._gate_gains[0] / 4096.0, self._gate_gains[1] / 4096.0, st['tiles_out_of_range'])
            LOGGER.info('Tile gate: %d of %d tiles detected (%d calls, %d forwards)%s' % (st['tiles_detected'], st['tiles_seen'], st['calls'],
                                                                                         st['forwards'], gains))
        LOGGER.info('Average model+NMS rate: %.1f FPS' % fps.accumulate())
        return results

    def _per_image(self, conf_thres, iou_thres, classes, agnostic_nms, max_det, save_crops, crop_size):
        """One frame per group: the reference's loop (on a GPU through the HIP letterbox / detect / rescale kernels), or with
        ``tile`` on the CPU every tile through the torch model and ``merge_tiles_np`` (``tiled_rows_cpu``).  The timed window
        is model + NMS alone, not the letterbox or the rescale."""
        gpu = self.device.type != 'cpu'
        if gpu:
            from yolov6.hip import runtime
        for img_src, img_path, _ in self.files:
            img_nv12 = None
            if self.nv12 is not None:       # (CPU only: a GPU takes NV12 through _gpu_groups) NV12 in, nv12_to_bgr_np, the existing path
                img_nv12 = self._as_nv12(img_src)
                img_src = nv12_to_bgr_np(img_nv12)
            if gpu:      # letterbox + BGR->RGB + /255 in one HIP kernel on the uploaded frame
                frame = torch.from_numpy(np.ascontiguousarray(img_src)).to(self.device)
                img = runtime.preprocess_letterbox(frame, self.img_size, self.stride,
                                                   torch.float16 if self.half else torch.float32, auto=self.auto)[None]
                runtime.prepare_for(self.model.model, img.shape, img.dtype)   # a new frame shape runs the kernel-variant tuner once: outside the FPS window
            elif self.tile is None:
                img, img_src = self.precess_image(img_src, self.img_size, self.stride, self.half, auto=self.auto)
                img = img.to(self.device)[None]
            t1 = time.time()
            if gpu:
                # model(img) -> non_max_suppression (reference :80-83) as one call: the detections-only forward, or forward +
                # lp_nms when most anchors pass the mask (runtime.Engine.detect) -- the same detections bit for bit either way
                det = runtime.detect(self.model.model, img, conf_thres, iou_thres, max_det)[0]
            elif self.tile is None:
                det = non_max_suppression(self.model(img), conf_thres, iou_thres, classes, agnostic_nms, max_det=max_det)[0]
            elif self.tile_gate:
                det = self.gated_rows_cpu(img_src, conf_thres, iou_thres, classes, agnostic_nms, max_det)
            else:
                det = self.tiled_rows_cpu(img_src, conf_thres, iou_thres, classes, agnostic_nms, max_det)
            seconds = time.time() - t1
            if len(det) and gpu:
                runtime.rescale_round(img.shape[2:], det, img_src.shape)
            elif len(det) and self.tile is None:      # (tiled_rows_cpu returns frame pixels)
                det[:, :12] = self.rescale(img.shape[2:], det[:, :12], img_src.shape).round()
            if self.track:
                det = self._track_frame(det, img_path, max_det, frame if gpu else img_src)
            crops = None
            if save_crops and len(det):
                if gpu:     # the uploaded frame and its detections are on the device: crop there
                    count = torch.tensor([len(det)], dtype=torch.int32, device=self.device)
                    crops, _ = runtime.plate_crops([frame], det[None], count, crop_size, max_crops=len(det))
                else:
                    from yolov6.utils.plate_crop import plate_crops_np
                    crops = [plate_crops_np(img_src, det.detach().float().cpu().numpy(), crop_size)[0]]
            self._redact_group([img_src if img_nv12 is None else img_nv12], [det], [frame] if gpu else None)     # last: it writes the frame
            self._overlay_group([img_src if img_nv12 is None else img_nv12], [det], [frame] if gpu else None)
            yield [(img_src, img_path)], [det], crops, seconds

    def _gpu_groups(self, conf_thres, iou_thres, max_det, save_crops, crop_size):
        """Several frames per group on a GPU.  Image files are decoded on a small thread pool ahead of the GPU and each group
        is uploaded with one copy from pinned memory (``FrameBatcher``).  Without ``tile``: consecutive frames of one
        letterboxed shape (``plan_batches``) go through ``runtime.detect_frames`` together, a short group padded to the bound
        batch size so that the engine is never set up for a new one.  With ``tile``: consecutive frames are grouped until
        their tiles fill a forward of ``batch_size`` tiles (at least one frame per group) and run through
        ``runtime.detect_tiled``.  The timed window is the upload through the runtime call (``..._with_crops`` with
        ``save_crops``: the crops of every detection are enqueued before the next put reuses the frames' buffer)."""
        from yolov6.hip import runtime
        from yolov6.core.frames import FrameBatcher, letterbox_hw, plan_batches, prefetch_frames
        from yolov6.core.tiles import plan_tiles
        from yolov6.data.datasets import imread_bgr
        B, dtype = self.batch_size, (torch.float16 if self.half else torch.float32)
        decode = imread_bgr if self.nv12 is None else (lambda p: self._as_nv12(imread_bgr(p)))     # the encoder runs on the pool too
        frames = ((self._as_nv12(f) if self.nv12 is not None else f, p) for f, p in self._frames_ahead(prefetch_frames, decode))

        def frame_groups():
            inputs = {}                     # (H, W) -> persistent [B,3,H,W] input buffer
            window = deque()
            while True:
                while len(window) < B:
                    nxt = next(frames, None)
                    if nxt is None:
                        break
                    window.append(nxt)
                if not window:
                    return
                group = plan_batches([f.shape for f, _ in window], self.img_size, self.stride, B, self.auto)[0]
                items = [window.popleft() for _ in group]
                H, W = letterbox_hw(items[0][0].shape, self.img_size, self.stride, self.auto)
                x = inputs.get((H, W))
                if x is None:
                    x = inputs[(H, W)] = torch.empty(B, 3, H, W, dtype=dtype, device=self.device)
                runtime.prepare_for(self.model.model, x.shape, dtype)      # a new shape tunes once: outside the FPS window
                yield items, dict(auto=self.auto, batch=B, out=x)

        def tile_groups():
            runtime.prepare_for(self.model.model, (B, 3, *self.img_size), dtype)
            kw = dict(tile_hw=self.tile, overlap=self.tile_overlap, overview=self.tile_overview, metric=self.merge_metric, batch=B)
            pending = next(frames, None)
            while pending is not None:
                items, n_tiles = [], 0
                while pending is not None:
                    k = len(plan_tiles(pending[0].shape, self.tile, self.tile_overlap, self.tile_overview))
                    if items and (n_tiles + k > B or self.tile_gate):      # the gate takes one frame of a stream per call
                        break
                    items.append(pending)
                    n_tiles += k
                    pending = next(frames, None)
                yield items, kw

        def gate_padded(model, dev_frames, img_size, conf, iou, mdet, **kw):
            """``detect_tiled_padded`` through the gate (made at the first frame, whose size is the stream's); copies, since the
            gate's outputs are persistent."""
            if self._gate is None:
                self._gate = runtime.TileGate(model, [tuple(dev_frames[0].shape[:2])], img_size, conf, iou, mdet, thres=self.tile_gate_thres,
                                              min_cells=self.tile_gate_min_cells, refresh=self.tile_gate_refresh, illum=self.tile_gate_illum,
                                              max_gain=self.tile_gate_max_gain, **kw)
            self._gate_check_shape(dev_frames[0].shape, self._gate.shapes[0])
            det, count = self._gate.detect_padded(dev_frames)
            self._gate_note_gains()
            return det.clone(), count.clone()

        def gate_detect(*a, **kw):
            det, count = gate_padded(*a, **kw)
            return runtime._unpad(det, count.cpu().tolist())

        def gate_with_crops(model, dev_frames, img_size, conf, iou, mdet, crop_hw, **kw):
            det, count = gate_padded(model, dev_frames, img_size, conf, iou, mdet, **kw)
            return runtime._unpad_with_crops(dev_frames, det, count, runtime._crop_size(crop_hw))

        if self.tile is None:
            groups, detect, detect_with_crops = frame_groups(), runtime.detect_frames, runtime.detect_frames_with_crops
            padded = runtime.detect_frames_padded
        elif self.tile_gate:
            groups, detect, detect_with_crops, padded = tile_groups(), gate_detect, gate_with_crops, gate_padded
        else:
            groups, detect, detect_with_crops = tile_groups(), runtime.detect_tiled, runtime.detect_tiled_with_crops
            padded = runtime.detect_tiled_padded
        batcher = FrameBatcher(self.device)
        for items, kw in groups:
            t1 = time.time()
            dev_frames = batcher.put([f for f, _ in items])
            if self.track:      # detect -> track -> (crops) enqueued back to back on the device, then the host reads
                det, count = padded(self.model.model, dev_frames, self.img_size, conf_thres, iou_thres, max_det, **kw)
                det, tid = self._track_update(det, count, [p for _, p in items], dev_frames)
                if save_crops:
                    dets, crops, _ = runtime._unpad_with_crops(dev_frames, det, count, runtime._crop_size(crop_size))
                else:
                    dets, crops = runtime._unpad(det, count.cpu().tolist(), len(items)), None
                self._track_tids.extend(tid[k, :len(d)].cpu().numpy() for k, d in enumerate(dets))
            elif save_crops:
                dets, crops, _ = detect_with_crops(self.model.model, dev_frames, self.img_size, conf_thres, iou_thres, max_det,
                                                   crop_size, **kw)
            else:
                dets, crops = detect(self.model.model, dev_frames, self.img_size, conf_thres, iou_thres, max_det, **kw), None
            self._redact_group([f for f, _ in items], dets, dev_frames)     # behind the crops and the shots, before the next put
            self._overlay_group([f for f, _ in items], dets, dev_frames, (det, count, tid) if self.track else None)    # behind the redaction, on clones
            yield items, dets, crops, time.time() - t1

    def tiled_rows_cpu(self, img_src, conf_thres, iou_thres, classes, agnostic_nms, max_det, border=1):
        """Tiled detection of one BGR frame on the CPU: [n, 28] fp32 tensor in frame pixels.  Every tile of the plan is
        letterboxed to exactly ``img_size``, run through the model and the NMS, rescaled to tile pixels and rounded; then
        ``merge_tiles_np`` (threshold ``iou_thres``)."""
        from yolov6.core.tiles import plan_tiles
        from yolov6.utils.tiles import MAX_CANDIDATES, merge_tiles_np
        tiles = plan_tiles(img_src.shape, self.tile, self.tile_overlap, self.tile_overview)
        tmd = max(1, min(int(max_det), MAX_CANDIDATES // len(tiles)))
        det_t, count_t = self._tiles_cpu([img_src], [(0,) + t for t in tiles], tmd, conf_thres, iou_thres, classes, agnostic_nms)
        det, count, _ = merge_tiles_np(det_t, count_t, [(0,) + t for t in tiles], [img_src.shape], iou_thres, max_det,
                                       self.merge_metric, border)
        return torch.from_numpy(det[0, :int(count[0])].copy())

    def _tiles_cpu(self, frames, tiles, tmd, conf_thres, iou_thres, classes, agnostic_nms):
        """The per-tile half of ``tiled_rows_cpu``: (det_t [T, tmd, 28] fp32, count_t [T]) of the tiles (frame index, y0, x0, th, tw)
        of the BGR ``frames``, in tile pixels, rounded."""
        det_t = np.zeros((len(tiles), tmd, 28), np.float32)
        count_t = np.zeros(len(tiles), np.int32)
        for t, (f, y0, x0, th, tw) in enumerate(tiles):
            img_src = frames[f]
            region = np.ascontiguousarray(img_src[y0:y0 + th, x0:x0 + tw])
            img, _ = self.precess_image(region, self.img_size, self.stride, self.half, auto=False)
            img = img.to(self.device)[None]
            det = non_max_suppression(self.model(img), conf_thres, iou_thres, classes, agnostic_nms, max_det=tmd)[0]
            if len(det):
                det[:, :12] = self.rescale(img.shape[2:], det[:, :12], region.shape).round()
                det_t[t, :len(det)] = det.detach().float().cpu().numpy()
            count_t[t] = len(det)
        return det_t, count_t

    def gated_rows_cpu(self, img_src, conf_thres, iou_thres, classes, agnostic_nms, max_det, border=1):
        """``tiled_rows_cpu`` through ``TileGateNp`` (made at the first frame): the per-tile inference runs on the flagged tiles
        only."""
        if self._gate is None:
            from yolov6.utils.tile_gate import TileGateNp
            run = lambda frames, tiles, tmd: self._tiles_cpu(frames, tiles, tmd, conf_thres, iou_thres, classes, agnostic_nms)   # noqa: E731
            self._gate = TileGateNp(run, [img_src.shape[:2]], self.tile, iou_thres, max_det, self.tile_overlap, self.tile_overview,
                                    self.merge_metric, border, thres=self.tile_gate_thres, min_cells=self.tile_gate_min_cells,
                                    refresh=self.tile_gate_refresh, illum=self.tile_gate_illum, max_gain=self.tile_gate_max_gain)
        self._gate_check_shape(img_src.shape, self._gate.state.shapes[0])
        det = self._gate.detect([img_src])[0]
        self._gate_note_gains()
        return torch.from_numpy(det)

    def _gate_note_gains(self):
        """Keep the smallest and largest gain the gate has estimated (0 = no estimate) for the log line."""
        seen = [g for gn in self._gate.last_gain for g in gn if g]
        if seen:
            self._gate_gains = [min(seen + self._gate_gains[:1]), max(seen + self._gate_gains[1:])]

    @staticmethod
    def _gate_check_shape(shape, first):
        if tuple(shape[:2]) != tuple(first):
            raise ValueError('tile_gate (--tile-gate) takes the source as one fixed camera: a frame of %d x %d after frames of %d x %d'
                             % (shape[0], shape[1], first[0], first[1]))

    # ---- tracking (``track=True``) ---------------------------------------------------------------------------------------
    TRACK_SLOTS = 64        # tracks alive at once per stream
    SHOT_ROWS = 16          # with best_shots: the first rows of a frame (the NMS's order) whose crops compete

    def _track_begin(self, crop_size=(64, 192)):
        """A fresh tracker: stream 0 = the image files of the source, stream 1 + k = its k-th video file."""
        from yolov6.utils.track import PlateTrackerNp
        videos = [p for p in self.files.files if self.files.checkext(p) != 'image']
        self._track_streams = {p: 1 + k for k, p in enumerate(videos)}
        kw = dict(max_tracks=self.TRACK_SLOTS, match_thres=self.track_iou, new_thres=0.0, expand=self.track_expand,
                  max_age=self.track_max_age, ncls=self.model.model)
        if self.device.type != 'cpu':
            from yolov6.hip import runtime
            self._tracker = runtime.PlateTracker(1 + len(videos), device=self.device, **kw)
        else:
            self._tracker = PlateTrackerNp(1 + len(videos), **kw)
        self._track_tids, self._track_lines, self._track_ended, self._track_shots = deque(), [], [], []
        self._track_stacks = []         # with stack_shots: (stack_i line, crop or None) of every ended record
        self._track_hits = []           # with watchlist: the match_i line of every ended record
        self._track_hit_align = []      # with watch_indel: its alignment code
        self._track_alert_align = []    # with watch_indel and watch_live: the alignment code of every alert
        if self.watchlist is not None:
            from yolov6.utils import watch
            with open(self.watchlist) as f:
                entries = watch.parse_watchlist(f, self.pro_names, self.alp_names, self.ads_names)
            confuse = None
            if self.watch_confusable:
                confuse = watch.confuse_table(watch.confusable_pairs(self.watch_confusable), 2, self.watch_confusable_weight, self.ads_names)
            wl = runtime.Watchlist(entries, confuse, self.device) if self.device.type != 'cpu' else watch.WatchlistNp(entries, confuse)
            indel = dict(indel=1, gap_cost=self.watch_gap_cost) if self.watch_indel else {}
            self._tracker.enable_watch(wl, self.watch_mismatch, self.watch_cost, **indel)
            if self.watch_live:
                self._tracker.enable_live_watch(wl, self.watch_live_min_hits, self.watch_mismatch, self.watch_cost, **indel)
        self._track_sights = []         # with sightings: (sight_i line, now) of every ended record
        self._track_seen = 0            # frames of the source handed to the tracker so far
        if self.sightings is not None:
            from yolov6.utils import sight, watch
            confuse = None
            if self.watch_confusable:
                confuse = watch.confuse_table(watch.confusable_pairs(self.watch_confusable), 2, self.watch_confusable_weight, self.ads_names)
            make = runtime.SightLog if self.device.type != 'cpu' else sight.SightLogNp
            log = make(self.sightings, 1 + len(videos), confuse, device=self.device)
            window = (1 << 31) - 1 if self.sight_window is None else self.sight_window      # the largest int32: no limit
            self._tracker.enable_sightings(log, window, self.sight_min_hits, self.sight_mismatch, self.sight_cost)
        self._track_alerts = []         # with watch_live: (frame, id, best [8], entry, mismatches, cost, n_hits, hits) per alert
        self._track_zone_events = []    # with zones: (stream, kind, index, frame, id, best [8] or None, value) per event
        if self.zones is not None:
            from yolov6.utils import zones as zn
            lines, polys, self._zone_line_names, self._zone_names = zn.parse_zones(self.zones, 1 + len(videos))
            make = runtime.ZoneMap if self.device.type != 'cpu' else zn.ZoneMapNp
            self._scene_map = make(1 + len(videos), lines, polys, device=self.device)
            self._tracker.enable_zones(self._scene_map, self.zones_min_hits)
        elif self.overlay_scene:            # speed tags alone: a map without lines and zones
            from yolov6.utils import zones as zn
            self._scene_map = (runtime.ZoneMap if self.device.type != 'cpu' else zn.ZoneMapNp)(1 + len(videos), device=self.device)
            self._zone_line_names = self._zone_names = [[] for _ in range(1 + len(videos))]
        self._track_speed_events = []   # with speed: (kind, frame, id, best [8] or None, value, aux) per event
        if self.speed is not None:
            from yolov6.utils import speed as sp
            make = runtime.GroundPlane if self.device.type != 'cpu' else sp.GroundPlaneNp
            ground = make(1 + len(videos), sp.parse_ground(self.speed, 1 + len(videos)), device=self.device)
            self._tracker.enable_speed(ground, self.speed_min_hits, self.speed_confirm)
        if self.redact_hold:
            self._tracker.enable_hold(min_hits=self.redact_hold_min_hits)
        if self.redact_lookback is not None:
            kw = dict(max_back=self.redact_lookback_max_back, mode=self.redact, cell=self.redact_cell, margin=self.redact_margin,
                      sigma=self.redact_sigma)
            if self.device.type != 'cpu':
                self._lookback = runtime.LookbackRedactor(self._tracker, self.redact_lookback, **kw)
            else:
                from yolov6.utils.lookback import LookbackNp
                self._lookback = LookbackNp(self._tracker, self.redact_lookback, **kw)
            self._lookback_paths = [deque() for _ in range(1 + len(videos))]     # per stream: the paths of the frames inside the delay
        if self.best_shots:
            if self.device.type != 'cpu':
                self._tracker.enable_best_shot(crop_size, max_crops=self.SHOT_ROWS)
            else:
                from yolov6.utils.best_shot import BestShotNp
                self._gallery = BestShotNp(1 + len(videos), self.TRACK_SLOTS, crop_size)
        if self.stack_shots:
            kw = dict(search=self.stack_search, max_frames=self.stack_max_frames, min_width=self.stack_min_width)
            if self.device.type != 'cpu':
                self._tracker.enable_stack(**kw)
            else:
                self._tracker.enable_stack(crop_hw=crop_size, max_crops=self.SHOT_ROWS, **kw)

    def _track_collect(self, ended_i, ended_f, ended_count, shot_crops=None, shot_i=None, shot_q=None, shot_det=None):
        """Keep the ended records of one update and, with ``best_shots``, their shots (the host read of a GPU update; of the
        crops only those of records with a shot are read)."""
        if torch.is_tensor(ended_count):
            ended_i, ended_f, ended_count = ended_i.cpu().numpy(), ended_f.cpu().numpy(), ended_count.cpu().numpy()
        if torch.is_tensor(shot_i):
            shot_i, shot_q = shot_i.cpu().numpy(), shot_q.cpu().numpy().view(np.uint64)
        match_i = self._tracker.last_watch          # of the same update, line-parallel to ended_i
        stack_crops, stack_i = self._tracker.last_stack if self.stack_shots else (None, None)
        if torch.is_tensor(stack_i):
            stack_i = stack_i.cpu().numpy()
        if torch.is_tensor(match_i):
            match_i = match_i.cpu().numpy()
        match_align = self._tracker.last_watch_align
        if torch.is_tensor(match_align):
            match_align = match_align.cpu().numpy()
        sight_i = self._tracker.last_sight if self.sightings is not None else None     # of the same update too
        if torch.is_tensor(sight_i):
            sight_i = sight_i.cpu().numpy()
        for s, c in enumerate(ended_count.tolist()):
            if c > ended_i.shape[1]:
                LOGGER.warning('stream %d: %d tracks ended in one step, %d recorded' % (s, c, ended_i.shape[1]))
            for k in range(min(c, ended_i.shape[1])):
                self._track_ended.append((ended_i[s, k].copy(), ended_f[s, k].copy()))
                if match_i is not None:
                    self._track_hits.append(match_i[s, k].copy())
                if match_align is not None:
                    self._track_hit_align.append(int(match_align[s, k]))
                if sight_i is not None:
                    self._track_sights.append((sight_i[s, k].copy(), self._track_now))
                if shot_i is not None:
                    crop = shot_crops[s, k] if shot_i[s, k, 3] else None
                    crop = crop.cpu().numpy() if torch.is_tensor(crop) else (None if crop is None else crop.copy())
                    self._track_shots.append((shot_i[s, k].copy(), int(shot_q[s, k]), crop))
                if stack_i is not None:
                    crop = stack_crops[s, k] if stack_i[s, k, 3] else None
                    crop = crop.cpu().numpy() if torch.is_tensor(crop) else (None if crop is None else crop.copy())
                    self._track_stacks.append((stack_i[s, k].copy(), crop))
        if self._tracker.last_live is not None:     # the alerts of the same update
            from yolov6.utils.watch_live import alerts_of
            live_i, (q_i, _, q_slot, _) = self._tracker.last_live, self._tracker.last_live_reads
            if torch.is_tensor(live_i):
                live_i, q_i, q_slot = live_i.cpu().numpy(), q_i.cpu().numpy(), q_slot.cpu().numpy()
            live_align = self._tracker.last_live_align
            if torch.is_tensor(live_align):
                live_align = live_align.cpu().numpy()
            for s, t in alerts_of(live_i):
                row, j = live_i[s, t], int(np.nonzero(q_slot[s] == t)[0][0])
                self._track_alerts.append((row[7], row[0], q_i[s, j, 4:12].copy()) + tuple(row[1:5]) + (row[6],))
                if live_align is not None:
                    self._track_alert_align.append(int(live_align[s, t]))
        if self._tracker.last_zone is not None:     # the line and zone events of the same update
            zone_ev, zone_count = self._tracker.last_zone[:2]
            if torch.is_tensor(zone_ev):
                zone_ev, zone_count = zone_ev.cpu().numpy(), zone_count.cpu().numpy()
            for s, c in enumerate(zone_count.tolist()):
                if c > zone_ev.shape[1]:
                    LOGGER.warning('stream %d: %d line and zone events in one step, %d recorded' % (s, c, zone_ev.shape[1]))
                for e in zone_ev[s, :min(c, zone_ev.shape[1])]:
                    if e[0] != 5:
                        best = [int(e[8 + p // 4]) >> 8 * (p % 4) & 0xFF for p in range(8)]
                    else:                           # ended inside: the read of the ended record of the same id in this call
                        ended = [ended_i[s, k, 4:12] for k in range(min(int(ended_count[s]), ended_i.shape[1])) if ended_i[s, k, 0] == e[2]]
                        best = ended[0].copy() if ended else None
                    self._track_zone_events.append((s, int(e[0]), int(e[1]), int(e[4]), int(e[2]), best, int(e[5])))

        if self._tracker.last_speed is not None:    # the speed events of the same update
            _, speed_ev, speed_count = self._tracker.last_speed
            if torch.is_tensor(speed_ev):
                speed_ev, speed_count = speed_ev.cpu().numpy(), speed_count.cpu().numpy()
            for s, c in enumerate(speed_count.tolist()):
                for e in speed_ev[s, :min(c, speed_ev.shape[1])]:      # (a slot yields at most one: none is lost)
                    if e[0] != 3:
                        best = [int(e[8 + p // 4]) >> 8 * (p % 4) & 0xFF for p in range(8)]
                    else:                           # ended: the read of the ended record of the same id in this call
                        ended = [ended_i[s, k, 4:12] for k in range(min(int(ended_count[s]), ended_i.shape[1])) if ended_i[s, k, 0] == e[2]]
                        best = ended[0].copy() if ended else None
                    self._track_speed_events.append((int(e[0]), int(e[4]), int(e[2]), best, int(e[5]), int(e[11])))

    def _track_update(self, det, count, paths, frames=None):
        """One tracker update of a padded group: det [B,max_det,28] + count [B] (numpy on the CPU, device tensors on a GPU) of
        the frames ``paths`` (consecutive frames; slots past them are padding): (voted det, tid [B,max_det]), copies.
        ``frames``: the frames themselves, for ``best_shots`` (device tensors on a GPU, BGR arrays on the CPU)."""
        B = det.shape[0]
        streams = self._track_last_streams = [self._track_streams.get(p, 0) for p in paths] + [-1] * (B - len(paths))
        self._track_last_paths = list(paths)
        # a slot's track lives at least max_age + 1 frames: so many records at most can end in B frames
        max_ended = self._tracker.max_tracks * (B // (self.track_max_age + 1) + 1)
        self._track_clock(len(paths))
        if not self.best_shots:
            det_out, tid, ended_i, ended_f, ended_count = self._tracker.update(det, count, streams, max_ended=max_ended)
            self._track_collect(ended_i, ended_f, ended_count)
        elif torch.is_tensor(det):
            det_out, tid, *rest = self._tracker.update_with_shots(list(frames), det, count, streams, max_ended=max_ended)
            self._track_collect(*rest)
        else:
            det_out, tid, ended_i, ended_f, ended_count = self._tracker.update(det, count, streams, max_ended=max_ended)
            shots = self._gallery.update_from_frames(frames, det, count, tid, self._tracker.last_slot, streams, ended_i, ended_count,
                                                     self.SHOT_ROWS)
            if self.stack_shots:
                self._tracker.update_stack(frames, det, count, streams)
            self._track_collect(ended_i, ended_f, ended_count, *shots)
        if torch.is_tensor(det_out):
            det_out, tid = det_out.clone(), tid.clone()     # the tracker's buffers are persistent
        return det_out, tid

    def _track_clock(self, n_frames):
        """Set the clock of the sightings for the tracker call that takes the next ``n_frames`` frames of the source: the number of
        the last of them (0 frames: the final flush, stamped with the number of frames)."""
        self._track_seen += n_frames
        self._track_now = self._track_seen - (1 if n_frames else 0)
        if self.sightings is not None:
            self._tracker.sight_now[0] = self._track_now

    def _track_frame(self, det, img_path, max_det, frame=None):
        """The voted rows of one frame's rescaled detections ([n, 28] tensor); its track ids are queued for ``infer``."""
        n, max_det = len(det), max(int(max_det), len(det), 1)
        if self.device.type != 'cpu':
            pad = torch.zeros(1, max_det, 28, dtype=torch.float32, device=self.device)
            pad[0, :n] = det
            out, tid = self._track_update(pad, torch.full((1,), n, dtype=torch.int32, device=self.device), [img_path], [frame])
            self._track_tids.append(tid[0, :n].cpu().numpy())
            return out[0, :n]
        pad = np.zeros((1, max_det, 28), np.float32)
        pad[0, :n] = det.detach().float().cpu().numpy()
        out, tid = self._track_update(pad, np.array([n], np.int32), [img_path], [frame])
        self._track_tids.append(tid[0, :n])
        return torch.from_numpy(out[0, :n].copy())

    def _track_finish(self, save_dir):
        """Flush every stream and write tracks.txt / plates.txt."""
        from yolov6.utils.track import plate_text
        self._track_clock(0)
        if not self.best_shots:
            self._track_collect(*self._tracker.flush_all()[2:])
        elif self.device.type != 'cpu':
            self._track_collect(*self._tracker.flush_all_with_shots()[2:])
        else:
            _, tid, ended_i, ended_f, ended_count = self._tracker.flush_all()
            shots = self._gallery.update_from_frames([], np.zeros((0, 1, 28), np.float32), [], tid, self._tracker.last_slot, [], ended_i,
                                                     ended_count, self.SHOT_ROWS)
            if self.stack_shots:
                self._tracker.update_stack([], np.zeros((0, 1, 28), np.float32), [], [])
            self._track_collect(ended_i, ended_f, ended_count, *shots)
        os.makedirs(save_dir, exist_ok=True)
        with open(osp.join(save_dir, 'tracks.txt'), 'w') as f:
            f.writelines(line + '\n' for line in self._track_lines)
        with open(osp.join(save_dir, 'plates.txt'), 'w') as f:
            for ri, rf in self._track_ended:
                text = plate_text(ri[4:12], self.pro_names, self.alp_names, self.ads_names)
                f.write('%d %d %d %d %s %s\n' % (ri[0], ri[1], ri[2], ri[3], text, ' '.join('%g' % v for v in rf[:8])))
        if self.watchlist is not None:
            from yolov6.utils.watch import align_text, entry_text
            names = (self.pro_names, self.alp_names, self.ads_names)
            entries = self._tracker._watch[0].entries_np
            with open(osp.join(save_dir, 'hits.txt'), 'w') as f:
                for k, ((ri, _), m) in enumerate(zip(self._track_ended, self._track_hits)):
                    if m[0] >= 0:
                        f.write('%d %d %d %s %d %s %d %d %d%s\n' % (ri[0], ri[1], ri[2], plate_text(ri[4:12], *names), m[0],
                                                                    entry_text(entries[m[0]], *names), m[1], m[2], m[3],
                                                                    ' ' + align_text(self._track_hit_align[k]) if self.watch_indel else ''))
        if self.sightings is not None:
            names = (self.pro_names, self.alp_names, self.ads_names)
            with open(osp.join(save_dir, 'resightings.txt'), 'w') as f:
                for (ri, _), (m, now) in zip(self._track_ended, self._track_sights):
                    if m[0] >= 0:
                        f.write('%d %d %d %s %d %d %d %d %d %d %d\n' % (ri[0], ri[1], ri[2], plate_text(ri[4:12], *names), m[4], m[5], m[6], now,
                                                                        m[1], m[2], m[3]))
        if self.watch_live:
            from yolov6.utils.watch import align_text, entry_text
            names = (self.pro_names, self.alp_names, self.ads_names)
            entries = self._tracker._watch[0].entries_np
            with open(osp.join(save_dir, 'alerts.txt'), 'w') as f:
                for k, (frame, tid, best, e, mism, cost, n, hits) in enumerate(self._track_alerts):
                    f.write('%d %d %s %d %s %d %d %d %d%s\n' % (frame, tid, plate_text(best, *names), e, entry_text(entries[e], *names), mism,
                                                                cost, n, hits,
                                                                ' ' + align_text(self._track_alert_align[k]) if self.watch_indel else ''))
        if self.zones is not None:
            from yolov6.utils.zones import EVENT_NAMES, KIND_CROSS
            names = (self.pro_names, self.alp_names, self.ads_names)
            with open(osp.join(save_dir, 'crossings.txt'), 'w') as fc, open(osp.join(save_dir, 'zones.txt'), 'w') as fz:
                for s, kind, index, frame, tid, best, value in self._track_zone_events:
                    text = '-' if best is None else plate_text(best, *names)
                    if kind == KIND_CROSS:
                        fc.write('%d %d %s %s %+d\n' % (frame, tid, text, self._zone_line_names[s][index], value))
                    else:
                        fz.write('%d %d %s %s %s %d\n' % (frame, tid, text, self._zone_names[s][index], EVENT_NAMES[kind], value))
            totals = self._tracker.last_zone[3]
            totals = totals.cpu().numpy() if torch.is_tensor(totals) else totals
            LOGGER.info('line totals: ' + ('; '.join('%s%s +%d -%d' % ('' if len(self._zone_line_names) == 1 else '%d:' % s, name,
                                                                      totals[s, 0, l], totals[s, 1, l])
                                                     for s, ns in enumerate(self._zone_line_names) for l, name in enumerate(ns)) or 'no lines'))
        if self.speed is not None:
            from yolov6.utils.speed import KIND_ALERT, kmh
            names = (self.pro_names, self.alp_names, self.ads_names)
            with open(osp.join(save_dir, 'speeds.txt'), 'w') as fs, open(osp.join(save_dir, 'speeding.txt'), 'w') as fa:
                for kind, frame, tid, best, value, aux in self._track_speed_events:
                    text = '-' if best is None else plate_text(best, *names)
                    if kind == KIND_ALERT:
                        fa.write('%d %d %s %.1f %.1f\n' % (frame, tid, text, kmh(value), kmh(aux)))
                    else:
                        fs.write('%d %s %.1f %.1f\n' % (tid, text, kmh(value), kmh(aux)))
        if self.best_shots:
            names = self._write_track_images(save_dir, 'shots', [s[2] for s in self._track_shots])
            with open(osp.join(save_dir, 'shots.txt'), 'w') as f:
                for (ri, _), (si, q, crop), name in zip(self._track_ended, self._track_shots, names):
                    f.write('%d %d %d %d %d %s\n' % (ri[0], si[0], si[1], si[2], q, name))
        if self.stack_shots:
            names = self._write_track_images(save_dir, 'stacks', [s[1] for s in self._track_stacks])
            with open(osp.join(save_dir, 'stacks.txt'), 'w') as f:
                for (ri, _), (ki, crop), name in zip(self._track_ended, self._track_stacks, names):
                    f.write('%d %d %d %d %s\n' % (ri[0], ki[0], ki[1], ki[2], name))

    def _frames_ahead(self, prefetch_frames, imread_bgr):
        """(frame, path) of every source in LoadData's order: image files decoded ahead on the pool, videos read in turn."""
        files = self.files.files
        images = [p for p in files if self.files.checkext(p) == 'image']
        yield from prefetch_frames(images, imread_bgr, threads=min(self.batch_size, 8), depth=2 * self.batch_size)
        for p in files:
            if self.files.checkext(p) != 'image':
                for frame in self.files._frames_of(p):
                    yield frame, p

    def _as_nv12(self, frame):
        """A frame as the host ``Nv12Frame`` the source would have delivered: a BGR array is encoded (``bgr_to_nv12_np``, an odd
        last row / column cut off first), an ``Nv12Frame`` is passed on."""
        if isinstance(frame, Nv12Frame):
            return frame
        h, w = frame.shape[0] & ~1, frame.shape[1] & ~1
        return bgr_to_nv12_np(np.ascontiguousarray(frame[:h, :w]), self.nv12)

    def save_outputs(self, img_src, img_path, det, save_dir, save_txt, save_img):
        """The label lines and the annotated image of one frame's rescaled, rounded detections (reference :100-120).  An
        ``Nv12Frame`` is converted on the host only when the image is saved."""
        if save_img and isinstance(img_src, Nv12Frame):
            img_src = nv12_to_bgr_np(img_src)
        rel_path = osp.relpath(osp.dirname(img_path), osp.dirname(self.source))
        save_path = osp.join(save_dir, rel_path, osp.basename(img_path))
        txt_path = osp.join(save_dir, rel_path, osp.splitext(osp.basename(img_path))[0])
        if save_txt or save_img:
            os.makedirs(osp.join(save_dir, rel_path), exist_ok=True)
        gn = torch.tensor(img_src.shape)[[1, 0, 1, 0]]
        gn_cor = torch.tensor(img_src.shape)[[1, 0, 1, 0, 1, 0, 1, 0]]
        if len(det):
            rows = det.detach().float().cpu()
            if save_txt:
                with open(txt_path + '.txt', 'a') as f:
                    for output in rows:
                        xywh = (self.box_convert(output[:4].view(1, 4)) / gn).view(-1).tolist()
                        corners_gn = (output[4:12] / gn_cor).tolist()
                        line = (*output[20:].tolist(), *xywh, *corners_gn)
                        f.write(('%g ' * len(line)).rstrip() % line + '\n')
            if save_img:
                self.save_annotated(img_src, rows, save_path)
        elif save_img:
            self.save_annotated(img_src, [], save_path)

    def _redact_group(self, frames, dets, dev_frames=None):
        """With ``redact``: queue for ``infer`` the frames of one group with the plates of their final rows ``dets`` redacted, host
        BGR arrays or host ``Nv12Frame``s.  On a GPU ``dev_frames`` (the group's device frames) are redacted in place
        (``runtime.redact_plates``: whatever reads them has been enqueued before) and read back; on the CPU ``frames`` are
        copied (``redact_plates_np``).  With ``redact_hold`` the rows are those the group's tracker update left in
        ``last_hold`` -- the same rows followed by the predicted rows of the tracks each frame missed -- taken where they lie."""
        if self.redact is None:
            return
        if self.redact_lookback is not None:
            self._redact_delayed(frames, dev_frames)
            return
        n, m = len(frames), max([len(d) for d in dets] + [1])
        hold = self._tracker.last_hold if self.redact_hold else None
        if dev_frames is not None:
            from yolov6.hip import runtime
            if hold is not None:
                det, count = hold[0], hold[1]       # [>= n, max_det + slots, 28] on the device: no host read, no copy
            else:
                det = torch.zeros(n, m, 28, dtype=torch.float32, device=self.device)
                for k, d in enumerate(dets):
                    det[k, :len(d)] = d
                count = torch.tensor([len(d) for d in dets], dtype=torch.int32).to(self.device)
            dev_frames = list(dev_frames)[:n]
            runtime.redact_plates(dev_frames, det, count, self.redact, self.redact_cell, self.redact_margin, sigma=self.redact_sigma)
            if self.save_jpeg is not None:      # the files leave the device, not the frames
                self._redacted.extend(self._jpeg_files(dev_frames))
            else:
                self._redacted.extend(Nv12Frame(f.y.cpu().numpy(), f.uv.cpu().numpy(), f.matrix) if isinstance(f, Nv12Frame)
                                      else f.cpu().numpy() for f in dev_frames)
        else:
            from yolov6.utils.redact import redact_plates_np
            if hold is not None:
                det, count = hold[0], hold[1]
            else:
                det, count = np.zeros((n, m, 28), np.float32), [len(d) for d in dets]
                for k, d in enumerate(dets):
                    det[k, :len(d)] = d.detach().float().cpu().numpy()
            self._redacted.extend(redact_plates_np(list(frames), det, count, self.redact, self.redact_cell, self.redact_margin,
                                                   sigma=self.redact_sigma)[0])

    #: with ``overlay`` and ``track``: quad and label plate take OVERLAY_PALETTE[track id % 8], (B, G, R)
    OVERLAY_PALETTE = ((40, 40, 200), (40, 140, 40), (200, 80, 40), (20, 140, 200), (160, 40, 160), (140, 140, 20), (90, 90, 90), (30, 80, 140))

    @staticmethod
    def make_overlay_styles(size, thickness, alpha):
        """The two styles of ``overlay``: 0 for a frame's own rows, 1 (another box and quad colour) for the rows ``redact_hold``
        predicts for missed tracks.  ``alpha`` = (outlines, label plate, text), 0..256."""
        from yolov6.utils.overlay import Style, check_styles
        a_line, a_plate, a_text = (int(v) for v in alpha)
        base = Style(t=int(thickness), a_line=a_line, a_plate=a_plate, a_text=a_text, pad=max(1, min(16, int(size) // 8)))
        return check_styles([base, base._replace(box=(0, 128, 255), quad=(0, 128, 255))])

    @staticmethod
    def make_scene_style(size, thickness, alpha):
        """The style of ``overlay_scene``: the overlay's thickness, opacities and padding, a marker half a glyph high."""
        from yolov6.utils.scene import SceneStyle, check_scene_style
        a_line, a_plate, a_text = (int(v) for v in alpha)
        return check_scene_style(SceneStyle(t=int(thickness), marker=max(4, int(size) // 2), a_line=a_line, a_plate=a_plate, a_text=a_text,
                                            pad=max(1, min(16, int(size) // 8))))

    def _overlay_group(self, frames, dets, dev_frames=None, dev_rows=None):
        """With ``overlay``: queue for ``infer`` the frames of one group with their final rows ``dets`` drawn on them, right behind
        ``_redact_group``.  On a GPU clones of ``dev_frames`` (redacted already where ``redact`` is on) are drawn on
        (``runtime.draw_plates``) and either encoded there (``save_jpeg``: only the files leave the device) or read back; on the
        CPU ``draw_plates_np`` draws on the redacted copies, or on ``frames``.  With ``track`` the label carries the track id and the
        voted read: ``dev_rows`` = (det_out, count, tid) where the group's tracker update left them on the device, else the rows
        are padded from ``dets`` and the ids queued for ``tracks.txt``.  With ``redact_hold`` the rows and ids are ``last_hold``'s,
        taken where they lie, the predicted ones -- arange(rows) >= count -- in style 1."""
        if self._overlay is None:
            return
        n = len(frames)
        hold = self._tracker.last_hold if self.redact_hold else None
        rows = int(hold[0].shape[1]) if hold is not None else max([len(d) for d in dets] + [1])
        counts = np.array([len(d) for d in dets], np.int32)
        tid = None
        if hold is not None:
            tid = hold[2]
        elif self.track and dev_rows is None:
            tid = np.full((n, rows), -1, np.int32)
            for k, t in enumerate(list(self._track_tids)[-n:]):
                tid[k, :len(t)] = t
        kw = dict(styles=self._overlay_styles, palette=np.array(self.OVERLAY_PALETTE, np.uint8) if self.track else None)
        if dev_frames is not None:
            from yolov6.hip import runtime
            if self._overlay_dev is None:
                self._overlay_dev = runtime.OverlayFont(*self._overlay, device=self.device)
            if hold is not None:
                own = torch.from_numpy(counts).to(self.device)
                kw['style'] = (torch.arange(rows, device=self.device)[None, :] >= own[:, None]).to(torch.int32).contiguous()
                det, count = hold[0], hold[1]       # on the device: no host read, no copy
            elif dev_rows is not None:
                det, count, tid = dev_rows
            else:
                det = torch.zeros(n, rows, 28, dtype=torch.float32, device=self.device)
                for k, d in enumerate(dets):
                    det[k, :len(d)] = d
                count = torch.from_numpy(counts).to(self.device)
            if tid is not None:
                kw['tid'] = tid if torch.is_tensor(tid) else torch.from_numpy(tid).to(self.device)
            clones = [Nv12Frame(f.y.clone(), f.uv.clone(), f.matrix) if isinstance(f, Nv12Frame) else f.clone() for f in list(dev_frames)[:n]]
            if self._scene is not None:         # the scene first: zone fills lie under the plate outlines
                from yolov6.utils.scene import names_of
                if self._scene_dev is None:
                    names = names_of((None, None, self._zone_line_names, self._zone_names), self._scene)
                    self._scene_dev = (runtime.SceneFont(self._scene, device=self.device), torch.from_numpy(names.view(np.int16)).to(self.device))
                tags = self._tracker.last_speed is not None and kw.get('tid') is not None
                runtime.draw_scene(clones, self._scene_map, self._scene_dev[0], names=self._scene_dev[1], stream_of=self._track_last_streams[:n],
                                   zone=self._tracker.last_zone, speed=self._tracker.last_speed if tags else None, det=det if tags else None,
                                   count=count if tags else None, tid=kw['tid'] if tags else None, style=self._scene_style)
            runtime.draw_plates(clones, det, count, self._overlay_dev, **kw)
            if self.save_jpeg is not None:      # the files leave the device, not the frames
                self._annotated.extend(self._jpeg_files(clones))
            else:
                self._annotated.extend(Nv12Frame(f.y.cpu().numpy(), f.uv.cpu().numpy(), f.matrix) if isinstance(f, Nv12Frame)
                                       else f.cpu().numpy() for f in clones)
        else:
            from yolov6.utils.overlay import draw_plates_np
            base = list(self._redacted)[-n:] if self.redact is not None else list(frames)
            if hold is not None:
                det, count = hold[0], hold[1]
                kw['style'] = (np.arange(rows)[None, :] >= counts[:, None]).astype(np.int32)
            else:
                det, count = np.zeros((n, rows, 28), np.float32), counts
                for k, d in enumerate(dets):
                    det[k, :len(d)] = d.detach().float().cpu().numpy()
            if self._scene is not None:         # the scene first: zone fills lie under the plate outlines
                from yolov6.utils.scene import draw_scene_np, names_of
                names = names_of((None, None, self._zone_line_names, self._zone_names), self._scene)
                zone, speed = self._tracker.last_zone, self._tracker.last_speed if tid is not None else None
                tags = {} if speed is None else dict(speed_i=speed[0], det=det, count=count, tid=tid)
                base = draw_scene_np(base, self._scene_map.packed, self._scene, names, self._track_last_streams[:n],
                                     *((None,) * 4 if zone is None else (zone[3], zone[2], zone[0], zone[1])), style=self._scene_style, **tags)[0]
            self._annotated.extend(draw_plates_np(base, det, count, *self._overlay, tid=tid, **kw)[0])

    def _redact_delayed(self, frames, dev_frames=None):
        """With ``redact_lookback``: hand the group's frames to the delay line behind the group's tracker update and queue, with
        their paths, the frames that leave it (host BGR arrays or host ``Nv12Frame``s).  On a GPU the device frames are copied
        first -- the delay line keeps references, and the uploader reuses its buffer for the next group."""
        streams = self._track_last_streams
        for path, s in zip(self._track_last_paths, streams):
            self._lookback_paths[s].append(path)
        if dev_frames is not None:
            held = [Nv12Frame(f.y.clone(), f.uv.clone(), f.matrix) if isinstance(f, Nv12Frame) else f.clone()
                    for f in list(dev_frames)[:len(frames)]]
        else:
            held = list(frames)
        self._lookback_collect(self._lookback.push(held, streams))

    def _lookback_collect(self, done):
        for s, _, f in done:
            if self.save_jpeg is not None and (f.is_cuda if isinstance(f, Nv12Frame) or torch.is_tensor(f) else False):
                f = self._jpeg_files([f])[0]
            elif isinstance(f, Nv12Frame) and f.is_tensor:
                f = Nv12Frame(f.y.cpu().numpy(), f.uv.cpu().numpy(), f.matrix)
            elif torch.is_tensor(f):
                f = f.cpu().numpy()
            self._redacted.append((self._lookback_paths[s].popleft(), f))

    def _write_delayed(self, save_dir):
        """With ``redact_lookback``: write the frames that have left the delay so far."""
        while self.redact_lookback is not None and self._redacted:
            self.write_redacted(*self._redacted.popleft(), save_dir)

    def write_redacted(self, img_path, frame, save_dir, folder='redacted'):
        """One redacted frame (BGR array or host ``Nv12Frame``) as ``<save_dir>/redacted/<image name>``, by the writer of
        ``save_annotated``; a frame that is no image file (video, raw stream) is named ``<stem>.png``.  With ``save_jpeg``:
        ``redacted/<stem>.jpg``, and ``frame`` may be the finished file (``bytes``).  ``folder``: 'annotated' for the frames
        of ``overlay``, written the same way."""
        from PIL import Image
        os.makedirs(osp.join(save_dir, folder), exist_ok=True)
        if self.save_jpeg is not None:      # ``frame`` may be the file already (encoded from the device frame)
            data = frame if isinstance(frame, bytes) else self._jpeg_files([frame])[0]
            with open(osp.join(save_dir, folder, osp.splitext(osp.basename(img_path))[0] + '.jpg'), 'wb') as f:
                f.write(data)
            return
        if isinstance(frame, Nv12Frame):
            frame = nv12_to_bgr_np(frame)
        name = osp.basename(img_path)
        if self.files.checkext(img_path) != 'image':
            name = osp.splitext(name)[0] + '.png'
        Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(osp.join(save_dir, folder, name))

    def write_crops(self, img_path, crops_bgr, save_dir):
        """Plate crops of one image (uint8 [n, h, w, 3] BGR, a tensor or an array) as ``<save_dir>/<rel>/crops/<stem>_<k>.png``, RGB."""
        from PIL import Image
        crop_dir = osp.join(save_dir, osp.relpath(osp.dirname(img_path), osp.dirname(self.source)), 'crops')
        os.makedirs(crop_dir, exist_ok=True)
        stem = osp.splitext(osp.basename(img_path))[0]
        if self.save_jpeg is not None:
            for k, data in enumerate(self._jpeg_files(list(crops_bgr))):
                with open(osp.join(crop_dir, '%s_%d.jpg' % (stem, k)), 'wb') as f:
                    f.write(data)
            return
        if torch.is_tensor(crops_bgr):
            crops_bgr = crops_bgr.cpu().numpy()
        for k, crop in enumerate(crops_bgr):
            Image.fromarray(np.ascontiguousarray(crop[:, :, ::-1])).save(osp.join(crop_dir, '%s_%d.png' % (stem, k)))

    def _jpeg_files(self, frames):
        """With ``save_jpeg``: the ``.jpg`` files (``bytes``) of a list of BGR frames or ``Nv12Frame``s, on the host or on the
        device.  On a GPU host frames are uploaded and every frame goes through ``runtime.encode_jpeg`` in one call; on the
        CPU each through ``encode_jpeg_np``: the same bytes."""
        frames = list(frames)
        if not frames:
            return []
        if self.device.type != 'cpu':
            from yolov6.hip import runtime
            dev = []
            for f in frames:
                if isinstance(f, Nv12Frame):
                    dev.append(f if f.is_cuda else f.to(self.device))
                else:
                    dev.append(f if torch.is_tensor(f) and f.is_cuda else torch.as_tensor(np.ascontiguousarray(f)).to(self.device))
            return runtime.encode_jpeg(dev, self.save_jpeg, self.JPEG_RESTART)
        from yolov6.utils.jpeg import encode_jpeg_np
        return [encode_jpeg_np(f.numpy() if torch.is_tensor(f) else f, self.save_jpeg, self.JPEG_RESTART) for f in frames]

    def _write_track_images(self, save_dir, folder, crops):
        """The shots or the stacks of the ended tracks (``crops``: a BGR array or None per line of ``plates.txt``) as
        ``<folder>/<line>_<id>.png`` (``.jpg`` with ``save_jpeg``, all encoded in one call); the relative names, '-' for None."""
        from PIL import Image
        os.makedirs(osp.join(save_dir, folder), exist_ok=True)
        ext = 'png' if self.save_jpeg is None else 'jpg'
        names = ['-' if crop is None else osp.join(folder, '%d_%d.%s' % (k, ri[0], ext))
                 for k, ((ri, _), crop) in enumerate(zip(self._track_ended, crops))]
        live = [(name, crop) for name, crop in zip(names, crops) if crop is not None]
        if self.save_jpeg is not None:
            for (name, _), data in zip(live, self._jpeg_files([crop for _, crop in live])):
                with open(osp.join(save_dir, name), 'wb') as f:
                    f.write(data)
        else:
            for name, crop in live:
                Image.fromarray(np.ascontiguousarray(crop[:, :, ::-1])).save(osp.join(save_dir, name))
        return names

    @staticmethod
    def save_annotated(img_bgr, rows, save_path):
        from PIL import Image, ImageDraw
        im = Image.fromarray(np.ascontiguousarray(img_bgr[:, :, ::-1]))
        draw = ImageDraw.Draw(im)
        for r in rows:
            draw.rectangle([float(v) for v in r[:4]], outline=(255, 64, 64), width=2)
            pts = [float(v) for v in r[4:12]]
            draw.polygon(pts, outline=(64, 255, 64))
        im.save(save_path)

    @staticmethod
    def precess_image(img_src, img_size, stride, half, auto=True):
        """letterbox -> CHW RGB -> fp16/fp32 in [0, 1] (reference :191-201)."""
        image = letterbox(img_src, img_size, stride=stride, auto=auto)[0]
        image = image.transpose((2, 0, 1))[::-1]
        image = torch.from_numpy(np.ascontiguousarray(image))
        image = image.half() if half else image.float()
        image /= 255
        return image, img_src

    @staticmethod
    def rescale(ori_shape, boxes_and_cors, target_shape):
        """Undo the letterbox on the 12 coordinates, in place: subtract the padding, divide by the ratio, clamp
        to the source image (reference :203-228)."""
        ratio = min(ori_shape[0] / target_shape[0], ori_shape[1] / target_shape[1])
        padding = (ori_shape[1] - target_shape[1] * ratio) / 2, (ori_shape[0] - target_shape[0] * ratio) / 2
        boxes_and_cors[:, [0, 2, 4, 6, 8, 10]] -= padding[0]
        boxes_and_cors[:, [1, 3, 5, 7, 9, 11]] -= padding[1]
        boxes_and_cors[:, :] /= ratio
        for k in range(12):
            boxes_and_cors[:, k].clamp_(0, target_shape[1] if k % 2 == 0 else target_shape[0])
        return boxes_and_cors

    def check_img_size(self, img_size, s=32, floor=0):
        """Round the inference size up to a multiple of the stride; always returns [h, w]."""
        if isinstance(img_size, int):
            new_size = max(self.make_divisible(img_size, int(s)), floor)
        elif isinstance(img_size, list):
            new_size = [max(self.make_divisible(x, int(s)), floor) for x in img_size]
        else:
            raise Exception(f"Unsupported type of img_size: {type(img_size)}")
        if new_size != img_size:
            print(f'WARNING: --img-size {img_size} must be multiple of max stride {s}, updating to {new_size}')
        return new_size if isinstance(img_size, list) else [new_size] * 2

    def make_divisible(self, x, divisor):
        return math.ceil(x / divisor) * divisor

    @staticmethod
    def box_convert(x):
        """xyxy -> xywh for an [n, 4] tensor / array."""
        y = x.clone() if isinstance(x, torch.Tensor) else np.copy(x)
        y[:, 0] = (x[:, 0] + x[:, 2]) / 2
        y[:, 1] = (x[:, 1] + x[:, 3]) / 2
        y[:, 2] = x[:, 2] - x[:, 0]
        y[:, 3] = x[:, 3] - x[:, 1]
        return y


class CalcFPS:
    def __init__(self, nsamples: int = 50):
        self.framerate = deque(maxlen=nsamples)

    def update(self, duration: float):
        self.framerate.append(duration)

    def accumulate(self):
        return np.average(self.framerate) if len(self.framerate) > 1 else 0.0
