"""Host side of the HIP engine: turns a ``yolov6.models.yolo.Model`` into the op
graph of libyololp_hip.so (folded weights, NHWC tensors, concat-free sources) and
runs forward / NMS through the C ABI on torch-owned device memory and torch's
current stream.

Replaces, on a GPU, ``Model.forward`` (reference yolov6/models/yolo.py:32-40)
and ``non_max_suppression`` (yolov6/utils/nms.py:31-130).  Weight preparation
follows the reference's order ``float -> fuse_model -> switch_to_deploy``
(inferer.py:25-68): modules that are still un-fused are folded on the fly with
the same formulas, without touching the caller's model.

One module per subsystem, imported in this order (each may import the ones above it): ``_base`` (what they share), ``nms``,
``engine``, ``frames``, ``crops``, ``redact``, ``overlay``, ``jpeg``, ``tiles``, ``tile_gate``, ``watch``, ``tracker``,
``lookback``.  This file only re-exports: ``yolov6.hip.runtime.X`` is the object its module defines, and the module-level
state (workspace caches, ``_engines``, ``jpeg_stats``) exists once, there.  A ``*_WS_CAP`` constant is read in its own module.
"""
from ._base import _DT, _stream_ptr, _stream_workspace, _unpad
from .nms import _nms_ws, eval_counts, nms_candidates, nms_padded, non_max_suppression
from .engine import (CLS_HEADS, DET_CROSSOVER, OP_KINDS, Engine, _engines, _f32, detect, detect_padded, drop_engine, engine_for,
                     model_forward, prepare_for)
from .frames import (detect_frames, detect_frames_padded, nv12_to_bgr, preprocess_frames, preprocess_letterbox, rescale_round,
                     rescale_round_batch)
from .crops import _crop_size, _unpad_with_crops, crop_sharpness, detect_frames_with_crops, plate_crops
from .redact import GAUSS_WS_CAP, _gauss_params, _redact_workspace, _redact_ws, redact_plates
from .overlay import (OverlayFont, SceneFont, _overlay_params, _overlay_params_memo, _overlay_ws, _scene_style, _scene_ws, draw_plates,
                      draw_scene)
from .jpeg import JPEG_WS_CAP, _jpeg_ws, encode_jpeg, encode_jpeg_padded, jpeg_stats
from .tiles import (_tile_inputs, detect_tiled, detect_tiled_padded, detect_tiled_with_crops, detect_tiles_padded, merge_tiles,
                    merge_tiles_buffers, plan_tiled, preprocess_tiles)
from .tile_gate import TileGate
from .watch import SightLog, Watchlist
from .tracker import GroundPlane, PlateTracker, ZoneMap
from .lookback import LookbackRedactor

# names of other packages that callers have always found here as well
from yolov6.core.frames import letterbox_placement
from yolov6.core.tiles import hw_pair, plan_frames, tiles_per_frame
from yolov6.utils.lookback import LookbackHost
from yolov6.utils.nv12 import Nv12Frame, is_nv12_list
