"""ctypes binding of libyololp_hip.so (C ABI declared in include/lp_hip.h).

The library is the only implementation of the GPU path: if it cannot be loaded
this module raises -- nothing falls back to eager torch ops on a GPU.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_size_t, c_void_p  # noqa: F401

LP_F16, LP_BF16, LP_F32 = 0, 1, 2
LP_ACT_NONE, LP_ACT_RELU, LP_ACT_SILU = 0, 1, 2
LP_PRED_COLS, LP_DET_COLS, LP_MAX_SRC = 290, 28, 4
LP_VARIANT_STREAM64, LP_VARIANT_STREAM128, LP_VARIANT_ROWS = 16, 17, 18   # lp_engine_set_op_variant codes beyond the tiles
LP_VARIANT_PIPE_D, LP_VARIANT_PIPE_B, LP_VARIANT_PIPE_F, LP_VARIANT_PIPE_C = 32, 33, 34, 35        # pipelined 3x3 stride-1 kernel (nbuf 3)
LP_VARIANT_PIPE16_D, LP_VARIANT_PIPE16_F = 39, 41                              # the same on v_mfma_f32_16x16x32 (another fp32 summation order)
LP_VARIANT_PIPE16_V0, LP_VARIANT_PIPE16_V1 = 42, 43                           # ... with tiles of any number of 16-pixel blocks
LP_VARIANT_PIPE16_S2A, LP_VARIANT_PIPE16_S2B = 48, 49                         # 3x3 stride 2 on v_mfma_f32_16x16x32 (two-slot ring, 16-pixel blocks)
LP_VARIANT_FUSED_BIFUSION = 45                                                                   # BiFusion's transposed conv + cv1 + cv3 as one kernel
LP_VARIANT_BOX_SPARSE, LP_VARIANT_BOX_DENSE = 46, 47                                                    # head_box in the detections-only forward: candidates only / every anchor
LP_VARIANT_FUSED_PW_S2 = 38                                                                      # a 1x1 layer + the 3x3 stride-2 layer behind it as one kernel
LP_VARIANT_FUSED_STEM2 = 37                                                                      # input op + stem + the layer behind it as one kernel
LP_VARIANT_PIPE_P = 36                                                                           # the stem reading the NCHW frame itself
#: short names of the variant codes above in ``Engine.profile`` (the plain tiles 0..7 print as 'A'..'H')
VARIANT_SHORT = {
    LP_VARIANT_STREAM64: 'S', LP_VARIANT_STREAM128: 'W', LP_VARIANT_ROWS: 'R',
    LP_VARIANT_PIPE_D: 'Pd', LP_VARIANT_PIPE_B: 'Pb', LP_VARIANT_PIPE_F: 'Pf', LP_VARIANT_PIPE_C: 'Pc', LP_VARIANT_PIPE_P: 'Pp',
    LP_VARIANT_FUSED_STEM2: 'Fz', LP_VARIANT_FUSED_PW_S2: 'Fp', LP_VARIANT_FUSED_BIFUSION: 'Fb',
    LP_VARIANT_PIPE16_D: 'Md', LP_VARIANT_PIPE16_F: 'Mf', LP_VARIANT_PIPE16_V0: 'V0', LP_VARIANT_PIPE16_V1: 'V1',
    LP_VARIANT_PIPE16_S2A: 'Xa', LP_VARIANT_PIPE16_S2B: 'Xb',
}
LP_FRAMES_PER_LAUNCH = 64   # lp_preprocess_letterbox_batch / lp_rescale_round_batch / lp_plate_crops_batch: frames per launch
LP_NV12_PER_LAUNCH = 32     # lp_preprocess_nv12_batch: slots per launch (its table entries are larger)
LP_MERGE_MAX_TILES, LP_MERGE_MAX_CANDIDATES = 64, 16384   # lp_merge_tiles: tiles per frame, tiles_of_frame * max_det_t
LP_TRACK_MAX_TRACKS, LP_TRACK_MAX_DETS, LP_TRACK_MAX_CLS = 128, 128, 64   # lp_track_update: slots per stream, rows per frame, classes per head
LP_REDACT_MAX_CELL = 64    # lp_redact_plates_batch: largest mosaic cell
LP_REDACT_MAX_RADIUS = 48  # lp_redact_gauss_batch: largest blur radius (taps per side)
LP_OVERLAY_MAX_STYLES, LP_OVERLAY_MAX_GLYPHS, LP_OVERLAY_MAX_PALETTE = 8, 20, 64   # lp_overlay_draw_batch: styles, glyphs of a label, palette entries
LP_SCENE_MAX_GLYPHS, LP_SCENE_MAX_NAME, LP_SCENE_MAX_MARKER, LP_SCENE_FIXED_GLYPHS = 36, 12, 64, 17   # lp_overlay_scene_batch: glyphs of a label, of a name, marker height, fixed glyphs
LP_JPEG_MAX_RESTART, LP_JPEG_PER_LAUNCH = 32, 32   # lp_jpeg_encode_batch: MCUs per restart interval, frames per launch
LP_LOOKBACK_MAX_DEPTH = 32   # lp_lookback_update: frames of delay
LP_WATCH_MAX_ENTRIES, LP_WATCH_MAX_COST = 1 << 24, 32768   # lp_watch_match: entries of a watchlist, the largest cost of an entry
LP_WATCH_BLOCK_ENTRIES, LP_WATCH_QUERY_BLOCK = 2048, 16   # ... entries per workgroup of its scan, reads per LDS table
LP_WATCH_MAX_GAP_COST, LP_WATCH_INDEL_QUERY_BLOCK = 4096, 16   # lp_watch_match_indel: the largest gap_cost, reads per LDS table of its scan
LP_SIGHT_MAX_CAPACITY = 1 << 24   # lp_sight_update: slots of a log of sightings
LP_ZONE_MAX_LINES, LP_ZONE_MAX_ZONES, LP_ZONE_MAX_VERTS, LP_ZONE_MAP_WORDS = 16, 8, 16, 368   # lp_zone_update: the packed geometry of a stream
LP_SPEED_MAP_WORDS, LP_SPEED_MEMO_WORDS, LP_SPEED_RING = 32, 48, 8   # lp_speed_update: the packed calibration of a stream, the memo of a slot
LP_SIGHT_BLOCK_ENTRIES, LP_SIGHT_QUERY_BLOCK = 1024, 16   # ... slots per workgroup of its scan, reads per LDS table
LP_TILE_GATE_TILE_WORDS = 8  # lp_tile_gate_update: int32 words per entry of the device tile table
LP_EVAL_NCOUNTS = 43  # lp_eval_counts: length of the counts vector (include/lp_hip.h)

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # .../yolo-lp_amd
LIB_PATH = os.environ.get('LP_HIP_LIB') or os.path.join(_PKG_ROOT, 'libyololp_hip.so')   # LP_HIP_LIB: debug builds
CSRC_DIR = os.path.join(_PKG_ROOT, 'csrc')


class FrameDesc(ctypes.Structure):
    """lp_frame_desc"""
    _fields_ = [('img', c_void_p), ('h0', c_int), ('w0', c_int), ('rh', c_int), ('rw', c_int), ('top', c_int), ('left', c_int)]


class RescaleDesc(ctypes.Structure):
    """lp_rescale_desc"""
    _fields_ = [('ratio', c_double), ('padx', c_double), ('pady', c_double), ('img_w', c_int), ('img_h', c_int)]


class CropDesc(ctypes.Structure):
    """lp_crop_desc"""
    _fields_ = [('img', c_void_p), ('h0', c_int), ('w0', c_int), ('max_crops', c_int), ('out_slot', c_int)]


class TileDesc(ctypes.Structure):
    """lp_tile_desc"""
    _fields_ = [('img', c_void_p), ('h0', c_int), ('w0', c_int), ('y0', c_int), ('x0', c_int), ('th', c_int), ('tw', c_int),
                ('rh', c_int), ('rw', c_int), ('top', c_int), ('left', c_int)]


class Nv12Desc(ctypes.Structure):
    """lp_nv12_desc"""
    _fields_ = [('y', c_void_p), ('uv', c_void_p), ('pitch_y', c_int), ('pitch_uv', c_int), ('h0', c_int), ('w0', c_int),
                ('y0', c_int), ('x0', c_int), ('th', c_int), ('tw', c_int), ('rh', c_int), ('rw', c_int), ('top', c_int),
                ('left', c_int), ('matrix', c_int)]


class Nv12BgrDesc(ctypes.Structure):
    """lp_nv12_bgr_desc"""
    _fields_ = [('y', c_void_p), ('uv', c_void_p), ('pitch_y', c_int), ('pitch_uv', c_int), ('h0', c_int), ('w0', c_int),
                ('matrix', c_int), ('out', c_void_p)]


class RedactDesc(ctypes.Structure):
    """lp_redact_desc"""
    _fields_ = [('p0', c_void_p), ('p1', c_void_p), ('pitch0', c_int), ('pitch1', c_int), ('h0', c_int), ('w0', c_int),
                ('format', c_int)]


class RedactParams(ctypes.Structure):
    """lp_redact_params"""
    _fields_ = [('mode', c_int), ('cell', c_int), ('margin', c_double), ('fill', ctypes.c_ubyte * 3)]


class RedactGaussParams(ctypes.Structure):
    """lp_redact_gauss_params"""
    _fields_ = [('margin', c_double), ('radius', c_int), ('radius_c', c_int), ('taps', ctypes.c_uint16 * (LP_REDACT_MAX_RADIUS + 1)),
                ('taps_c', ctypes.c_uint16 * (LP_REDACT_MAX_RADIUS + 1))]


class OverlayStyle(ctypes.Structure):
    """lp_overlay_style"""
    _fields_ = [('box', ctypes.c_ubyte * 3), ('quad', ctypes.c_ubyte * 3), ('plate', ctypes.c_ubyte * 3), ('text', ctypes.c_ubyte * 3),
                ('t', c_int), ('a_line', c_int), ('a_plate', c_int), ('a_text', c_int), ('pad', c_int)]


class OverlayParams(ctypes.Structure):
    """lp_overlay_params"""
    _fields_ = [('n_styles', c_int), ('styles', OverlayStyle * LP_OVERLAY_MAX_STYLES), ('n_palette', c_int),
                ('palette', (ctypes.c_ubyte * 3) * LP_OVERLAY_MAX_PALETTE), ('n_glyphs', c_int), ('gh', c_int), ('gw', c_int),
                ('show_id', c_int), ('label', c_int), ('draw_box', c_int)]


class SceneStyle(ctypes.Structure):
    """lp_scene_style"""
    _fields_ = [(name, ctypes.c_ubyte * 3) for name in ('zone', 'alert', 'line', 'mark', 'plate', 'text', 'tag')] + \
               [(name, c_int) for name in ('t', 'marker', 'a_fill', 'a_fill_busy', 'a_line', 'a_plate', 'a_text', 'pad', 'n_glyphs', 'gh', 'gw')]


class JpegDesc(ctypes.Structure):
    """lp_jpeg_desc"""
    _fields_ = [('p0', c_void_p), ('p1', c_void_p), ('pitch0', c_int), ('pitch1', c_int), ('h0', c_int), ('w0', c_int),
                ('format', c_int), ('matrix', c_int)]


class JpegParams(ctypes.Structure):
    """lp_jpeg_params"""
    _fields_ = [('quality', c_int), ('restart', c_int)]


class TileGateDesc(ctypes.Structure):
    """lp_tile_gate_desc"""
    _fields_ = [('p0', c_void_p), ('pitch0', c_int), ('h0', c_int), ('w0', c_int), ('format', c_int), ('blocks', c_void_p)]


class TileRef(ctypes.Structure):
    """lp_tile_ref"""
    _fields_ = [('frame', c_int), ('y0', c_int), ('x0', c_int), ('th', c_int), ('tw', c_int)]


class TrackParams(ctypes.Structure):
    """lp_track_params"""
    _fields_ = [('match_thres', c_double), ('new_thres', c_double), ('expand', c_double), ('max_age', c_int), ('ncls', c_int * 8)]


class TrackHoldParams(ctypes.Structure):
    """lp_track_hold_params"""
    _fields_ = [('min_hits', c_int), ('max_misses', c_int)]


class StackParams(ctypes.Structure):
    """lp_stack_params"""
    _fields_ = [('min_score', c_double), ('min_width', c_double), ('min_sharp', ctypes.c_ulonglong), ('search', c_int),
                ('max_frames', c_int)]


class ConvDesc(ctypes.Structure):
    """lp_conv_desc"""
    _fields_ = [('n_src', c_int), ('src', c_int * LP_MAX_SRC), ('dst', c_int), ('ksize', c_int), ('stride', c_int),
                ('act', c_int), ('res', c_int), ('res_alpha', c_float), ('weight', c_void_p), ('bias', c_void_p), ('dst2', c_int)]


#: name -> (restype, argtypes): every symbol include/lp_hip.h declares
SYMBOLS = {
    'lp_version': (c_char_p, []),
    'lp_last_error': (c_char_p, []),
    'lp_engine_create': (c_int, [POINTER(c_void_p), c_int]),
    'lp_engine_destroy': (None, [c_void_p]),
    'lp_engine_tensor': (c_int, [c_void_p, c_int, c_int]),
    'lp_engine_set_lane': (c_int, [c_void_p, c_int]),
    'lp_engine_add_input': (c_int, [c_void_p, c_int]),
    'lp_engine_add_conv': (c_int, [c_void_p, POINTER(ConvDesc)]),
    'lp_engine_add_deconv2x2': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'lp_engine_add_pool5_chain': (c_int, [c_void_p, c_int, c_int, c_int, c_int]),
    'lp_engine_add_head_cls': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'lp_engine_add_head_box': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'lp_engine_finalize': (c_int, [c_void_p, c_int]),
    'lp_engine_weight_bytes': (c_size_t, [c_void_p]),
    'lp_engine_upload': (c_int, [c_void_p, c_void_p, c_void_p]),
    'lp_engine_arena_bytes': (c_size_t, [c_void_p, c_int, c_int, c_int]),
    'lp_engine_bind': (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_int]),
    'lp_engine_tensor_info': (c_int, [c_void_p, c_int, POINTER(c_size_t), POINTER(c_int), POINTER(c_int),
                                      POINTER(c_int), POINTER(c_int)]),
    'lp_engine_num_anchors': (c_int, [c_void_p]),
    'lp_engine_forward': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'lp_engine_set_graph': (c_int, [c_void_p, c_int]),
    'lp_engine_set_single_lane': (c_int, [c_void_p, c_int]),
    'lp_engine_set_mfma16': (c_int, [c_void_p, c_int]),
    'lp_engine_op_carrier': (c_int, [c_void_p, c_int, c_int]),
    'lp_engine_op_io': (c_int, [c_void_p, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    'lp_engine_num_ops': (c_int, [c_void_p]),
    'lp_engine_op_info': (c_int, [c_void_p, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int),
                                  POINTER(c_double), POINTER(c_double)]),
    'lp_engine_forward_det': (c_int, [c_void_p, c_void_p, c_int, ctypes.c_double, c_void_p, c_size_t, c_void_p]),
    'lp_nms_candidates': (c_int, [c_int, c_int, ctypes.c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'lp_engine_profile': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, POINTER(c_float), c_int]),
    'lp_engine_profile_ops': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, POINTER(c_float), c_int, c_int]),
    'lp_engine_autotune': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int]),
    'lp_engine_op_variant': (c_int, [c_void_p, c_int, POINTER(c_int), POINTER(c_int)]),
    'lp_engine_set_op_variant': (c_int, [c_void_p, c_int, c_int, c_int]),
    'lp_engine_set_op_tile': (c_int, [c_void_p, c_int, c_int]),
    'lp_engine_op_tile': (c_int, [c_void_p, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    'lp_engine_copy_tuning': (c_int, [c_void_p, c_void_p]),
    'lp_nms_workspace_bytes': (c_size_t, [c_int, c_int]),
    'lp_nms_candidate_counts': (c_void_p, [c_void_p, c_int, c_int]),
    'lp_preprocess_letterbox': (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p]),
    'lp_rescale_round': (c_int, [c_void_p, c_int, c_double, c_double, c_double, c_int, c_int, c_void_p]),
    'lp_preprocess_letterbox_batch': (c_int, [POINTER(FrameDesc), c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    'lp_rescale_round_batch': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(RescaleDesc), c_void_p]),
    'lp_preprocess_tiles_batch': (c_int, [POINTER(TileDesc), c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    'lp_preprocess_nv12_batch': (c_int, [POINTER(Nv12Desc), c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    'lp_nv12_to_bgr_batch': (c_int, [POINTER(Nv12BgrDesc), c_int, c_void_p]),
    'lp_merge_tiles_workspace_bytes': (c_size_t, [c_int, c_int]),
    'lp_merge_tiles': (c_int, [c_void_p, c_void_p, POINTER(TileRef), c_int, c_int, POINTER(c_int), c_int, c_double, c_int, c_int, c_int,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'lp_track_state_bytes': (c_size_t, [c_int, c_int]),
    'lp_track_dropped_offset': (c_size_t, [c_int, c_int]),
    'lp_track_update': (c_int, [c_void_p, c_int, c_int, POINTER(TrackParams), c_void_p, c_void_p, c_int, c_int, POINTER(c_int),
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    'lp_track_update_slots': (c_int, [c_void_p, c_int, c_int, POINTER(TrackParams), c_void_p, c_void_p, c_int, c_int, POINTER(c_int),
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    'lp_track_update_hold': (c_int, [c_void_p, c_int, c_int, POINTER(TrackParams), c_void_p, c_void_p, c_int, c_int, POINTER(c_int),
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                     POINTER(TrackHoldParams), c_void_p, c_void_p, c_void_p, c_void_p]),
    'lp_plate_crops_batch': (c_int, [POINTER(CropDesc), c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                     c_void_p]),
    'lp_crop_sharpness': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'lp_best_shot_state_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
    'lp_best_shot_update': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_int, POINTER(c_int), c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p]),
    'lp_stack_state_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
    'lp_stack_update': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_int, POINTER(c_int), c_void_p, c_void_p, c_int, POINTER(StackParams), c_void_p,
                                c_void_p, c_void_p]),
    'lp_redact_workspace_bytes': (c_size_t, [POINTER(RedactDesc), c_int, POINTER(RedactParams)]),
    'lp_redact_plates_batch': (c_int, [POINTER(RedactDesc), c_int, c_void_p, c_void_p, c_int, POINTER(RedactParams), c_void_p, c_void_p,
                                       c_size_t, c_void_p]),
    'lp_redact_gauss_workspace_bytes': (c_size_t, [POINTER(RedactDesc), c_int, POINTER(RedactGaussParams)]),
    'lp_redact_gauss_batch': (c_int, [POINTER(RedactDesc), c_int, c_void_p, c_void_p, c_int, POINTER(RedactGaussParams), c_void_p, c_void_p,
                                      c_size_t, c_void_p]),
    'lp_overlay_workspace_bytes': (c_size_t, [c_int, c_int]),
    'lp_overlay_draw_batch': (c_int, [POINTER(RedactDesc), c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, POINTER(OverlayParams),
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'lp_overlay_scene_workspace_bytes': (c_size_t, [c_int, c_int]),
    'lp_overlay_scene_batch': (c_int, [POINTER(RedactDesc), c_int, POINTER(c_int32), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, POINTER(SceneStyle), c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_size_t, c_void_p]),
    'lp_jpeg_workspace_bytes': (c_size_t, [POINTER(JpegDesc), c_int, c_int]),
    'lp_jpeg_encode_batch': (c_int, [POINTER(JpegDesc), c_int, POINTER(JpegParams), c_void_p, c_int, c_void_p, c_size_t, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    'lp_lookback_state_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
    'lp_lookback_update': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'lp_watch_workspace_bytes': (c_size_t, [c_int, c_int]),
    'lp_watch_match': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                               c_size_t, c_void_p]),
    'lp_watch_match_indel': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                     c_void_p, c_void_p, c_size_t, c_void_p]),
    'lp_watch_live_state_bytes': (c_size_t, [c_int, c_int]),
    'lp_watch_live_workspace_bytes': (c_size_t, [c_int, c_int]),
    'lp_watch_live': (c_int, [c_void_p, c_int, c_int, POINTER(c_int), c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'lp_watch_live_indel_workspace_bytes': (c_size_t, [c_int, c_int]),
    'lp_watch_live_indel': (c_int, [c_void_p, c_int, c_int, POINTER(c_int), c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'lp_sight_state_bytes': (c_size_t, [c_int]),
    'lp_sight_workspace_bytes': (c_size_t, [c_int, c_int]),
    'lp_sight_update': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int,
                                c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'lp_zone_state_bytes': (c_size_t, [c_int, c_int]),
    'lp_zone_update': (c_int, [c_void_p, c_int, c_int, POINTER(c_int), c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                               c_void_p, c_void_p]),
    'lp_speed_state_bytes': (c_size_t, [c_int, c_int]),
    'lp_speed_update': (c_int, [c_void_p, c_int, c_int, POINTER(c_int), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_int, c_void_p]),
    'lp_tile_gate_luma_batch': (c_int, [POINTER(TileGateDesc), c_int, c_void_p]),
    'lp_tile_gate_update': (c_int, [POINTER(TileGateDesc), c_int, POINTER(c_int), c_int, c_void_p, POINTER(c_int), c_int, c_void_p,
                                    ctypes.c_longlong, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'lp_tile_gate_update_gain': (c_int, [POINTER(TileGateDesc), c_int, POINTER(c_int), c_int, c_void_p, POINTER(c_int), c_int, c_void_p,
                                         ctypes.c_longlong, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    'lp_eval_counts': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'lp_check_sigmoid_monotone': (c_int, [c_void_p, c_void_p]),
    'lp_debug_poison_lds': (c_int, [c_void_p]),
    'lp_check_iou_predicate': (c_int, [c_void_p, ctypes.c_longlong, c_double, c_void_p, c_void_p]),
    'lp_plan_stem_tile': (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'lp_plan_block_tile': (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'lp_nms': (c_int, [c_void_p, c_int, c_int, c_double, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                       c_size_t, c_void_p]),
}

_lib = None


def load():
    """Load the library once and attach prototypes; raises RuntimeError when it is missing."""
    global _lib
    if _lib is None:
        # torch bundles its own libamdhip64; importing it first makes this library bind to that same HIP
        # runtime (one runtime per process: a second copy loaded from /opt/rocm finds no device)
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError('HIP extension %s is missing: build it with `make -C %s` (or '
                               '`python -c "import __graft_entry__ as g; g.build()"`). The GPU path has no '
                               'eager fallback.' % (LIB_PATH, CSRC_DIR))
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SYMBOLS.items():
            fn = getattr(lib, name)      # AttributeError here = header and library are out of sync
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
    return _lib


def check(rc, what=''):
    """Raise RuntimeError with the library's message for a negative lp_status."""
    if rc < 0:
        msg = load().lp_last_error()
        raise RuntimeError('%s failed (%d): %s' % (what or 'libyololp_hip', rc, msg.decode() if msg else '?'))
    return rc
