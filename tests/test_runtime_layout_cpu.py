"""CPU-only checks of the layout of ``yolov6.hip.runtime``: the package exposes every name the single-file module exposed, each as
the object of its owning module; every module imports on its own and only from modules before it; and the helpers that the
per-frame launches share (runs of frames, descriptor arrays, the aligned span of a workspace) do what their callers rely on."""
import ast
import ctypes
import importlib
import os
import subprocess
import sys

import pytest
import torch

from conftest import REPO

#: import order of the package: a module imports only from modules before it
MODULES = ['_base', 'nms', 'engine', 'frames', 'crops', 'redact', 'overlay', 'jpeg', 'tiles', 'tile_gate', 'watch', 'tracker',
           'lookback']
#: the public names of the single-file ``runtime`` module, recorded on the commit before the split
PUBLIC = ['CLS_HEADS', 'DET_CROSSOVER', 'Engine', 'GAUSS_WS_CAP', 'JPEG_WS_CAP', 'LookbackHost', 'LookbackRedactor', 'Nv12Frame',
          'OP_KINDS', 'OverlayFont', 'PlateTracker', 'SightLog', 'TileGate', 'Watchlist', 'crop_sharpness', 'detect', 'detect_frames',
          'detect_frames_padded', 'detect_frames_with_crops', 'detect_padded', 'detect_tiled', 'detect_tiled_padded',
          'detect_tiled_with_crops', 'detect_tiles_padded', 'draw_plates', 'drop_engine', 'encode_jpeg', 'encode_jpeg_padded',
          'engine_for', 'eval_counts', 'hw_pair', 'is_nv12_list', 'jpeg_stats', 'letterbox_placement', 'merge_tiles',
          'merge_tiles_buffers', 'model_forward', 'nms_candidates', 'nms_padded', 'non_max_suppression', 'nv12_to_bgr', 'plan_frames',
          'plan_tiled', 'plate_crops', 'prepare_for', 'preprocess_frames', 'preprocess_letterbox', 'preprocess_tiles', 'redact_plates',
          'rescale_round', 'rescale_round_batch', 'tiles_per_frame']
#: names of other packages among them: they have no owning module in the package
FOREIGN = ['LookbackHost', 'Nv12Frame', 'hw_pair', 'is_nv12_list', 'letterbox_placement', 'plan_frames', 'tiles_per_frame']
#: the private names that code outside the module used on that commit (``_f32`` and ``_DT``: by tests)
PRIVATE = ['_unpad', '_unpad_with_crops', '_crop_size', '_stream_ptr', '_engines', '_redact_workspace', '_gauss_params',
           '_stream_workspace', '_overlay_ws', '_overlay_params', '_f32', '_DT']
#: module-level state: created once in its module, re-exported by reference
STATE = {'_engines': 'engine', '_nms_ws': 'nms', '_redact_ws': 'redact', '_overlay_ws': 'overlay', '_overlay_params_memo': 'overlay',
         '_jpeg_ws': 'jpeg', '_tile_inputs': 'tiles', 'jpeg_stats': 'jpeg'}


def _sub(name):
    return importlib.import_module('yolov6.hip.runtime.' + name)


def test_surface():
    from yolov6.hip import runtime
    for n in PUBLIC + PRIVATE + list(STATE):
        assert hasattr(runtime, n), n
    owned = set()
    for m in MODULES:
        sub = _sub(m)
        assert getattr(runtime, m) is sub
        for n in PUBLIC + PRIVATE + list(STATE):
            if n in vars(sub):
                assert getattr(runtime, n) is getattr(sub, n), (m, n)
                owned.add(n)
    assert owned - set(FOREIGN) == set(PUBLIC + PRIVATE + list(STATE)) - set(FOREIGN)
    for n, m in STATE.items():
        assert getattr(runtime, n) is vars(_sub(m))[n], n
        assert isinstance(getattr(runtime, n), (dict, type(runtime._engines))), n
    # a function's globals are its owning module's: the dict it mutates is the one the facade hands out
    assert runtime.engine_for.__globals__['_engines'] is runtime._engines
    assert runtime.draw_plates.__globals__['_overlay_ws'] is runtime._overlay_ws
    assert runtime.encode_jpeg.__globals__['jpeg_stats'] is runtime.jpeg_stats
    assert runtime.Engine.__module__ == 'yolov6.hip.runtime.engine'


@pytest.mark.parametrize('name', MODULES)
def test_module_imports_alone(name):
    """Each module in a fresh interpreter: no cycle, no reliance on what another import happened to load first."""
    r = subprocess.run([sys.executable, '-c', 'import yolov6.hip.runtime.%s' % name], cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_import_graph_is_ordered():
    """Read from the sources: a module's relative imports name only modules before it in ``MODULES``, all at module level; the
    facade has nothing but imports; and the library is reached as ``abi.load()``, which the GPU tests replace."""
    pkg = os.path.join(REPO, 'yolo-lp_amd', 'yolov6', 'hip', 'runtime')
    assert sorted(f[:-3] for f in os.listdir(pkg) if f.endswith('.py')) == sorted(MODULES + ['__init__'])
    for k, m in enumerate(MODULES):
        tree = ast.parse(open(os.path.join(pkg, m + '.py')).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level:
                assert node in tree.body, '%s: relative import inside a function' % m
                assert node.level == 1 and node.module in MODULES[:k], '%s imports from %s' % (m, node.module)
            if isinstance(node, ast.ImportFrom):
                assert not any(a.name in ('*', 'load') for a in node.names), m
    facade = ast.parse(open(os.path.join(pkg, '__init__.py')).read())
    assert all(isinstance(n, ast.ImportFrom) or (isinstance(n, ast.Expr) and isinstance(n.value, ast.Constant)) for n in facade.body)
    assert not any(a.name == '*' for n in facade.body if isinstance(n, ast.ImportFrom) for a in n.names)


def test_runs_by_key():
    from yolov6.hip.runtime._base import _runs_by_key
    assert _runs_by_key([]) == []
    assert _runs_by_key(['a', 'a', 'b', 'a']) == [(0, 2), (2, 3), (3, 4)]
    assert _runs_by_key([None] * 3) == [(0, 3)]


def test_runs_under_cap():
    from yolov6.hip.runtime._base import _runs_under_cap
    assert _runs_under_cap([5, 5], 10) == [(0, 2)]                                       # the bound is inclusive
    assert _runs_under_cap([5, 5, 5, 11, 1], 10) == [(0, 2), (2, 3), (3, 4), (4, 5)]     # an item above the cap goes alone
    assert _runs_under_cap([3, 3, 3], 1) == [(0, 1), (1, 2), (2, 3)]
    assert _runs_under_cap([], 10) == []


def test_plane_descs_and_desc_run():
    from yolov6.hip import abi
    from yolov6.hip.runtime._base import _desc_run, _plane_descs
    frames = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in ((4, 6), (7, 5), (3, 9))]
    desc = _plane_descs(abi.RedactDesc, frames, False)
    assert len(desc) == 3 and isinstance(desc[0], abi.RedactDesc)
    for d, f in zip(desc, frames):
        assert d.p0 == f.data_ptr() and d.p1 is None
        assert (d.pitch0, d.pitch1, d.format, d.h0, d.w0) == (3 * f.shape[1], 0, 0, f.shape[0], f.shape[1])
    run = _desc_run(desc, 2)
    assert isinstance(run, ctypes.POINTER(abi.RedactDesc))
    assert (run[0].h0, run[0].w0, run[0].p0) == (3, 9, frames[2].data_ptr())
    assert ctypes.addressof(run.contents) == ctypes.addressof(desc) + 2 * ctypes.sizeof(abi.RedactDesc)
    first = _desc_run(desc, 0)
    assert (first[1].h0, first[1].w0) == (7, 5)


def test_aligned_span():
    from yolov6.hip.runtime._base import _aligned_span
    ws = torch.zeros(1000, dtype=torch.uint8)
    base, nbytes = _aligned_span(ws)
    assert isinstance(base, ctypes.c_void_p)
    assert base.value % 256 == 0 and base.value >= ws.data_ptr()
    assert base.value + nbytes == ws.data_ptr() + 1000
    assert base.value - ws.data_ptr() < 256
