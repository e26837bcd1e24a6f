"""The overlay on the GPU: lp_overlay_draw_batch (runtime.draw_plates) byte for byte against the numpy specification
(yolov6/utils/overlay.py): a sweep over shapes, thicknesses, opacities, counts, ids, styles and palettes with guard and padding
bytes, poisoned status and workspace; a cull list longer than one chunk; the 64-frame split; composition on the device; graph
capture; every argument error; behind detect_frames_padded and PlateTracker.update on the tiny golden model, and into encode_jpeg;
and Inferer(overlay=True) at batch sizes 1 and 4."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
from test_overlay_cpu import row_of, seeded_font
from test_redact_cpu import quad_rows
from test_redact_gpu import bgr_buffer, expect_buffer, host_frames, nv12_buffer

pytestmark = pytest.mark.gpu

CFG = lambda n: os.path.join(REPO, 'configs', n + '.py')   # noqa: E731
ST_POISON = -7
MAX_DET = 12
COUNTS = [-1, 0, 5, 12, MAX_DET + 3]
BGR_SHAPES = [(33, 65), (64, 96), (1, 1), (5, 200), (37, 53)]
NV12_SHAPES = [(38, 54, 70, 60), (66, 130, 140, 134), (2, 2, 5, 6)]        # h, w, pitch_y, pitch_uv
FONTS = [seeded_font(11, 7, 5, 40), seeded_font(12, 16, 9, 21)]
PALETTE = np.array([[9, 99, 199], [250, 150, 50], [77, 7, 177]], np.uint8)


def styles_for(t, a):
    from yolov6.utils.overlay import Style
    return [Style((10, 200, 30), (250, 40, 90), (60, 70, 200), (240, 250, 5), t, a, a, a, 1),
            Style((0, 0, 255), (255, 0, 0), (1, 2, 3), (200, 100, 50), max(t - 1, 0), 256 - a, a, 131, 3)]


def overlay_rows(shapes, n, seed):
    """det [B, n, 28] on the device: the quads of the redaction tests with head columns that exercise the label: ids 0..63, and per
    frame a NaN, a -1, a 64 and a 1e30.  Frame (64, 96) gets a row that straddles the tile corner at (32, 32), whose label
    crosses the tile edge at x = 32."""
    rng = np.random.default_rng(seed)
    det = np.stack([quad_rows(s[0], s[1], n, seed + b) for b, s in enumerate(shapes)])
    det[:, :, 20:28] = rng.integers(0, 64, det[:, :, 20:28].shape)
    det[:, 0, 20:24] = [np.nan, -1.0, 64.0, 1e30]
    for b, s in enumerate(shapes):
        if (s[0], s[1]) == (64, 96):
            det[b, 1] = row_of((25, 26, 42, 38), ((26, 28), (40, 27), (41, 36), (27, 37)), heads=(7, 9, 63, 0, 1, 2, 3, 4))
    return torch.from_numpy(det).cuda()


def ids_for(B, n, seed):
    rng = np.random.default_rng(seed)
    tid = rng.integers(-1, 40, (B, n)).astype(np.int32)
    tid[:, 0] = [(-1, 0, 9, 10, 2 ** 31 - 1)[b % 5] for b in range(B)]
    style = rng.integers(-1, 3, (B, n)).astype(np.int32)                   # -1 skips, 2 is past the last style
    return torch.from_numpy(tid).cuda(), torch.from_numpy(style).cuda()


def check_call(buf, frames, det, count, font, fonts_np, ws_poison=(0xA5, 0x00), **kw):
    """draw_plates on ``frames`` (views of ``buf``) with the workspace and the status poisoned, once per workspace poison from the
    same start: every byte of the buffer and every status must be the specification's.  Returns the number of changed bytes."""
    from yolov6.hip import runtime
    from yolov6.utils.overlay import draw_plates_np
    start = buf.clone()
    host_kw = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in kw.items()}
    want, want_st = draw_plates_np(host_frames(frames), det.cpu().numpy(), count.cpu().numpy(), *fonts_np, **host_kw)
    want_buf = expect_buffer(buf, start, frames, want)
    for poison in ws_poison:
        buf.copy_(start)
        runtime._stream_workspace(runtime._overlay_ws, buf.device, 1 << 20).fill_(poison)
        status = torch.full((len(frames), det.shape[1]), ST_POISON, dtype=torch.int32, device='cuda')
        got_st = runtime.draw_plates(frames, det, count, font, status=status, **kw)
        torch.cuda.synchronize()
        assert got_st.data_ptr() == status.data_ptr()
        assert np.array_equal(status.cpu().numpy(), want_st)
        assert torch.equal(buf, want_buf)                           # the frames, and every guard and padding byte
    changed = int((want_buf != start).sum())
    buf.copy_(start)
    return changed


@pytest.fixture(scope='module')
def fonts():
    from yolov6.hip import runtime
    return [runtime.OverlayFont(a, g) for a, g in FONTS]


CASES = [(t, a) for t in (0, 1, 2, 16) for a in (0, 97, 256)]


@pytest.mark.parametrize('k', range(len(CASES)), ids=['t%d-a%d' % c for c in CASES])
def test_kernels_equal_specification(k, fonts):
    t, a = CASES[k]
    f = k % 2
    kw = dict(styles=styles_for(t, a))
    tid, style = ids_for(5, MAX_DET, 50 + k)
    if k % 4 >= 1:
        kw['tid'] = tid
    if k % 4 >= 2:
        kw['style'] = style
    if k % 3 >= 1:
        kw['palette'] = PALETTE
    kw.update(show_id=k % 5 != 4, draw_box=k % 6 != 5)
    buf, frames = bgr_buffer(BGR_SHAPES, 100 + k)
    count = torch.tensor([COUNTS[(b + k) % 5] for b in range(5)], dtype=torch.int32, device='cuda')
    changed = check_call(buf, frames, overlay_rows(BGR_SHAPES, MAX_DET, 200 + 10 * k), count, fonts[f], FONTS[f], **kw)
    nbuf, nframes = nv12_buffer(NV12_SHAPES, 300 + k)
    ncount = torch.tensor([COUNTS[(b + k + 3) % 5] for b in range(3)], dtype=torch.int32, device='cuda')
    nkw = {key: (v[:3] if torch.is_tensor(v) else v) for key, v in kw.items()}
    changed += check_call(nbuf, nframes, overlay_rows(NV12_SHAPES, MAX_DET, 400 + 10 * k), ncount, fonts[1 - f], FONTS[1 - f], **nkw)
    assert (changed > 0) == (a > 0 or 'style' in kw)                   # style 1 draws its outlines at opacity 256 - a


def test_every_count_on_every_frame(fonts):
    """The sweep rotates the counts over the frames; here the two largest frames of each kind take every count, without labels too."""
    for c in COUNTS:
        buf, frames = bgr_buffer(BGR_SHAPES[:2], 500)
        count = torch.tensor([c, c], dtype=torch.int32, device='cuda')
        kw = dict(styles=styles_for(2, 200), label=c != 12)
        changed = check_call(buf, frames, overlay_rows(BGR_SHAPES[:2], MAX_DET, 510), count, fonts[0], FONTS[0], ws_poison=(0xA5,), **kw)
        nbuf, nframes = nv12_buffer(NV12_SHAPES[:2], 520)
        changed += check_call(nbuf, nframes, overlay_rows(NV12_SHAPES[:2], MAX_DET, 530), count, fonts[0], FONTS[0], ws_poison=(0xA5,), **kw)
        assert (changed > 0) == (c > 0)


def test_two_nv12_matrices_in_one_list(fonts):
    """Colours are given as BGR and drawn in the frame's own bytes: two matrices in one list are two runs of the entry point."""
    nbuf, nframes = nv12_buffer([(38, 54, 70, 60), (38, 54, 54, 54), (2, 2, 5, 6)], 540)
    nframes[1].matrix = 'bt601f'
    count = torch.tensor([12, 12, 1], dtype=torch.int32, device='cuda')
    tid, _ = ids_for(3, MAX_DET, 541)
    assert check_call(nbuf, nframes, overlay_rows([(38, 54)] * 2 + [(2, 2)], MAX_DET, 550), count, fonts[0], FONTS[0],
                      styles=styles_for(2, 256), tid=tid, palette=PALETTE) > 0


def test_cull_list_longer_than_one_chunk(fonts):
    """300 live rows, all small, on a 64 x 64 frame: the cull runs two chunks, and row order holds across them."""
    n = 300
    rng = np.random.default_rng(560)
    det = np.zeros((1, n, 28), np.float32)
    det[:, :, 4:12] = np.nan
    x1, y1 = rng.integers(0, 56, n), rng.integers(0, 56, n)
    det[0, :, 0], det[0, :, 1] = x1, y1
    det[0, :, 2], det[0, :, 3] = x1 + rng.integers(2, 9, n), y1 + rng.integers(2, 9, n)
    det[0, :, 20:28] = rng.integers(0, 64, (n, 8))
    style = torch.from_numpy((np.arange(n) % 2).astype(np.int32)[None]).cuda()
    count = torch.tensor([n], dtype=torch.int32, device='cuda')
    for shapes, make in (([(64, 64)], bgr_buffer), ([(64, 64, 64, 64)], nv12_buffer)):
        buf, frames = make(shapes, 561)
        assert check_call(buf, frames, torch.from_numpy(det).cuda(), count, fonts[0], FONTS[0], ws_poison=(0xA5,),
                          styles=styles_for(1, 97), style=style, label=False) > 0
    buf, frames = bgr_buffer([(64, 64)], 562)
    assert check_call(buf, frames, torch.from_numpy(det).cuda(), count, fonts[0], FONTS[0], ws_poison=(0xA5,),
                      styles=styles_for(1, 200), style=style) > 0


def test_crosses_the_64_frame_split(fonts):
    det = torch.zeros(65, 3, 28, device='cuda')
    det[:, :, 4:12] = float('nan')
    det[:, 0, :4] = torch.tensor([0.0, 0.0, 2.0, 2.0])
    det[:, 1, :4] = torch.tensor([0.0, 0.0, 1.0, 1.5])
    count = torch.from_numpy((np.arange(65) % 3).astype(np.int32)).cuda()
    tid = torch.from_numpy(np.arange(65 * 3, dtype=np.int32).reshape(65, 3)).cuda()
    kw = dict(styles=styles_for(1, 256), tid=tid, palette=PALETTE)
    buf, frames = bgr_buffer([(2, 2)] * 65, 600)
    assert check_call(buf, frames, det, count, fonts[0], FONTS[0], **kw) > 65
    nbuf, nframes = nv12_buffer([(2, 2, 2, 2)] * 65, 602)
    assert check_call(nbuf, nframes, det, count, fonts[0], FONTS[0], **kw) > 65


@pytest.mark.parametrize('nv12', [False, True], ids=['bgr', 'nv12'])
def test_one_call_with_12_rows_equals_12_calls(nv12, fonts):
    from yolov6.hip import runtime
    shapes = [(66, 130, 140, 134)] if nv12 else [(64, 96)]
    buf, frames = (nv12_buffer if nv12 else bgr_buffer)(shapes, 650)
    det = overlay_rows(shapes, MAX_DET, 651)
    tid, style = ids_for(1, MAX_DET, 652)
    kw = dict(styles=styles_for(3, 97), palette=PALETTE)
    start = buf.clone()
    st = runtime.draw_plates(frames, det, torch.tensor([12], dtype=torch.int32, device='cuda'), fonts[1], tid=tid, style=style, **kw)
    once = buf.clone()
    buf.copy_(start)
    one = torch.ones(1, dtype=torch.int32, device='cuda')
    for r in range(12):
        st1 = runtime.draw_plates(frames, det[:, r:r + 1].contiguous(), one, fonts[1], tid=tid[:, r:r + 1].contiguous(),
                                  style=style[:, r:r + 1].contiguous(), **kw)
        assert int(st1[0, 0]) == int(st[0, r])
    torch.cuda.synchronize()
    assert torch.equal(buf, once) and not torch.equal(once, start)


def test_draw_plates_graph_capture(fonts):
    from yolov6.hip import runtime
    from yolov6.utils.overlay import draw_plates_np
    buf, frames = bgr_buffer(BGR_SHAPES, 700)
    det = overlay_rows(BGR_SHAPES, MAX_DET, 710)
    count = torch.tensor([12, 5, 3, 12, 7], dtype=torch.int32, device='cuda')
    tid, style = ids_for(5, MAX_DET, 711)
    status = torch.empty(5, MAX_DET, dtype=torch.int32, device='cuda')
    kw = dict(styles=styles_for(2, 160), palette=PALETTE)
    runtime.draw_plates(frames, det, count, fonts[0], tid=tid, style=style, status=status, **kw)     # eager once: code loaded, workspace allocated
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                           # one stream, no parallel branches
        runtime.draw_plates(frames, det, count, fonts[0], tid=tid, style=style, status=status, **kw)
    rng = np.random.default_rng(720)
    start = torch.from_numpy(rng.integers(0, 256, buf.numel(), dtype=np.uint8)).cuda()     # new pixels, rows, ids and counts, same buffers
    buf.copy_(start)
    det.copy_(overlay_rows(BGR_SHAPES, MAX_DET, 730))
    count.copy_(torch.tensor([2, 12, 12, 0, 12], dtype=torch.int32))
    tid2, style2 = ids_for(5, MAX_DET, 731)
    tid.copy_(tid2)
    style.copy_(style2)
    status.fill_(ST_POISON)
    want, want_st = draw_plates_np(host_frames(frames), det.cpu().numpy(), count.cpu().numpy(), *FONTS[0], tid=tid.cpu().numpy(),
                                   style=style.cpu().numpy(), **kw)
    want_buf = expect_buffer(buf, start, frames, want)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(status.cpu().numpy(), want_st)
    assert torch.equal(buf, want_buf) and not torch.equal(buf, start)


def test_argument_errors_leave_the_frames_alone(fonts):
    from yolov6.hip import abi, runtime
    lib = abi.load()
    buf, frames = bgr_buffer([(37, 53), (64, 96)], 800)
    nbuf, nframes = nv12_buffer(NV12_SHAPES[:2], 801)
    start, nstart = buf.clone(), nbuf.clone()
    det = overlay_rows([(37, 53), (64, 96)], MAX_DET, 810)
    count = torch.tensor([12, 12], dtype=torch.int32, device='cuda')
    status = torch.full((2, MAX_DET), ST_POISON, dtype=torch.int32, device='cuda')
    ws = torch.empty(1 << 16, dtype=torch.uint8, device='cuda')
    assert ws.data_ptr() % 16 == 0
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    font = fonts[0]
    good = runtime._overlay_params(font, styles_for(2, 97), PALETTE, None, True, True, True)

    def descs(nv12):
        d = (abi.RedactDesc * 2)()
        for e, f in zip(d, nframes if nv12 else frames):
            if nv12:
                e.p0, e.p1, e.pitch0, e.pitch1, e.format = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, 1
            else:
                e.p0, e.p1, e.pitch0, e.format = f.data_ptr(), None, 3 * f.shape[1], 0
            e.h0, e.w0 = f.shape[0], f.shape[1]
        return d

    def call(nv12=False, mods=(), par=(), sty=(), **over):
        """The entry point on good arguments with some replaced: mods = ((frame, field, value), ...) on the descriptors, par =
        ((field, value), ...) on the parameters, sty = ((style, field, value), ...) on their styles, anything else by name."""
        d = descs(nv12)
        for b, field, value in mods:
            setattr(d[b], field, value)
        p = abi.OverlayParams.from_buffer_copy(good)
        for field, value in par:
            setattr(p, field, value)
        for s, field, value in sty:
            setattr(p.styles[s], field, value)
        a = dict(desc=d, n=2, det=det.data_ptr(), count=count.data_ptr(), max_det=MAX_DET, tid=None, style=None, p=ctypes.byref(p),
                 atlas=font.atlas.data_ptr(), glyph_of=font.glyph_of.data_ptr(), status=status.data_ptr(), ws=ws.data_ptr(),
                 ws_bytes=ws.numel())
        a.update(over)
        return lib.lp_overlay_draw_batch(a['desc'], a['n'], a['det'], a['count'], a['max_det'], a['tid'], a['style'], a['p'], a['atlas'],
                                         a['glyph_of'], a['status'], a['ws'], a['ws_bytes'], stream)

    need = lib.lp_overlay_workspace_bytes(2, MAX_DET)
    assert need == 2 * MAX_DET * 288 and lib.lp_overlay_workspace_bytes(0, MAX_DET) == 0 and lib.lp_overlay_workspace_bytes(2, 0) == 0
    uv1 = nframes[1].uv.data_ptr()
    bad = [dict(desc=None), dict(p=None), dict(status=None), dict(det=None), dict(count=None), dict(atlas=None), dict(glyph_of=None),
           dict(max_det=0), dict(n=-1),
           dict(mods=((1, 'format', 2),)), dict(mods=((1, 'format', -1),)), dict(mods=((1, 'p0', None),)),
           dict(mods=((1, 'p1', frames[0].data_ptr()),)), dict(mods=((1, 'pitch0', 3 * 96 - 1),)), dict(mods=((1, 'h0', 0),)),
           dict(mods=((1, 'w0', 0),)), dict(mods=((0, 'w0', -5),)),
           dict(nv12=True, mods=((1, 'p1', None),)), dict(nv12=True, mods=((1, 'p0', None),)), dict(nv12=True, mods=((1, 'h0', 3),)),
           dict(nv12=True, mods=((1, 'w0', 1),)), dict(nv12=True, mods=((1, 'h0', 0),)), dict(nv12=True, mods=((1, 'pitch0', 1),)),
           dict(nv12=True, mods=((1, 'pitch1', 1),)), dict(nv12=True, mods=((0, 'pitch1', 61),)),
           dict(nv12=True, mods=((1, 'p1', uv1 + 1),)),
           dict(par=(('n_styles', 0),)), dict(par=(('n_styles', 9),)), dict(par=(('n_palette', -1),)), dict(par=(('n_palette', 65),)),
           dict(par=(('n_glyphs', 12),)), dict(par=(('n_glyphs', 1025),)), dict(par=(('gh', 0),)), dict(par=(('gh', 65),)),
           dict(par=(('gw', 0),)), dict(par=(('gw', 65),)),
           dict(sty=((0, 't', -1),)), dict(sty=((1, 't', 17),)), dict(sty=((0, 'pad', -1),)), dict(sty=((1, 'pad', 17),)),
           dict(sty=((0, 'a_line', 257),)), dict(sty=((0, 'a_plate', -1),)), dict(sty=((1, 'a_text', 300),)),
           dict(ws=None), dict(ws=ws.data_ptr() + 8), dict(ws_bytes=need - 1)]
    for kw in bad:
        rc = call(**kw)
        assert rc == -1, kw                                             # LP_ERR_ARG
        with pytest.raises(RuntimeError) as e:
            abi.check(rc, 'lp_overlay_draw_batch')
        if kw.get('mods'):
            assert 'frame %d' % kw['mods'][0][0] in str(e.value), (kw, str(e.value))
    torch.cuda.synchronize()
    assert torch.equal(buf, start) and torch.equal(nbuf, nstart) and bool((status == ST_POISON).all())
    # what is no error: no frames; a style past n_styles with bad fields; exactly the bytes asked for
    assert call(n=0) == 0 and call(n=0, det=None, count=None) == 0
    assert call(par=(('n_styles', 1),), sty=((1, 't', 99),), ws_bytes=need) == 0
    torch.cuda.synchronize()
    assert not torch.equal(buf, start)
    # the runtime's own checks
    with pytest.raises(ValueError):
        runtime.draw_plates(frames, det, count, font, tid=torch.zeros(2, MAX_DET, device='cuda'))
    with pytest.raises(ValueError):
        runtime.draw_plates(frames, det, count, font, styles=styles_for(2, 97) * 5)
    with pytest.raises(ValueError):
        runtime.draw_plates([], det, count, font)


def _tiny_golden_model():
    from yolov6.utils.synth import build_synthetic
    m = build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5)
    m.load_state_dict(load_golden('lps_tiny_weights'))
    return m.eval().cuda()


def test_behind_the_detector_and_the_tracker_and_into_the_encoder(fonts):
    from yolov6.hip import runtime
    from yolov6.utils.jpeg import encode_jpeg_np
    from yolov6.utils.overlay import draw_plates_np
    m = _tiny_golden_model()
    rng = np.random.default_rng(900)
    host = [rng.integers(0, 256, (120, 96, 3), dtype=np.uint8) for _ in range(3)]
    kw = dict(styles=styles_for(2, 160), palette=PALETTE)
    with torch.no_grad():
        frames = [torch.from_numpy(f).cuda() for f in host]
        det, count = runtime.detect_frames_padded(m, frames, [128, 128], 0.06, 0.45, 20)
        tracker = runtime.PlateTracker(3, device=frames[0].device)
        det_out, tid = tracker.update(det, count)[:2]
        status = runtime.draw_plates(frames, det_out, count, fonts[1], tid=tid, **kw)
        files = runtime.encode_jpeg(frames, 85, 16)
        torch.cuda.synchronize()
        count_h = count.cpu().numpy()
        assert count_h.min() > 0 and int(tid.max()) >= 0
        want, want_st = draw_plates_np(host, det_out.cpu().numpy(), count_h, *FONTS[1], tid=tid.cpu().numpy(), **kw)
        assert np.array_equal(status.cpu().numpy(), want_st) and (want_st[0, :count_h[0]] > 0).all()
        for f, w, h, data in zip(frames, want, host, files):
            assert np.array_equal(f.cpu().numpy(), w) and (w != h).any()
            assert data == encode_jpeg_np(w, 85, 16)


def test_infer_overlay_batch_size_1_and_4(tmp_path, monkeypatch):
    """Inferer(overlay=True) on a GPU, one frame at a time and four, BGR and NV12: the same files, and the files the CPU path of
    the overlay (draw_plates_np with the Inferer's own font and styles) writes for the rows returned; with save_jpeg the files of
    ``encode_jpeg_np`` of those frames.  (The detections of the CPU model itself may differ from the GPU's by a pixel at a
    rounding boundary, so the rows are the GPU's.)"""
    from PIL import Image
    from yolov6.utils.jpeg import encode_jpeg_np
    from yolov6.utils.nv12 import bgr_to_nv12_np, nv12_to_bgr_np
    from yolov6.utils.overlay import build_atlas, draw_plates_np
    from yolov6.utils.synth import build_synthetic
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    from yolov6.core.inferer import Inferer
    ckpt = tmp_path / 'tiny.pt'
    torch.save({'model': build_synthetic(CFG('yololps'), width=0.0625, sigma=1.5).half(), 'ema': None}, str(ckpt))
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    rng = np.random.default_rng(12)
    shapes = [(232, 144), (232, 144), (232, 144), (150, 250), (150, 250), (232, 144), (100, 60)]
    frames = []
    for i, (h, w) in enumerate(shapes):
        frames.append(rng.integers(0, 255, (h, w, 3), dtype=np.uint8))
        Image.fromarray(frames[-1]).save(str(img_dir / ('f%d.png' % i)))
    kw = dict(weights=str(ckpt), source=str(img_dir), yaml=None, img_size=[128, 128], conf_thres=0.06, iou_thres=0.45,
              max_det=20, device='0', not_save_img=True, overlay=True, overlay_size=12)
    plain = infer.run(save_dir=str(tmp_path / 'plain'), **dict(kw, overlay=False))
    assert not (tmp_path / 'plain' / 'annotated').exists()
    runs = dict(o1=dict(), o4=dict(batch_size=4), n4=dict(batch_size=4, nv12='bt709'), j4=dict(batch_size=4, save_jpeg=85),
                t1=dict(track=True), t4=dict(batch_size=4, track=True), h4=dict(batch_size=4, track=True, redact='fill', redact_hold=True))
    dets = {tag: infer.run(save_dir=str(tmp_path / tag), **kw, **extra) for tag, extra in runs.items()}
    assert sum(len(d) for d in dets['o1']) > 0
    font, styles = build_atlas([], [], [], 12, None), Inferer.make_overlay_styles(12, 2, (256, 160, 256))
    for i, f in enumerate(frames):
        assert torch.equal(dets['o1'][i], plain[i]) and torch.equal(dets['o1'][i], dets['o4'][i]) and torch.equal(dets['o1'][i], dets['j4'][i])
        name = 'f%d.png' % i
        assert (tmp_path / 'o1' / 'annotated' / name).read_bytes() == (tmp_path / 'o4' / 'annotated' / name).read_bytes()
        for tag in ('o1', 'n4', 'j4', 't1', 't4'):
            d = dets[tag][i].cpu().numpy()
            det = np.zeros((1, max(len(d), 1), 28), np.float32)
            det[0, :len(d)] = d
            src = np.ascontiguousarray(f[:, :, ::-1])
            if tag in ('t1', 't4'):      # the voted rows returned, the ids of tracks.txt, the palette
                tid = np.full((1, det.shape[1]), -1, np.int32)
                for line in (tmp_path / tag / 'tracks.txt').read_text().splitlines():
                    path, r, t = line.rsplit(' ', 2)
                    if os.path.basename(path) == name:
                        tid[0, int(r)] = int(t)
                assert len(d) == 0 or tid[0, :len(d)].max() >= 0
                (want,), _ = draw_plates_np([src], det, [len(d)], *font, tid=tid, styles=styles, palette=np.array(Inferer.OVERLAY_PALETTE, np.uint8))
            elif tag == 'n4':
                (want,), _ = draw_plates_np([bgr_to_nv12_np(src, 'bt709')], det, [len(d)], *font, styles=styles)
                want = nv12_to_bgr_np(want)
            else:
                (want,), _ = draw_plates_np([src], det, [len(d)], *font, styles=styles)
            if len(d):
                assert (want != src).any()
            if tag == 'j4':
                assert (tmp_path / tag / 'annotated' / ('f%d.jpg' % i)).read_bytes() == encode_jpeg_np(want, 85, 16)
            else:
                got = np.asarray(Image.open(str(tmp_path / tag / 'annotated' / name)))
                assert np.array_equal(got, want[:, :, ::-1])
        assert Image.open(str(tmp_path / 'h4' / 'annotated' / name)).size == (f.shape[1], f.shape[0])      # with the hold: the files are there
