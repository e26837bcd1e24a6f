"""The scene overlay on the GPU: lp_overlay_scene_batch (runtime.draw_scene) byte for byte against the numpy specification
(yolov6/utils/scene.py), guard and padding bytes included, with the workspace and the status poisoned: frames across the 32 x 32 tile
seams, the last partial tile and the last odd 2 x 2 block; zones that straddle, fill and cover; the LDS list at its maximum; the
style edges; the numbers at their edges; the tag lookup; full-mantissa vertices on which a contraction decides pixels; batches of
two streams, two NV12 matrices and more than one launch; the tracker end to end; ``tools/infer.py --overlay-scene``;
``draw_plates`` after the shared-include refactor; every argument error."""
import ctypes
import os

import numpy as np
import pytest
import torch

import test_scene_cpu as C
import test_track_cpu as T
import test_zones_cpu as Z
from test_overlay_cpu import row_of, seeded_font
from test_redact_gpu import bgr_buffer, expect_buffer, host_frames, nv12_buffer

pytestmark = pytest.mark.gpu

ST_POISON = -7
BGR_SHAPES = [(37, 53), (64, 96)]
NV12_SHAPES = [(48, 64, 70, 66), (34, 66, 80, 72)]          # h, w, pitch_y, pitch_uv: a row pitch above the width
ATLASES = [C.seeded_atlas(7, 24, 7, 5), C.seeded_atlas(8, 19, 16, 9)]
STAR = [(32 + (30 if k % 2 == 0 else 11) * np.cos(k * np.pi / 8), 30 + (27 if k % 2 == 0 else 9) * np.sin(k * np.pi / 8)) for k in range(16)]


def style_for(t=2, marker=9, a=(60, 131, 200, 97, 256), pad=1):
    from yolov6.utils.scene import SceneStyle
    return SceneStyle((200, 160, 0), (0, 0, 255), (0, 255, 255), (9, 200, 90), (32, 40, 50), (255, 250, 245), (96, 0, 96), t, marker, *a, pad)


def geometry(h, w, kind):
    """(lines, zones) of one stream for an h x w frame."""
    if kind == 'straddle':      # a zone across x = 32 and y = 32, one inside a tile, vertices on pixel centres, lines across the seams
        return ([(5, h - 6.5, w - 4, h - 11.25), (30.5, 4.5, 30.5, 28.5), (w + 5, 3, w - 9, 20)],
                [([(20.5, 18.5), (45.25, 21), (43, 44.5), (24, 40.75)], 2), ([(3, 3), (14.5, 4.5), (9, 15)], 0)])
    if kind == 'cover':         # the whole frame and beyond; the 16-vertex concave polygon over it
        return ([(w / 2, h / 2, w / 2, h / 2)], [([(-3, -3), (w + 3, -2), (w + 2, h + 3), (-2, h + 2)], 1), (STAR, 0)])
    if kind == 'max':           # 8 zones and 16 lines: the list at its maximum
        rng = np.random.default_rng(h * 1000 + w)
        zs = [([(rng.uniform(-4, w + 4), rng.uniform(-4, h + 4)) for _ in range(3 + (5 * z) % 14)], z % 3) for z in range(8)]
        zs[3] = (STAR, 0)
        ls = [tuple(rng.uniform(-6, max(h, w) + 6, 4)) for _ in range(16)]
        return ls, zs
    return [], []


def scene_inputs(S, max_events=6, seed=1, T_=6):
    """totals / occ / events / speed rows of S streams with the numbers at their edges."""
    rng = np.random.default_rng(seed)
    edge = np.array([0, 9, 10, 2 ** 31 - 1, -1], np.int64).astype(np.int32)
    totals = edge[rng.integers(0, 5, (S, 2, 16))]
    totals[0, 0, :5], totals[0, 1, :5] = edge, edge[::-1]
    occ = edge[rng.integers(0, 5, (S, 8))]
    occ[0, :5] = edge
    ev = rng.integers(0, 8, (S, max_events, 12)).astype(np.int32)
    ev[:, :, 0] = rng.integers(1, 6, (S, max_events))
    ev[0, 0, :2], ev[0, max_events - 1, :2] = (4, 1), (4, 0)
    cnt = np.array([(max_events - 1, max_events + 3, 0, -2)[s % 4] for s in range(S)], np.int32)
    speed_i = np.zeros((S, T_, 8), np.int32)
    speed_i[:, :, 0] = -1
    for s in range(S):
        speed_i[s, :5, 0] = (7, 7, 7, 8, 9)
        speed_i[s, :5, 1] = (-1, 1249 + s, 27778, 0, 1250)     # id 7: slot 0 has no estimate, slot 1 wins over slot 2
    return totals, occ, ev, cnt, speed_i


def tag_rows(shapes, max_det, seed):
    """det / count / tid: boxes and quads inside and at the right edge, a status-3 row, ids with two slots, one slot, none."""
    rng = np.random.default_rng(seed)
    B = len(shapes)
    det = np.zeros((B, max_det, 28), np.float32)
    tid = np.full((B, max_det), -1, np.int32)
    for b, s in enumerate(shapes):
        h, w = s[0], s[1]
        for r in range(max_det):
            x, y = rng.uniform(-4, w - 6), rng.uniform(-4, h - 4)
            bw, bh = rng.uniform(4, 14), rng.uniform(3, 8)
            det[b, r] = row_of((x, y, x + bw, y + bh), ((x + 0.5, y + 1), (x + bw, y + 0.25), (x + bw - 0.5, y + bh), (x, y + bh - 0.75)) if r % 2 else None)
            tid[b, r] = (7, 8, 9, 99, -1)[r % 5]
        det[b, 2] = row_of((3, 3, 3.5, 9))                      # status 3 with an id that has a slot
        tid[b, 2] = 7
        det[b, 0, :4] = (w - 9, 2, w - 1, 8)                    # the tag is shifted left at the right edge
    count = np.array([(max_det, max_det - 1, max_det + 2, 0)[b % 4] for b in range(B)], np.int32)
    return det, count, tid


@pytest.fixture(scope='module')
def fonts():
    from yolov6.hip import runtime
    return [runtime.SceneFont(a) for a in ATLASES]


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_scene(buf, frames, lines, polys, font, atlas, stream_of=None, names=None, inputs=None, tags=None, style=None, ws_poison=(0xA5, 0x00),
                groups=(True, True, True)):
    """draw_scene on ``frames`` (views of ``buf``) with the workspace and the status poisoned, once per workspace poison from the same
    start: every byte of the buffer and every status must be the specification's.  Returns the number of changed bytes."""
    from yolov6.hip import runtime
    from yolov6.utils.scene import draw_scene_np
    S = len(lines)
    zm = runtime.ZoneMap(S, lines, polys)
    totals, occ, ev, cnt, speed_i = inputs if inputs is not None else scene_inputs(S)
    kw_np, kw = {}, {}
    zone = [None, None, None, None]
    if groups[0]:
        kw_np.update(totals=totals, occ=occ)
        zone[2], zone[3] = cuda(occ), cuda(totals)
    if groups[1]:
        kw_np.update(zone_ev=ev, zone_count=cnt)
        zone[0], zone[1] = cuda(ev), cuda(cnt)
    if groups[0] and groups[1]:
        kw['zone'] = tuple(zone)
    else:
        assert not groups[0] and not groups[1]                     # the host API passes last_zone whole
    if groups[2] and tags is not None:
        det, count, tid = tags
        kw_np.update(speed_i=speed_i, det=det, count=count, tid=tid)
        kw.update(speed=(cuda(speed_i),), det=cuda(det), count=cuda(count), tid=cuda(tid))
    start = buf.clone()
    want, want_st = draw_scene_np(host_frames(frames), zm.packed_np, atlas, names, stream_of, style=style, **kw_np)
    want_buf = expect_buffer(buf, start, frames, want)
    for poison in ws_poison:
        buf.copy_(start)
        runtime._stream_workspace(runtime._scene_ws, buf.device, 1 << 20).fill_(poison)
        status = None
        if 'det' in kw:
            status = torch.full((len(frames), kw['det'].shape[1]), ST_POISON, dtype=torch.int32, device='cuda')
        got = runtime.draw_scene(frames, zm, font, names=names, stream_of=stream_of, style=style, status=status, **kw)
        torch.cuda.synchronize()
        if status is None:
            assert got is None and want_st is None
        else:
            assert got.data_ptr() == status.data_ptr() and np.array_equal(status.cpu().numpy(), want_st)
        assert torch.equal(buf, want_buf)                          # the frames, and every guard and padding byte
    changed = int((want_buf != start).sum())
    buf.copy_(start)
    return changed


KINDS = ['straddle', 'cover', 'max']


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('nv12', [False, True], ids=['bgr', 'nv12'])
def test_kernels_equal_specification(kind, nv12, fonts):
    shapes = NV12_SHAPES if nv12 else BGR_SHAPES
    buf, frames = (nv12_buffer if nv12 else bgr_buffer)(shapes, 100 + KINDS.index(kind))
    geo = [geometry(s[0], s[1], kind) for s in shapes]
    f = KINDS.index(kind) % 2
    max_det = 12
    changed = check_scene(buf, frames, [g[0] for g in geo], [g[1] for g in geo], fonts[f], ATLASES[f], names=C.names_for(2, 3, 19),
                          tags=tag_rows(shapes, max_det, 7), style=style_for(2 + f, 9))
    assert changed > 0


STYLE_EDGES = [(0, 0, (0, 0, 0, 0, 0)), (1, 1, (256, 256, 256, 256, 256)), (2, 64, (60, 131, 0, 256, 97)), (16, 9, (0, 256, 256, 0, 256)),
               (16, 64, (256, 0, 97, 200, 0))]


@pytest.mark.parametrize('k', range(len(STYLE_EDGES)), ids=['t%d-m%d' % e[:2] for e in STYLE_EDGES])
def test_style_edges(k, fonts):
    t, marker, a = STYLE_EDGES[k]
    geo = [geometry(s[0], s[1], ('straddle', 'max')[b]) for b, s in enumerate(BGR_SHAPES)]
    buf, frames = bgr_buffer(BGR_SHAPES, 200 + k)
    changed = check_scene(buf, frames, [g[0] for g in geo], [g[1] for g in geo], fonts[0], ATLASES[0], tags=tag_rows(BGR_SHAPES, 5, 8),
                          style=style_for(t, marker, a, pad=(0, 16, 3, 1, 2)[k]), ws_poison=(0xA5,))
    ngeo = [geometry(s[0], s[1], ('max', 'straddle')[b]) for b, s in enumerate(NV12_SHAPES)]
    nbuf, nframes = nv12_buffer(NV12_SHAPES, 210 + k)
    changed += check_scene(nbuf, nframes, [g[0] for g in ngeo], [g[1] for g in ngeo], fonts[1], ATLASES[1], tags=tag_rows(NV12_SHAPES, 5, 9),
                           style=style_for(t, marker, a), ws_poison=(0xA5,))
    assert (changed > 0) == (k > 0)                                  # every opacity 0: no byte changes


def test_absent_groups_draw_fewer_layers(fonts):
    geo = [geometry(s[0], s[1], 'straddle') for s in BGR_SHAPES]
    buf, frames = bgr_buffer(BGR_SHAPES, 300)
    n = [check_scene(buf, frames, [g[0] for g in geo], [g[1] for g in geo], fonts[0], ATLASES[0], tags=tag_rows(BGR_SHAPES, 6, 10),
                     style=style_for(), groups=g) for g in ((False, False, False), (False, False, True), (True, True, False), (True, True, True))]
    assert 0 < n[0] < n[1] < n[3] and n[0] < n[2] < n[3]
    buf, frames = bgr_buffer(BGR_SHAPES, 301)                        # a map without lines and zones: the tags alone; nothing at all
    assert check_scene(buf, frames, [[], []], [[], []], fonts[0], ATLASES[0], tags=tag_rows(BGR_SHAPES, 6, 10), style=style_for()) > 0
    assert check_scene(buf, frames, [[], []], [[], []], fonts[0], ATLASES[0], style=style_for()) == 0


def test_full_mantissa_vertices_where_a_contraction_decides_pixels(fonts):
    """The thin triangles of tests/test_scene_cpu.py::test_wrong_fused_multiply_add: on this seed either fused form of the toggle
    expression flips a pixel, so a kernel built with contraction fails here.  Seeded random fp32 lines beside them."""
    polys = [(v, 0) for v in C.fma_sliver_zones(C.FMA_SEED)]
    rng = np.random.default_rng(C.FMA_SEED)
    lines = [tuple(rng.uniform(0, 96, 4).astype(np.float32)) for _ in range(16)]
    buf, frames = bgr_buffer([(64, 96)], 400)
    assert check_scene(buf, frames, [lines], [polys], fonts[0], ATLASES[0], style=style_for(1, 7, (256, 256, 256, 97, 256))) > 0
    nbuf, nframes = nv12_buffer([(64, 96, 100, 96)], 401)
    assert check_scene(nbuf, nframes, [lines], [polys], fonts[0], ATLASES[0], style=style_for(1, 7, (256, 256, 256, 97, 256)), ws_poison=(0xA5,)) > 0


def test_two_streams_with_a_stream_of_that_repeats_and_skips(fonts):
    shapes = [(37, 53)] * 5
    buf, frames = bgr_buffer(shapes, 500)
    geo = [geometry(37, 53, 'straddle'), geometry(37, 53, 'max')]
    stream_of = [1, 0, 5, 1, -1]
    n = check_scene(buf, frames, [g[0] for g in geo], [g[1] for g in geo], fonts[0], ATLASES[0], stream_of=stream_of, names=C.names_for(2, 4, 24),
                    tags=tag_rows(shapes, 12, 11), style=style_for())
    assert n > 0


def test_two_nv12_matrices_in_one_list(fonts):
    shapes = [(34, 66, 80, 72), (34, 66, 66, 66), (48, 64, 70, 66)]
    nbuf, nframes = nv12_buffer(shapes, 510)
    nframes[1].matrix = 'bt601f'
    geo = [geometry(s[0], s[1], 'straddle') for s in shapes]
    assert check_scene(nbuf, nframes, [g[0] for g in geo], [g[1] for g in geo], fonts[1], ATLASES[1], tags=tag_rows(shapes, 4, 12),
                       style=style_for()) > 0


def test_crosses_the_64_frame_split(fonts):
    B = 65                                                           # LP_FRAMES_PER_LAUNCH + 1
    shapes = [(16, 16)] * B
    lines = [[(2, 13.5, 14, 11)], [(8, 1, 8, 15), (1, 1, 15, 15)]]
    polys = [[([(2.5, 2.5), (13, 3), (12, 12)], 0)], []]
    stream_of = [b % 3 for b in range(B)]                           # stream 2 does not exist: skipped
    buf, frames = bgr_buffer(shapes, 520)
    assert check_scene(buf, frames, lines, polys, fonts[0], ATLASES[0], stream_of=stream_of, tags=tag_rows(shapes, 3, 13), style=style_for(1, 3),
                       ws_poison=(0xA5,)) > 65
    nbuf, nframes = nv12_buffer([(16, 16, 16, 16)] * B, 521)
    assert check_scene(nbuf, nframes, lines, polys, fonts[0], ATLASES[0], stream_of=stream_of, tags=tag_rows(shapes, 3, 13), style=style_for(1, 3),
                       ws_poison=(0xA5,)) > 65


def test_tracker_end_to_end(fonts):
    """enable_zones + enable_speed over a short synthetic sequence, then tracker.draw_scene, then draw_plates, against PlateTrackerNp
    + draw_scene_np + draw_plates_np: the frames agree byte for byte."""
    import test_speed_cpu as P
    from yolov6.hip import runtime
    from yolov6.utils.overlay import draw_plates_np
    from yolov6.utils.scene import draw_scene_np
    from yolov6.utils.speed import GroundPlaneNp
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.zones import ZoneMapNp
    lines = [[(48, 0, 48, 64), (0, 40, 96, 40)], [(20, 64, 30, 0)]]
    polys = [[([(40, 10), (90, 12), (88, 60), (44, 56)], 2)], [([(5, 5), (60, 5), (60, 50), (5, 50)], 1)]]
    planes = [P.plane(), P.plane()]
    kw = dict(max_tracks=4, max_age=1)
    trk, ref = runtime.PlateTracker(2, device='cuda', **kw), PlateTrackerNp(2, **kw)
    zm = runtime.ZoneMap(2, lines, polys)
    trk.enable_zones(zm)
    ref.enable_zones(ZoneMapNp(2, lines, polys))
    trk.enable_speed(runtime.GroundPlane(2, planes))
    ref.enable_speed(GroundPlaneNp(2, planes))
    ofont = seeded_font(12, 7, 5, 24)
    odev = runtime.OverlayFont(*ofont)
    names = C.names_for(2, 5, 24)
    drawn = 0
    for k in range(6):
        rows = [[T.make_row(Z.box_at(20 + 9 * k, 30 + 2 * k, 16, 8)), T.make_row(Z.box_at(70, 20 + 6 * k, 14, 6))],
                [T.make_row(Z.box_at(50 - 7 * k, 25, 18, 8))]]
        det, count = T.frames_of(rows, 4)
        d_dev, c_dev = torch.from_numpy(det).cuda(), torch.from_numpy(count).cuda()
        det_out, tid = trk.update(d_dev, c_dev)[:2]
        r_out, r_tid = ref.update(det, count)[:2]
        buf, frames = bgr_buffer([(64, 96), (64, 96)], 600 + k)
        start = buf.clone()
        host = host_frames(frames)
        st = trk.draw_scene(frames, fonts[0], det_out, c_dev, tid, names=names, style=style_for())
        runtime.draw_plates(frames, det_out, c_dev, odev, tid=tid)
        torch.cuda.synchronize()
        zev, zcnt, zocc, ztot = ref.last_zone
        want, want_st = draw_scene_np(host, zm.packed_np, ATLASES[0], names, None, ztot, zocc, zev, zcnt, ref.last_speed[0], r_out, count, r_tid,
                                      style_for())
        want, _ = draw_plates_np(want, r_out, count, *ofont, tid=r_tid)
        assert np.array_equal(st.cpu().numpy(), want_st)
        assert torch.equal(buf, expect_buffer(buf, start, frames, want))
        drawn += int(want_st.sum())
    assert drawn > 0 and int(ref.last_zone[3].sum()) > 0 and int(ref.last_zone[2].sum()) > 0      # tags, crossings and occupancy were shown


def test_infer_tool_overlay_scene_on_the_gpu(tmp_path, monkeypatch):
    """tools/infer.py --track --overlay --overlay-scene --zones --speed on a GPU: every annotated file equals PlateTrackerNp by hand on
    the run's untracked detections + draw_scene_np + draw_plates_np; a batched run writes its files too; without the flag nothing changes."""
    from PIL import Image
    from yolov6.core.inferer import Inferer
    from yolov6.utils.overlay import build_atlas, draw_plates_np
    from yolov6.utils.scene import build_scene_atlas, draw_scene_np, names_of
    from yolov6.utils.speed import GroundPlaneNp, parse_ground
    from yolov6.utils.track import PlateTrackerNp
    from yolov6.utils.zones import ZoneMapNp, parse_zones
    infer, kw, untracked, tkw = Z.infer_zones_case(tmp_path, monkeypatch, '0', half=True)
    ground = 'plane 0.125 0 0 0 0.125 0 0 0 1\nfps 25\nspan_ms 1\n'
    (tmp_path / 'ground.txt').write_text(ground)
    kw = dict(kw, save_txt=False, track=True, overlay=True, overlay_size=8, zones=str(tmp_path / 'zones.txt'), speed=str(tmp_path / 'ground.txt'))
    infer.run(save_dir=str(tmp_path / 'plain'), **kw)
    infer.run(save_dir=str(tmp_path / 's1'), overlay_scene=True, **kw)
    infer.run(save_dir=str(tmp_path / 's4'), overlay_scene=True, batch_size=4, **kw)
    lines, polys, line_names, zone_names = parse_zones(Z.ZONES_TXT, 1)
    zm = ZoneMapNp(1, lines, polys)
    trk = PlateTrackerNp(1, **tkw)
    trk.enable_zones(zm)
    trk.enable_speed(GroundPlaneNp(1, parse_ground(ground, 1)), 1, 2)
    atlas, font = build_scene_atlas(8), build_atlas([], [], [], 8, None)
    names = names_of((None, None, line_names, zone_names), atlas)
    style, styles = Inferer.make_scene_style(8, 2, (256, 160, 256)), Inferer.make_overlay_styles(8, 2, (256, 160, 256))
    files = sorted(os.listdir(tmp_path / 'imgs'))
    assert len(files) == len(untracked) == 8
    tagged = 0
    for name, d in zip(files, untracked):
        src = np.ascontiguousarray(np.asarray(Image.open(str(tmp_path / 'imgs' / name)))[:, :, ::-1])
        pad = np.zeros((1, 20, 28), np.float32)
        pad[0, :len(d)] = d
        r_out, r_tid = trk.update(pad, [len(d)], max_ended=2 * trk.max_tracks)[:2]
        zev, zcnt, zocc, ztot = trk.last_zone
        want, st = draw_scene_np([src], zm.packed, atlas, names, [0], ztot, zocc, zev, zcnt, trk.last_speed[0], r_out, [len(d)], r_tid, style)
        tagged += int(st.sum())
        (want,), _ = draw_plates_np(want, r_out, [len(d)], *font, tid=r_tid, styles=styles, palette=np.array(Inferer.OVERLAY_PALETTE, np.uint8))
        got = np.asarray(Image.open(str(tmp_path / 's1' / 'annotated' / name)))
        assert np.array_equal(got, want[:, :, ::-1]), name
        plain = np.asarray(Image.open(str(tmp_path / 'plain' / 'annotated' / name)))
        assert not np.array_equal(got, plain)
        assert not np.array_equal(np.asarray(Image.open(str(tmp_path / 's4' / 'annotated' / name))), plain)
    assert tagged > 0


def test_draw_plates_after_the_shared_include_refactor():
    """One case of tests/test_overlay_gpu.py's sweep as a pure call: lp_overlay_draw_batch draws the bytes of draw_plates_np."""
    from test_overlay_gpu import FONTS, MAX_DET, PALETTE, check_call, ids_for, overlay_rows, styles_for
    from yolov6.hip import runtime
    font = runtime.OverlayFont(*FONTS[1])
    tid, style = ids_for(5, MAX_DET, 55)
    shapes = [(33, 65), (64, 96), (1, 1), (5, 200), (37, 53)]
    buf, frames = bgr_buffer(shapes, 105)
    count = torch.tensor([5, 12, 15, -1, 12], dtype=torch.int32, device='cuda')
    assert check_call(buf, frames, overlay_rows(shapes, MAX_DET, 250), count, font, FONTS[1], styles=styles_for(2, 97), tid=tid, style=style,
                      palette=PALETTE) > 0
    nshapes = [(38, 54, 70, 60), (66, 130, 140, 134)]
    nbuf, nframes = nv12_buffer(nshapes, 305)
    assert check_call(nbuf, nframes, overlay_rows(nshapes, MAX_DET, 450), count[:2].contiguous(), font, FONTS[1], styles=styles_for(16, 200),
                      tid=tid[:2].contiguous(), palette=PALETTE) > 0


def test_argument_errors_leave_the_frames_alone(fonts):
    from yolov6.hip import abi, runtime
    from yolov6.utils.zones import ZoneMapNp
    lib = abi.load()
    buf, frames = bgr_buffer(BGR_SHAPES, 800)
    nbuf, nframes = nv12_buffer(NV12_SHAPES, 801)
    start, nstart = buf.clone(), nbuf.clone()
    geo = [geometry(s[0], s[1], 'straddle') for s in BGR_SHAPES]
    packed = cuda(ZoneMapNp(2, [g[0] for g in geo], [g[1] for g in geo]).packed)
    totals, occ, ev, cnt, speed_i = (cuda(a) for a in scene_inputs(2))
    det, count, tid = (cuda(a) for a in tag_rows(BGR_SHAPES, 6, 14))
    status = torch.full((2, 6), ST_POISON, dtype=torch.int32, device='cuda')
    ws = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device='cuda')
    assert ws.data_ptr() % 16 == 0
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    font = fonts[0]
    good = runtime._scene_style(font, style_for(), None)

    def descs(nv12):
        d = (abi.RedactDesc * 2)()
        for e, f in zip(d, nframes if nv12 else frames):
            if nv12:
                e.p0, e.p1, e.pitch0, e.pitch1, e.format = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, 1
            else:
                e.p0, e.p1, e.pitch0, e.format = f.data_ptr(), None, 3 * f.shape[1], 0
            e.h0, e.w0 = f.shape[0], f.shape[1]
        return d

    def call(nv12=False, mods=(), sty=(), **over):
        d = descs(nv12)
        for b, field, value in mods:
            setattr(d[b], field, value)
        p = abi.SceneStyle.from_buffer_copy(good)
        for field, value in sty:
            setattr(p, field, value)
        a = dict(desc=d, n=2, stream_of=None, S=2, packed=packed.data_ptr(), totals=totals.data_ptr(), occ=occ.data_ptr(), ev=ev.data_ptr(),
                 cnt=cnt.data_ptr(), max_events=ev.shape[1], speed_i=speed_i.data_ptr(), T=speed_i.shape[1], det=det.data_ptr(),
                 count=count.data_ptr(), tid=tid.data_ptr(), max_det=6, p=ctypes.byref(p), atlas=font.atlas.data_ptr(), names=None,
                 status=status.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel())
        a.update(over)
        return lib.lp_overlay_scene_batch(a['desc'], a['n'], a['stream_of'], a['S'], a['packed'], a['totals'], a['occ'], a['ev'], a['cnt'],
                                          a['max_events'], a['speed_i'], a['T'], a['det'], a['count'], a['tid'], a['max_det'], a['p'], a['atlas'],
                                          a['names'], a['status'], a['ws'], a['ws_bytes'], stream)

    need = lib.lp_overlay_scene_workspace_bytes(2, 6)
    assert need == 2 * 4640 + 2 * 6 * 48 and lib.lp_overlay_scene_workspace_bytes(0, 6) == 0 and lib.lp_overlay_scene_workspace_bytes(2, -1) == 0
    bad = [dict(desc=None), dict(p=None), dict(atlas=None), dict(packed=None), dict(n=-1), dict(S=0),
           dict(totals=None), dict(occ=None), dict(ev=None), dict(cnt=None), dict(max_events=0),
           dict(speed_i=None), dict(det=None), dict(count=None), dict(tid=None), dict(status=None), dict(T=0), dict(max_det=0),
           dict(mods=((1, 'format', 2),)), dict(mods=((1, 'p0', None),)), dict(mods=((1, 'pitch0', 3 * 96 - 1),)), dict(mods=((1, 'h0', 0),)),
           dict(mods=((0, 'w0', -5),)), dict(nv12=True, mods=((1, 'p1', None),)), dict(nv12=True, mods=((1, 'h0', 3),)),
           dict(nv12=True, mods=((0, 'pitch1', 61),)),
           dict(sty=(('t', -1),)), dict(sty=(('t', 17),)), dict(sty=(('marker', -1),)), dict(sty=(('marker', 65),)), dict(sty=(('pad', -1),)),
           dict(sty=(('pad', 17),)), dict(sty=(('a_fill', 257),)), dict(sty=(('a_fill_busy', -1),)), dict(sty=(('a_line', 300),)),
           dict(sty=(('a_plate', -1),)), dict(sty=(('a_text', 257),)),
           dict(sty=(('n_glyphs', 16),)), dict(sty=(('n_glyphs', 1025),)), dict(sty=(('gh', 0),)), dict(sty=(('gh', 65),)), dict(sty=(('gw', 0),)),
           dict(sty=(('gw', 65),)),
           dict(ws=None), dict(ws=ws.data_ptr() + 8), dict(ws_bytes=need - 1)]
    for kw in bad:
        rc = call(**kw)
        assert rc == -1, kw                                             # LP_ERR_ARG
        with pytest.raises(RuntimeError) as e:
            abi.check(rc, 'lp_overlay_scene_batch')
        if kw.get('mods'):
            assert 'frame %d' % kw['mods'][0][0] in str(e.value), (kw, str(e.value))
    torch.cuda.synchronize()
    assert torch.equal(buf, start) and torch.equal(nbuf, nstart) and bool((status == ST_POISON).all()) and bool((ws == 0x5A).all())
    # what is no error: no frames; whole groups absent; exactly the bytes asked for
    assert call(n=0) == 0
    assert call(totals=None, occ=None, ev=None, cnt=None, max_events=0, speed_i=None, det=None, count=None, tid=None, status=None, T=0, max_det=0,
                ws_bytes=lib.lp_overlay_scene_workspace_bytes(2, 0)) == 0
    assert call(ws_bytes=need) == 0
    torch.cuda.synchronize()
    assert not torch.equal(buf, start)
    # the runtime's own checks
    zm = runtime.ZoneMap(2, [g[0] for g in geo], [g[1] for g in geo])
    with pytest.raises(ValueError):
        runtime.draw_scene(frames, zm, font, det=det, count=count)              # half a group
    with pytest.raises(ValueError):
        runtime.draw_scene(frames, zm, font, stream_of=[0])
    with pytest.raises(ValueError):
        runtime.draw_scene(frames, zm, font, style=style_for(17))
    with pytest.raises(ValueError):
        runtime.draw_scene(frames, zm, ATLASES[0])
    with pytest.raises(ValueError):
        runtime.draw_scene([], zm, font)
