"""lp_nms and lp_nms_candidates on the scenes at the edges of greedy_kernel's schedule, bit for bit against the C oracle.

The scenes and what each of them pins are lp_testing's (section "scenes at the edges of the greedy NMS schedule");
tests/test_nms_schedule_cpu.py shows from float64 geometry that every decision in them has a margin of more than 0.07 in IoU, that
the oracle keeps the closed-form expectation, and that a model of the kernel's schedule with any one of eleven defects gets at least
one of them wrong.  Here every scene is scattered over the anchors of a prediction tensor (the sort is part of every case), several
scenes go into one launch (the images of a launch differ in their number of candidates), and count, kept anchors and rows must equal
the oracle's on the same tensor; the rows behind the count are zero, keep is -1 there, and the caller's tensor is unchanged.  The
kept anchors are also compared with the closed-form expectation, so a failure names the ranks it got wrong."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lp_testing as X

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(names, N, max_det, seed):
    """One batch of scenes, built once: (pred [B,N,290] read-only, perms, scenes, the oracle's rows and kept anchors)."""
    from oracle import lp_post
    scenes = []
    for name in names:
        if name.startswith('sort_'):
            scenes.append(X.scene_sort(int(name[5:])))
        elif name.startswith('thr_'):
            scenes.append(X.scene_threshold(name == 'thr_below'))
        else:
            scenes.append(dict(X.nms_schedule_scenes()[name]))
    perms = [X.scene_perm(sc, N, seed + 7 * i) for i, sc in enumerate(scenes)]
    pred = np.concatenate([X.to_pred(sc, N, p) for sc, p in zip(scenes, perms)])
    iou = scenes[0]['iou']
    assert all(sc['iou'] == iou and sc['conf'] == scenes[0]['conf'] for sc in scenes)
    rows, keep, after = lp_post.nms_c(pred, scenes[0]['conf'], iou, max_det)
    assert np.array_equal(after, pred)
    pred.setflags(write=False)
    return pred, perms, scenes, rows, keep


def _check(out, case, max_det, what):
    pred, perms, scenes, rows_o, keep_o = case
    det, count, keep = (t.cpu().numpy() for t in out)
    for i, (sc, perm) in enumerate(zip(scenes, perms)):
        tag = '%s, image %d (%s)' % (what, i, sc['name'])
        n = int(count[i])
        want = perm[sc['expect'][:max_det]]
        got = keep[i, :max(n, 0)]
        rank_of = np.full(pred.shape[1], -1, np.int64)
        rank_of[perm] = np.arange(sc['n'])
        got_r, want_r = set(rank_of[np.clip(got, 0, pred.shape[1] - 1)].tolist()), set(sc['expect'][:max_det].tolist())
        assert np.array_equal(keep_o[i], want), tag + ': the oracle and the closed form differ'
        assert n == len(want) and np.array_equal(got, want), \
            '%s: %d kept, expected %d; ranks kept wrongly %s, ranks missing %s, first difference at position %s' % (
                tag, n, len(want), sorted(got_r - want_r)[:16], sorted(want_r - got_r)[:16],
                next((k for k in range(min(n, len(want))) if got[k] != want[k]), None))
        assert np.array_equal(det[i, :n].view(np.int32), rows_o[i].view(np.int32)), tag + ': rows'
        assert not det[i, n:].view(np.int32).any() and (keep[i, n:] == -1).all(), tag + ': behind the count'


def _run(names, N, max_det, seed, candidates=False, reverse=False):
    from yolov6.hip import abi, runtime
    case = _case(tuple(names), N, max_det, seed)
    if reverse:
        case = tuple(v[::-1] for v in case)
    pred_np, scenes = np.array(case[0]), case[2]                              # (a writable copy: the shared case stays as it is)
    conf, iou, B = scenes[0]['conf'], scenes[0]['iou'], len(scenes)
    what = '%s N=%d max_det=%d%s' % ('+'.join(names), N, max_det, ' reversed' if reverse else '')
    pred = torch.from_numpy(pred_np).cuda()
    _check(runtime.nms_padded(pred, conf, iou, max_det, want_keep=True), case, max_det, 'lp_nms ' + what)
    assert np.array_equal(pred.cpu().numpy().view(np.int32), pred_np.view(np.int32)), what + ': the prediction tensor changed'
    if candidates:
        # lp_nms on a workspace of our own, then lp_nms_candidates on the candidate lists it left there
        lib = abi.load()
        need = lib.lp_nms_workspace_bytes(B, N)
        ws = torch.empty(need + 256, dtype=torch.uint8, device=pred.device)
        base = (ws.data_ptr() + 255) // 256 * 256
        det = torch.empty(B, max_det, 28, dtype=torch.float32, device=pred.device)
        count = torch.empty(B, dtype=torch.int32, device=pred.device)
        keep = torch.empty(B, max_det, dtype=torch.int32, device=pred.device)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        abi.check(lib.lp_nms(ptr(pred), B, N, conf, iou, max_det, ptr(det), ptr(count), ptr(keep), ctypes.c_void_p(base), need, st), 'lp_nms')
        _check((det, count, keep), case, max_det, 'lp_nms (own workspace) ' + what)
        _check(runtime.nms_candidates((ws, B, N), iou, max_det, want_keep=True), case, max_det, 'lp_nms_candidates ' + what)
        assert np.array_equal(pred.cpu().numpy().view(np.int32), pred_np.view(np.int32)), what + ': the prediction tensor changed'
    return case


BATCH = ('chunk_edges', 'ring', 'batch_edges', 'share_119', 'share_241')


@pytest.mark.parametrize('reverse', [False, True], ids=['in-order', 'reversed'])
def test_chunk_ring_batch_and_share_scenes_in_one_launch(reverse):
    """448, 960, 2176, 366 and 610 candidates in one launch of five blocks (N = 2200: the score kernel's runs of 16 rows straddle images),
    through lp_nms and through lp_nms_candidates."""
    case = _run(BATCH, 2200, 2200, 11, candidates=True, reverse=reverse)
    assert sorted(len(k) for k in case[4]) == sorted([424, 640, 2132, 119, 241])


def test_every_share_of_the_kept_list():
    """Kept lists of 1 .. 241 entries: below one share each, the last share, one short of / exactly / one past a trip of 120, a trip
    and a full remainder, two trips and one past them.  A skipped list position leaves its one copy alive."""
    case = _run(['share_%d' % K for K in X.SHARE_KS], 620, 300, 21)
    assert [len(k) for k in case[4]] == list(X.SHARE_KS)


@pytest.mark.parametrize('M', X.CUT_MS)
def test_cut_at_max_det(M):
    """The loop leaves after the chunk in which the kept list reaches max_det, and the list is cut: inside chunk 0 (1, 63), at its
    end (64), in chunk 1 (65) and behind the chains of the first boundary (190, 200)."""
    case = _run(['cut_%d' % M], 400, M, 31, candidates=(M == 190))
    uncut = X.scene_chunk_edges((192, 256))
    assert len(case[4][0]) == M and np.array_equal(case[4][0], case[1][0][uncut['expect'][:M]])    # the first M of the uncut greedy


def test_candidate_counts_around_chunk_and_batch_sizes():
    """Eleven images with 1 .. 1025 candidates in one launch, N = 1100 (no multiple of 16), every third candidate a copy of the one
    before it."""
    case = _run(['nc_%d' % n for n in X.NC_EDGES], 1100, 1100, 41)
    assert [len(k) for k in case[4]] == [n - n // 3 for n in X.NC_EDGES]


@pytest.mark.parametrize('n', X.SORT_EDGES)
def test_sort_at_the_lds_block_edge(n):
    """16383, 16384 and 16385 candidates at seeded anchors of 16400: one LDS block of the sort, exactly one, and the first list with a
    compare-exchange step in global memory.  All singles and max_det = 31000: keep is the whole sorted order."""
    case = _run(['sort_%d' % n], 16400, 31000, 51)
    assert len(case[4][0]) == n


def test_ties_and_the_pair_at_the_threshold():
    """Equal scores: the order is the anchor order, and of two overlapping boxes the lower anchor wins, across both chunk edges.  A
    pair at IoU = 0.5 exactly is kept at iou_thres 0.5 (strict >) and suppressed at the next double below 0.5."""
    case = _run(['ties'], 200, 130, 61)
    assert len(case[4][0]) == 66
    assert len(_run(['thr_at'], 16, 2, 62)[4][0]) == 2
    assert len(_run(['thr_below'], 16, 2, 62)[4][0]) == 1
