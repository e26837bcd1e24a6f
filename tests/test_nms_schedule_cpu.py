"""CPU side of the greedy-NMS schedule tests: the scenes of lp_testing are what their construction says, and they
discriminate.

Per scene, from float64 geometry and the C oracle alone: the scores and boxes are exact fp32 values, every IoU is the one its
construction names and none is within 0.07 of the threshold; the oracle, the textbook greedy loop over the overlap matrix and the
closed-form expectation (cells are independent; in a cell a member lives unless a kept member is at most one shift away) keep the
same ranks.  Then a numpy model of greedy_kernel's decomposition (lp_testing.greedy_schedule_np: kept-list strikes in fifteen
shares and trips of 120, xt against the survivors of the chunk before, mt in candidate order, the cut) equals the textbook loop on
every scene, and each of its eleven one-line mutants differs from it on at least one scene; which scene catches which mutant is
appended to nms_schedule.log in the folder of the test logs.  No kernel runs here: tests/test_nms_schedule_gpu.py holds lp_nms
and lp_nms_candidates to the oracle on the same scenes."""
import functools
import os

import numpy as np
import pytest

import lp_testing as X

LOG_NAME = 'nms_schedule.log'
SCENES = list(X.nms_schedule_scenes())
KEPT = dict([('chunk_edges', 424), ('ring', 640), ('batch_edges', 2132), ('ties', 66)] + [('share_%d' % K, K) for K in X.SHARE_KS]
            + [('cut_%d' % M, M) for M in X.CUT_MS] + [('nc_%d' % n, n - n // 3) for n in X.NC_EDGES])


@functools.lru_cache(maxsize=None)
def _over(name):
    over = X.assert_scene_geometry(X.nms_schedule_scenes()[name])
    over.setflags(write=False)
    return over


def _oracle_ranks(sc, N, seed):
    """The ranks the C oracle keeps for the scene scattered over N anchors (and the check that it returned the scene's rows)."""
    from oracle import lp_post
    perm = X.scene_perm(sc, N, seed)
    pred = X.to_pred(sc, N, perm)
    rows, keep, after = lp_post.nms_c(pred, sc['conf'], sc['iou'], sc['max_det'])
    assert np.array_equal(after, pred)                                       # obj = 1: the oracle's copy is unchanged
    rank_of = np.full(N, -1, np.int64)
    rank_of[perm] = np.arange(sc['n'])
    ranks = rank_of[keep[0]]
    assert np.array_equal(rows[0][:, :4].astype(np.float64), sc['box'][ranks])
    assert np.array_equal(rows[0][:, 12].astype(np.float64), sc['score'][ranks])
    return ranks


def test_the_scene_list_is_the_one_the_tests_name():
    assert sorted(SCENES) == sorted(KEPT) and len(SCENES) == 4 + len(X.SHARE_KS) + len(X.CUT_MS) + len(X.NC_EDGES)
    sc = X.nms_schedule_scenes()
    assert (sc['chunk_edges']['n'], sc['ring']['n'], sc['batch_edges']['n'], sc['cut_190']['n']) == (448, 960, 2176, 384)
    offs = [-1, 0, 1, -4, -3, 2, -6, 6, -130, -8, 8, -71, -10, 10, -133, 12, 20, 21, 22, 23]
    assert len({o % 64 for o in offs}) == len(offs)                          # boundaries 64 apart do not collide
    assert sorted(r - 192 for r in X._edge_chains(192)) == sorted(offs)


@pytest.mark.parametrize('name', SCENES)
def test_scene_oracle_plain_loop_closed_form_and_model_agree(name):
    sc = X.nms_schedule_scenes()[name]
    over = _over(name)
    plain = X.greedy_plain_np(over, sc['max_det'])
    assert np.array_equal(plain, sc['expect']) and len(plain) == KEPT[name], (name, len(plain))
    assert np.array_equal(_oracle_ranks(sc, sc['n'] + 37, 5), plain), name
    assert np.array_equal(X.greedy_schedule_np(over, sc['max_det']), plain), name
    if name.startswith('cut_'):                                              # the first M of the uncut greedy, in order
        assert np.array_equal(plain, X.greedy_plain_np(over, sc['n'])[:sc['max_det']])
    if name.startswith('share_'):                                            # every copy has one killer, at kept position = its rank
        K = KEPT[name]
        assert np.array_equal(plain, np.arange(K)) and np.array_equal(over[:K, K:].sum(0), np.ones(K + 128, np.int64))
        assert sorted(over[:K, K + 128:].argmax(0).tolist()) == list(range(K))


def test_ring_has_every_combination_three_chunks_apart():
    pattern = 'SSCSSSCCSCSSCSS'
    assert {pattern[c - 3] + pattern[c] for c in range(3, len(pattern))} == {'SS', 'SC', 'CS', 'CC'}
    sc = X.nms_schedule_scenes()['ring']
    dead = ~np.isin(np.arange(sc['n']), sc['expect']).reshape(-1, 64)
    assert [('C' if d.all() else 'S' if not d.any() else '?') for d in dead] == list(pattern)


@pytest.mark.parametrize('n', X.SORT_EDGES)
def test_sort_scenes(n):
    sc = X.scene_sort(n)
    assert X.assert_scene_geometry(sc) is None and np.array_equal(sc['expect'], np.arange(n))
    assert np.array_equal(_oracle_ranks(sc, 16400, n), np.arange(n))


@pytest.mark.parametrize('below', [False, True], ids=['at-the-threshold', 'next-double-below'])
def test_threshold_pair(below):
    sc = X.scene_threshold(below)
    over = X.assert_scene_geometry(sc)
    assert bool(over[0, 1]) == below and (sc['iou'] == 0.5) != below and sc['iou'] > 0.5 - 1e-15
    assert np.array_equal(X.greedy_plain_np(over, 2), sc['expect'])
    assert np.array_equal(_oracle_ranks(sc, 16, 1), sc['expect'])
    assert np.array_equal(X.greedy_schedule_np(over, 2), sc['expect'])


def test_ties_go_to_the_lower_anchor():
    sc = X.nms_schedule_scenes()['ties']
    perm = X.scene_perm(sc, 200, 3)
    assert np.all(np.diff(perm) > 0)
    assert sc['expect'].tolist() == [0] + list(range(1, 129, 2)) + [129]
    assert {63, 127} <= set(sc['expect'].tolist()) and sc['cell'][64] == 63 and sc['cell'][128] == 127     # pairs across both chunk edges


def test_every_mutant_of_the_schedule_model_is_caught():
    """Each of the eleven defects changes the kept list of at least one scene; the two that noise misses are caught by
    the constructed chunk-edge scene."""
    caught = {}
    for m in X.NMS_MUTANTS:
        caught[m] = []
        for name in SCENES:
            sc = X.nms_schedule_scenes()[name]
            over = _over(name)
            if not np.array_equal(X.greedy_schedule_np(over, sc['max_det'], m), X.greedy_plain_np(over, sc['max_det'])):
                caught[m].append(name)
    with open(os.path.join(X.log_dir(), LOG_NAME), 'a') as f:
        for m in X.NMS_MUTANTS:
            f.write('mutant %-14s caught by %2d scenes: %s\n' % (m, len(caught[m]), ' '.join(caught[m]) or '-'))
    assert all(caught[m] for m in X.NMS_MUTANTS), {m: v for m, v in caught.items() if not v}
    assert 'chunk_edges' in caught['xt_alive'] and 'chunk_edges' in caught['xt_any'] and caught['mt_dead_kills'] == ['chunk_edges']
    assert caught['late_batch'] == ['batch_edges']
    assert {'batch_edges', 'cut_200'} <= set(caught['xt_alive']) and {'batch_edges', 'cut_200'} <= set(caught['xt_any'])
    assert {'cut_1', 'cut_63', 'cut_65', 'cut_190', 'cut_200'} <= set(caught['no_cut'])
    assert 'ring' in caught['ring2'] and any(s.startswith('share_') for s in caught['no_remainder'])
    assert any(s.startswith('share_') for s in caught['last_share']) and any(s.startswith('share_') for s in caught['stale_T'])
