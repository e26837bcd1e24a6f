"""The tracker's add-ons together, on the CPU: the scene of the all-on tests reaches every edge it is there for, the numpy chain
with everything enabled (``lp_testing.AllOnNp``: PlateTrackerNp with every ``enable_*``, BestShotNp, LookbackNp) equals every feature
enabled alone, a handful of deliberate mis-compositions of that chain each change an output on this scene, ``reset(streams)`` leaves
the other streams alone, and ``tools/infer.py`` with every flag writes, on the CPU path, the files of every flag alone.

No kernel runs here: this is the reference of tests/test_all_on_gpu.py and the proof that it discriminates."""
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import REPO
import lp_testing as L

P = L.ALL_ON


def test_the_scene_reaches_every_condition():
    """Asserted from the all-on numpy chain alone, before anything else uses the scene."""
    calls = L.all_on_case()[0]
    assert tuple(len(c[0]) for c in calls) == P['Bs'] == (1, 3, 70, 2, 0) and calls[-1][3] == [1, 1, 1]
    assert all(f.shape == P['frame_hw'] + (3,) for c in calls for f in c[4]) and all(len(c[4]) == len(c[0]) for c in calls)
    n = L.all_on_conditions()
    print('all-on scene:', n)
    for name in ('by_age', 'by_flush', 'overflow', 'held', 'back_before_first', 'shot_replaced', 'stack_n2', 'watch_hit', 'alert', 'resighting',
                 'slot_64', 'split', 'untracked', 'idle_flush', 'dropped', 'shot_valid'):
        assert n[name] > 0, (name, n)
    # the reset of stream 1 falls between frames of that stream
    before = [s for c in calls[:P['reset_before']] for s in c[2]]
    after = [s for c in calls[P['reset_before']:] for s in c[2]]
    assert all(s in before and s in after for s in P['reset_streams'])


@pytest.mark.parametrize('feature', L.ALL_ON_FEATURES)
def test_all_on_equals_the_feature_alone(feature):
    """Call by call, bit for bit: the tracker's own outputs, the feature's and those of what it needs."""
    _, want = L.all_on_reference()
    on = L.all_on_features((feature,))
    chain, got = L.all_on_run((feature,))
    assert chain.on == on
    names = [n for f in ('track',) + on for n in L.ALL_ON_OUTPUTS[f]]
    assert set(got[0]) == set(names) and len(got) == len(want) == len(P['Bs'])
    assert L.all_on_differences(want, got, names) == []


def test_the_tracker_alone_equals_all_on():
    _, want = L.all_on_reference()
    _, got = L.all_on_run(())
    assert set(got[0]) == set(L.ALL_ON_OUTPUTS['track']) and L.all_on_differences(want, got, L.ALL_ON_OUTPUTS['track']) == []


def test_every_mis_composition_changes_an_all_on_output():
    """Each mutant of the chain is caught by at least one output on this scene; which one goes to the log."""
    _, want = L.all_on_reference()
    table = {}
    for m in L.ALL_ON_MUTANTS:
        _, got = L.all_on_run(mutant=m)
        table[m] = L.all_on_differences(want, got)
    with open(os.path.join(L.log_dir(), 'all_on_mutants.log'), 'a') as f:
        for m, diff in table.items():
            f.write('%-22s %s\n' % (m, ' '.join(diff) or '-'))
    print(table)
    assert all(table.values()), table
    # the mutants are what their names say: each one leaves the outputs in front of its defect alone
    assert not set(table['redact_first']) & set(L.ALL_ON_OUTPUTS['track'] + L.ALL_ON_OUTPUTS['hold']) and 'shot_crops' in table['redact_first']
    assert set(table['stale_ended']) | set(table['stale_slot']) <= set(L.ALL_ON_OUTPUTS['shot'] + L.ALL_ON_OUTPUTS['stack'])
    assert table['lookback_no_copy'] == ['released']
    assert set(table['reset_skips_gallery']) <= set(L.ALL_ON_OUTPUTS['shot']) and set(table['reset_skips_stack']) <= set(L.ALL_ON_OUTPUTS['stack'])
    assert set(table['reset_skips_memo']) <= set(L.ALL_ON_OUTPUTS['live']) and table['reset_skips_lookback'] == ['released']


def test_reset_of_one_stream_leaves_the_others_alone_and_starts_that_one_afresh():
    """From the reset on: streams 0 and 2 give what they give in a run without the reset, stream 1 what a fresh chain gives that
    starts at that call.  The sightings are left out: the log is shared by all streams and survives a reset by design."""
    calls = L.all_on_case()[0]
    first = P['reset_before']
    _, with_reset = L.all_on_reference()
    _, without = L.all_on_run(reset=False)
    _, fresh = L.all_on_run(reset=False, first=first)
    differs = 0
    for c in range(first, len(calls)):
        so = calls[c][2]
        for s in range(P['n_streams']):
            a = L.all_on_stream_part(with_reset[c], so, s)
            b = L.all_on_stream_part(fresh[c - first] if s in P['reset_streams'] else without[c], so, s)
            assert L.all_on_differences([a], [b]) == [], (c, s)
            if s in P['reset_streams']:
                differs += len(L.all_on_differences([a], [L.all_on_stream_part(without[c], so, s)]))
    assert differs > 0                                                          # ... and the reset did change that stream


def test_what_is_left_after_the_final_flush_is_the_occupants_of_cut_off_records():
    """After the last call no track is live and the live memo is empty.  The gallery and the stack keep an occupant only where its
    record was cut off by ``max_ended`` (their rule: such an occupant goes when its slot is reused); a stream whose records all fit
    is all zero."""
    chain, outs = L.all_on_reference()
    trk, gal, stk = chain.trk, chain.gal, chain.trk._stack['np']
    assert not trk.hits.any() and not trk.votes.any() and not trk._live.memo.any()
    assert np.array_equal(gal.idp1 != 0, stk.idp1 != 0)
    cut = [any(int(o['ended_count'][s]) > P['max_ended'] for o in outs) for s in range(P['n_streams'])]
    recorded = [{int(o['ended_i'][s, j, 0]) for o in outs for j in range(min(int(o['ended_count'][s]), P['max_ended']))} for s in range(P['n_streams'])]
    assert any(cut) and not all(cut)
    for s in range(P['n_streams']):
        left = gal.idp1[s][gal.idp1[s] != 0] - 1
        assert cut[s] or not len(left), s
        if s not in P['reset_streams']:                                         # (ids restart with a reset: the names are unique without one)
            assert not set(left.tolist()) & recorded[s], s


def test_infer_with_every_flag_writes_the_files_of_every_flag_alone_cpu(tmp_path, monkeypatch):
    monkeypatch.chdir(REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    infer = importlib.import_module('infer')
    ckpt, src = L.all_on_infer_source(tmp_path)
    files = L.all_on_infer(infer, tmp_path, ckpt, src, 'cpu', device='cpu')
    n = L.assert_all_on_files(files, 'cpu')
    print('files compared:', n, 'of', len(files['all']))
    assert n['lookback'] > n['hold'] == n['track'] and n['stacks'] > n['shots'] > n['track'] and n['crops'] > n['track']
