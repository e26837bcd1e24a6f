"""CPU tests of the containment checker of lp_testing (ByteWatch, merge_intervals, layout_regions) that tests/test_containment_gpu.py
relies on, and of the inputs of its spilled-kept-list case: the checker must report a single changed byte with its offset and the
name of the region it lies in, wherever it lies, and must stay silent about writes inside the allowed intervals."""
import numpy as np
import pytest
import torch

import lp_testing as X

# a buffer laid out like an engine's arena: 37 unaligned bytes, then tensors of 1000, 256 and 300 bytes, each rounded up to 256
BASE, TOTAL = 37, 37 + 2304 + 219
TENSORS = [('guard before dst0', 0, 1000), ('dst0', 1024, 256), ('src1', 1280, 300)]
NEED = 1792 + 256 + 256                                  # tensors, 256 bytes behind them (a scratch), the arena's +256 tail


def _watch():
    buf = torch.full((TOTAL,), 0xA5, dtype=torch.uint8)
    regions = X.layout_regions(BASE, NEED, TOTAL, TENSORS)
    return buf, X.ByteWatch(buf, regions), regions


def test_layout_regions_tile_the_buffer():
    regions = X.layout_regions(BASE, NEED, TOTAL, TENSORS)
    assert [r[0] for r in regions] == ['unaligned head', 'guard before dst0', 'slack after guard before dst0', 'dst0', 'src1',
                                       'slack after src1', 'behind the tensors', 'arena tail', 'allocation slack']
    assert regions[0][1] == 0 and regions[-1][2] == TOTAL
    assert all(a[2] == b[1] for a, b in zip(regions, regions[1:]))         # no gap, no overlap
    named = dict((r[0], r[1:]) for r in regions)
    assert named['dst0'] == (BASE + 1024, BASE + 1280) and named['slack after src1'] == (BASE + 1580, BASE + 1792)
    assert named['arena tail'] == (BASE + NEED - 256, BASE + NEED)


@pytest.mark.parametrize('intervals,want', [
    ([(10, 20), (30, 40)], [(10, 20), (30, 40)]),
    ([(30, 40), (10, 20)], [(10, 20), (30, 40)]),                          # unsorted
    ([(10, 20), (20, 30)], [(10, 30)]),                                    # adjacent
    ([(10, 25), (20, 30), (29, 31)], [(10, 31)]),                          # overlapping chain
    ([(10, 40), (15, 20)], [(10, 40)]),                                    # contained
    ([(10, 10), (7, 5), (3, 4)], [(3, 4)]),                                # empty ones dropped
    ([], []),
])
def test_merge_intervals(intervals, want):
    assert X.merge_intervals(intervals) == want


def test_writes_inside_the_allowed_intervals_pass():
    buf, watch, regions = _watch()
    d0 = (BASE + 1024, BASE + 1280)
    s1 = (BASE + 1280, BASE + 1580)
    buf[d0[0]:d0[1]] = 7
    buf[s1[0]:s1[1]] = 9
    for allowed in ([d0, s1], [s1, d0], [(d0[0], s1[1])], [(d0[0], d0[0] + 200), (d0[0] + 100, s1[1])]):   # adjacent, one, overlapping
        r = watch.report(allowed)
        assert r['count'] == 0 and r['first'] is None and r['last'] is None and r['regions'] == []
        assert int(watch.count(allowed)) == 0
        watch.assert_contained(allowed)
    # rewriting a byte with the value it had is no change
    buf[5] = 0xA5
    assert watch.report([d0, s1])['count'] == 0


@pytest.mark.parametrize('where,offset,region', [
    ('directly before an interval', BASE + 1024 - 1, 'slack after guard before dst0'),
    ('directly after an interval', BASE + 1280, 'src1'),
    ('in a 256-byte slack', BASE + 1580 + 100, 'slack after src1'),
    ('last byte of the slack', BASE + 1791, 'slack after src1'),
    ('in the unaligned head', 3, 'unaligned head'),
    ('first byte of the buffer', 0, 'unaligned head'),
    ('in the guard', BASE + 999, 'guard before dst0'),
    ('behind the tensors', BASE + 1792, 'behind the tensors'),
    ('in the arena tail', BASE + NEED - 1, 'arena tail'),
    ('in the tail of the allocation', TOTAL - 1, 'allocation slack'),
])
def test_a_single_changed_byte_is_reported_with_offset_and_region(where, offset, region):
    buf, watch, regions = _watch()
    allowed = [(BASE + 1024, BASE + 1280)]                                 # dst0
    buf[allowed[0][0]:allowed[0][1]] = 1                                   # the legitimate write
    buf[offset] = 0x5A
    r = watch.report(allowed)
    assert r['count'] == 1 and r['first'] == r['last'] == offset, (where, r)
    assert r['offsets'].tolist() == [offset] and r['regions'] == [(region, 1, offset, offset)], (where, r)
    assert int(watch.count(allowed)) == 1
    with pytest.raises(AssertionError, match='%s: 1 byte' % region):
        watch.assert_contained(allowed, where)


def test_changes_in_several_regions_are_counted_per_region():
    buf, watch, regions = _watch()
    allowed = [(BASE + 1024, BASE + 1280)]
    buf[BASE + 1020:BASE + 1030] = 1                                       # four bytes of slack in front, six allowed
    buf[BASE + 1278:BASE + 1284] = 2                                       # two allowed, four of src1
    buf[TOTAL - 2:] = 3
    r = watch.report(allowed)
    assert r['count'] == 10 and r['first'] == BASE + 1020 and r['last'] == TOTAL - 1
    assert r['regions'] == [('slack after guard before dst0', 4, BASE + 1020, BASE + 1023), ('src1', 4, BASE + 1280, BASE + 1283),
                            ('allocation slack', 2, TOTAL - 2, TOTAL - 1)]


def test_shrinking_the_allowed_set_flags_exactly_the_removed_bytes():
    """How the GPU tests show that the checker is sensitive without running a wrong kernel."""
    buf, watch, regions = _watch()
    d0, s1 = (BASE + 1024, BASE + 1280), (BASE + 1280, BASE + 1580)
    buf[d0[0]:d0[1]] = 1
    buf[s1[0]:s1[1]] = 2
    r = watch.report([(d0[0] + 16, d0[1]), (s1[0], s1[1] - 16)])
    assert r['offsets'].tolist() == list(range(d0[0], d0[0] + 16)) + list(range(s1[1] - 16, s1[1]))
    assert r['regions'] == [('dst0', 16, d0[0], d0[0] + 15), ('src1', 16, s1[1] - 16, s1[1] - 1)]


def test_a_new_snapshot_forgets_earlier_changes():
    buf, watch, regions = _watch()
    buf[100] = 1
    assert watch.report([])['count'] == 1
    watch.snapshot()
    assert watch.report([])['count'] == 0
    buf[100] = 2
    assert watch.report([])['offsets'].tolist() == [100]


@pytest.mark.parametrize('first_rank,n_copy', [(4100, 1900), (4000, 2000)], ids=['beyond-the-cache', 'straddling-the-cache'])
def test_spill_case_preconditions(first_rank, n_copy):
    """The crafted image of the spilled-kept-list test (lp_testing.spill_case) from the C oracle and float64 geometry alone: the
    oracle keeps exactly the 6000 originals in rank order; every copy is over the IoU threshold with its original and with nothing
    else; those originals have kept ranks beyond the 4096 entries the greedy kernel caches in LDS (first case), or on both sides of
    that boundary (second case)."""
    p, box, score = X.spill_case(first_rank, 6000, n_copy)
    assert p.shape == (1, 6000 + n_copy, 290) and len(np.unique(score)) == len(score)
    s32 = score.astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), score)                   # the scores are fp32 values
    eight = s32.copy()
    for _ in range(7):
        eight = eight + s32                                                # the left-to-right fp32 sum of the eight maxima
    assert np.array_equal(eight / np.float32(8.0), s32)                    # mask value = score = the probability, exactly
    rows, keep, orig = X.assert_spill_preconditions(p, box, score, first_rank, 6000, n_copy, 0.25, 0.5, 8000)
    assert len(rows[0]) == 6000
    if first_rank >= 4096:
        assert orig.min() >= 4096
    else:
        assert orig.min() < 4096 - 64 and orig.max() >= 4096 + 64
