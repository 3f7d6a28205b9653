"""Host logic of the deferred partial sums (`param_grads.DeferredPartialSums`): `flush()` hands the queued reductions to
`native.sum_partials_multi` sixteen at a time, and the jobs of one launch run side by side in no order — so two jobs whose
output floats overlap (a fused module reached twice in a direct-mode backward: both ADD into its span of the flat gradient
buffer) must never share a launch, and must keep the order they were queued in.  CPU: the launch is replaced by a recorder;
what is checked is which jobs leave together and in which order."""
import pytest
import torch


@pytest.fixture
def recorder(monkeypatch):
    import asac_amd  # noqa: F401
    from asac_amd import native
    from algorithm.param_grads import DeferredPartialSums
    launches = []
    monkeypatch.setattr(native, 'sum_partials_multi', lambda jobs: launches.append(list(jobs)))
    return DeferredPartialSums(), launches


def _add(later, out, n, tag, accumulate=True):
    """queue a job of `n` floats into `out`; `tag` (its slab count) identifies it in what the recorder saw"""
    later.add(torch.zeros(tag * n), tag, 1, n, n, out, accumulate=accumulate)


def _tags(launches):
    return [[job[1] for job in launch] for launch in launches]


def _span(job):
    return job[5].data_ptr(), job[5].data_ptr() + 4 * job[4]


def _assert_no_launch_holds_overlapping_outputs(launches):
    for launch in launches:
        assert 1 <= len(launch) <= 16
        for i, a in enumerate(launch):
            for b in launch[:i]:
                (a0, a1), (b0, b1) = _span(a), _span(b)
                assert a1 <= b0 or b1 <= a0, 'two jobs of one launch write the same floats'


def test_seventeen_disjoint_jobs_leave_sixteen_and_one(recorder):
    later, launches = recorder
    buf = torch.zeros(17 * 10)
    for k in range(17):
        _add(later, buf[10 * k:10 * k + 10], 10, k + 1, accumulate=k % 2 == 0)
    assert not launches          # (nothing before the flush)
    later.flush()
    assert _tags(launches) == [list(range(1, 17)), [17]]
    assert not later.jobs
    _assert_no_launch_holds_overlapping_outputs(launches)


def test_a_module_reached_twice_waits_for_the_launch_that_holds_its_first_sum(recorder):
    later, launches = recorder
    a, b = torch.zeros(40), torch.zeros(40)
    _add(later, a, 40, 1)
    _add(later, b, 40, 2)
    _add(later, a, 40, 3)
    later.flush()
    assert _tags(launches) == [[1, 2], [3]]
    _assert_no_launch_holds_overlapping_outputs(launches)


def test_a_module_reached_three_times_is_three_launches_in_the_order_queued(recorder):
    later, launches = recorder
    a = torch.zeros(40)
    for tag in (1, 2, 3):
        _add(later, a, 40, tag)
    later.flush()
    assert _tags(launches) == [[1], [2], [3]]


def test_once_used_modules_ride_in_the_first_launch(recorder):
    later, launches = recorder
    a, b, c = torch.zeros(40), torch.zeros(24), torch.zeros(8)
    _add(later, a, 40, 1)
    _add(later, b, 24, 2)
    _add(later, a, 40, 3)
    _add(later, c, 8, 4)
    later.flush()
    # (greedy and in order: a job never overtakes one queued before it, so the last rides with the second use)
    assert _tags(launches) == [[1, 2], [3, 4]]
    _assert_no_launch_holds_overlapping_outputs(launches)


@pytest.mark.parametrize('first, second', [((0, 40), (39, 10)),       # the last float of the first is the second's first
                                           ((10, 30), (0, 11)),       # ... and the other way round
                                           ((0, 40), (8, 4)),         # a view at an offset, inside
                                           ((8, 4), (0, 40))])        # ... and around
def test_partly_overlapping_outputs_are_separated(recorder, first, second):
    later, launches = recorder
    buf = torch.zeros(64)
    _add(later, buf[first[0]:], first[1], 1)
    _add(later, buf[second[0]:], second[1], 2)
    later.flush()
    assert _tags(launches) == [[1], [2]]


def test_outputs_that_only_touch_share_a_launch(recorder):
    later, launches = recorder
    buf = torch.zeros(64)
    _add(later, buf[0:], 40, 1)           # floats [0, 40)
    _add(later, buf[40:], 24, 2)          # floats [40, 64)
    later.flush()
    assert _tags(launches) == [[1, 2]]


def test_ensemble_members_are_disjoint_although_their_views_run_on(recorder):
    """`StockMLP._launch_backward` queues one job per member with out = gp[e * member_stride:] and n = the member's used
    floats <= member_stride: the VIEWS extend over every later member's memory, the floats written do not"""
    later, launches = recorder
    E, member_stride, used = 4, 100, 97
    gp = torch.zeros(E * member_stride)
    for e in range(E):
        out = gp[e * member_stride:]
        assert out.numel() > used or e == E - 1
        _add(later, out, used, e + 1)
    later.flush()
    assert _tags(launches) == [[1, 2, 3, 4]]
    _assert_no_launch_holds_overlapping_outputs(launches)
    # the same network once more (its second use in the backward): every member waits for its first sum
    for e in range(E):
        _add(later, gp[e * member_stride:], used, e + 1)
    for e in range(E):
        _add(later, gp[e * member_stride:], used, e + 11)
    launches.clear()
    later.flush()
    assert _tags(launches) == [[1, 2, 3, 4], [11, 12, 13, 14]]


@pytest.mark.parametrize('overwrites', [(False, True), (True, False), (False, False)])
def test_an_overwriting_job_is_separated_like_an_adding_one(recorder, overwrites):
    later, launches = recorder
    buf = torch.zeros(64)
    _add(later, buf, 40, 1, accumulate=not overwrites[0])
    _add(later, buf[20:], 30, 2, accumulate=not overwrites[1])
    later.flush()
    assert _tags(launches) == [[1], [2]]
    assert [job[6] for launch in launches for job in launch] == [not overwrites[0], not overwrites[1]]


def test_the_sixteen_limit_and_the_overlap_rule_together(recorder):
    later, launches = recorder
    buf = torch.zeros(40 * 10)
    order = list(range(20)) + [19, 3]           # twenty disjoint spans, then two of them again
    for tag, k in enumerate(order, start=1):
        _add(later, buf[10 * k:], 10, tag)
    later.flush()
    # sixteen | tags 17..20 | tag 21 is span 19 again, which tag 20 of the open launch holds: a new launch
    assert _tags(launches) == [list(range(1, 17)), [17, 18, 19, 20], [21, 22]]
    _assert_no_launch_holds_overlapping_outputs(launches)
    assert [job[1] for launch in launches for job in launch] == list(range(1, 23))          # the order queued
