"""CPU: the host planner of the episode batch queue (`algorithm/batch_buffer.BatchPlanner`) against the reference
BatchBuffer (golden `f12_batch_buffer.npz`): with the reference's own permutations injected it must form the same
batches, window by window, and its pool slots must never exceed P nor be handed out while live."""
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / 'golden'


def _planner_run(g, check_slots=None):
    from algorithm.batch_buffer import BatchPlanner
    perms = [g[f'put{i}/perm'] for i in range(int(g['n_put']))]
    planner = BatchPlanner(int(g['batch_size']), int(g['max_size']), permutation=lambda n: perms.pop(0))
    got, n_put = [], 0
    for op in g['ops']:
        if op == 0:
            T = g[f'put{n_put}/ep_indexes'].shape[1]
            planner.put(T - 1, tags=[(n_put, i) for i in range(T - 1)])
            assert len(perms) == int(g['n_put']) - n_put - 1, 'one permutation per put'
            n_put += 1
        else:
            got.append(None if not planner.queue else [planner.tags[s] for s in planner.queue[0]])
            planner.pop()
        if check_slots is not None:
            check_slots(planner)
    return got


def test_planner_forms_the_reference_batches():
    g = np.load(GOLDEN / 'f12_batch_buffer.npz')
    got = _planner_run(g)
    assert len(got) == int(g['n_get'])
    for j, batch in enumerate(got):
        if bool(g[f'get{j}/empty']):
            assert batch is None, f'get {j}: the reference queue was empty'
            continue
        assert batch is not None, f'get {j}: the reference returned a batch'
        want = [tuple(int(x) for x in w) for w in g[f'get{j}/windows']]
        assert [tuple(t) for t in batch] == want, f'get {j}'


def test_planner_slots_stay_in_pool_and_unique():
    g = np.load(GOLDEN / 'f12_batch_buffer.npz')
    P = (int(g['max_size']) + 1) * int(g['batch_size'])
    peak = [0]

    def check(planner):
        live = planner.live_slots()
        assert len(live) == len(set(live)), 'a pool slot is used twice while live'
        assert all(0 <= s < P for s in live)
        assert len(live) <= P
        assert len(planner.queue) <= planner.max_size and len(planner.rest) < planner.batch_size
        assert set(live).isdisjoint(planner._free) and len(live) + len(planner._free) == P
        assert planner.tail - planner.head == len(planner.queue)
        peak[0] = max(peak[0], len(live))

    _planner_run(g, check)
    assert peak[0] > 10 * int(g['batch_size']) - int(g['batch_size']), 'the script must fill the queue'


def test_planner_queue_rows_and_head():
    """the queue rows a put writes are the batches' absolute numbers mod (max_size + 1); a drop moves the head"""
    from algorithm.batch_buffer import BatchPlanner
    p = BatchPlanner(4, max_size=2, permutation=lambda n: np.arange(n))
    plan = p.put(9)                       # 9 windows: batches 0, 1, rest 1
    assert plan['queue_rows'] == [0, 1] and plan['head'] == 0 and len(p.rest) == 1
    plan = p.put(11)                      # 1 + 11 = 12: batches 2, 3, 4 -> 0, 1, 2 dropped
    assert plan['queue_rows'] == [0, 1] and plan['head'] == 3 and p.rest == []
    assert len(plan['win_slot']) == 8       # batch 2's windows (with the old rest window) never got a slot
    assert p.pop() is not None and p.head == 4 and p.pop() is not None and p.pop() is None
    assert p.put(0) is None


@pytest.mark.parametrize('B', [1, 3, 8])
def test_planner_random_scripts_keep_the_invariants(B):
    from algorithm.batch_buffer import BatchPlanner
    rng = np.random.default_rng(B)
    p = BatchPlanner(B, max_size=3, permutation=lambda n: rng.permutation(n))
    P = p.pool_slots
    for _ in range(200):
        if rng.random() < 0.5:
            p.put(int(rng.integers(0, 3 * B + 2)))
        else:
            p.pop()
        live = p.live_slots()
        assert len(live) == len(set(live)) and len(live) <= P and all(0 <= s < P for s in live)
