"""Engine.reactive_pathways (csrc/pathways.hip) against the numpy restatement of its rule (tests/_pathways_ref.py):
paths equal, capacities equal bit for bit (np.array_equal), status equal.  No tolerance anywhere: every operation of
the rule is exact or pinned.

The shapes are the smallest at which each mechanism can go wrong: N = n + 2 nodes straddling a wave (64, 65) and
the workgroup of 1024 threads (1023, 1024, 1025), three nodes per thread (n = 2048), several sources and sinks (the
virtual edges), several launches of the resumable entry, ties, a cycle, an unreachable sink, every status word."""
import functools

import numpy as np
import pytest

from pmarlo_amd import _lib
from tests import _pathways_ref as R

pytestmark = pytest.mark.gpu


def run(engine, net, role, **kw):
    return engine.reactive_pathways(engine.to_device(np.ascontiguousarray(net, np.float64)), role, **kw)


def check(engine, net, role, fraction, maxiter, want=None, **kw):
    want = R.pathways(net, role, fraction, maxiter) if want is None else want
    paths, caps, status = run(engine, net, role, fraction=fraction, maxiter=maxiter, keep=max(1, len(want[0])), **kw)
    assert status == want[2]
    assert paths == want[0]
    assert caps.dtype == np.float64 and np.array_equal(caps, want[1])
    return want


@functools.lru_cache(maxsize=None)
def table_case(n, n_source, n_sink, fraction, mask, maxiter):
    _, _, _, _, role, net = R.chain_case(n, n_source, n_sink, 1, mask)
    net.setflags(write=False)
    return net, role, R.pathways(net, role, fraction, maxiter)


def lattice(side=4):
    n = side * side
    F = np.zeros((n, n))
    for r in range(side):
        for c in range(side):
            if c < side - 1:
                F[side * r + c, side * r + c + 1] = 1.0
            if r < side - 1:
                F[side * r + c, side * r + c + side] = 1.0
    role = np.zeros(n, np.int32)
    role[0], role[-1] = 1, 2
    return F, role


def test_one_edge(engine):
    net = np.array([[0.0, 0.3], [0.0, 0.0]])
    want = check(engine, net, [1, 2], 0.99, 10)
    assert want[0] == [[0, 1]] and want[1].tolist() == [0.3] and want[2] == R.FRACTION


def test_three_state_line(engine):
    net = np.zeros((3, 3))
    net[0, 1], net[1, 2] = 0.5, 0.25
    want = check(engine, net, [1, 0, 2], 0.99, 10)
    assert want[0] == [[0, 1, 2]] and want[2] == R.NO_PATH      # 0.25 of 0.5 is all that arrives


# N = 64 and 65 straddle a wave; |A| = 3, |B| = 2 exercises the virtual edges; 1021 .. 1023 straddle the workgroup
@pytest.mark.parametrize("case", R.TABLE + [(1021, 1, 1, 0.99, None, 3)], ids=lambda c: f"n{c[0]}")
def test_generator_chains(engine, case):
    net, role, want = table_case(*case)
    assert len(want[0]) > 0
    check(engine, net, role, case[3], case[5], want=want)


def test_three_nodes_a_thread(engine):
    # n = 2048, N = 2050: threads 0 and 1 own three nodes.  Banded flux i -> i + 1, i + 2, i + 3 with distinct weights
    n = 2048
    net = np.zeros((n, n))
    i = np.arange(n)
    for d, scale in ((1, 1.0), (2, 0.75), (3, 0.5)):
        net[i[:-d], i[:-d] + d] = scale * (1.0 + ((i[:-d] * 37 + d * 11) % 101) / 101.0)
    role = np.zeros(n, np.int32)
    role[0], role[-1] = 1, 2
    want = check(engine, net, role, 0.99, 4)
    assert len(want[0]) == 4 and all(len(p) > 600 for p in want[0])


def test_a_run_over_many_launches_gives_the_same_bytes(engine):
    net, role, want = table_case(*R.TABLE[1])
    check(engine, net, role, 0.99, 10_000, want=want, launch_paths=7)
    assert engine.last_pathway_launches >= max(3, len(want[0]) // 7)
    check(engine, net, role, 0.99, 10_000, want=want)
    assert engine.last_pathway_launches == 1


def test_ties_go_to_the_lowest_index(engine):
    net, role = lattice()
    want = check(engine, net, role, 0.99, 100)
    assert want[0][0] == [0, 1, 2, 3, 7, 11, 15]


def test_cycle_in_a_non_reversible_flux(engine):
    net = np.zeros((6, 6))
    net[0, 1], net[1, 2], net[2, 3], net[3, 1] = 1.0, 0.9, 0.8, 0.7     # the cycle 1 -> 2 -> 3 -> 1
    net[3, 5], net[2, 4], net[4, 5], net[0, 4] = 0.6, 0.3, 0.5, 0.2
    role = np.array([1, 0, 0, 0, 0, 2], np.int32)
    want = check(engine, net, role, 1.0, 50)
    assert want[0][0] == [0, 1, 2, 3, 5] and want[2] == R.NO_PATH


def test_sink_unreachable(engine):
    net = np.zeros((5, 5))
    net[0, 1], net[1, 2], net[4, 3] = 0.4, 0.2, 0.1
    paths, caps, status = run(engine, net, [1, 0, 0, 2, 0], fraction=0.99, maxiter=10, keep=3)
    assert paths == [] and caps.shape == (0,) and status == _lib.PATHWAYS_NO_PATH == R.NO_PATH


def test_maxiter_smaller_than_the_number_of_paths(engine):
    net, role, full = table_case(*R.TABLE[0])
    want = check(engine, net, role, 0.99, 4)
    assert want[2] == R.MAXITER == _lib.PATHWAYS_MAXITER and want[0] == full[0][:4]


def test_keep_smaller_than_the_number_of_paths(engine):
    net, role, want = table_case(*R.TABLE[0])
    paths, caps, status = run(engine, net, role, fraction=0.99, maxiter=10_000, keep=5)
    assert paths == want[0][:5] and np.array_equal(caps, want[1]) and status == want[2] == _lib.PATHWAYS_FRACTION
    paths, caps, _ = run(engine, net, role, fraction=0.99, maxiter=10_000, keep=0)
    assert paths == [] and np.array_equal(caps, want[1])


def test_fraction_one_ends_on_the_capacity_floor(engine):
    # the edge 0 -> 1 carries (0.1 + 0.2) and loses 0.2, then 0.1: 2.8e-17 is left, positive, and a third path
    # 0 -> 1 -> 6 -> 5 exists through it; its capacity is under 1e-14 * total, so the decomposition ends there
    net = np.zeros((7, 7))
    net[0, 1], net[0, 4] = 0.1 + 0.2, 0.5
    net[1, 2], net[1, 3], net[1, 6] = 0.2, 0.1, 1e-3
    net[2, 5] = net[3, 5] = net[6, 5] = 1.0
    assert (0.1 + 0.2) - 0.2 - 0.1 > 0.0
    want = check(engine, net, np.array([1, 0, 0, 0, 0, 2, 0], np.int32), 1.0, 10_000)
    assert want[0] == [[0, 1, 2, 5], [0, 1, 3, 5]] and want[1].tolist() == [0.2, 0.1] and want[2] == R.NO_PATH
    # on a generator chain the sum of the capacities reaches the total within the rule's 1e-14 first
    net, role, _ = table_case(*R.TABLE[0])
    check(engine, net, role, 1.0, 10_000)


def test_more_states_than_the_kernel_takes(engine):
    n = 2049
    net = engine.zeros((n, n), np.float64)
    role = np.zeros(n, np.int32)
    role[0], role[-1] = 1, 2
    with pytest.raises(NotImplementedError, match=r"2049.*2048"):
        engine.reactive_pathways(net, role)


def test_bad_input_raises_before_any_walk(engine):
    net, role = lattice()
    engine.last_pathway_launches = -1
    for bad in (np.nan, -1e-300, np.inf):
        m = net.copy()
        m[5, 6] = bad
        with pytest.raises(ValueError, match="negative, infinite or NaN"):
            run(engine, m, role)
    no_source = role.copy()
    no_source[0] = 0
    with pytest.raises(ValueError, match="at least one"):
        run(engine, net, no_source)
    with pytest.raises(ValueError, match="at least one"):
        run(engine, net, np.where(role == 2, 0, role))
    for fraction in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="fraction"):
            run(engine, net, role, fraction=fraction)
    with pytest.raises(ValueError, match="square"):
        engine.reactive_pathways(engine.zeros((4, 5), np.float64), [1, 0, 0, 2])
    assert engine.last_pathway_launches == -1
