"""The numpy restatement of the reactive-pathway rule (tests/_pathways_ref.py) against the repository's host walk,
markov_state_model/tpt.py::_widest_path inside the loop of pathway_decomposition.  No GPU: the net flux comes from
the generator's numpy TPT, and the loop of pathway_decomposition is replayed around the real _widest_path."""
import numpy as np
import pytest

from pmarlo_amd.markov_state_model.tpt import _widest_path
from tests import _pathways_ref as R


def host_walk(net, source, sink, fraction, maxiter):
    """pathway_decomposition from its net flux on (markov_state_model/tpt.py), with its own numpy sums."""
    n = net.shape[0]
    G = np.zeros((n + 2, n + 2))
    G[:n, :n] = net
    out_A = net[source].sum(axis=1)
    G[n, source] = out_A
    G[sink, n + 1] = net[:, sink].sum(axis=0)
    total = float(out_A.sum())
    paths, caps, got = [], [], 0.0
    while len(paths) < int(maxiter) and total > 0 and got < fraction * total * (1.0 - 1e-14):
        path, cap = _widest_path(G, n, n + 1)
        if path is None or cap <= 1e-14 * total:
            break
        for a, b in zip(path[:-1], path[1:]):
            G[a, b] = max(0.0, G[a, b] - cap)
        paths.append([int(v) for v in path[1:-1]])
        caps.append(cap)
        got += cap
    return paths, np.asarray(caps, dtype=float)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("n,n_source,n_sink,fraction,mask,maxiter", R.TABLE)
def test_restatement_equals_the_host_walk(n, n_source, n_sink, fraction, mask, maxiter, seed):
    _, _, source, sink, role, net = R.chain_case(n, n_source, n_sink, seed, mask)
    want_paths, want_caps = host_walk(net, source, sink, fraction, maxiter)
    paths, caps, status = R.pathways(net, role, fraction, maxiter)
    print(f"n={n} seed={seed}: {len(paths)} paths, status {status}")
    assert len(want_paths) > 0
    assert paths == want_paths
    assert np.array_equal(caps, want_caps)
    assert status == (R.MAXITER if len(paths) == maxiter else R.FRACTION)


def test_widest_path_alone_on_ties_and_dead_ends():
    # 4 x 4 lattice, every edge 1 (right and down): the lowest index wins every tie
    n = 16
    F = np.zeros((n, n))
    for r in range(4):
        for c in range(4):
            if c < 3:
                F[4 * r + c, 4 * r + c + 1] = 1.0
            if r < 3:
                F[4 * r + c, 4 * r + c + 4] = 1.0
    assert R.widest_path(F, 0, 15) == _widest_path(F, 0, 15)
    # a sink no positive edge reaches
    F[:, 15] = 0.0
    assert R.widest_path(F, 0, 15) == (None, 0.0) == _widest_path(F, 0, 15)


def test_status_words():
    net = np.zeros((3, 3))
    net[0, 1], net[1, 2] = 0.5, 0.25
    role = np.array([1, 0, 2])
    paths, caps, status = R.pathways(net, role, 0.99, 10)
    # the virtual sink edge carries 0.25 and bounds the one path; the total is the 0.5 that leaves the source
    assert paths == [[0, 1, 2]] and caps.tolist() == [0.25] and status == R.NO_PATH
    assert R.pathways(net, role, 0.5, 10)[2] == R.FRACTION
    assert R.pathways(net, role, 0.99, 1)[2] == R.MAXITER
    assert R.pathways(np.zeros((3, 3)), role, 0.99, 10) == ([], pytest.approx([]), R.NO_PATH)
