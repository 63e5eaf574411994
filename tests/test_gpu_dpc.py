"""GPU: ``sit_dpc_graph`` and ``sit_dpc_assign`` against the numpy restatement (tests/dpc_ref.py: a dense matrix, a sort, loops).

``kernel_size`` must be the restatement's sorted element bit for bit: both evaluate the distance in the order of
``csrc/dpc_plan.h``.  Every ``density`` must be within ``1e-12 * rho_i``.  That is derived, not measured: at most 4097 positive
terms summed in another order differ by at most ``N * 2^-53 < 5e-13`` of their sum, the rest is left for the device's ``exp``,
whose argument the cases keep at ``(d / dc)^2 <= 700`` (asserted; where ``dc`` is 0 a term is exactly 0 or 1).  ``delta`` must be
bit-equal and ``neighbour`` equal to what the restatement gives when handed the DEVICE's densities: rounding in ``rho`` then
cannot flip an order.  The shapes are the smallest at which the kernels can go wrong: N around the wave width and the tile, more
than one tile, more tiles than segments (a segment of two tiles), d of 1, 2, one that is padded and the cap."""
import contextlib
import functools

import numpy as np
import pytest

from tests import dpc_ref as DR

pytestmark = pytest.mark.gpu

CELL = np.eye(3) * 10.0
RANK0, MIDDLE, LAST = 1e-12, 0.3, 1.0 - 1e-12


def plan():
    from sitator_amd import _lib
    return _lib.dpc_plan(1)


def points(kind, N, d, seed):
    rng = np.random.default_rng(seed)
    if kind == "cloud":                                             # two blobs
        Y = rng.normal(size=(N, d)) * 0.3
        Y[N // 2:, 0] += 3.0
    elif kind == "uniform":
        Y = rng.uniform(0.0, 1.0, size=(N, d))
    elif kind == "grid":                                            # many equal distances, densities equal by symmetry
        side = int(np.ceil(np.sqrt(N)))
        Y = np.zeros((N, d))
        Y[:, 0] = np.arange(N) % side
        Y[:, d - 1] += np.arange(N) // side * (1.0 if d > 1 else float(side))
    elif kind == "duplicates":                                      # every point three times, and a few once
        base = rng.normal(size=((N + 2) // 3, d))
        Y = np.concatenate([base, base, base])[:N]
    elif kind == "equal":
        Y = np.full((N, d), 0.37)
    elif kind == "outlier":
        Y = rng.normal(size=(N, d)) * 0.3
        Y[N // 3] = 6.0 / np.sqrt(d)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(Y)


# (name, N, d, kind, fractions)
RAW = [
    ("n2", 2, 1, "uniform", (RANK0, 0.5, LAST)),
    ("n3", 3, 2, "uniform", (RANK0, 0.5, LAST)),
    ("n63_grid", 63, 2, "grid", (RANK0, MIDDLE, LAST)),
    ("n64_cap", 64, "cap", "cloud", (MIDDLE, LAST)),
    ("n65_d1", 65, 1, "uniform", (MIDDLE, LAST)),
    ("n65_dup", 65, 2, "duplicates", (RANK0, MIDDLE)),
    ("n40_equal", 40, 3, "equal", (RANK0, MIDDLE, LAST)),
    ("tile", "tile", 2, "cloud", (MIDDLE,)),
    ("tile+1_outlier", "tile+1", 5, "outlier", (MIDDLE, LAST)),
    ("tiles3+1_cap", "3tiles+1", "cap", "uniform", (0.02, MIDDLE)),
    ("tiles8+1", "8tiles+1", 2, "cloud", (MIDDLE,)),
    ("tiles8+1_dup", "8tiles+1", 1, "duplicates", (RANK0,)),
]


@functools.lru_cache(maxsize=None)
def case(name):
    _, N, d, kind, fractions = next(c for c in RAW if c[0] == name)
    pl = plan()
    N = {"tile": pl["tile"], "tile+1": pl["tile"] + 1, "3tiles+1": 3 * pl["tile"] + 1, "8tiles+1": pl["segments"] * pl["tile"] + 1}.get(N, N)
    d = pl["max_d"] if d == "cap" else d
    Y = points(kind, N, d, 100 + len(name))
    dist = DR.distances(Y)
    dist.setflags(write=False)
    return {"Y": Y, "dist": dist, "fractions": fractions, "N": N}


@pytest.mark.parametrize("name", [c[0] for c in RAW])
def test_graph_against_restatement(name):
    from sitator_amd import _lib
    c = case(name)
    Y, dist, N = c["Y"], c["dist"], c["N"]
    assert N <= 4097                                                 # the term count the density bound was derived for
    ranks = set()
    with contextlib.closing(_lib.HipContext(CELL)) as ctx:
        for fraction in c["fractions"]:
            dc, rank, n = DR.kernel_size(dist, fraction)
            ranks.add(rank)
            ks, rho, delta, nbr, info = ctx.dpc_graph(Y, fraction)
            again = ctx.dpc_graph(Y, fraction)
            assert info["pairs"] == n == N * (N - 1) // 2
            assert np.float64(ks).view(np.uint64) == np.float64(dc).view(np.uint64), "kernel size %r, the sorted element is %r" % (ks, dc)
            if dc > 0.0:
                assert np.max((dist / dc) ** 2) <= 700.0
            exp_rho = DR.density(dist, dc)
            print("%s fraction %g: rank %d of %d, dc %.6g, worst |rho - ref| / ref %.3e" % (
                name, fraction, rank, n, dc, np.max(np.abs(rho - exp_rho) / np.where(exp_rho > 0, exp_rho, 1.0))))
            assert np.all(np.abs(rho - exp_rho) <= 1e-12 * exp_rho)
            exp_delta, exp_nbr = DR.delta_neighbour(dist, rho)
            assert np.array_equal(nbr, exp_nbr)
            assert np.array_equal(delta.view(np.uint64), exp_delta.view(np.uint64))
            assert again[0] == ks and all(a.tobytes() == b.tobytes() for a, b in zip(again[1:4], (rho, delta, nbr)))
    if RANK0 in c["fractions"]:
        assert 0 in ranks
    if LAST in c["fractions"]:
        assert N * (N - 1) // 2 - 1 in ranks


def forest(N, seed, roots):
    """Densities, deltas and neighbours of a forest with several points without a neighbour."""
    rng = np.random.default_rng(seed)
    rho = rng.permutation(N).astype(np.float64) + 1.0
    delta = rng.uniform(0.0, 1.0, N)
    nbr = np.full(N, -1, dtype=np.int32)
    order = np.argsort(-rho)
    for pos in range(roots, N):
        nbr[order[pos]] = order[rng.integers(0, pos)]
    delta[order[:roots]] = np.linspace(5.0, 2.0, roots)
    return rho, delta, nbr, order


@pytest.mark.parametrize("what", ["one_cluster", "several", "chain_to_nowhere", "none"])
def test_assign_against_restatement(what):
    from sitator_amd import _lib
    pl = plan()
    N, K = 2 * pl["tile"] + 1, 7
    rho, delta, nbr, order = forest(N, 5, 1 if what == "one_cluster" else 4)
    site = np.random.default_rng(6).integers(0, K, N)
    thr = {"one_cluster": (0.0, 1.5), "several": (N * 0.5, 0.8), "chain_to_nowhere": (0.0, 3.5), "none": (2.0 * N, 0.0)}[what]
    member, clusters = DR.assign(rho, delta, nbr, *thr)
    assert {"one_cluster": len(clusters) == 1 and (member == 0).all(), "several": len(clusters) > 3,
            "chain_to_nowhere": len(clusters) == 2 and (member < 0).any() and (member >= 0).any(),
            "none": len(clusters) == 0 and (member < 0).all()}[what]
    with contextlib.closing(_lib.HipContext(CELL)) as ctx:
        got_member, got_clusters, votes = ctx.dpc_assign(rho, delta, nbr, thr[0], thr[1], site, K)
        no_votes = ctx.dpc_assign(rho, delta, nbr, thr[0], thr[1])
    assert np.array_equal(got_member, member) and np.array_equal(got_clusters, clusters)
    assert votes.shape == (K, len(clusters)) and np.array_equal(votes, DR.votes(member, site, K, len(clusters)))
    assert np.array_equal(no_votes[0], member) and no_votes[2] is None


def test_assign_a_chain_as_long_as_the_points():
    from sitator_amd import _lib
    N = 3000
    rho, delta, nbr = np.arange(N, 0, -1.0), np.ones(N), np.arange(-1, N - 1, dtype=np.int32)
    delta[0] = 5.0
    with contextlib.closing(_lib.HipContext(CELL)) as ctx:
        member, clusters, _ = ctx.dpc_assign(rho, delta, nbr, 0.0, 2.0)
    assert list(clusters) == [0] and (member == 0).all()


def test_error_returns():
    import ctypes as C
    from sitator_amd import _lib
    pl = plan()
    Y = points("cloud", 20, 2, 1)
    rho, delta, nbr, _ = forest(20, 2, 2)
    with contextlib.closing(_lib.HipContext(CELL)) as ctx:
        with pytest.raises(ValueError):
            ctx.dpc_graph(Y[:1], 0.1)                                # N < 2
        for fraction in (0.0, 1.0, -0.5, float("nan")):
            with pytest.raises(ValueError):
                ctx.dpc_graph(Y, fraction)
        for bad in (np.nan, np.inf, 1e200):
            Z = Y.copy()
            Z[7, 1] = bad
            with pytest.raises(ValueError):
                ctx.dpc_graph(Z, 0.1)
        with pytest.raises(RuntimeError, match="d at most 32"):
            ctx.dpc_graph(np.zeros((5, pl["max_d"] + 1)), 0.1)       # a limit of the plan, named
        ks = C.c_double(0.0)
        out = np.zeros(20)
        assert ctx.lib.sit_dpc_graph(ctx._h, None, 20, 2, 0.1, C.byref(ks), _lib._d(out), _lib._d(out), None, None) == _lib.E_INVALID
        with pytest.raises(ValueError):
            ctx.dpc_assign(rho, delta, nbr, 0.0, 0.0, np.full(20, 3), 3)          # a site index outside [0, K)
        with pytest.raises(ValueError):
            ctx.dpc_assign(rho, delta, nbr, 0.0, 0.0, np.full(20, -1), 3)
        wrong = nbr.copy()
        wrong[4] = 20
        with pytest.raises(ValueError):
            ctx.dpc_assign(rho, delta, wrong, 0.0, 0.0)
        with pytest.raises(ValueError):
            ctx.dpc_assign(np.where(np.arange(20) == 3, np.nan, rho), delta, nbr, 0.0, 0.0)
        # the context is as good as before
        ks2, rho2, _, _, _ = ctx.dpc_graph(Y, 0.3)
        assert ks2 == DR.kernel_size(DR.distances(Y), 0.3)[0]
    with pytest.raises(RuntimeError):
        _lib.dpc_plan(pl["max_d"] + 1)
    assert _lib.dpc_plan(pl["max_d"])["lds_bytes"] == pl["tile"] * pl["max_d"] * 8 + 2048
