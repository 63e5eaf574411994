"""GPU: ``sit_pca_covariance`` and ``sit_pca_project`` against numpy.

Every mean, covariance entry and projection must be within ``1e-12 * B`` of numpy's, ``B`` being the same sum with every term
replaced by its absolute value.  That is derived, not measured: a term (two subtractions and a product) is good to ``3 eps``, a
float64 sum of N terms in any order to ``N eps`` of the sum of their absolute values, and N is at most 4096 (asserted):
``(N + 3) 2^-53 < 5e-13``.  The device centres with its own mean, which is within ``N eps`` of numpy's; that enters the
covariance in second order only.  The shapes are the smallest at which the kernels can go wrong: one row, two, rows around the
16-row steps of a workgroup, one chunk of rows + 1, columns of 1, below and above a multiple of the 16-column block, fewer rows
than columns."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CELL = np.eye(3) * 10.0
TOL = 1e-12


def plan():
    from sitator_amd import _lib
    return _lib.dpc_plan(1)


def rows(N, D, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(N, D)) * rng.uniform(0.1, 3.0, D) + rng.uniform(-1.0, 1.0, D)


SHAPES = [(1, 1), (1, 63), (2, 1), (2, 65), (65, 63), (65, 65), (17, 1), ("chunk+1", 1), ("chunk+1", 63), ("chunk+1", 65), (40, 65),
          ("2chunks+17", 20)]


def shape_of(N, D):
    pl = plan()
    return {"chunk+1": pl["pca_rows"] + 1, "2chunks+17": 2 * pl["pca_rows"] + 17}.get(N, N), D


@pytest.mark.parametrize("N,D", SHAPES)
def test_mean_and_covariance_against_numpy(N, D):
    from sitator_amd import _lib
    N, D = shape_of(N, D)
    assert N <= 4096
    X = rows(N, D, 7 * N + D)
    with contextlib.closing(_lib.HipContext(CELL)) as ctx:
        mean, cov = ctx.pca_covariance(X)
        mean2, cov2 = ctx.pca_covariance(X)
    exp_mean = np.sum(X, axis=0) / N
    B_mean = np.sum(np.abs(X), axis=0) / N
    Xc = X - exp_mean
    div = max(N - 1, 1)
    exp_cov = Xc.T @ Xc / div
    B_cov = np.abs(Xc).T @ np.abs(Xc) / div
    print("N %d D %d: worst mean %.3e, worst cov %.3e (of B)" % (N, D, np.max(np.abs(mean - exp_mean) / B_mean),
                                                             np.max(np.abs(cov - exp_cov) / np.where(B_cov > 0, B_cov, 1.0))))
    assert np.all(np.abs(mean - exp_mean) <= TOL * B_mean)
    assert np.all(np.abs(cov - exp_cov) <= TOL * B_cov + (0.0 if N > 1 else 1e-300))
    assert mean.tobytes() == mean2.tobytes() and cov.tobytes() == cov2.tobytes()
    assert cov.tobytes() == np.ascontiguousarray(cov.T).tobytes()     # symmetric bit for bit
    if N == 1:
        assert np.all(cov == 0.0)


@pytest.mark.parametrize("N,D,d", [(1, 1, 1), (2, 65, 2), (65, 63, 32), ("chunk+1", 65, 5), (40, 65, 3), (300, 1, 1)])
def test_projection_against_numpy(N, D, d):
    from sitator_amd import _lib
    N, D = shape_of(N, D)
    X = rows(N, D, 3 * N + D)
    rng = np.random.default_rng(d)
    mean = X.mean(axis=0)
    comps = np.linalg.qr(rng.normal(size=(D, D)))[0][:d] if d <= D else rng.normal(size=(d, D))
    comps = np.ascontiguousarray(comps)
    with contextlib.closing(_lib.HipContext(CELL)) as ctx:
        Y = ctx.pca_project(X, mean, comps)
        Y2 = ctx.pca_project(X, mean, comps)
    exp = (X - mean) @ comps.T
    B = np.abs(X - mean) @ np.abs(comps.T)
    assert D <= 4096 and Y.shape == (N, d)
    assert np.all(np.abs(Y - exp) <= TOL * B)
    assert Y.tobytes() == Y2.tobytes()


def test_error_returns():
    from sitator_amd import _lib
    pl = plan()
    X = rows(20, 5, 1)
    with contextlib.closing(_lib.HipContext(CELL)) as ctx:
        for bad in (np.nan, -np.inf, 1e200):
            Z = X.copy()
            Z[11, 3] = bad
            with pytest.raises(ValueError):
                ctx.pca_covariance(Z)
            with pytest.raises(ValueError):
                ctx.pca_project(Z, np.zeros(5), np.eye(5)[:2])
        with pytest.raises(ValueError):
            ctx.pca_covariance(np.zeros((0, 5)))
        with pytest.raises(ValueError):
            ctx.pca_project(X, np.zeros(5), np.full((2, 5), np.nan))
        with pytest.raises(RuntimeError, match="columns"):
            ctx.pca_covariance(np.zeros((2, pl["pca_max_d"] + 1)))
        with pytest.raises(RuntimeError, match="d at most 32"):
            ctx.pca_project(np.zeros((3, 40)), np.zeros(40), np.zeros((pl["max_d"] + 1, 40)))
        mean, cov = ctx.pca_covariance(X)                             # the context is as good as before
        assert np.allclose(mean, X.mean(axis=0), rtol=1e-12, atol=0) and np.allclose(cov, np.cov(X.T), rtol=1e-10, atol=1e-14)
