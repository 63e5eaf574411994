"""CPU-only: the numpy restatement of the intermediate scattering function (tests/scattering_ref.py) held to an independent
``np.longdouble`` evaluation within the derived error bound and to closed forms, so that the GPU tests compare the kernels with
something that is itself pinned.  The bound is that of DESIGN.md section 22; nothing here is taken from what the code gives."""
import numpy as np
import pytest

from tests import msd_ref as R
from tests import scattering_ref as S
from tests import vanhove_ref as V

Q_EDGE = np.array([[0, 0, 0], [32, 0, 0], [0, -32, 0], [0, 0, 32], [-32, 32, -32], [32, 32, 32], [1, -2, 3], [-1, 0, 0]])


def q_list(seed, n=40):
    return np.concatenate([Q_EDGE, np.random.default_rng(seed).integers(-32, 33, size=(n, 3))])


def modulus(re, im):
    return np.sqrt((re * re + im * im).astype(np.float64))


def test_sincos_error_is_within_what_the_bound_keeps():
    """The measurement of the error model: a dense sample and the designed arguments, each +-1 ulp."""
    v = np.array([0.0, 0.125, -0.125, 0.25, -0.25, 0.375, -0.375, 0.5, -0.5])
    designed = np.concatenate([v, np.nextafter(v, 1.0), np.nextafter(v, -1.0)])
    dense = np.concatenate([np.random.default_rng(1).uniform(-0.5, 0.5, 1000000), np.linspace(-0.5, 0.5, 1000001)])
    worst = []
    for f in (dense, designed):
        c, s = S.sincos2pi(f)
        xc, xs = S.exact_unit(f)
        worst.append(modulus(c - xc, s - xs).max() / S.U)
    print("sc_sincos2pi: worst error %.3f u over the dense sample, %.3f u at the designed arguments; the bound keeps %.2f u"
          % (worst[0], worst[1], S.E_SINCOS))
    assert max(worst) <= S.E_SINCOS and 1.2 * max(worst) <= S.E_SINCOS          # the bound keeps a factor over the measurement
    assert np.all(np.abs(modulus(*S.sincos2pi(dense)) - 1.0) <= 2 * S.E_SINCOS * S.U)


@pytest.mark.parametrize("n", [1, 3, 64, 65, 130])
def test_density_modes_are_within_the_bound_of_the_long_double_evaluation(n):
    rng = np.random.default_rng(10 + n)
    q = q_list(n)
    f = rng.uniform(-0.5, 0.5, size=(6, n, 3))
    f[0, 0] = [0.5, -0.5, 0.25]
    f[1, n - 1] = [0.125, -0.375, 0.0]
    f[2] = np.round(f[2] * 8.0) / 8.0                                 # a frame of designed arguments only
    re, im = S.density(f, q)
    xr, xi = S.exact_term(f, q)                                       # [6, n, n_q]
    err = modulus(re - xr.sum(axis=1), im - xi.sum(axis=1))
    assert np.all(err <= S.sum_bound(q, n)[None, :])
    assert np.all(re[:, 0] == n) and np.all(im[:, 0] == 0.0)          # (0, 0, 0) counts the atoms


def test_sums_are_within_the_bound_of_the_definition():
    """Self and coherent sums of a walk in a triclinic cell across a block of origins, against the long-double sum of the
    exact terms of the same float64 phases."""
    cell = R.TRICLINIC
    ci = V.cell_matrices(cell)[1]
    F, a, b = S.BLOCK + 9, np.array([0, 2, 3]), np.array([1, 4])
    x = R.random_walk(F, 5, seed=3) * 3.0
    q, lags = q_list(7, 12), [0, 1, 8, F - 1]
    f = S.frac(x, ci)
    ss, cs = S.sums(x, cell, a, b, False, q, lags, 2)
    er_a, ei_a = S.exact_term(f[:, a], q)
    er_b, ei_b = S.exact_term(f[:, b], q)
    rho_a, rho_b = (er_a + 1j * ei_a).sum(axis=1), (er_b + 1j * ei_b).sum(axis=1)
    for x_l, tau in enumerate(lags):
        n_or = S.n_origins(F, tau, 2)
        t = np.arange(n_or) * 2
        exact_c = (rho_b[t + tau] * np.conj(rho_a[t])).sum(axis=0)
        assert np.all(np.abs(cs[x_l] - exact_c).astype(np.float64) <= S.coherent_bound(q, 3, 2, n_or))
        dr, di = S.exact_term(S.delta(f[t + tau][:, a], f[t][:, a]), q)
        exact_s = (dr + 1j * di).sum(axis=(0, 1))
        assert np.all(np.abs(ss[x_l] - exact_s).astype(np.float64) <= S.sum_bound(q, n_or * 3))
    assert np.all(ss[0] == S.n_origins(F, 0, 2) * 3)                  # lag 0: exactly origins x n_a + 0i
    origins = np.array([S.n_origins(F, t, 2) for t in lags])[:, None]
    assert np.all((ss / (origins * 3))[0] == 1.0)
    assert np.all(np.abs(ss) <= origins * 3 * (1 + 1e-12)) and np.abs(ss[1:, 1:]).min() < 0.9 * origins[1:].min() * 3


@pytest.mark.parametrize("n,edge,offset", [(4, 8.0, 0.0), (3, 6.0, 0.37)])
def test_simple_cubic_lattice_at_rest(n, edge, offset):
    """n^3 atoms on a simple cubic lattice in its supercell: S(q) = N where all three indices are multiples of n (exactly so for
    n = 4 in a cell of edge 8, where every phase is a multiple of 1/4), and nothing but rounding elsewhere."""
    g = np.arange(n) * (edge / n)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + offset
    N = n ** 3
    x = np.repeat(pos[None], 3, axis=0)
    cell = np.eye(3) * edge
    r = np.arange(-2 * n, 2 * n + 1)
    q = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    cs = S.coherent_sums(x, cell, np.arange(N), None, q, [0, 1], 1)
    s_q = cs[0] / (3.0 * N)
    bragg = np.all(q % n == 0, axis=1)
    delta = S.sum_bound(q, N)
    # phases a rounding of x . ci away from the lattice's: the aligned terms lose modulus at second order only
    eps = 2.0 * np.pi * np.abs(q).sum(axis=1) * 8.0 * S.U
    if offset == 0.0:
        assert np.all(s_q[bragg] == N) and np.all(cs[1, bragg] == 2.0 * N * N)
    tol = S.coherent_bound(q, N, N, 3) / (3.0 * N)                    # of C / (origins N): twice delta and the product's rounding
    assert np.all(np.abs(np.abs(s_q[bragg]) - N) <= tol[bragg] + N * eps[bragg] ** 2)
    assert bragg.sum() == 5 ** 3 and np.all(np.abs(s_q[~bragg]) <= N * (S.term_bound(q[~bragg]) + eps[~bragg]))
    assert np.all(np.abs(s_q[~bragg]) <= (delta[~bragg] + N * eps[~bragg]) ** 2 / N * (1 + 1e-6))


def test_uniform_motion_has_a_pure_phase():
    """x = x_0 + v t in a cell with power-of-two edges and a velocity of whole 1/256 of an edge per frame: every phase is exact and
    F_s(q, tau) = exp(i q . v tau) for every origin, so the mean over origins and atoms is that number to the bound of one term
    and of the sum."""
    cell = np.diag([8.0, 4.0, 16.0])
    v = np.array([3.0 / 256, -5.0 / 256, 1.0 / 64]) * np.diag(cell)
    rng = np.random.default_rng(5)
    x0 = np.round(rng.uniform(0.0, 4.0, size=(4, 3)) * 1024.0) / 1024.0
    F = S.BLOCK + 40
    x = x0[None] + np.arange(F)[:, None, None] * v[None, None, :]
    q = q_list(9, 20)
    lags = [1, 7, 100]
    ss = S.self_sums(x, cell, np.arange(4), q, lags, 1)
    for x_l, tau in enumerate(lags):
        n = S.n_origins(F, tau, 1) * 4
        er, ei = S.exact_unit((q.astype(np.float64) @ (v / np.diag(cell))) * tau)
        assert np.all(np.abs(ss[x_l] / n - (er + 1j * ei)).astype(np.float64) <= S.sum_bound(q, n) / n)
    assert np.abs(ss[0, 6] / (S.n_origins(F, 1, 1) * 4) - 1.0) > 0.01                    # and it is a phase that turns


def test_whole_cell_vectors_change_no_bit():
    """An orthorhombic cell with power-of-two edges, positions on a grid of 2^-20: moving any atom by any whole number of cell
    vectors, a different one in every frame, leaves every sum bit-identical."""
    cell = np.diag([8.0, 4.0, 16.0])
    rng = np.random.default_rng(6)
    F, n = 20, 5
    x = rng.integers(0, 1 << 22, size=(F, n, 3)) / float(1 << 20)
    moved = x + rng.integers(-1000, 1001, size=(F, n, 3)) * np.diag(cell)[None, None, :]
    assert np.abs(moved).max() > 1000.0
    q, lags = q_list(11, 10), [0, 1, 5, 19]
    a, b = np.array([0, 1, 2]), np.array([3, 4])
    for got, exp in zip(S.sums(moved, cell, a, b, False, q, lags, 1), S.sums(x, cell, a, b, False, q, lags, 1)):
        assert got.tobytes() == exp.tobytes()


def test_minus_q_is_the_conjugate():
    cell = R.HEX
    x = R.random_walk(30, 4, seed=8) * 2.0
    q = q_list(12, 10)
    a = np.arange(4)
    plus = S.coherent_sums(x, cell, a, None, q, [0, 3], 1)
    minus = S.coherent_sums(x, cell, a, None, -q, [0, 3], 1)
    for x_l, tau in enumerate([0, 3]):
        assert np.all(np.abs(minus[x_l] - np.conj(plus[x_l])) <= 2.0 * S.coherent_bound(q, 4, 4, S.n_origins(30, tau, 1)))
    assert np.all(plus[0].imag == 0.0) and np.all(plus[0].real >= 0.0)                   # S(q) of one selection is |rho|^2
    sp = S.self_sums(x, cell, a, q, [3], 1)
    sm = S.self_sums(x, cell, a, -q, [3], 1)
    assert np.all(np.abs(sm - np.conj(sp)) <= 2.0 * S.sum_bound(q, S.n_origins(30, 3, 1) * 4))


def test_nan_stays_in_its_selection():
    cell = R.ORTHO
    x = R.random_walk(12, 4, seed=9)
    x[5, 1, 2] = np.nan
    q = q_list(13, 5)
    ss, cs = S.sums(x, cell, np.array([0, 1]), np.array([2, 3]), False, q, [0, 2], 1)
    assert np.all(np.isnan(cs.real)) and np.all(np.isnan(ss[1].real)) and np.all(ss[0] == 24.0)
    ss, cs = S.sums(x, cell, np.array([2, 3]), np.array([0, 3]), False, q, [0, 2], 1)
    assert np.all(np.isfinite(ss.real)) and np.all(np.isfinite(cs.real))


def test_operators_helpers_on_the_host():
    """``q_vectors`` and the shell average need no device."""
    from sitator_amd.dynamics import _shell_average, q_vectors
    cell = R.TRICLINIC
    recip = 2.0 * np.pi * np.linalg.inv(cell.T)
    full = q_vectors(cell, 4.0, half_space=False)
    half = q_vectors(cell, 4.0)
    norm = np.linalg.norm(full @ recip, axis=1)
    assert np.all((norm > 0) & (norm <= 4.0)) and np.all(np.diff(norm) >= -1e-12) and len(full) == 2 * len(half) > 20
    assert {tuple(v) for v in full} == {tuple(v) for v in half} | {tuple(-v) for v in half}
    r = np.arange(-9, 10)
    brute = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    bn = np.linalg.norm(brute @ recip, axis=1)
    assert {tuple(v) for v in full} == {tuple(v) for v in brute[(bn > 0) & (bn <= 4.0)]}
    with pytest.raises(ValueError, match="cell length"):
        q_vectors(np.eye(3) * 10.0, 25.0)
    assert np.abs(q_vectors(np.eye(3) * 10.0, 2.0 * np.pi * 3.2 * (1 + 1e-9))).max() == 32
    mean, count = _shell_average(np.array([0.5, 1.5, 1.7, 9.0]), np.array([[1.0, 2.0, 4.0, 8.0]]), [0.0, 1.0, 2.0, 3.0])
    assert list(count) == [1, 2, 0] and mean[0, 0] == 1.0 and mean[0, 1] == 3.0 and np.isnan(mean[0, 2])
