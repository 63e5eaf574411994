"""GPU: the landmark pruning tables as they lie on the device (sit_candidate_table), against the exhaustive periodic
reference of tests/candidates_ref.py and, integer for integer, against the table the host probe of
tests/test_candidates_plan.py builds from the same header (candidates_plan.h) - and landmark rows at the edge the bound
of candidates.hip exists for: static atoms displaced by almost static_thr towards an ion in the corner of its bin.

Every landmark vector passes through these tables: a landmark missing from an ion's bin is written as 0.0 unevaluated.
The rows-against-oracle tests elsewhere notice a missing landmark only if an ion happens to need it; here the tables
themselves are read."""
import numpy as np
import pytest

from tests import candidates_ref as R
from tests import test_candidates_plan as P

pytestmark = pytest.mark.gpu

DEVICE_CASES = ["ortho_c1d", "ortho_2x2x2", "hexagonal_7", "triclinic_skewed", "slab_1p4", "large_400x300x100", "ragged",
                "ragged_with_empty", "on_planes"]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return P.build_probe(tmp_path_factory.mktemp("candidates_plan_gpu"))


def _context(case):
    from sitator_amd import _lib
    ctx = _lib.HipContext(case.cell)
    ctx.set_basis(case.ref_static, case.verts, case.vcd, P.MIDPOINT, P.STEEPNESS, P.STATIC_THR)
    return ctx


def _differences(case, ref, dev, host):
    """The (bin, landmark) pairs on which two tables differ, with their reference margins."""
    a = np.zeros((ref.nb, ref.D), dtype=bool)
    b = np.zeros((ref.nb, ref.D), dtype=bool)
    a[np.repeat(np.arange(ref.nb), np.diff(dev["off"])), dev["list"]] = True
    b[np.repeat(np.arange(ref.nb), np.diff(host["off"])), host["list"]] = True
    return ["bin %d landmark %d: device %s, host %s, margin %.3e" % (i, k, a[i, k], b[i, k], ref.margin[i, k])
            for i, k in np.argwhere(a != b)[:10]]


def _check_device_table(case, probe, dev, W, mean, grid, bin_target, label):
    assert dev["grid"] == list(grid) == R.grid_of(case.cell, bin_target), label
    ref = case.reference(dev["displacement"], dev["grid"])
    assert abs(dev["rb"] - (ref.rb_true + 1e-6)) < 1e-12, label
    total, undecided, share = R.check_table(ref, dev, W=W, mean=mean, label=label)
    host, W_host, _ = probe(case, dev["displacement"], bin_target)
    same = np.array_equal(dev["off"], host["off"]) and np.array_equal(dev["list"], host["list"])
    assert same, "%s: device and host tables differ: %s" % (label, _differences(case, ref, dev, host))
    assert W_host == W and host["rb"] == dev["rb"], label
    print("%s: grid %s, displacement %.6f, %d pairs, %d undecided (%.4f %%)" % (label, dev["grid"], dev["displacement"], total,
                                                                             undecided, 100 * share))


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_device_tables_against_reference_and_host_table(probe, name):
    """The loose table after set_basis and the tight table after one fill of 32 slightly jittered frames: each passes
    the reference's checker (complete, not padded beyond the code's pads, well formed, critical vertices), equals the
    host probe's table for the displacement the DEVICE reports, and agrees with sit_info's W, mean and grid."""
    case = P.cases()[name]
    ctx = _context(case)
    with pytest.raises(ValueError, match="no tight table"):
        ctx.candidate_table(1)
    info = ctx.info()
    loose = ctx.candidate_table(0)
    assert loose["displacement"] == P.STATIC_THR
    _check_device_table(case, probe, loose, info["row_width"], info["mean_candidates_loose"], info["grid_loose"], 1.0, name + "/loose")
    rng = np.random.default_rng(17)
    frames = np.empty((32, case.S + 1, 3))
    frames[:, :-1] = case.ref_static + rng.normal(scale=0.01, size=(32, case.S, 3))
    frames[:, -1] = case.centers[0] + rng.normal(scale=0.05, size=(32, 3))
    ctx.set_frames(frames, np.arange(case.S), np.array([case.S]))
    rc, nz, err = ctx.fill(check_for_zeros=False)
    info = ctx.info()
    assert rc == 0 and info["fill_kernel"] == 3
    tight = ctx.candidate_table(1)
    assert 0.02 < tight["displacement"] < 0.2 and tight["displacement"] == info["delta"]
    _check_device_table(case, probe, tight, info["tight_width"], info["mean_candidates_tight"], info["grid_tight"], 0.5, name + "/tight")
    again = ctx.candidate_table(0)                                  # the loose table is still the loose table
    assert np.array_equal(again["off"], loose["off"]) and np.array_equal(again["list"], loose["list"])
    ctx.close()


def test_a_second_basis_replaces_the_tables(probe):
    """set_basis with another basis on the same context: the loose table is that basis's, the tight table of the first
    is no longer handed out."""
    first = P.cases()["ortho_c1d"]
    second = P.Case("ortho_c1d_reversed", first.cell, first.ref_static[::-1], first.centers[::-1][:5],
                    [[first.S - 1 - s for s in v] for v in first.vertices[::-1][:5]])
    ctx = _context(first)
    frames = np.concatenate([first.ref_static, first.centers[:1]])[None].repeat(4, axis=0)
    ctx.set_frames(frames, np.arange(first.S), np.array([first.S]))
    assert ctx.fill(check_for_zeros=False)[0] == 0
    assert ctx.candidate_table(1)["total"] > 0
    ctx.set_basis(second.ref_static, second.verts, second.vcd, P.MIDPOINT, P.STEEPNESS, P.STATIC_THR)
    with pytest.raises(ValueError, match="no tight table"):
        ctx.candidate_table(1)
    info = ctx.info()
    dev = ctx.candidate_table(0)
    assert dev["list"].max() == 4
    _check_device_table(second, probe, dev, info["row_width"], info["mean_candidates_loose"], info["grid_loose"], 1.0, "second basis")
    ctx.close()


def _fill_rows(case, frames, monkeypatch, general_kernel=False):
    if general_kernel:
        monkeypatch.setenv("SITATOR_FILL_KERNEL", "1")
    else:
        monkeypatch.delenv("SITATOR_FILL_KERNEL", raising=False)
    ctx = _context(case)
    ctx.set_frames(frames, np.arange(case.S), np.array([case.S]))
    rc, nz, err = ctx.fill(check_for_zeros=False)
    assert rc == 0, (rc, err.frame, err.index)
    return ctx, ctx.rows_dense(), nz


@pytest.mark.parametrize("name", P.EDGE_CELLS)
def test_rows_where_the_bound_has_nothing_to_spare(oracle, monkeypatch, name):
    """Frames of P.edge_frames - the ion on a corner of the loose grid (and its ulp neighbours: every bin that meets
    there), the vertex atoms of a landmark displaced by (1 - 1e-6) static_thr towards it - through the general kernel,
    the default kernel, and the default kernel with the frames interleaved among undisplaced ones, so that the sampled
    delta is small and every displaced frame takes the fallback (loose) table.  Zero pattern entry for entry, values
    within 1e-6 relative, the same number of all-zero rows.  (The displaced frames sit on the odd positions of 4096
    frames: sample_static_dmax (fill.hip) takes delta from frames 0, stride, 2 stride, ... with stride = F / 2048 - every
    second frame of a trajectory of that length - so a LEADING undisplaced block would have to be a thousand times
    longer to keep them out of the sample.)"""
    case = P.cases()[name]
    frames, exp, nz_exp = P.edge_frames(name)
    near, far = P.edge_reach(name, frames, exp)
    assert near >= 20 and far >= 20, (near, far)

    def compare(got, nz, want, nz_want, what):
        assert np.array_equal(got != 0, want != 0), "%s: zero pattern differs from the oracle's at %s" % (
            what, np.argwhere((got != 0) != (want != 0))[:5].tolist())
        assert nz == nz_want, what
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=what)

    ctx, got, nz = _fill_rows(case, frames, monkeypatch, general_kernel=True)
    assert ctx.info()["fill_kernel"] == 1
    compare(got, nz, exp, nz_exp, "general kernel")
    ctx.close()
    ctx, got, nz = _fill_rows(case, frames, monkeypatch)
    info = ctx.info()
    assert info["fill_kernel"] == 3 and info["fallback_frames"] == 0 and info["delta"] == P.STATIC_THR
    compare(got, nz, exp, nz_exp, "default kernel, tight table for the full displacement")
    ctx.close()
    n = len(frames)
    assert n <= 2048
    calm = np.concatenate([case.ref_static, case.centers[:1]])
    mixed = np.repeat(calm[None], 4096, axis=0)
    mixed[1:2 * n:2] = frames
    S = case.S
    calm_row, calm_nz = oracle.fill(case.cell, oracle.wrap_points(case.cell, calm[None]), np.arange(S), np.array([S]),
                                    case.ref_static, case.verts, case.vcd, P.MIDPOINT, P.STEEPNESS, P.STATIC_THR, check_for_zeros=False)
    want = np.repeat(calm_row, 4096, axis=0)
    want[1:2 * n:2] = exp
    ctx, got, nz = _fill_rows(case, mixed, monkeypatch)
    info = ctx.info()
    assert info["fill_kernel"] == 3 and info["delta"] < 0.05
    assert info["fallback_frames"] == n, (info["fallback_frames"], n)
    compare(got, nz, want, nz_exp + calm_nz * (4096 - n), "fallback table")
    ctx.close()


def test_a_landmark_without_vertices_is_one_for_every_ion(oracle, monkeypatch):
    """sit_set_basis and the oracle both accept a landmark with no vertex at all; the oracle's component for it is 1.0
    wherever the ion is (an empty product, then its root).  Rows of the ragged basis with such a landmark, ions spread
    over the cell, static atoms jittered: the general and the default kernel give the oracle's zero pattern and values,
    and exactly 1.0 in that landmark's column."""
    case = P.cases()["ragged_with_empty"]
    k = case.D - 1
    assert case.vertices[k] == []
    rng = np.random.default_rng(23)
    F, S = 96, case.S
    frames = np.empty((F, S + 1, 3))
    frames[:, :-1] = case.ref_static + rng.normal(scale=0.02, size=(F, S, 3))
    frames[:, -1] = (rng.random((F, 3)) * 3.0 - 1.0) @ case.cell              # unwrapped: in and around the cell
    exp, nz_exp = oracle.fill(case.cell, oracle.wrap_points(case.cell, frames), np.arange(S), np.array([S]), case.ref_static,
                              case.verts, case.vcd, P.MIDPOINT, P.STEEPNESS, P.STATIC_THR, check_for_zeros=False)
    assert (exp[:, k] == 1.0).all() and nz_exp == 0
    assert ((exp[:, :k] != 0).sum(axis=1) > 0).sum() > F // 4, "the other landmarks must be seen too"
    for general in (True, False):
        ctx, got, nz = _fill_rows(case, frames, monkeypatch, general_kernel=general)
        assert ctx.info()["fill_kernel"] == (1 if general else 3)
        assert np.array_equal(got != 0, exp != 0), general
        assert (got[:, k] == 1.0).all(), general
        assert nz == nz_exp
        np.testing.assert_allclose(got, exp, rtol=1e-6, atol=0)
        ctx.close()
