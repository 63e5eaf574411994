"""The second stage of the analysis on designed inputs: the exact reductions of the mcl plugin (cluster.hip: k_gram,
k_gram_runs, k_gram_fold, k_gram_mirror, k_weighted_row_sums(_runs), k_limbs_to_double), its best-match kernels
(k_best_match, k_best_match_groups and their row kernels) and the site centres (sites.hip: k_site_wmax / k_site_first
with and without LDS, k_site_anchor_pts, k_site_sums, k_site_sums_final).

Every device input is a designed array pushed through the C-ABI (set_rows_dense, then set_assignments; designed ion
positions in set_frames).  The exact accumulators are compared limb for limb with an independent integer model
(tests/reduction_ref.py), their doubles with the correctly rounded quotient, the arg-max kernels with numpy's argmax on
data where every sum is exact, the site sums with a long-double sum under the forward error bound of a sum.  The tests
without a mark check the references and the generators themselves, and the numpy stand-in of tests/fake_ctx.py that
the gloo tests rest on."""
import functools
import os
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

from tests import reduction_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(range(len(R.REDUCTION_CASES)))
FOLD_ROWS, FOLD_D = 32768, 48          # gram_impl halves its 8 accumulator copies while N < 4096 * copies
WIDE_D, WIDE_ROWS = 3100, 2500         # k_gram<false>: D * 20 bytes of LDS no longer fit 60 KiB (D > 3072)


@functools.lru_cache(maxsize=None)
def _case(i):
    F, M, D, K, values = R.REDUCTION_CASES[i]
    return R.make_reduction_case(F, M, D, K, values, seed=100 + i) + (K,)


@functools.lru_cache(maxsize=None)
def _gram_ref(i):
    return R.gram_reference(_case(i)[0])


@functools.lru_cache(maxsize=None)
def _sums_ref(i, weighted):
    X, lab, confs, K = _case(i)
    return R.row_sums_reference(X, lab, confs, K, weighted)


@functools.lru_cache(maxsize=None)
def _fold_case():
    X = R.make_narrow_rows(FOLD_ROWS, FOLD_D, seed=7)
    return X, R.gram_reference(X)


def _old_exact_value(hi, lo):
    """exact_value / exact_sum_across before negative accumulators were converted by their magnitude."""
    return np.ldexp(hi.view(np.int64).astype(np.float64), -16) + np.ldexp(lo.astype(np.float64), -80)


# ---- the references and the generators (CPU) ------------------------------------------------------------------------------

def test_integer_model_equals_rational_arithmetic_and_numpy():
    rng = np.random.default_rng(0)
    p = np.concatenate([rng.uniform(-1, 1, 150), np.ldexp(rng.uniform(-1, 1, 150), rng.integers(-100, 40, 150)),
                        [0.0, -0.0, np.nan, 2.0 ** -80, -2.0 ** -80, 2.0 ** -81, -2.0 ** -81, 1.0, -1.0, 2.0 ** 46,
                         -2.0 ** -70, 2.0 ** -27 * (1 + 2.0 ** -52), -(2.0 ** -28) * (1 + 2.0 ** -52)]])
    acc = rng.integers(0, 7, len(p))
    acc[-3] = 8                                              # -2^-70 alone: the example of a cancelled negative sum
    hi, lo = R.exact_limbs(acc, p, 10)
    for a in range(10):
        want = sum(R.fix_fraction(x) for x in p[acc == a]) & ((1 << 128) - 1)
        assert (int(hi[a]) << 64) | int(lo[a]) == want, a
    assert hi[9] == 0 and lo[9] == 0
    assert hi[8] == 2 ** 64 - 1 and lo[8] == 2 ** 64 - 2 ** 10
    assert R.rounded_values(hi[8:9], lo[8:9])[0] == -2.0 ** -70
    X, _, _, _ = _case(4)                                    # uniform in (0, 1]: X^T X is well conditioned
    ghi, glo, seen = _gram_ref(4)
    np.testing.assert_allclose(R.rounded_values(ghi, glo), X.T @ X, rtol=1e-13, atol=0)
    assert np.array_equal(ghi, ghi.T) and np.array_equal(glo, glo.T)
    shi, slo = _sums_ref(4, True)
    _, lab, confs, K = _case(4)
    D = X.shape[1]
    want = np.zeros((K, D))
    for k in range(K):
        m = lab.reshape(-1) == k
        want[k] = (confs.reshape(-1)[m][:, None] * X[m]).sum(axis=0)
    np.testing.assert_allclose(R.rounded_values(shi, slo)[:K * D].reshape(K, D), want, rtol=1e-12, atol=0)


def test_reference_terms_stay_within_a_few_million():
    total = sum(R.gram_term_count(_case(i)[0]) for i in CASES) + R.gram_term_count(_fold_case()[0])
    total += R.gram_term_count(_wide_case()[0])
    assert total < 5e6, total


@pytest.mark.parametrize("i", CASES)
def test_generated_reduction_arrays_hold_every_feature(i):
    F, M, D, K, values = R.REDUCTION_CASES[i]
    X, lab, confs, _ = _case(i)
    assert X.shape == (F * M, D) and lab.shape == confs.shape == (F, M)
    missing = R.expected_reduction_features(F, M, values) - R.reduction_features(X, lab, confs, K)
    assert not missing, missing


def test_reduction_cases_cover_the_shapes_and_all_features():
    assert {c[0] for c in R.REDUCTION_CASES} == {2, 63, 64, 65, 129, 1000}
    assert {c[1] for c in R.REDUCTION_CASES} == {1, 3, 64, 300}
    held = set()
    for i in CASES:
        X, lab, confs, K = _case(i)
        held |= R.reduction_features(X, lab, confs, K)
    every = set()
    for F, M, D, K, values in R.REDUCTION_CASES:
        every |= R.expected_reduction_features(1000, 300, values)
    assert every <= held, every - held
    X, _ = _fold_case()
    assert len(X) >= 4096 * 8 and np.count_nonzero(X, axis=1).max() <= 3
    assert _wide_case()[0].shape[1] * 20 > 60 * 1024


def test_negative_sums_keep_their_digits_on_the_host():
    """sharding.exact_sum_across rounds what the library's exact_value rounds: a small negative sum (hi = -1, lo just below
    2^64) used to cancel to 0; accumulators with hi >= 0 keep their bits."""
    from sitator_amd import sharding
    hi, lo = np.array([2 ** 64 - 1], dtype=np.uint64), np.array([2 ** 64 - 2 ** 10], dtype=np.uint64)
    assert sharding.exact_sum_across(None, hi, lo)[0] == -2.0 ** -70
    worst, n_small = 0.0, 0
    for i in CASES:
        if R.REDUCTION_CASES[i][4] != "signed":
            continue
        for h, l in (_gram_ref(i)[:2], _sums_ref(i, True)):
            got = sharding.exact_sum_across(None, h, l)
            ref = R.rounded_values(h, l)
            worst = max(worst, R.ulp_distance(got, ref))
            n_small += int(np.sum((ref < 0) & (ref > -2.0 ** -16)))
            pos = h.view(np.int64) >= 0
            assert np.array_equal(got[pos], _old_exact_value(h, l)[pos])
    assert n_small > 100, "the signed cases must hold small negative sums"
    assert worst <= 1.0, worst


# ---- the exact reductions on the device -----------------------------------------------------------------------------------

def _rows_ctx(X, lab=None, confs=None):
    """Rows first (sit_set_rows_dense clears the assignments), then the labels, which give the context its M."""
    from sitator_amd import _lib
    c = _lib.HipContext(np.eye(3) * 10.0)
    c.set_rows_dense(np.ascontiguousarray(X))
    if lab is not None:
        assert lab.size == len(X)
        c.set_assignments(np.ascontiguousarray(lab), np.ascontiguousarray(confs))
    return c


def _set_runs(monkeypatch, runs):
    if runs is None:
        monkeypatch.delenv("SITATOR_RUNS", raising=False)
    else:
        monkeypatch.setenv("SITATOR_RUNS", runs)


@pytest.mark.gpu
@pytest.mark.parametrize("runs", [None, "0"])
@pytest.mark.parametrize("i", CASES)
def test_gram_limbs_equal_the_integer_model(i, runs, monkeypatch):
    """The whole D x D array, lower triangle included; accumulators no row touches are zero in the model and must be on
    the device.  SITATOR_RUNS unset: k_gram_runs (the labels gave the context its M); 0: k_gram."""
    X, lab, confs, K = _case(i)
    _set_runs(monkeypatch, runs)
    hi, lo, seen = _rows_ctx(X, lab, confs).gram_limbs()
    rhi, rlo, rseen = _gram_ref(i)
    assert np.array_equal(seen, rseen)
    assert np.array_equal(hi, rhi), np.argwhere(hi != rhi)[:5]
    assert np.array_equal(lo, rlo), np.argwhere(lo != rlo)[:5]


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("runs", [None, "0"])
@pytest.mark.parametrize("i", CASES)
def test_weighted_row_sums_limbs_equal_the_integer_model(i, runs, weighted, monkeypatch):
    X, lab, confs, K = _case(i)
    _set_runs(monkeypatch, runs)
    hi, lo = _rows_ctx(X, lab, confs).weighted_row_sums_limbs(K, weighted=weighted)
    rhi, rlo = _sums_ref(i, weighted)
    assert np.array_equal(hi, rhi), np.nonzero(hi != rhi)[0][:5]
    assert np.array_equal(lo, rlo), np.nonzero(lo != rlo)[0][:5]


@pytest.mark.gpu
@pytest.mark.parametrize("i", CASES)
def test_double_results_are_the_rounded_integers(i, monkeypatch):
    """gram() and weighted_row_sums() within 1 ulp of the correctly rounded exact integer / 2^80: exact_value rounds the
    low word and the sum, each by at most half an ulp of the result.  The signed cases hold sums in (-2^-16, 0), which
    exact_value used to cancel to (nearly) nothing.  Measured on an MI355X: 0 ulp in all eight cases."""
    X, lab, confs, K = _case(i)
    D = X.shape[1]
    _set_runs(monkeypatch, None)
    c = _rows_ctx(X, lab, confs)
    G, seen = c.gram()
    ghi, glo, _ = _gram_ref(i)
    d_gram = R.ulp_distance(G, R.rounded_values(ghi, glo))
    sums, wsum = c.weighted_row_sums(K)
    ref = R.rounded_values(*_sums_ref(i, True))
    d_sums = R.ulp_distance(np.concatenate([sums.reshape(-1), wsum]), ref)
    print("case %d: gram %.3g ulp, row sums %.3g ulp" % (i, d_gram, d_sums))
    assert d_gram <= 1.0 and d_sums <= 1.0, (d_gram, d_sums)
    pos = ghi.view(np.int64) >= 0
    assert np.array_equal(G[pos], _old_exact_value(ghi, glo)[pos]), "the bits of non-negative sums must not change"


@pytest.mark.gpu
def test_gram_with_eight_accumulator_copies_folds_to_the_same_integers(monkeypatch):
    """32768 rows and SITATOR_RUNS=0: k_gram adds into 8 copies of the accumulators and k_gram_fold sums them with the
    carries of the low words (uniform values: the low words are dense, most sums carry)."""
    X, (rhi, rlo, rseen) = _fold_case()
    _set_runs(monkeypatch, "0")
    hi, lo, seen = _rows_ctx(X).gram_limbs()
    assert np.array_equal(seen, rseen) and np.array_equal(hi, rhi) and np.array_equal(lo, rlo)


def _child_gram(path):
    X, _ = _fold_case()
    hi, lo, seen = _rows_ctx(X).gram_limbs()
    np.savez(path, hi=hi, lo=lo, seen=seen)


@pytest.mark.gpu
@pytest.mark.parametrize("copies", [None, "1", "3"])
def test_gram_copies_setting_in_a_fresh_process(copies):
    """SITATOR_GRAM_COPIES is read once per process: each setting gets a process of its own.  One copy (no fold), the
    default, and a number of copies that is not a power of two give the same integers."""
    env = dict(os.environ, SITATOR_RUNS="0")
    env.pop("SITATOR_GRAM_COPIES", None)
    if copies is not None:
        env["SITATOR_GRAM_COPIES"] = copies
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "gram.npz")
        code = "import sys; sys.path.insert(0, %r); from tests.test_gpu_reductions import _child_gram; _child_gram(%r)" % (ROOT, path)
        subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, check=True, timeout=600)
        got = dict(np.load(path))
    _, (rhi, rlo, rseen) = _fold_case()
    assert np.array_equal(got["seen"], rseen) and np.array_equal(got["hi"], rhi) and np.array_equal(got["lo"], rlo)


@functools.lru_cache(maxsize=None)
def _wide_case():
    rng = np.random.default_rng(3)
    X = np.zeros((WIDE_ROWS, WIDE_D))
    for r in range(WIDE_ROWS):
        w = int(rng.choice([0, 1, 2, 5, 13]))
        X[r, rng.choice(WIDE_D, size=w, replace=False)] = rng.uniform(-1, 1, size=w)
    X[:40, WIDE_D - 1] = 0.5                                    # the last landmark, and its last accumulator
    return X, R.gram_reference(X)


@pytest.mark.gpu
def test_gram_beyond_the_lds_table_of_hit_counts(monkeypatch):
    """D = 3100 > 3072 and SITATOR_RUNS=0: k_gram<false> counts the hits and adds the diagonal with global atomics."""
    X, (rhi, rlo, rseen) = _wide_case()
    _set_runs(monkeypatch, "0")
    hi, lo, seen = _rows_ctx(X).gram_limbs()
    assert np.array_equal(seen, rseen) and np.array_equal(hi, rhi) and np.array_equal(lo, rlo)


@pytest.mark.gpu
@pytest.mark.parametrize("i,split", [(4, 50), (7, 33), (6, 501)])
def test_two_shards_add_up_to_the_whole(i, split, monkeypatch):
    """Rows split at a frame that is no multiple of 64; the limbs added as integers equal the model of the whole, and
    sharding.exact_sum_across between two ranks gives the rounded value of the whole."""
    from sitator_amd import sharding
    X, lab, confs, K = _case(i)
    F, M = lab.shape
    _set_runs(monkeypatch, None)
    parts = [_rows_ctx(X[:split * M], lab[:split], confs[:split]), _rows_ctx(X[split * M:], lab[split:], confs[split:])]
    g = [c.gram_limbs() for c in parts]
    s = [c.weighted_row_sums_limbs(K) for c in parts]
    rhi, rlo, rseen = _gram_ref(i)
    shi, slo = _sums_ref(i, True)
    hi, lo = R.add_limbs([p[:2] for p in g])
    assert np.array_equal(hi, rhi) and np.array_equal(lo, rlo) and np.array_equal(g[0][2] + g[1][2], rseen)
    hi, lo = R.add_limbs(s)
    assert np.array_equal(hi, shi) and np.array_equal(lo, slo)
    comms = sharding.ThreadComm.group(2)
    out = [None, None]

    def rank(r):
        out[r] = (sharding.exact_sum_across(comms[r], g[r][0], g[r][1]), sharding.exact_sum_across(comms[r], s[r][0], s[r][1]))

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    [t.start() for t in threads]
    [t.join(60) for t in threads]
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert R.ulp_distance(out[0][0], R.rounded_values(rhi, rlo)) <= 1.0
    assert R.ulp_distance(out[0][1], R.rounded_values(shi, slo)) <= 1.0
    whole = _rows_ctx(X, lab, confs)
    assert np.array_equal(out[0][0], whole.gram()[0])
    sums, wsum = whole.weighted_row_sums(K)
    assert np.array_equal(out[0][1], np.concatenate([sums.reshape(-1), wsum]))


# ---- best match -----------------------------------------------------------------------------------------------------------

MATCH_D, FREE = 64, 4
MATCH_N = [1, 255, 256, 257, 70001]


@functools.lru_cache(maxsize=None)
def _match_rows(N):
    return R.make_match_rows(N, MATCH_D, seed=N, free_dims=FREE)


def _partition(seed=0):
    """6 groups over 64 dimensions: 0..3 share the dimensions 0..55, 56..59 belong to no group, group 4 owns 60 and 61
    (no generated row has them), group 5 owns 62 and 63."""
    grp = np.random.default_rng(seed).integers(0, 4, size=MATCH_D).astype(np.int32)
    grp[56:60] = -1
    grp[60:62] = 4
    grp[62:64] = 5
    return grp, 6


def _planted(N):
    """[(name, X, a, b)]: the champion row planted at the rows a < b, per tie the shape has room for (first: no tie)."""
    X, c = _match_rows(N)
    champ = R.champion_row(c, np.arange(MATCH_D - FREE))
    out = [("none", X, None, None)]
    for name, a, b in R.tie_pairs(N):
        Xt = X.copy()
        Xt[a] = champ
        Xt[b] = champ
        out.append((name, Xt, a, b))
    return out


@pytest.mark.parametrize("N", MATCH_N)
def test_planted_ties_are_first_maxima(N):
    X, c = _match_rows(N)
    assert np.all(X * 1024 == np.round(X * 1024)) and np.abs(X).max() < 1 and np.count_nonzero(X, axis=1).max() <= 24
    assert N < 9 or np.any(~X.any(axis=1)), "rows with no non-zero"
    assert not X[:, MATCH_D - FREE:].any()
    names = [p[0] for p in _planted(N)]
    if N == 70001:
        assert names == ["none", "same_wave", "two_waves_of_a_block", "rows_255_256", "first_and_last_block", "row_0_and_row_N-1"]
    for name, Xt, first, _ in _planted(N)[1:]:
        proj = np.abs(Xt @ c)
        top = np.nonzero(proj == proj.max())[0]
        assert len(top) == 2 and top[0] == first, name
        assert R.sparse_products_argmax(Xt, c)[0] == first == int(np.argmax(proj))
        if name == "same_wave":
            assert top[0] // 64 == top[1] // 64
        if name == "two_waves_of_a_block":
            assert top[0] // 64 != top[1] // 64 and top[0] // 256 == top[1] // 256
        if name == "first_and_last_block":
            assert top[0] // 256 == 0 and top[1] // 256 == (N - 1) // 256 > 0


def _same_match(got, want, what):
    row, dot, nrm = got
    wrow, wdot, wx2 = want
    assert row == wrow, (what, row, wrow)
    assert dot == wdot or (np.isnan(dot) and np.isnan(wdot)), (what, dot, wdot)
    assert nrm == np.sqrt(wx2), (what, nrm, np.sqrt(wx2))


@pytest.mark.gpu
@pytest.mark.parametrize("N", MATCH_N)
def test_best_match_is_numpys_first_maximum(N):
    """Dyadic rows and centre: every sum is exact in any order, so the row, |dot| and the norm are numpy's, identically."""
    from sitator_amd import _lib
    _, c = _match_rows(N)
    ctx = _lib.HipContext(np.eye(3) * 10.0)
    for name, Xt, a, b in _planted(N):
        ctx.set_rows_dense(Xt)
        want = R.sparse_products_argmax(Xt, c)
        assert a is None or want[0] == a
        _same_match(ctx.best_match(c), want, name)
        # the NaN-first rule: rows a < b hold the dimension where the centre is NaN; the champion (finite, larger than
        # anything) sits before, between and after them
        if a is not None:
            Xn = _match_rows(N)[0].copy()
            cn = c.copy()
            cn[MATCH_D - 1] = np.nan
            Xn[a, MATCH_D - 1] = 0.25
            Xn[b, MATCH_D - 1] = 0.5
            champ = R.champion_row(c, np.arange(MATCH_D - FREE))
            for r in (a - 1, b + 1, (a + b) // 2):
                if 0 <= r < N and r not in (a, b):
                    Xn[r] = champ
            ctx.set_rows_dense(Xn)
            want = R.sparse_products_argmax(Xn, cn)
            assert want[0] == a and np.isnan(want[1])
            _same_match(ctx.best_match(cn), want, name + "/nan")


def _group_reference(X, grp, c, G):
    return [R.sparse_products_argmax(X, np.where(grp == g, c, 0.0)) for g in range(G)]


def _same_groups(got, want, what):
    rows, dots, nrms = got
    for g, w in enumerate(want):
        _same_match((rows[g], dots[g], nrms[g]), w, "%s group %d" % (what, g))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 257, 70001])
def test_best_match_groups_are_numpys_first_maxima(N):
    """Six groups (one no row overlaps: numpy's argmax of zeros is row 0; one whose only row is the last; dimensions of
    no group), one group, and a group per dimension; ties planted in group 0; a NaN of the centre in one group."""
    from sitator_amd import _lib
    _, c = _match_rows(N)
    grp, G = _partition()
    ctx = _lib.HipContext(np.eye(3) * 10.0)
    champ0 = R.champion_row(c, np.nonzero(grp[:MATCH_D - FREE] == 0)[0])
    for name, Xt, first, second in _planted(N):
        Xt = Xt.copy()
        twice = (first, second)
        if first is not None:
            Xt[list(twice)] = champ0
        Xt[N - 1, 62] = 0.5                                           # group 5: the last row only
        ctx.set_rows_dense(Xt)
        want = _group_reference(Xt, grp, c, G)
        assert first is None or want[0][0] == first
        assert want[4][:2] == (0, 0.0) and want[5][0] == N - 1
        _same_groups(ctx.best_match_groups(grp, c, G), want, name)
        one = np.zeros(MATCH_D, dtype=np.int32)
        _same_groups(ctx.best_match_groups(one, c, 1), _group_reference(Xt, one, c, 1), name + "/G=1")
        if first is not None:
            cn = c.copy()
            cn[60] = np.nan                                           # group 4 only
            Xn = Xt.copy()
            Xn[twice[0], 60] = 0.25
            Xn[twice[1], 61] = 0.5
            Xn[twice[1], 60] = 0.5
            ctx.set_rows_dense(Xn)
            want = _group_reference(Xn, grp, cn, G)
            assert want[4][0] == twice[0] and np.isnan(want[4][1]) and not any(np.isnan(w[1]) for w in want[:4])
            _same_groups(ctx.best_match_groups(grp, cn, G), want, name + "/nan")
    if N <= 257:
        each = np.arange(MATCH_D, dtype=np.int32)
        X = _planted(N)[-1][1]
        ctx.set_rows_dense(X)
        _same_groups(ctx.best_match_groups(each, c, MATCH_D), _group_reference(X, each, c, MATCH_D), "G=D")


@pytest.mark.gpu
def test_best_match_on_random_rows_within_the_dot_product_bound():
    """Not dyadic: the returned |dot| is within (nnz + 1) 2^-53 sum|v c| of the long-double one (the forward bound of a
    dot product of nnz terms), and no row's long-double |dot| beats the winner's by more than the two rows' bounds."""
    from sitator_amd import _lib
    rng = np.random.default_rng(11)
    N, D = 70001, MATCH_D
    X, _ = _match_rows(N)
    X = np.where(X != 0, rng.uniform(-1, 1, size=X.shape), 0.0)
    c = rng.normal(size=D)
    ctx = _lib.HipContext(np.eye(3) * 10.0)
    ctx.set_rows_dense(X)
    Xl, cl = X.astype(np.longdouble), c.astype(np.longdouble)
    u = np.longdouble(2.0 ** -53)
    grp, G = _partition(1)
    rows, dots, _ = ctx.best_match_groups(grp, c, G)
    row, dot, _ = ctx.best_match(c)
    for what, cg, r, d in [("all", cl, row, dot)] + [(g, np.where(grp == g, cl, 0), rows[g], dots[g]) for g in range(G)]:
        prod = Xl * cg[None, :]
        ld = np.abs(prod.sum(axis=1))
        bound = (np.count_nonzero(prod, axis=1) + 1) * u * np.abs(prod).sum(axis=1)
        print(what, "row", r, "|dot| error", float(abs(ld[r] - d)), "bound", float(bound[r]))
        assert abs(ld[r] - d) <= bound[r], what
        assert np.all(ld - ld[r] <= bound + bound[r]), what


@pytest.mark.gpu
@pytest.mark.parametrize("runs", [None, "0"])
@pytest.mark.parametrize("D", [5, 7])
def test_reductions_and_matches_at_an_odd_landmark_dimension(D, runs, monkeypatch):
    """F = 5, M = 3, K = 3, G = 3 and an odd D: every table of gram, weighted_row_sums, best_match and best_match_groups
    ends off a 16-byte boundary in the scratch buffer.  Dyadic values, so the integer model, its rounded doubles and
    numpy's argmax are the references, as above."""
    F, M, K, G = 5, 3, 3, 3
    rng = np.random.default_rng(900 + D)
    X = np.where(rng.random((F * M, D)) < 0.6, rng.integers(1, 512, size=(F * M, D)) * rng.choice([-1.0, 1.0], size=(F * M, D)), 0.0) / 1024.0
    lab = rng.integers(-1, K, size=(F, M))
    confs = rng.integers(0, 65, size=(F, M)) / 64.0
    cvec = rng.integers(1, 512, size=D) * rng.choice([-1.0, 1.0], size=D) / 1024.0
    grp = (np.arange(D) % G).astype(np.int32)
    _set_runs(monkeypatch, runs)
    c = _rows_ctx(X, lab, confs)
    ghi, glo, gseen = R.gram_reference(X)
    hi, lo, seen = c.gram_limbs()
    assert np.array_equal(seen, gseen) and np.array_equal(hi, ghi) and np.array_equal(lo, glo)
    Gm, seen = c.gram()
    assert np.array_equal(seen, gseen) and R.ulp_distance(Gm, R.rounded_values(ghi, glo)) <= 1.0
    for weighted in (True, False):
        rhi, rlo = R.row_sums_reference(X, lab, confs, K, weighted)
        hi, lo = c.weighted_row_sums_limbs(K, weighted=weighted)
        assert np.array_equal(hi, rhi) and np.array_equal(lo, rlo), weighted
        sums, wsum = c.weighted_row_sums(K, weighted=weighted)
        assert R.ulp_distance(np.concatenate([sums.reshape(-1), wsum]), R.rounded_values(rhi, rlo)) <= 1.0, weighted
    _same_match(c.best_match(cvec), R.sparse_products_argmax(X, cvec), "D=%d" % D)
    _same_groups(c.best_match_groups(grp, cvec, G), _group_reference(X, grp, cvec, G), "D=%d" % D)


# ---- site anchors and sums ------------------------------------------------------------------------------------------------

# (host, M, F, K): N in {1, 255, 16384, 16385, 3 * 16384 + 5, 4095, 4097}, K in {1, 480, 8192, 8193, 4266}; an orthorhombic,
# a triclinic and a hexagonal cell
SITE_CASES = [("C1", 1, 1, 1), ("C1b", 3, 85, 480), ("C2", 64, 256, 480), ("C1b", 1, 16385, 8192), ("C1", 1, 49157, 8193),
              ("C1b", 63, 65, 300), ("C2h", 17, 241, 40), ("C2", 64, 300, 4266),
              ("C1b", 3, 5, 3), ("C1", 3, 5, 5)]         # the last two: every table of the two calls ends off a 16-byte boundary
SITE_K_LIMIT = 4266                         # sit_site_sums: K * 36 bytes of LDS within 150 KiB


def _cell(cfg):
    from sitator_amd import synth
    return np.asarray(synth.config_host(cfg).cell, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _site_case(n):
    from oracle import oracle as orc
    cfg, M, F, K = SITE_CASES[n]
    return R.make_site_case(orc, _cell(cfg), F, M, K, seed=40 + n)


def test_site_cases_cover_the_shapes_and_keep_away_from_the_faces(oracle):
    assert {c[1] * c[2] for c in SITE_CASES} >= {1, 255, 16384, 16385, 3 * 16384 + 5, 4095, 4097}
    assert {c[3] for c in SITE_CASES} >= {1, 480, 8192, 8193, SITE_K_LIMIT}
    cells = [_cell(cfg) for cfg in ("C2", "C1b", "C1")]
    assert np.count_nonzero(cells[0] - np.diag(np.diag(cells[0]))) == 0          # orthorhombic
    assert np.count_nonzero(cells[1] - np.diag(np.diag(cells[1]))) >= 3          # triclinic
    assert np.count_nonzero(cells[2] - np.diag(np.diag(cells[2]))) >= 1          # hexagonal
    held = set()
    for n, (cfg, M, F, K) in enumerate(SITE_CASES):
        pos, lab, confs = _site_case(n)
        cell = _cell(cfg)
        for weighted in (True, False):
            assert R.face_margin(oracle, cell, pos, lab, confs, K, weighted) >= 1e-6, (n, weighted)
        held |= R.site_features(lab, confs, K)
        if F * M > 1000 and K < 1000:
            # members on both sides of a periodic face
            u = pos.reshape(-1, 3) @ np.linalg.inv(cell)
            assert np.any(np.floor(u) != 0), n
    assert held >= {"site_without_rows", "maximal_weight_twice_in_one_block", "maximal_weight_first_in_two_blocks",
                    "label_-1", "label_beyond_K", "chunk_of_256_rows_on_one_site"}, held


def _site_ctx(cfg, M, pos, lab, confs, frame0=0):
    from sitator_amd import synth
    from tests.test_gpu_kernels import _setup
    ctx, _, sm, mm, ref = _setup(synth.config_host(cfg), M, 2, seed=5)
    frames = np.empty((len(pos), len(ref), 3))
    frames[:] = ref[None]
    frames[:, np.where(mm)[0]] = pos
    ctx.set_frames(frames, np.where(sm)[0], np.where(mm)[0], frame0)
    ctx.set_assignments(np.ascontiguousarray(lab), np.ascontiguousarray(confs), frame0)
    return ctx


def _same_anchors(got, want, what):
    for g, w, name in zip(got, want, ("wmax", "first_row", "anchor")):
        assert np.array_equal(g, w, equal_nan=True), (what, name, np.argwhere(~((g == w) | ((g != g) & (w != w))))[:5])


def _check_sums(oracle, cell, ctx, pos, lab, confs, K, weighted, anchors, sums, what):
    ref, tol = R.sums_reference(oracle, cell, pos, lab, confs, K, weighted, anchors)
    err = np.abs(sums.astype(np.longdouble) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(what, "largest error / tolerance", float(np.nanmax(np.where(tol > 0, err / tol, 0))))
    assert np.all(err <= tol), (what, np.argwhere(err > tol)[:5])
    # the centre landmark._site_centers makes of the sums, against PBCCalculator.average per site
    centers = R.centres_from_sums(oracle, cell, ctx.cell_centroid, sums, anchors)
    pw = oracle.wrap_points(cell, pos.reshape(-1, 3))
    order, start = R.sorted_sites(lab, K)
    w = confs.reshape(-1)
    for k in range(K):
        rows = order[start[k]:start[k + 1]]
        if len(rows) and (not weighted or w[rows].sum() > 0):
            exp = oracle.average(cell, pw[rows], w[rows] if weighted else None)
            np.testing.assert_allclose(centers[k], exp, rtol=1e-6, atol=1e-9, err_msg="%s site %d" % (what, k))


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(len(SITE_CASES)))
def test_site_anchors_and_sums(oracle, n):
    """wmax, first_row (global: frame0 = 7 shifts it) and the anchor point exactly; K = 8193 takes the kernels without
    the LDS table.  The sums against the long-double sum; K above 4266 is refused."""
    cfg, M, F, K = SITE_CASES[n]
    pos, lab, confs = _site_case(n)
    cell = _cell(cfg)
    ctx = _site_ctx(cfg, M, pos, lab, confs)
    for weighted in (True, False):
        for frame0 in (0, 7):
            ctx.set_assignments(np.ascontiguousarray(lab), np.ascontiguousarray(confs), frame0)
            want = R.anchors_reference(oracle, cell, pos, lab, confs, K, weighted, frame0)
            got = ctx.site_anchors(K, weighted)
            _same_anchors(got, want, (n, weighted, frame0))
            if K > SITE_K_LIMIT:
                with pytest.raises((ValueError, RuntimeError), match="too many sites"):
                    ctx.site_sums(K, weighted, got[2])
                continue
            sums = ctx.site_sums(K, weighted, got[2])
            assert np.array_equal(sums, ctx.site_sums(K, weighted, got[2])), "two runs, different bits"
            if frame0 == 0:
                _check_sums(oracle, cell, ctx, pos, lab, confs, K, weighted, got[2], sums, (n, weighted))


@pytest.mark.gpu
def test_site_sums_refuse_more_sites_than_their_lds_holds(oracle):
    n = 1
    cfg, M, F, K = SITE_CASES[n]
    pos, lab, confs = _site_case(n)
    ctx = _site_ctx(cfg, M, pos, lab, confs)
    anchors = np.zeros((SITE_K_LIMIT + 1, 3))
    assert ctx.site_sums(SITE_K_LIMIT, True, anchors[:SITE_K_LIMIT]).shape == (SITE_K_LIMIT, 4)
    with pytest.raises((ValueError, RuntimeError), match="too many sites"):
        ctx.site_sums(SITE_K_LIMIT + 1, True, anchors)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 5, 6])
def test_two_contexts_hold_the_halves_of_the_frames(oracle, n):
    """Combined as landmark._site_centers combines ranks: the anchors are the single context's, the added sums within the
    same bound."""
    cfg, M, F, K = SITE_CASES[n]
    pos, lab, confs = _site_case(n)
    cell = _cell(cfg)
    h = F // 2 + 1
    whole = _site_ctx(cfg, M, pos, lab, confs)
    parts = [_site_ctx(cfg, M, pos[:h], lab[:h], confs[:h], 0), _site_ctx(cfg, M, pos[h:], lab[h:], confs[h:], h)]
    for weighted in (True, False):
        wmax, first, anchors = whole.site_anchors(K, weighted)
        got = [p.site_anchors(K, weighted) for p in parts]
        allw, allf, alla = (np.stack([g[q] for g in got]) for q in range(3))
        allf = np.where(allf < 0, np.iinfo(np.int64).max, allf)
        cand = np.where(allw == allw.max(axis=0)[None, :], allf, np.iinfo(np.int64).max)
        owner = np.argmin(cand, axis=0)
        merged = alla[owner, np.arange(K)]
        assert np.array_equal(merged, anchors, equal_nan=True)
        assert np.array_equal(np.where(first < 0, np.iinfo(np.int64).max, first), cand.min(axis=0))
        sums = parts[0].site_sums(K, weighted, merged) + parts[1].site_sums(K, weighted, merged)
        _check_sums(oracle, cell, whole, pos, lab, confs, K, weighted, anchors, sums, (n, weighted, "halves"))


BIG = ("C3", 448, 9400, 1000)              # 4.2e6 rows > 1024 * 4096: the rows per workgroup of k_site_sums grow to 4352


@pytest.mark.gpu
def test_site_sums_when_the_rows_per_workgroup_grow(oracle):
    cfg, M, F, K = BIG
    assert (F * M + 1023) // 1024 > 4096
    cell = _cell(cfg)
    pos, lab, confs = R.make_site_case(oracle, cell, F, M, K, seed=77)
    assert R.face_margin(oracle, cell, pos, lab, confs, K, True) >= 1e-6
    ctx = _site_ctx(cfg, M, pos, lab, confs)
    got = ctx.site_anchors(K, True)
    _same_anchors(got, R.anchors_reference(oracle, cell, pos, lab, confs, K, True), "big")
    sums = ctx.site_sums(K, True, got[2])
    _check_sums(oracle, cell, ctx, pos, lab, confs, K, True, got[2], sums, "big")


# ---- the CPU double of the gloo tests -------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", [4, 7])
def test_the_numpy_double_agrees_with_the_references_on_the_reductions(i):
    """FakeContext sums in floating point: its Gram matrix and row sums are within the forward bound of a sum of n terms
    of the rounded exact value (n u sum|terms|, n the number of rows), its hit counts exact."""
    from tests.fake_ctx import FakeContext
    X, lab, confs, K = _case(i)
    N, D = X.shape
    fake = FakeContext(np.eye(3) * 10.0)
    fake.set_rows_dense(X)
    fake.set_assignments(lab, confs)
    G, seen = fake.gram()
    ghi, glo, rseen = _gram_ref(i)
    assert np.array_equal(seen, rseen)
    u = 2.0 ** -53
    assert np.all(np.abs(G - R.rounded_values(ghi, glo)) <= (N + 2) * u * (np.abs(X).T @ np.abs(X)))
    for weighted in (True, False):
        sums, wsum = fake.weighted_row_sums(K, weighted=weighted)
        ref = R.rounded_values(*_sums_ref(i, weighted))
        w = np.where((lab >= 0) & (lab < K), confs if weighted else 1.0, 0.0).reshape(-1)
        mags = np.stack([(w * (lab.reshape(-1) == k)) @ np.abs(X) for k in range(K)])
        assert np.all(np.abs(sums - ref[:K * D].reshape(K, D)) <= (N + 2) * u * mags)
        np.testing.assert_allclose(wsum, ref[K * D:], rtol=(N + 2) * u, atol=0)


@pytest.mark.parametrize("N", [257, 4097])
def test_the_numpy_double_agrees_with_the_references_on_best_match(N):
    from tests.fake_ctx import FakeContext
    if N not in MATCH_N:
        X, c = R.make_match_rows(N, MATCH_D, seed=N, free_dims=FREE)
        champ = R.champion_row(c, np.arange(MATCH_D - FREE))
        planted = [("none", X, None, None)]
        for name, a, b in R.tie_pairs(N):
            Xt = X.copy()
            Xt[[a, b]] = champ
            planted.append((name, Xt, a, b))
    else:
        _, c = _match_rows(N)
        planted = _planted(N)
    grp, G = _partition()
    fake = FakeContext(np.eye(3) * 10.0)
    for name, Xt, first, _ in planted:
        Xt = Xt.copy()
        Xt[N - 1, 62] = 0.5
        fake.set_rows_dense(Xt)
        _same_match(fake.best_match(c), R.sparse_products_argmax(Xt, c), name)
        _same_groups(fake.best_match_groups(grp, c, G), _group_reference(Xt, grp, c, G), name)
        if first is not None:
            cn = c.copy()
            cn[60] = np.nan
            Xn = Xt.copy()
            Xn[first + 1, 60] = 0.25
            Xn[N - 2, 60] = 0.5
            fake.set_rows_dense(Xn)
            want = R.sparse_products_argmax(Xn, cn)
            assert want[0] == min(first + 1, N - 2)
            _same_match(fake.best_match(cn), want, name + "/nan")
            _same_groups(fake.best_match_groups(grp, cn, G), _group_reference(Xn, grp, cn, G), name + "/nan")


@pytest.mark.parametrize("n", [1, 2, 5, 6])
def test_the_numpy_double_agrees_with_the_references_on_the_site_centres(oracle, n):
    from tests.fake_ctx import FakeContext
    cfg, M, F, K = SITE_CASES[n]
    pos, lab, confs = _site_case(n)
    cell = _cell(cfg)
    fake = FakeContext(cell)
    fake.set_frames(pos, np.zeros(0, dtype=np.int64), np.arange(M), frame0=7)
    fake.set_assignments(lab, confs, frame0=7)
    for weighted in (True, False):
        got = fake.site_anchors(K, weighted)
        _same_anchors(got, R.anchors_reference(oracle, cell, pos, lab, confs, K, weighted, 7), (n, weighted))
        sums = fake.site_sums(K, weighted, got[2])
        ref, tol = R.sums_reference(oracle, cell, pos, lab, confs, K, weighted, got[2])
        assert np.all(np.abs(sums.astype(np.longdouble) - ref) <= tol), (n, weighted)
