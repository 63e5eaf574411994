"""CPU-only: the host side of ``SiteTypeAnalysis`` against what the TRUE reference and sklearn give
(tests/golden/site_types_known_answers.npz, written by tools/make_site_type_goldens.py from the reference's own ``run``).

``sitator_amd.elbow.index_of_elbow`` must give the reference's recorded indices exactly.  ``pca_from_covariance`` - the rule the
operator applies to the covariance the device returns - is handed numpy's covariance of the golden inputs and must take sklearn's
``n_components`` (the fallback to ``min_pca_dimensions`` included), its ``explained_variance_ratio_`` and its projection up to
column signs.  The bounds: a ratio is a quotient of eigenvalues of a float64 covariance summed over N <= 4096 rows, each good to
about ``N eps ||C||``, so the ratios agree within ``8 N eps`` (a factor 8 for the two roundings of numerator and denominator and
LAPACK's own few eps).  An eigenvector moves by at most ``||E|| / gap`` under a perturbation ``E`` (Davis-Kahan), here
``||E|| <= N eps ||C||``, so a pairwise distance of two projections moves by at most ``2 sqrt(d) N eps (||C|| / gap) ||x_i - x_j||``; the test
allows a safety factor of 16 on it and asserts the gap of its own inputs (at least a factor 10 between the last eigenvalue taken
and the first left out)."""
import os

import numpy as np
import pytest

from tests import dpc_ref as DR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "site_types_known_answers.npz")
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def case_names():
    return [str(n) for n in np.load(GOLDEN)["cases"]]


def test_index_of_elbow_gives_the_reference_indices(golden):
    from sitator_amd.elbow import index_of_elbow
    expected = golden["elbow_index"]
    assert len(expected) >= 5
    for k, want in enumerate(expected):
        assert index_of_elbow(golden["elbow_curves/%d" % k]) == want


@pytest.mark.parametrize("name", case_names())
def test_pca_rule_against_sklearn(golden, name):
    from sklearn.decomposition import PCA
    from sitator_amd.site_descriptors import pca_from_covariance
    X = golden[name + "/dvecs"]
    variance, min_dims = float(golden[name + "/min_pca_variance"]), int(golden[name + "/min_pca_dimensions"])
    N, D = X.shape
    assert N <= 4096
    sk = PCA(variance)
    Y_sk = sk.fit_transform(X)
    forced = Y_sk.shape[1] < min_dims
    assert forced == (name == "line_forced_second_dimension")
    if forced:
        sk = PCA(n_components=min_dims)
        Y_sk = sk.fit_transform(X)
    mean = X.mean(axis=0)
    cov = (X - mean).T @ (X - mean) / (N - 1)
    pca = pca_from_covariance(mean, cov, N, variance, min_dims)
    d = pca.n_components_
    assert d == sk.n_components_ == int(golden[name + "/n_components"])
    assert np.all(np.abs(pca.explained_variance_ratio_ - sk.explained_variance_ratio_) <= 8 * N * EPS)
    assert np.all(np.abs(pca.explained_variance_ratio_ - golden[name + "/explained_variance_ratio"]) <= 8 * N * EPS)
    assert np.all(np.abs(pca.explained_variance_ - sk.explained_variance_) <= 8 * N * EPS * sk.explained_variance_[0])
    # the gap of these inputs, then the distances of the projections
    spectrum = np.linalg.eigvalsh(cov)[::-1]
    assert spectrum[d - 1] >= 10.0 * spectrum[d]
    gap = spectrum[d - 1] - spectrum[d]
    Y = (X - pca.mean_) @ pca.components_.T
    bound = 16 * 2 * np.sqrt(d) * N * EPS * (spectrum[0] / gap) * DR.distances(X)
    assert np.all(np.abs(DR.distances(Y) - DR.distances(Y_sk)) <= bound)
    assert np.max(bound) < 1e-9 * np.max(DR.distances(Y))            # the bound says something


@pytest.mark.parametrize("name", case_names())
def test_restatement_reproduces_the_reference_run(golden, name):
    """The whole of ``run`` on the host from the restatement's pieces (numpy covariance, the PCA rule, tests/dpc_ref.py, the elbow):
    the yardstick the GPU test holds the operator to is consistent with the reference's recorded answers."""
    from sitator_amd.elbow import index_of_elbow
    from sitator_amd.site_descriptors import pca_from_covariance
    X, to_site, K = golden[name + "/dvecs"], golden[name + "/dvecs_to_site"], int(golden[name + "/n_sites"])
    mean = X.mean(axis=0)
    pca = pca_from_covariance(mean, (X - mean).T @ (X - mean) / (len(X) - 1), len(X), float(golden[name + "/min_pca_variance"]),
                              int(golden[name + "/min_pca_dimensions"]))
    dpc = DR.Cluster((X - mean) @ pca.components_.T)
    curve = dpc.density * dpc.delta
    order = np.argsort(curve)[::-1]
    elbow = index_of_elbow(curve[order[:int(int(golden[name + "/n_site_types_max"]) * 1.5)]])
    assert elbow == int(golden[name + "/elbow"])
    dpc.assign(np.min(dpc.density[order[:elbow]]) - 0.001, np.min(dpc.delta[order[:elbow]]) - 0.001)
    assert np.array_equal(dpc.membership, golden[name + "/membership"]) and np.array_equal(dpc.clusters, golden[name + "/clusters"])
    votes = DR.votes(dpc.membership, to_site, K, len(dpc.clusters))
    assert np.array_equal(np.argmax(votes, axis=1), golden[name + "/site_types"])
    assert np.array_equal(votes.max(axis=1) / np.bincount(to_site, minlength=K), golden[name + "/winning_vote_percentages"])


def test_pca_rule_refuses_what_sklearn_refuses():
    from sitator_amd.site_descriptors import pca_from_covariance
    cov = np.diag([5.0, 1.0, 0.1])
    assert pca_from_covariance(np.zeros(3), cov, 10, 0.9, 1).n_components_ == 2
    assert pca_from_covariance(np.zeros(3), cov, 10, 0.5, 1).n_components_ == 1
    assert pca_from_covariance(np.zeros(3), cov, 10, 0.5, 3).n_components_ == 3
    with pytest.raises(ValueError):
        pca_from_covariance(np.zeros(3), cov, 10, 0.5, 4)            # more than min(n_samples, n_features)
    with pytest.raises(ValueError):
        pca_from_covariance(np.zeros(3), cov, 2, 0.5, 3)
    with pytest.raises(ValueError):
        pca_from_covariance(np.zeros(3), cov, 10, 1.5, 1)
