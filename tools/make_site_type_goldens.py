"""Writes ``tests/golden/site_types_known_answers.npz``: what the TRUE reference's ``SiteTypeAnalysis.run``
(``site_descriptors/SiteTypeAnalysis.py:54-165``) makes of designed descriptor vectors, and what its ``index_of_elbow``
(``util/elbow.py``) says about a handful of curves.  Needs the reference (``oracle.ref_build``) and sklearn; without the
reference the script says so and writes nothing.  Run from the repository root:

    python tools/make_site_type_goldens.py

The reference's files stay as they are.  ``SiteTypeAnalysis.py`` is loaded from its file under a stand-in for its package, as
``tools/make_soap_goldens.py`` loads ``SOAP.py``; ``np.int`` / ``np.float`` reach it through a proxy in the module's namespace;
``pydpc``, which is not installed, is stood in by ``tests/dpc_ref.Cluster`` (the numpy restatement of the definitions in
``csrc/dpc_plan.h``); the descriptor is a stub that returns fixed ``dvecs`` / ``dvecs_to_site``; the PCA is sklearn's own.

The inputs are designed so that no decision is close, and the script asserts it: well-separated Gaussian blobs of at least 30
points in all, distinct ``density * delta`` among the top 30, an eigenvalue gap of at least a factor 10 where the PCA cuts, and the
types the reference finds are the blobs.

Per case ``<name>/dvecs [N, D]``, ``dvecs_to_site [N]``, ``n_sites``, ``min_pca_variance``, ``min_pca_dimensions``,
``n_site_types_max``, ``blob [N]`` (the design), and of the reference's run ``site_types``, ``n_types``, ``elbow``,
``winning_vote_percentages``, ``membership``, ``clusters``, ``n_components``, ``explained_variance_ratio``, ``n_unassigned``.
``elbow_curves/<k>`` and ``elbow_index [k]``: the curves and the reference's answers."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

from oracle import ref_build  # noqa: E402
from tests import dpc_ref  # noqa: E402

SEED = 20261020


class NpProxy(object):
    """numpy with the aliases numpy 1.24 removed."""
    int = int
    float = float
    bool = bool

    def __getattr__(self, name):
        return getattr(np, name)


def load_site_type_module(root):
    base = os.path.join(root, "sitator", "site_descriptors")
    pkg = types.ModuleType("sitator_ref_site_descriptors")
    pkg.__path__ = [base]
    sys.modules[pkg.__name__] = pkg
    spec = importlib.util.spec_from_file_location(pkg.__name__ + ".SiteTypeAnalysis", os.path.join(base, "SiteTypeAnalysis.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    if "sitator.misc" not in sys.modules:
        # the module imports GenerateAroundSites without using it in run(); sitator.misc's own __init__ needs
        # GenerateClampedTrajectory.pyx, which Cython 3 rejects (oracle/ref_build.py)
        misc = types.ModuleType("sitator.misc")
        misc.GenerateAroundSites = None
        sys.modules["sitator.misc"] = misc
    spec.loader.exec_module(mod)
    mod.np = NpProxy()
    stand_in = types.ModuleType("pydpc")
    stand_in.Cluster = dpc_ref.Cluster
    mod.pydpc = stand_in
    mod.has_pydpc = True
    return mod


def blobs(rng, D, centres, sigma, per_site, site_blob, strays=()):
    """Descriptor vectors: site s has per_site[s] vectors around centre site_blob[s]; strays: (site, count, blob) moves the first
    `count` vectors of a site to another blob (a vote that is not unanimous)."""
    dvecs, to_site, blob = [], [], []
    for s, (n, b) in enumerate(zip(per_site, site_blob)):
        which = np.full(n, b)
        for site, count, other in strays:
            if site == s:
                which[:count] = other
        dvecs.append(centres[which] + rng.normal(size=(n, D)) * sigma)
        to_site.append(np.full(n, s))
        blob.append(which)
    return np.concatenate(dvecs), np.concatenate(to_site).astype(np.int64), np.concatenate(blob).astype(np.int64)


def designed_cases():
    rng = np.random.default_rng(SEED)
    cases = []
    # three blobs in 12 dimensions, nine sites of ten vectors; site 0 gives three of its votes to another blob
    centres = np.zeros((3, 12))
    centres[0, :3], centres[1, :3], centres[2, :3] = [0.0, 0.0, 0.0], [6.0, 0.5, 0.0], [2.0, 5.5, 0.3]
    sigma = np.full(12, 0.08)
    cases.append(("three_blobs", blobs(rng, 12, centres, sigma, [10] * 9, [0, 1, 2, 0, 1, 2, 0, 1, 2], strays=[(0, 3, 1)]), 9, 0.9, 2, 20))
    # two blobs on a line: one component explains the variance, min_pca_dimensions forces a second (its noise stands out by design)
    centres = np.zeros((2, 6))
    centres[1, 0] = 8.0
    sigma = np.array([0.1, 0.5, 0.02, 0.02, 0.02, 0.02])
    cases.append(("line_forced_second_dimension", blobs(rng, 6, centres, sigma, [12, 8, 15, 10], [0, 1, 1, 0]), 4, 0.9, 2, 20))
    # five blobs in 20 dimensions, sites of unequal size, a higher variance threshold
    centres = np.zeros((5, 20))
    centres[:, :4] = [[0, 0, 0, 0], [7, 0, 0, 0], [0, 7, 0, 0], [0, 0, 7, 0], [4, 4, 4, 6]]
    sigma = np.full(20, 0.05)
    per_site = [9, 14, 20, 11, 16, 13, 25, 10, 12, 18]
    cases.append(("five_blobs_uneven", blobs(rng, 20, centres, sigma, per_site, [0, 1, 2, 3, 4, 4, 3, 2, 1, 0], strays=[(6, 5, 0)]), 10,
                  0.95, 2, 20))
    return cases


ELBOW_CURVES = [
    [10.0, 9.0, 8.5, 1.0, 0.9, 0.8, 0.7, 0.6],
    [0.6, 0.7, 10.0, 0.8, 9.0, 1.0, 8.5, 0.9],                      # the same, unsorted
    [5.0, 1.0, 0.5, 0.4, 0.3, 0.2, 0.1],
    [100.0, 90.0, 80.0, 70.0, 5.0, 4.0, 3.0, 2.0, 1.0, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05, 0.04, 0.03, 0.02, 0.01, 0.005],
    [3.0, 1.0, 0.9],
    [8.0, 7.9, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1],
]


def main():
    if not ref_build.available():
        print("reference not present; site type goldens can only be generated where it is")
        return 0
    root = ref_build.build()
    ref_build.import_reference()
    import ase
    from sitator import SiteNetwork
    from sitator.util.elbow import index_of_elbow
    STA = load_site_type_module(root)

    blob, names = {}, []
    for name, (dvecs, to_site, design), K, variance, min_dims, types_max in designed_cases():
        assert len(dvecs) >= 30
        rng = np.random.default_rng(SEED + len(name))
        n_atoms = K + 4
        mobile = np.zeros(n_atoms, dtype=bool)
        mobile[:2] = True
        at = ase.Atoms(positions=rng.uniform(0.0, 7.0, size=(n_atoms, 3)), numbers=np.where(mobile, 3, 8), cell=np.eye(3) * 7.0)
        sn = SiteNetwork(at, ~mobile, mobile)
        sn.centers = rng.uniform(0.0, 7.0, size=(K, 3))

        class Stub(object):
            def get_descriptors(self, stn, **kwargs):
                return dvecs.copy(), to_site.copy()

        op = STA.SiteTypeAnalysis(Stub(), min_pca_variance=variance, min_pca_dimensions=min_dims, n_site_types_max=types_max)
        out = op.run(sn)
        # nothing is close
        from sklearn.decomposition import PCA
        spectrum = PCA().fit(dvecs).explained_variance_
        d = op.dvecs.shape[1]
        assert spectrum[d - 1] >= 10.0 * spectrum[d], "eigenvalue gap at the cut: %r" % (spectrum[:d + 1],)
        top = np.sort(op.dpc.density * op.dpc.delta)[::-1][:30]
        assert np.all(np.diff(top) < 0) and np.min(-np.diff(top) / top[:-1]) > 1e-9, "density * delta not distinct among the top 30"
        n_blobs = len(np.unique(design))
        assert op.n_types == n_blobs and op._decision_elbow == n_blobs and op._n_unassigned == 0
        site_blob = np.array([np.bincount(design[to_site == s]).argmax() for s in range(K)])
        relabel = {b: t for b, t in zip(site_blob, out.site_types)}
        assert len(set(relabel.values())) == n_blobs and all(relabel[b] == t for b, t in zip(site_blob, out.site_types))
        assert np.array_equal(np.array([relabel[b] for b in design]), op.dpc.membership)
        names.append(name)
        for k, v in (("dvecs", dvecs), ("dvecs_to_site", to_site), ("n_sites", np.int64(K)), ("min_pca_variance", np.float64(variance)),
                     ("min_pca_dimensions", np.int64(min_dims)), ("n_site_types_max", np.int64(types_max)), ("blob", design),
                     ("site_types", np.asarray(out.site_types, dtype=np.int64)), ("n_types", np.int64(op.n_types)),
                     ("elbow", np.int64(op._decision_elbow)), ("winning_vote_percentages", np.asarray(op.winning_vote_percentages)),
                     ("membership", np.asarray(op.dpc.membership, dtype=np.int64)), ("clusters", np.asarray(op.dpc.clusters, dtype=np.int64)),
                     ("n_components", np.int64(d)), ("explained_variance_ratio", np.asarray(op.pca.explained_variance_ratio_)),
                     ("n_unassigned", np.int64(op._n_unassigned))):
            blob["%s/%s" % (name, k)] = v
        print("%s: N %d, D %d -> d %d, %d types, elbow %d, votes %s" % (name, len(dvecs), dvecs.shape[1], d, op.n_types, op._decision_elbow,
                                                                        np.round(op.winning_vote_percentages, 3)))
    blob["cases"] = np.array(names)
    for k, curve in enumerate(ELBOW_CURVES):
        blob["elbow_curves/%d" % k] = np.array(curve)
    blob["elbow_index"] = np.array([int(index_of_elbow(np.array(curve))) for curve in ELBOW_CURVES], dtype=np.int64)
    print("elbows:", blob["elbow_index"])
    path = os.path.join(GOLDEN, "site_types_known_answers.npz")
    np.savez_compressed(path, **blob)
    print("wrote %s (%d bytes): %s" % (path, os.path.getsize(path), ", ".join(names)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
