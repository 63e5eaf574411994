"""Writes ``tests/golden/site_groups_known_answers.npz``: what the TRUE reference gives for the per-site point clouds of a
``SiteTrajectory`` and for the two operators that loop over them, ``misc.NAvgsPerSite`` and ``site_descriptors.SiteVolumes``.
Needs the reference (``oracle.ref_build``); without it the script says so and writes nothing.  Run from the repository root:
``python tools/make_group_goldens.py``.

Two things are put into the namespaces of the reference's modules, as ``tools/make_threshold_goldens.py`` injects
``iterlimit`` for ``MergeSitesByDynamics``; the reference's files stay as they are.

* ``NAvgsPerSite.run`` does not run under numpy 2: ``types.fill(np.nan)`` on an integer array raises ``ValueError``
  (``NAvgsPerSite.py:42-43``).  The module is loaded from its file (``sitator/misc/__init__.py`` imports the clamp module the
  stock build leaves out) and its global ``np`` is replaced by a proxy whose ``nan`` is ``0`` and which forwards everything
  else to numpy (both modules are loaded from their files).  The two ``fill`` calls then fill with zeros; every element that
  is returned is overwritten afterwards.
* ``SiteVolumes.compute_accessable_volumes`` runs as it is.  To record the recentred points it hands to qhull, the module's
  global ``ConvexHull`` is wrapped by a function that keeps a copy of its argument and calls scipy's.

Layout (``<case>`` in ``names``):
  scipy_version                 the scipy the volumes were computed with
  empty_site_error              class name of what compute_accessable_volumes raises for a site without points
  <case>/in_cell, in_ref_positions [A, 3], in_mobile_mask [A], in_centers [K, 3], in_vertices [K, V] (static numbering, -1
  <case>/                       padded; absent without static atoms), in_real [F, A, 3], in_confs [F, M]
  <case>/in_labels [F, M]       unassigned entries, several ions on one site in one frame
  <case>/in_labels_few          the same with the last site cut down to 3 points, in_labels_empty: to none
  <case>/out_offsets [K + 1], out_points [N, 3], out_confs [N]   real_positions_for_site(s, True) of in_labels, s ascending
  <case>/out_navg_w<weighted>_n<n>_centers / _types             NAvgsPerSite(n, True, weighted).run on in_labels
  <case>/out_navg_few_n4_centers / _types                       NAvgsPerSite(4, False, True).run on in_labels_few
  <case>/out_navg_few_n4_error                                  "<class>: <message>" of NAvgsPerSite(4, True, True) on it
  <case>/out_recentered_r<n> [n, N, 3]   the points of all sites as qhull got them at every recentring (in_labels)
  <case>/out_access_vol_r<n> [K]         accessable_site_volumes, n_recenterings = n in {1, 8}
  <case>/out_site_volumes, out_site_surface_areas [K]            compute_volumes (cases with static atoms)
  <case>/margin_floor           the smallest distance (cell units) of a floored crystal coordinate to an integer over every
                                recentring step, every bucket's shifted points and mean, and the vertices' wrap
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

from oracle import ref_build  # noqa: E402
from tests import group_ref as GR  # noqa: E402

SEED = 20261019
N_VALUES = (2, 4)
RECENTERINGS = (1, 8)
# (name, cell, F, M, static atoms, layout, K, unassigned entries, spread: None = up to three cells away, else Angstrom)
CASES = [("tri_far_allmobile", GR.TRICLINIC, 40, 5, 0, "first", 4, 25, None),
         ("ortho_clustered_static", GR.ORTHO, 60, 6, 8, "interleaved", 5, 40, 0.3)]


class NpProxy(object):
    """numpy with ``nan`` = 0 (see the module docstring)."""
    nan = 0

    def __getattr__(self, name):
        return getattr(np, name)


def load_from_file(root, *path):
    """A module of the reference by its file: the packages ``sitator.misc`` and ``sitator.site_descriptors`` import the clamp
    module, which the stock build leaves out."""
    spec = importlib.util.spec_from_file_location("sitator_ref_" + path[-1][:-3], os.path.join(root, "sitator", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def error_text(fn):
    try:
        fn()
    except Exception as e:                                       # noqa: BLE001 - class and message are the golden
        return "%s: %s" % (type(e).__name__, e)
    return ""


def cut_site(labels, site, keep):
    out = labels.copy()
    flat = out.reshape(-1)
    where = np.nonzero(flat == site)[0]
    flat[where[keep:]] = -1
    return out


def main():
    if not ref_build.available():
        print("reference not present; group goldens can only be generated where it is")
        return 0
    root = ref_build.build()
    ref_build.import_reference()
    import ase
    import scipy
    from sitator import SiteNetwork, SiteTrajectory
    SVM = load_from_file(root, "site_descriptors", "SiteVolumes.py")
    navgs_module = load_from_file(root, "misc", "NAvgsPerSite.py")
    navgs_module.np = NpProxy()
    NAvgs = navgs_module.NAvgsPerSite

    captured = []
    true_hull = SVM.ConvexHull

    def recording_hull(points, *a, **k):
        captured.append(np.array(points, copy=True))
        return true_hull(points, *a, **k)
    SVM.ConvexHull = recording_hull

    blob = {"scipy_version": np.array(scipy.__version__)}
    names = []
    for ci, (name, cell, F, M, S, kind, K, n_unknown, spread) in enumerate(CASES):
        seed = SEED + ci
        while True:
            labels, mobile_pos, confs = GR.designed(cell, F, M, K, seed, n_unknown=n_unknown, spread=spread)
            assert np.any(labels == -1) and any(len(set(r[r >= 0])) < np.sum(r >= 0) for r in labels)
            few, empty = cut_site(labels, K - 1, 3), cut_site(labels, K - 1, 0)
            mobile = GR.layout(M, S, kind, seed + 1)
            rng = np.random.default_rng(seed + 2)
            ref_positions = rng.uniform(size=(M + S, 3)) @ cell
            real = ref_positions[None] + rng.normal(scale=0.05, size=(F, M + S, 3))
            real[:, mobile] = mobile_pos
            centers = rng.uniform(size=(K, 3)) @ cell
            midx = np.where(mobile)[0]
            m = np.inf
            for lab in (labels, few):
                off, _, pts, cf = GR.grouped(lab, K, real, midx, confs)
                m = min(m, GR.margin(cell, off, pts, cf, N_VALUES, RECENTERINGS))
            vertices = None
            if S:
                vertices = np.full((K, 5), -1, dtype=np.int64)
                for s in range(K):
                    nv = 4 if s == 0 else 5
                    vertices[s, :nv] = np.sort(rng.choice(S, size=nv, replace=False))
                    m = min(m, GR.floor_margin(cell, ref_positions[~mobile][vertices[s, :nv]] + (GR.centroid(cell) - centers[s])))
            if m >= GR.MARGIN:
                break
            seed += 1000
        names.append(name)

        def make_st(lab, with_confs=True, with_vertices=False):       # (ragged vertices: the reference's copy() fails on them)
            at = ase.Atoms(positions=ref_positions, numbers=np.where(mobile, 3, 8), cell=cell)
            sn = SiteNetwork(at, ~mobile, mobile)
            sn.centers = centers.copy()
            if with_vertices:
                sn.vertices = [[int(v) for v in row if v >= 0] for row in vertices]
            st = SiteTrajectory(sn, lab.copy(), confidences=confs.copy() if with_confs else None)
            st.set_real_traj(real.copy())
            return st

        for k, v in (("cell", cell), ("ref_positions", ref_positions), ("mobile_mask", mobile), ("centers", centers),
                     ("real", real), ("confs", confs), ("labels", labels), ("labels_few", few), ("labels_empty", empty)):
            blob["%s/in_%s" % (name, k)] = v
        if vertices is not None:
            blob[name + "/in_vertices"] = vertices
        blob[name + "/margin_floor"] = np.float64(m)

        st = make_st(labels)
        per_site = [st.real_positions_for_site(s, return_confidences=True) for s in range(K)]
        blob[name + "/out_offsets"] = np.concatenate([[0], np.cumsum([len(p) for p, _ in per_site])]).astype(np.int64)
        blob[name + "/out_points"] = np.concatenate([p for p, _ in per_site])
        blob[name + "/out_confs"] = np.concatenate([c for _, c in per_site])
        N = len(blob[name + "/out_points"])

        for w in (0, 1):
            for n in N_VALUES:
                out = NAvgs(n, True, bool(w)).run(make_st(labels))
                assert out.centers.shape == (K * n, 3)
                # the issue's check of the proxy: the output is PBCCalculator.average of the reference's own buckets
                blob["%s/out_navg_w%d_n%d_centers" % (name, w, n)] = np.array(out.centers)
                blob["%s/out_navg_w%d_n%d_types" % (name, w, n)] = np.array(out.site_types, dtype=np.int64)
        out = NAvgs(4, False, True).run(make_st(few))
        blob[name + "/out_navg_few_n4_centers"] = np.array(out.centers)
        blob[name + "/out_navg_few_n4_types"] = np.array(out.site_types, dtype=np.int64)
        blob[name + "/out_navg_few_n4_error"] = np.array(error_text(lambda: NAvgs(4, True, True).run(make_st(few))))
        assert str(blob[name + "/out_navg_few_n4_error"]).startswith("ValueError: Insufficient")

        for nr in RECENTERINGS:
            del captured[:]
            st = make_st(labels)
            SVM.SiteVolumes().compute_accessable_volumes(st, n_recenterings=nr)
            assert len(captured) == K * nr
            steps = np.empty((nr, N, 3))
            off = blob[name + "/out_offsets"]
            for s in range(K):
                for i in range(nr):
                    steps[i, off[s]:off[s + 1]] = captured[s * nr + i]
            blob["%s/out_recentered_r%d" % (name, nr)] = steps
            blob["%s/out_access_vol_r%d" % (name, nr)] = np.array(st.site_network.accessable_site_volumes)
        if vertices is not None:
            st = make_st(labels, with_vertices=True)
            SVM.SiteVolumes().compute_volumes(st.site_network)
            blob[name + "/out_site_volumes"] = np.array(st.site_network.site_volumes)
            blob[name + "/out_site_surface_areas"] = np.array(st.site_network.site_surface_areas)
        if ci == 0:
            blob["empty_site_error"] = np.array(error_text(
                lambda: SVM.SiteVolumes().compute_accessable_volumes(make_st(empty))).split(":")[0])
        print("%-24s F=%d M=%d A=%d K=%d N=%d: floor margin %.3g" % (name, F, M, M + S, K, N, m))

    print("errors: empty site %s; insufficient %r" % (blob["empty_site_error"], str(blob[names[0] + "/out_navg_few_n4_error"])))
    blob["names"] = np.array(names)
    path = os.path.join(GOLDEN, "site_groups_known_answers.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    print("site_groups_known_answers %.1f KB, scipy %s" % (size / 1024.0, scipy.__version__))
    assert size < 300 * 1024
    return 0


if __name__ == "__main__":
    sys.exit(main())
