"""Writes ``tests/golden/threshold_known_answers.npz``: what the TRUE reference's ``MergeSitesByThreshold`` and
``RemoveUnoccupiedSites`` give on the label / centre sets of ``tests/golden/merge_known_answers.npz`` (those inputs are
read from there and not stored again).  Needs the reference (``oracle.ref_build``); without it the script says so and
writes nothing.  Run from the repository root: ``python tools/make_threshold_goldens.py``.

Layout of the file (``<case>`` in ``names``, ``<variant>`` in ``variants``):
  <case>/cooccupancy              bool[K, K], by a plain loop over the frames
  <case>/<variant>/params         JSON: attrname, threshold, relation (by name), kw (constructor keywords)
  <case>/<variant>/error          class name of what the reference raised, or ""
  <case>/<variant>/centers, traj  the merged network's centres and the merged trajectory (no error only)
  <case>/rm_a/...                 RemoveUnoccupiedSites on the network with three never-visited sites put in
                                  (``dead``: their indices; ``in_*``: the inputs that are not in the merge goldens)
  <case>/rm_b/same_object         the unmodified network: did run() return its argument?
  <case>/rm_c/...                 labels folded onto ``modulus`` sites (fewer than mobile ions): the error's class name
"""
import json
import operator
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

from oracle import ref_build  # noqa: E402

# (name, attrname, threshold, relation, constructor keywords)
VARIANTS = [
    ("n1", "n_ij", 1, "ge", {}),
    ("n1_d25", "n_ij", 1, "ge", dict(distance_threshold=2.5)),
    ("n1_forbid", "n_ij", 1, "ge", dict(forbid_multiple_occupancy=True)),
    ("n2_forbid_d40", "n_ij", 2, "ge", dict(forbid_multiple_occupancy=True, distance_threshold=4.0)),
    ("p001_weak_undirected", "p_ij", 0.01, "ge", dict(directed=False, connection="weak")),
    ("n1_weak_forbid", "n_ij", 1, "ge", dict(connection="weak", forbid_multiple_occupancy=True)),
    ("p002_gt", "p_ij", 0.02, "gt", dict(connection="weak")),
    ("p0005_gt_forbid", "p_ij", 0.005, "gt", dict(forbid_multiple_occupancy=True)),
    ("lag150_le_forbid", "jump_lag", 150.0, "le", dict(forbid_multiple_occupancy=True)),
    ("n1_too_distant", "n_ij", 1, "ge", dict(maximum_merge_distance=1.0)),
]


def cooccupancy(labels, n_sites):
    co = np.zeros((n_sites, n_sites), dtype=bool)
    for frame in labels:
        known = frame[frame >= 0]
        for site in known:
            co[site, known] = True
    return co


def with_dead_sites(centers, labels):
    """Three sites nobody visits at positions 0, K'//2 and K'-1 of the K' = K + 3 sites; labels moved accordingly."""
    K = len(centers)
    dead = np.array([0, (K + 3) // 2, K + 2])
    alive = np.setdiff1d(np.arange(K + 3), dead)
    cen = np.empty((K + 3, 3))
    cen[alive] = centers
    cen[dead] = centers[:3] + 0.1
    lab = np.where(labels >= 0, alive[np.where(labels >= 0, labels, 0)], -1)
    return dead, cen, lab


def main():
    if not ref_build.available():
        print("reference not present; threshold goldens can only be generated where it is")
        return 0
    ref_build.import_reference()
    import ase
    from sitator import SiteNetwork, SiteTrajectory
    from sitator.dynamics import JumpAnalysis
    from sitator.dynamics.MergeSitesByThreshold import MergeSitesByThreshold
    from sitator.dynamics.RemoveUnoccupiedSites import RemoveUnoccupiedSites

    src = np.load(os.path.join(GOLDEN, "merge_known_answers.npz"), allow_pickle=False)
    blob = {"names": src["names"], "variants": np.array([v[0] for v in VARIANTS])}
    for name in (str(n) for n in src["names"]):
        lab, cen, cell = src[name + "/labels"], src[name + "/centers"], src[name + "/cell"]
        sm, mm, refp = src[name + "/static_mask"], src[name + "/mobile_mask"], src[name + "/ref_positions"]
        at = ase.Atoms(positions=refp, numbers=np.where(mm, 3, 8), cell=cell)
        K = len(cen)

        def make_st(centers=cen, labels=lab):
            sn = SiteNetwork(at, sm, mm)
            sn.centers = centers.copy()
            return SiteTrajectory(sn, labels.copy())

        co = cooccupancy(lab, K)
        blob[name + "/cooccupancy"] = co
        off = ~np.eye(K, dtype=bool)
        print("%s: K=%d, co-occupancy %.0f%% of the off-diagonal" % (name, K, 100.0 * co[off].mean()))
        for vname, attr, thr, rel, kw in VARIANTS:
            key = "%s/%s" % (name, vname)
            blob[key + "/params"] = json.dumps({"attrname": attr, "threshold": thr, "relation": rel, "kw": kw})
            st = make_st()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                JumpAnalysis().run(st)
                try:
                    out = MergeSitesByThreshold(attr, relation=getattr(operator, rel), check_types=False, **kw).run(
                        st, threshold=thr)
                    blob[key + "/error"] = ""
                    blob[key + "/centers"] = np.asarray(out.site_network.centers)
                    blob[key + "/traj"] = out.traj.copy()
                    print("  %-22s %d -> %d" % (vname, K, out.site_network.n_sites))
                except Exception as e:                       # noqa: BLE001 - the class name is the golden
                    blob[key + "/error"] = type(e).__name__
                    print("  %-22s %s" % (vname, type(e).__name__))

        # RemoveUnoccupiedSites (a): three dead sites, types and attributes set
        dead, cen_a, lab_a = with_dead_sites(cen, lab)
        Ka = K + 3
        st = make_st(cen_a, lab_a)
        types = np.arange(Ka) % 3
        score = np.arange(Ka) * 1.5 + 0.25
        weight = np.arange(Ka * Ka, dtype=np.float64).reshape(Ka, Ka)
        st.site_network.site_types = types.copy()
        st.site_network.add_site_attribute("score", score.copy())
        st.site_network.add_edge_attribute("weight", weight.copy())
        out, kept = RemoveUnoccupiedSites().run(st, return_kept_sites=True)
        assert out is not st
        key = name + "/rm_a"
        blob[key + "/dead"] = dead
        blob[key + "/in_types"], blob[key + "/in_score"], blob[key + "/in_weight"] = types, score, weight
        blob[key + "/kept"] = np.asarray(kept[0])
        blob[key + "/traj"] = out.traj.copy()
        blob[key + "/centers"] = np.asarray(out.site_network.centers)
        blob[key + "/types"] = np.asarray(out.site_network.site_types)
        blob[key + "/score"] = np.asarray(out.site_network.score)
        blob[key + "/weight"] = np.asarray(out.site_network.weight)
        print("  rm_a %d -> %d, kept all but %s" % (Ka, out.site_network.n_sites, dead))
        # (b): nothing to remove
        st = make_st()
        blob[name + "/rm_b/same_object"] = np.bool_(RemoveUnoccupiedSites().run(st, return_kept_sites=True) is st)
        # (c): fewer visited sites than mobile ions
        modulus = int(mm.sum()) - 1
        st = make_st(labels=np.where(lab >= 0, lab % modulus, -1))
        try:
            RemoveUnoccupiedSites().run(st)
            err = ""
        except Exception as e:                               # noqa: BLE001
            err = type(e).__name__
        blob[name + "/rm_c/modulus"] = np.int64(modulus)
        blob[name + "/rm_c/error"] = err
        print("  rm_b same object: %s; rm_c (labels mod %d): %s" % (bool(blob[name + "/rm_b/same_object"]), modulus, err))
    path = os.path.join(GOLDEN, "threshold_known_answers.npz")
    np.savez_compressed(path, **blob)
    print("threshold_known_answers %.1f KB" % (os.path.getsize(path) / 1024.0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
