"""Writes ``tests/golden/pathway_known_answers.npz``: what the TRUE reference's ``network.DiffusionPathwayAnalysis`` gives on
the designed and random site networks of ``tests/pathway_ref.py`` (``golden_case_inputs``).  Needs the reference
(``oracle.ref_build``); without it the script says so and writes nothing.  Run from the repository root:
``python tools/make_pathway_goldens.py``.

How the reference is run.  Its files stay as they are; ``oracle.ref_build.import_reference()`` supplies the ``np.bool`` /
``np.int`` aliases its ``run`` uses.  To record the component labels scipy returns inside ``run`` - the reference keeps them
in a local variable - the global ``connected_components`` of the reference's module is wrapped by a function that calls
scipy's and keeps a copy of the result (as ``tools/make_group_goldens.py`` wraps ``ConvexHull``).  The image codes are the
return values of the reference's own ``PBCCalculator.min_image`` for every connected pair, called from here exactly as
``_build_mic_connmat`` calls it.  ``return_direction`` is asked for with ``true_periodic_pathways`` only: without, the
reference's ``run`` ends in ``UnboundLocalError`` (recorded as ``plain_direction_error``).

Layout (``<case>`` in ``names``):
  scipy_version, plain_direction_error
  <case>/cell [3, 3], centers [K, 3], n_ij [K, K], kw (JSON: the constructor keywords)
  <case>/out_codes  int16 [K, K]   100 i + 10 j + k of min_image(centers[from], centers[to]) where n_ij >= threshold, else 0
  <case>/out_labels int32 [27 K]   scipy's component numbers of the supercell graph ([K] of the plain graph without
                                   true_periodic_pathways)
  <case>/out_site [K], out_edge int16 [K, K], out_count            site_diffusion_pathway, edge_diffusion_pathway, n_pathways
  <case>/out_dir_rows uint8 [n, 3], out_dir_offsets [count + 1]    per pathway its direction triples, sorted
  <case>/n_candidates, n_dropped   components that touch the reference's home nodes (13 ... 13 + K - 1) and hold a site twice; (edge, image) pairs that the
                                   +-1 rule dropped - both counted by tests/pathway_ref.py from the reference's labels and codes
"""
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

from oracle import ref_build  # noqa: E402
from tests import pathway_ref as PR  # noqa: E402


def main():
    if not ref_build.available():
        print("reference not present; pathway goldens can only be generated where it is")
        return 0
    ref_build.import_reference()
    import ase
    import scipy
    from sitator import SiteNetwork
    from sitator.util import PBCCalculator
    import importlib
    dpa_module = importlib.import_module("sitator.network.DiffusionPathwayAnalysis")
    DiffusionPathwayAnalysis = dpa_module.DiffusionPathwayAnalysis

    seen = []
    scipy_components = dpa_module.connected_components

    def recording_components(*args, **kwargs):
        result = scipy_components(*args, **kwargs)
        seen.append(np.array(result[1]))
        return result
    dpa_module.connected_components = recording_components

    def network(cell, centers, n_ij):
        at = ase.Atoms(positions=np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]), numbers=np.array([8, 3]), cell=cell)
        sn = SiteNetwork(at, np.array([True, False]), np.array([False, True]))
        sn.centers = centers.copy()
        sn.add_edge_attribute("n_ij", n_ij.copy())
        return sn

    cases = PR.golden_case_inputs()
    blob = {"names": np.array(list(cases)), "scipy_version": scipy.__version__}
    tally = {"multi": [], "merged": [], "dropped": [], "plain": []}
    for name, (cell, centers, n_ij, kw) in cases.items():
        K = len(centers)
        periodic = kw.get("true_periodic_pathways", True)
        sn = network(cell, centers, n_ij)
        del seen[:]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = DiffusionPathwayAnalysis(**kw).run(sn, return_count=True, return_direction=periodic)
        assert out[0] is sn and len(seen) == 1
        count = int(out[1])
        dirs = list(out[2]) if periodic else []
        labels = seen[0]
        # the codes, by the reference's PBCCalculator as _build_mic_connmat calls it
        conn = PR.connectivity(n_ij, kw.get("connectivity_threshold", 1))
        pbcc = PBCCalculator(cell)
        codes = np.zeros((K, K), dtype=np.int16)
        buf = np.empty(3)
        for a, b in zip(*np.where(conn)):
            buf[:] = centers[b]
            codes[a, b] = pbcc.min_image(centers[a], buf)
        n_candidates, n_dropped = 0, 0
        if periodic:
            n_candidates = PR.pathways_of(labels, K)[2]
            n_dropped = PR.supercell_edges(conn, codes.astype(np.int64))[2]
        rows, offsets = PR.directions_arrays(dirs)
        assert len(offsets) == (count + 1 if periodic else 1)
        key = name + "/"
        blob[key + "cell"], blob[key + "centers"], blob[key + "n_ij"] = np.asarray(cell, dtype=np.float64), centers, n_ij
        blob[key + "kw"] = json.dumps(kw)
        blob[key + "out_codes"] = codes
        blob[key + "out_labels"] = labels.astype(np.int32)
        blob[key + "out_site"] = np.asarray(sn.site_diffusion_pathway).astype(np.int64)
        blob[key + "out_edge"] = np.asarray(sn.edge_diffusion_pathway).astype(np.int16)
        blob[key + "out_count"] = np.int64(count)
        blob[key + "out_dir_rows"], blob[key + "out_dir_offsets"] = rows, offsets
        blob[key + "n_candidates"], blob[key + "n_dropped"] = np.int64(n_candidates), np.int64(n_dropped)
        if count >= 2:
            tally["multi"].append(name)
        if n_candidates > count:
            tally["merged"].append(name)
        if n_dropped > 0:
            tally["dropped"].append(name)
        if periodic and count < 2 and n_candidates <= count and n_dropped == 0:
            tally["plain"].append(name)
        print("%-22s K=%3d connected %4d  components %5d  candidates %2d  pathways %2d  dropped %5d  directions %s"
              % (name, K, int(conn.sum()), int(labels.max()) + 1 if K else 0, n_candidates, count, n_dropped,
                 [sorted(tuple(int(x) for x in t) for t in d) for d in dirs]))
    # the plain mode with directions: the departure network.py documents
    try:
        DiffusionPathwayAnalysis(true_periodic_pathways=False).run(network(*cases["chain_x"][:3]), return_direction=True)
        blob["plain_direction_error"] = ""
    except Exception as e:                                       # noqa: BLE001 - the class name is the golden
        blob["plain_direction_error"] = type(e).__name__
    # coverage this file is there for
    assert tally["multi"], "no case with two or more pathways"
    assert tally["merged"], "no case where components were merged into one pathway"
    assert tally["dropped"], "no case with an edge dropped by the +-1 rule"
    assert tally["plain"], "no case without any of these"
    print("two or more pathways: %s\nmerged: %s\nnone of these: %s\nplain mode with directions: %s"
          % (tally["multi"], tally["merged"], tally["plain"], blob["plain_direction_error"]))
    path = os.path.join(GOLDEN, "pathway_known_answers.npz")
    np.savez_compressed(path, **blob)
    print("pathway_known_answers %.1f KB" % (os.path.getsize(path) / 1024.0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
