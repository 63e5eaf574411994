"""Writes ``tests/golden/barrier_known_answers.npz``: what the TRUE reference's ``network.MergeSitesByBarrier.run`` gives on the
designed cases of ``tests/barrier_ref.py`` (``golden_case_inputs``).  Needs the reference (``oracle.ref_build``); without it the
script says so and writes nothing.  Run from the repository root: ``python tools/make_barrier_goldens.py``.

How the reference is run.  Its files and everything under ``oracle/`` stay as they are.  The stand-in ``ase.Atoms`` of
``oracle/ase_stub`` holds data only, so three methods are added to the imported class at run time: ``set_calculator`` and
``get_potential_energy`` (the latter asks the attached calculator), and an ``extend`` that also takes the single atom
``sn.structure[index]`` yields (its ``numbers`` is a scalar there).  The calculator attached is ``barrier_ref``'s brute force
over the whole structure: the last atom is the mobile one, and the lattice's own energy (``barrier_ref.lattice_energy``), a
constant, is added so that totals and not only differences go through the reference's subtraction.  ``n_ij`` is supplied as an
edge attribute: the reference's own fallback ends in ``NameError`` (it never imports ``JumpAnalysis``; recorded as
``no_n_ij_error``).  The ``mergable`` matrix is a local variable of the reference; the global ``connected_components`` of its
module is wrapped to keep a copy of what it is handed (as ``tools/make_pathway_goldens.py`` does).

Layout (``<case>`` in ``names``):
  names, kinds (JSON: kind -> the cases that show it), margin, no_n_ij_error
  <case>/cell, positions, numbers, static_mask, mobile_mask, centers, n_ij, traj, site_types, coordinating_mask (empty: none),
         lj (JSON: epsilon, sigma, rc), kw (JSON: the constructor keywords)
  <case>/out_error                        class name of what the reference raised, or ""
  <case>/out_mergable bool [K, K]         what the reference handed to connected_components
  <case>/out_group_members, out_group_offsets   the reference's merge groups, concatenated
  <case>/out_traj, out_centers, out_site_types  of the merged trajectory (no error only; site_types with check_types only)
  <case>/out_pairs int64 [P, 2], out_energies [P, n], out_abs_sums [P, n], out_n_terms [P, n]   barrier_ref: the mobile atom only
  <case>/out_totals [P, n]                the totals the reference's loop saw
  <case>/out_margins [P, 2]               |barrier - threshold| and |max interior - max end|, over max |E| of the pair
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
from tests import barrier_ref as BR  # noqa: E402


class BruteForceCalculator(object):
    """The total energy of a structure whose last atom is the mobile one."""

    def __init__(self, case):
        self.cell = case["cell"]
        self.static_pos, self.eps, self.sigma, self.rc = BR.case_arrays(case)
        self.constant = BR.lattice_energy(self.cell, self.static_pos, self.eps, self.sigma, self.rc)
        self.totals = []

    def get_potential_energy(self, atoms):
        assert len(atoms) == len(self.static_pos) + 1 and np.array_equal(atoms.positions[:-1], self.static_pos)
        total = self.constant + BR.mobile_energy(self.cell, self.static_pos, self.eps, self.sigma, self.rc, atoms.positions[-1])[0]
        self.totals.append(total)
        return total


def patch_atoms(Atoms):
    def set_calculator(self, calc):
        self._calc = calc

    def get_potential_energy(self):
        return self._calc.get_potential_energy(self)

    def extend(self, other):
        self.positions = np.concatenate([self.positions, np.asarray(other.positions, dtype=np.float64).reshape(-1, 3)])
        self.numbers = np.concatenate([self.numbers, np.atleast_1d(other.numbers)])
    Atoms.set_calculator, Atoms.get_potential_energy, Atoms.extend = set_calculator, get_potential_energy, extend


def main():
    if not ref_build.available():
        print("reference not present; barrier goldens can only be generated where it is")
        return 0
    ref_build.import_reference()
    import ase
    import importlib
    from sitator import SiteNetwork, SiteTrajectory
    module = importlib.import_module("sitator.network.MergeSitesByBarrier")
    MergeSitesByBarrier = module.MergeSitesByBarrier
    patch_atoms(ase.Atoms)

    seen = []
    scipy_components = module.connected_components

    def recording_components(graph, *args, **kwargs):
        seen.append(np.array(graph, copy=True))
        return scipy_components(graph, *args, **kwargs)
    module.connected_components = recording_components

    def trajectory(case, with_n_ij=True):
        at = ase.Atoms(positions=case["positions"], numbers=case["numbers"], cell=case["cell"])
        sn = SiteNetwork(at, case["static_mask"], case["mobile_mask"])
        sn.centers = case["centers"].copy()
        if case["site_types"] is not None:
            sn.site_types = case["site_types"].copy()
        if with_n_ij:
            sn.add_edge_attribute("n_ij", case["n_ij"].copy())
        return SiteTrajectory(sn, case["traj"].copy())

    cases = BR.golden_case_inputs()
    blob = {"names": np.array(list(cases)), "margin": np.float64(BR.MARGIN)}
    shown = {k: [] for k in BR.KINDS}
    for name, case in cases.items():
        blob.update(BR.case_to_blob(name, case))
        calc = BruteForceCalculator(case)
        st = trajectory(case)
        run_kw = {} if case["coordinating_mask"] is None else {"coordinating_mask": case["coordinating_mask"].copy()}
        del seen[:]
        groups_seen = []
        inner = MergeSitesByBarrier._get_sites_to_merge

        def keeping(self, *a, **k):
            groups_seen.append(inner(self, *a, **k))
            return groups_seen[-1]
        MergeSitesByBarrier._get_sites_to_merge = keeping
        error, out = "", None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                out = MergeSitesByBarrier(calc, **case["kw"]).run(st, **run_kw)
            except Exception as e:                               # noqa: BLE001 - the class name is the golden
                error = type(e).__name__
            finally:
                MergeSitesByBarrier._get_sites_to_merge = inner
        assert len(seen) == 1 and len(groups_seen) == 1, "the reference did not reach connected_components"
        groups = [np.asarray(g, dtype=np.int64) for g in groups_seen[0]]
        key = name + "/out_"
        blob[key + "error"] = error
        blob[key + "mergable"] = seen[0].astype(bool)
        blob[key + "group_members"] = np.concatenate(groups) if groups else np.zeros(0, dtype=np.int64)
        blob[key + "group_offsets"] = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
        if not error:
            blob[key + "traj"] = out.traj.copy()
            blob[key + "centers"] = np.asarray(out.site_network.centers)
            if case["kw"].get("check_types"):
                blob[key + "site_types"] = np.asarray(out.site_network.site_types).astype(np.int64)

        # the mobile atom's energies by barrier_ref, the margins of every decision, and the restatement against the reference
        res = BR.run_case(case)
        n = case["kw"].get("n_driven_images", 20)
        P = len(res["pairs"])
        totals = np.array(calc.totals).reshape(P, n)
        assert np.allclose(totals - calc.constant, res["energies"], rtol=0, atol=1e-9 * max(1.0, abs(calc.constant)))
        margins = np.array([BR.margins(row, case["kw"]["barrier_threshold"]) for row in res["energies"]]).reshape(P, 2)
        assert (margins >= BR.MARGIN).all(), "%s: a decision within %g of its tie: redesign the case" % (name, BR.MARGIN)
        assert res["error"] == error and np.array_equal(res["mergable"], seen[0].astype(bool)), name
        assert len(res["groups"]) == len(groups) and all(np.array_equal(a, b) for a, b in zip(res["groups"], groups)), name
        blob[key + "pairs"], blob[key + "energies"] = res["pairs"], res["energies"]
        blob[key + "abs_sums"], blob[key + "n_terms"] = res["abs_sums"], res["n_terms"]
        blob[key + "totals"], blob[key + "margins"] = totals, margins
        kinds = BR.coverage(case, res)
        for k in kinds:
            shown[k].append(name)
        print("%-24s K=%d P=%d %-28s groups %-22s lattice %9.4f  min margin %.2e  %s"
              % (name, len(case["centers"]), P, error or "ok", [g.tolist() for g in groups], calc.constant,
                 margins.min() if P else np.inf, sorted(kinds)))

    # without n_ij: the departure network.py documents
    case = cases["low_barrier"]
    try:
        MergeSitesByBarrier(BruteForceCalculator(case), **case["kw"]).run(trajectory(case, with_n_ij=False))
        blob["no_n_ij_error"] = ""
    except Exception as e:                                       # noqa: BLE001
        blob["no_n_ij_error"] = type(e).__name__
    for kind, names in shown.items():
        assert names, "no case shows: %s" % kind
    blob["kinds"] = json.dumps(shown)
    print("without n_ij the reference raises: %s" % blob["no_n_ij_error"])
    path = os.path.join(GOLDEN, "barrier_known_answers.npz")
    np.savez_compressed(path, **blob)
    print("barrier_known_answers %.1f KB" % (os.path.getsize(path) / 1024.0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
