"""Records tests/golden/entropy_known_answers.npz: what the reference's ConfigurationalEntropy returns (or raises) on the small
label arrays of tests/entropy_ref.py.  Run by hand where a checkout of the reference is at hand, never by a test:

    python tests/make_entropy_golden.py /path/to/sitator

The reference's file is loaded by its path.  It imports ``sitator`` and ``sitator.dynamics`` for two names; stand-in modules
expose this project's ``SiteTrajectory`` and ``JumpAnalysis`` under them (``compute`` reads only ``st._traj``, ``n_frames`` and
the network's attributes).  ``total_corrected_residences`` is put on the network beforehand from ``entropy_ref.residences``, so no
GPU is needed to record; tests/test_gpu_coordenv.py pins the device's residences to the same function.  ``np.float`` is aliased:
the reference predates its removal."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import entropy_ref as ER  # noqa: E402


def network(labels, n_sites, site_types):
    from sitator_amd import SiteNetwork, SiteTrajectory, Structure
    ions = labels.shape[1]
    pos = np.random.default_rng(0).uniform(0.0, 10.0, (ions + 1, 3))
    mobile = np.array([False] + [True] * ions)
    sn = SiteNetwork(Structure(pos, np.eye(3) * 10.0), ~mobile, mobile)
    sn.centers = np.random.default_rng(1).uniform(0.0, 10.0, (n_sites, 3))
    if site_types is not None:
        sn.site_types = site_types
    sn.add_site_attribute("total_corrected_residences", ER.residences(labels, n_sites))
    return SiteTrajectory(sn, labels)


def main(reference_root):
    import sitator_amd
    if not hasattr(np, "float"):
        np.float = float
    top, dyn = types.ModuleType("sitator"), types.ModuleType("sitator.dynamics")
    top.SiteTrajectory, dyn.JumpAnalysis = sitator_amd.SiteTrajectory, sitator_amd.JumpAnalysis
    sys.modules["sitator"], sys.modules["sitator.dynamics"] = top, dyn
    path = os.path.join(reference_root, "sitator", "descriptors", "ConfigurationalEntropy.py")
    spec = importlib.util.spec_from_file_location("reference_entropy", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cases = ER.cases()
    out = {"names": np.array(json.dumps(list(cases)))}
    for name, (labels, n_sites, site_types, overshoot) in cases.items():
        st = network(labels, n_sites, site_types)
        out[name + "/labels"] = labels
        try:
            out[name + "/expected"] = np.array([float(mod.ConfigurationalEntropy(acceptable_overshoot=overshoot).compute(st))])
        except ValueError as e:
            out[name + "/raises"] = np.array(str(e))
    rng = np.random.default_rng(2)
    p2, N = rng.uniform(0.0, 1.0, 9), rng.integers(1, 6, 9)
    p2[2], p2[5] = 0.0, 1.0
    out["s_tilde/p2"], out["s_tilde/N"], out["s_tilde/n"] = p2, N, np.array([3.25])
    out["s_tilde/expected"] = np.array([float(mod.ConfigurationalEntropy().s_tilde(p2.copy(), 3.25, N))])
    np.savez_compressed(ER.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (ER.GOLDEN, os.path.getsize(ER.GOLDEN)))


if __name__ == "__main__":
    main(sys.argv[1])
