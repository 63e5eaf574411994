"""Writes ``tests/golden/soap_averages_known_answers.npz``: what the TRUE reference's ``SOAPDescriptorAverages._get_descriptors``
(``site_descriptors/SOAP.py:248-320``) does with the vectors of a trajectory - which (frame, ion) goes to which output row with
which weight.  Needs the reference (``oracle.ref_build``); without it the script says so and writes nothing.  Run from the
repository root:

    python tools/make_soap_goldens.py

The reference's files stay as they are.  ``SOAP.py`` is loaded from its file under a stand-in for its package (the package's own
``__init__`` imports ``SiteTypeAnalysis``, which needs ``pydpc``), and ``np.int`` / ``np.bool`` reach it through a proxy in the
module's namespace.  The SOAP engine is replaced by a fake backend that returns a one-hot vector of length ``F * M`` per position,
so the returned ``descs`` IS the weight matrix ``W[row, frame * M + ion]``.

Per case ``<name>/labels [F, M]``, ``n_sites``, ``stepsize``, ``averaging`` (0: not given), ``avg_descriptors_per_site`` (0: not
given), ``real [F, A, 3]``, ``mobile_mask [A]``, ``W [R, F * M]`` and ``desc_to_site [R]``."""
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

SEED = 20261019
F, K = 40, 4
# (name, M, stepsize, averaging, avg_descriptors_per_site)
CASES = [("m3_step1_avg1", 3, 1, 1, None), ("m3_step1_avg4", 3, 1, 4, None), ("m5_step3_avg4", 5, 3, 4, None),
         ("m5_step1_avg_beyond", 5, 1, 1000, None), ("m4_step3_per_site2", 4, 3, None, 2), ("m4_step1_per_site_zero", 4, 1, None, 50),
         ("m5_step1_avg4", 5, 1, 4, None)]


class NpProxy(object):
    """numpy with the aliases numpy 1.24 removed."""
    int = int
    bool = bool

    def __getattr__(self, name):
        return getattr(np, name)


def load_soap_module(root):
    base = os.path.join(root, "sitator", "site_descriptors")
    pkg = types.ModuleType("sitator_ref_site_descriptors")
    pkg.__path__ = [base]
    sys.modules[pkg.__name__] = pkg
    spec = importlib.util.spec_from_file_location(pkg.__name__ + ".SOAP", os.path.join(base, "SOAP.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    mod.np = NpProxy()
    return mod


def designed_labels(M, seed):
    """[F, M] labels over K sites: site K - 1 is never visited, some entries are -1, and some frames put two ions on one site."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, K - 1, size=(F, M))
    labels[rng.random((F, M)) < 0.2] = -1
    for f in range(0, F, 7):
        labels[f, 0] = labels[f, M - 1] = f % (K - 1)            # two ions on one site
    labels[3] = -1                                               # a frame with nobody assigned
    return labels.astype(np.int64)


def main():
    if not ref_build.available():
        print("reference not present; SOAP goldens can only be generated where it is")
        return 0
    root = ref_build.build()
    ref_build.import_reference()
    import ase
    from sitator import SiteNetwork, SiteTrajectory
    SOAP = load_soap_module(root)

    blob, names = {}, []
    for ci, (name, M, stepsize, averaging, per_site) in enumerate(CASES):
        rng = np.random.default_rng(SEED + ci)
        labels = designed_labels(M, SEED + 100 + M)
        assert (labels == -1).any() and not (labels == K - 1).any()
        assert any(len(set(r[r >= 0])) < np.sum(r >= 0) for r in labels[::stepsize])
        S = 6
        mobile = np.zeros(M + S, dtype=bool)
        mobile[rng.choice(M + S, size=M, replace=False)] = True
        cell = np.eye(3) * 7.0
        real = rng.uniform(0.0, 7.0, size=(F, M + S, 3))
        at = ase.Atoms(positions=real[0], numbers=np.where(mobile, 3, 8), cell=cell)
        sn = SiteNetwork(at, ~mobile, mobile)
        sn.centers = rng.uniform(0.0, 7.0, size=(K, 3))
        st = SiteTrajectory(sn, labels.copy())
        st.set_real_traj(real.copy())

        where = {}
        for f in range(F):
            for m, a in enumerate(np.where(mobile)[0]):
                where[real[f, a].tobytes()] = f * M + m

        def soaper(structure, positions):
            out = np.zeros((len(positions), F * M))
            for i, p in enumerate(positions):
                out[i, where[np.asarray(p, dtype=np.float64).tobytes()]] = 1.0
            return out
        soaper.n_dim = F * M

        kw = {"stepsize": stepsize}
        if averaging is not None:
            kw["averaging"] = averaging
        else:
            kw["avg_descriptors_per_site"] = per_site
        op = SOAP.SOAPDescriptorAverages(3, backend=lambda *a: soaper, **kw)
        # (_make_structure is not run: it asks the structure for set_pbc, which the stand-in for ase.Atoms does not have)
        structure, tracer, soap_mask = sn.static_structure.copy(), 3, sn.static_mask
        W, desc_to_site = op._get_descriptors(st, structure, tracer, soap_mask, soaper)
        names.append(name)
        for k, v in (("labels", labels), ("n_sites", np.int64(K)), ("stepsize", np.int64(stepsize)), ("averaging", np.int64(averaging or 0)),
                     ("avg_descriptors_per_site", np.int64(per_site or 0)), ("real", real), ("mobile_mask", mobile), ("W", W),
                     ("desc_to_site", np.asarray(desc_to_site, dtype=np.int64))):
            blob["%s/%s" % (name, k)] = v
    blob["cases"] = np.array(names)
    path = os.path.join(GOLDEN, "soap_averages_known_answers.npz")
    np.savez_compressed(path, **blob)
    print("wrote %s (%d bytes): %s" % (path, os.path.getsize(path), ", ".join(names)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
