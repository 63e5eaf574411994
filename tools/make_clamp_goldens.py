"""Writes ``tests/golden/clamped_known_answers.npz``: what the TRUE reference's ``GenerateClampedTrajectory.run`` gives on
all-mobile structures - the only ones it runs on.  Needs the reference (``oracle.ref_build``); without it the script says
so and writes nothing.  Run from the repository root: ``python tools/make_clamp_goldens.py``.

The stock build leaves ``misc/GenerateClampedTrajectory.pyx`` out because Cython 3 rejects it (``:117``: ``10**(2 - dim)``
is a float there).  With the directive ``cpow=True`` (C semantics of ``**``, Cython 0.29's) it compiles unchanged, so this
script cythonizes that one module, in the scratch tree of ``ref_build.build()`` and nowhere else.

Layout (``<case>`` in ``names``: two cells x two sizes):
  static_atom_error            class name of what the reference raises on a structure with a static atom (documentation)
  empty_mask_error             ... for a clamp mask that selects no mobile atom
  unassigned_error             ... for an unassigned label with pass_through_unassigned=False
  partial_no_real_error        ... for a partial mask on a trajectory without a real trajectory
  <case>/in_cell, in_centers [K, 3], in_positions [F, M, 3] (the real trajectory), in_ref_positions [M, 3] (the structure),
  <case>/in_labels [F, M] (no unassigned entry), in_labels_unassigned [F, M] (one single frame, one whole column, the first
                               and the last frame of another column), in_partial_mask [M]
  <case>/out_<labels key>_w<wrap>p<pass_through_unassigned>   float64 [F, M, 3]; absent where the reference raises
  <case>/out_partial           in_labels_unassigned, wrap=False, pass_through_unassigned=True, clamp_mask=in_partial_mask
  <case>/out_no_real           in_labels, wrap=True, no real trajectory set
  <case>/margin_image          the smallest gap (Angstrom) between the nearest and the second nearest of the 27 images
  <case>/margin_floor          the smallest distance (cell units) of a crystal coordinate that is floored to an integer
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

from oracle import ref_build  # noqa: E402
from tests import clamp_ref as CR  # noqa: E402

MARGIN = 1e-9            # Angstrom / cell units: no decision of the goldens may be nearer to a tie than this
SEED = 20261018
MODULE = os.path.join("sitator", "misc", "GenerateClampedTrajectory.pyx")


def build_clamp_module():
    """The one extra module, next to the ones ``ref_build.build()`` made."""
    root = ref_build.build()
    stamp = os.path.join(root, ".built_clamp")
    if os.path.exists(stamp):
        return root
    script = (
        "import numpy as np, Cython.Compiler.Options as O\n"
        "O.cimport_from_pyx = True\n"
        "from setuptools import setup\n"
        "from Cython.Build import cythonize\n"
        "setup(name='sitator_ref_clamp', script_args=['build_ext', '--inplace', '-q'],\n"
        "      ext_modules=cythonize([%r], language_level=3, quiet=True, compiler_directives={'cpow': True}),\n"
        "      include_dirs=[np.get_include()])\n" % MODULE)
    subprocess.check_call([sys.executable, "-c", script], cwd=root, stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT)
    open(stamp, "w").write("ok\n")
    return root


def error_name(fn):
    try:
        fn()
    except Exception as e:                                       # noqa: BLE001 - the class name is the golden
        return type(e).__name__
    return ""


def main():
    if not ref_build.available():
        print("reference not present; clamp goldens can only be generated where it is")
        return 0
    build_clamp_module()
    ref_build.import_reference()
    import ase
    from sitator import SiteNetwork, SiteTrajectory
    from sitator.misc.GenerateClampedTrajectory import GenerateClampedTrajectory as GCT

    def make_st(cell, ref_positions, centers, labels, real, n_static=0):
        n = len(ref_positions)
        sm = np.arange(n) < n_static
        at = ase.Atoms(positions=ref_positions, numbers=np.where(sm, 8, 3), cell=cell)
        sn = SiteNetwork(at, sm, ~sm)
        sn.centers = centers.copy()
        st = SiteTrajectory(sn, labels.copy())
        if real is not None:
            st.set_real_traj(real)
        return st

    blob = {}
    names = []
    seed = SEED
    for cname, cell in (("triclinic", CR.TRICLINIC), ("ortho", CR.ORTHO)):
        for sname, (F, M, K) in (("big", (300, 5, 6)), ("one", (1, 1, 1))):
            name = "%s_%s" % (cname, sname)
            names.append(name)
            seed += 1
            centers, labels, positions = CR.designed(cell, F, M, K, seed)
            ref_positions = np.random.default_rng(seed + 7).uniform(size=(M, 3)) @ cell
            un = labels.copy()
            if F > 1:
                un[17, 1] = -1                                   # a single frame
                un[:, 3] = -1                                    # a whole column
                un[0, 0] = un[-1, 0] = -1                        # the first and the last frame
            else:
                un[:] = -1
            partial = np.arange(M) % 2 == 0
            m_img, m_floor = CR.margins(cell, centers, labels, positions)
            assert m_img >= MARGIN and m_floor >= MARGIN, "%s: a decision within %g of a tie; choose another SEED" % (name, MARGIN)
            for k, v in (("cell", cell), ("centers", centers), ("positions", positions), ("ref_positions", ref_positions),
                         ("labels", labels), ("labels_unassigned", un), ("partial_mask", partial)):
                blob["%s/in_%s" % (name, k)] = v
            blob[name + "/margin_image"] = np.float64(m_img)
            blob[name + "/margin_floor"] = np.float64(m_floor)
            for key, lab in (("labels", labels), ("labels_unassigned", un)):
                for w, p in CR.COMBOS:
                    try:
                        out = GCT(wrap=w, pass_through_unassigned=p).run(make_st(cell, ref_positions, centers, lab, positions))
                    except RuntimeError:
                        assert key == "labels_unassigned" and not p
                        continue
                    assert out.dtype == np.float64 and out.shape == (F, M, 3)
                    blob["%s/out_%s_w%dp%d" % (name, key, w, p)] = out
            blob[name + "/out_partial"] = GCT(wrap=False, pass_through_unassigned=True).run(
                make_st(cell, ref_positions, centers, un, positions), clamp_mask=partial)
            blob[name + "/out_no_real"] = GCT(wrap=True).run(make_st(cell, ref_positions, centers, labels, None))
            print("%-16s F=%d M=%d K=%d: image margin %.3g A, floor margin %.3g" % (name, F, M, K, m_img, m_floor))

    # the reference's errors, on the first case
    i = {k: blob["%s/in_%s" % (names[0], k)] for k in ("cell", "centers", "positions", "ref_positions", "labels",
                                                       "labels_unassigned", "partial_mask")}
    static_ref = np.concatenate([i["ref_positions"][:1], i["ref_positions"]])
    static_real = np.concatenate([i["positions"][:, :1], i["positions"]], axis=1)
    blob["static_atom_error"] = error_name(lambda: GCT(wrap=True).run(
        make_st(i["cell"], static_ref, i["centers"], i["labels"], static_real, n_static=1)))
    blob["empty_mask_error"] = error_name(lambda: GCT(wrap=True).run(
        make_st(i["cell"], i["ref_positions"], i["centers"], i["labels"], i["positions"]),
        clamp_mask=np.zeros(len(i["ref_positions"]), dtype=bool)))
    blob["unassigned_error"] = error_name(lambda: GCT().run(
        make_st(i["cell"], i["ref_positions"], i["centers"], i["labels_unassigned"], i["positions"])))
    blob["partial_no_real_error"] = error_name(lambda: GCT(wrap=True).run(
        make_st(i["cell"], i["ref_positions"], i["centers"], i["labels"], None), clamp_mask=i["partial_mask"]))
    print("errors: static atom %s, empty mask %s, unassigned %s, partial mask without a real trajectory %s"
          % tuple(blob[k] for k in ("static_atom_error", "empty_mask_error", "unassigned_error", "partial_no_real_error")))
    blob["names"] = np.array(names)
    path = os.path.join(GOLDEN, "clamped_known_answers.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    print("clamped_known_answers %.1f KB" % (size / 1024.0))
    assert size < 300 * 1024
    return 0


if __name__ == "__main__":
    sys.exit(main())
