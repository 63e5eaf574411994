"""Writes ``tests/golden/replace_unassigned_known_answers.npz``: what the TRUE reference's
``ReplaceUnassignedPositions.run`` gives on the label / centre sets of ``tests/golden/merge_known_answers.npz`` (read from
there and not stored again) and on a few small label sets made here (stored as ``<case>/in_*``).  Needs the reference
(``oracle.ref_build``); without it the script says so and writes nothing.  Run from the repository root:
``python tools/make_replace_goldens.py``.

The reference's ``ReplaceUnassignedPositions()`` raises and its ``replace_with_closer()`` returns nothing (recorded
below as ``default_ctor_error`` / ``closer_factory_returns``), so every strategy is handed to the constructor: the two
static methods, a recording callable, and a closer-site callable written HERE from the docstring of
``replace_with_closer`` on the reference's own ``PBCCalculator.distances`` (it reads the position of the run's ion, that
is atom ``where(mobile_mask)[mob]`` of the real trajectory).

Layout (``<case>`` in ``names``; ``own`` lists the cases whose inputs are stored here):
  default_ctor_error, closer_factory_returns   class names: documentation of the reference's state, nothing to reproduce
  <case>/in_labels, in_centers, in_cell, in_static_mask, in_mobile_mask, in_ref_positions     (own cases only)
  <case>/unknown_positions        float64[n, 3]: the mobile ions' real-space positions at the unknown (frame, ion)
                                  entries in ``np.nonzero(labels == -1)`` order; at every known entry the ion stands on
                                  the centre of its site, every static atom on its reference position
  <case>/last, <case>/next        the output labels of replace_with_last_known / replace_with_next_known
  <case>/calls                    int64[n, 5]: (mobile_atom, before, start, after, end) of every call of the recording
                                  callable in call order; call i returns the scalar (3 i) % K when i is even and the
                                  float64 array ((start + arange(end - start)) % K) + 0.0 when it is odd
  <case>/recorded                 the output labels with that callable
  <case>/closer                   the output labels of the closer-site callable
  <case>/closer_margin            the smallest |d_before - d_after| (Angstrom) over the frames it decided (inf: none)
  <case>/kept_plain, kept_computed   does a site attribute added with computed=False / an edge attribute added with
                                  computed=True exist on the result's network
  <case>/confidences_kept         are the result's confidences the input's (the same memory, not a copy)
  <case>/real_traj_kept           is the result's real trajectory the input's (the same memory, not a copy)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

from oracle import ref_build  # noqa: E402

MARGIN = 1e-9            # Angstrom: no decided frame of the goldens may be a nearer tie than this
POSITION_SEED = 20261018


def own_cases():
    """Small label sets in a triclinic cell: {name: (labels, centers, cell, static_mask, mobile_mask, ref_positions)}."""
    cell = np.array([[7.0, 0.0, 0.0], [1.5, 6.5, 0.0], [-1.0, 0.8, 8.0]])
    rng = np.random.default_rng(7)
    out = {}

    def case(name, labels, K):
        labels = np.asarray(labels, dtype=np.int64)
        M = labels.shape[1]
        sm = np.array([True, True] + [False] * M)
        ref = rng.uniform(0.0, 1.0, size=(M + 2, 3)) @ cell
        centers = rng.uniform(0.0, 1.0, size=(K, 3)) @ cell
        out[name] = (labels, centers, cell, sm, ~sm, ref)

    u = -1
    # ion 0: a run from frame 0, before == after, a run to the last frame; ion 1: never assigned; ion 2: no run at all;
    # ion 3: single unknown frames between different sites, and one known frame between two runs
    case("edges", np.array([[u, u, 2, 2, u, u, 2, 3, u, u, u, u],
                            [u] * 12,
                            [4, 4, 4, 0, 0, 0, 1, 1, 1, 1, 1, 1],
                            [0, u, 1, u, 2, u, u, 3, u, 3, 4, u]]).T, 5)
    case("one_frame", np.array([[u, 1, u]]), 3)
    # 700 frames, 2 ions: runs over the frames 256 and 512, a run of exactly 256..511, dwells of random length
    lab = np.empty((700, 2), dtype=np.int64)
    f = 0
    site = 0
    while f < 700:
        n = int(rng.integers(1, 40))
        lab[f:f + n, 0] = site if rng.uniform() < 0.6 else u
        site = int(rng.integers(0, 6))
        f += n
    lab[:, 1] = 5
    lab[100:250, 1] = 2
    lab[256:512, 1] = u
    lab[600:, 1] = 1
    lab[650:, 1] = u
    case("chunks", lab, 6)
    return out


def real_trajectory(labels, centers, cell, mobile_mask, ref_positions, rng):
    """The layout the docstring describes; the unknown entries' positions are uniform in the cell."""
    F, M = labels.shape
    real = np.broadcast_to(ref_positions, (F,) + ref_positions.shape).copy()
    mob = np.where(mobile_mask)[0]
    unknown = labels == -1
    pos = centers[np.where(unknown, 0, labels)]
    upos = rng.uniform(0.0, 1.0, size=(int(unknown.sum()), 3)) @ cell
    pos[unknown] = upos
    real[:, mob] = pos
    return real, upos


def main():
    if not ref_build.available():
        print("reference not present; replace goldens can only be generated where it is")
        return 0
    ref_build.import_reference()
    import ase
    from sitator import SiteNetwork, SiteTrajectory
    from sitator.util import PBCCalculator
    from sitator.dynamics.ReplaceUnassignedPositions import ReplaceUnassignedPositions as RUP

    src = np.load(os.path.join(GOLDEN, "merge_known_answers.npz"), allow_pickle=False)
    cases = {}
    for name in (str(n) for n in src["names"]):
        cases[name] = tuple(src[name + "/" + k] for k in ("labels", "centers", "cell", "static_mask", "mobile_mask",
                                                          "ref_positions"))
    own = own_cases()
    cases.update(own)
    blob = {"names": np.array(list(cases)), "own": np.array(list(own))}

    try:
        RUP()
        blob["default_ctor_error"] = ""
    except Exception as e:                                   # noqa: BLE001 - the class name is the golden
        blob["default_ctor_error"] = type(e).__name__
    blob["closer_factory_returns"] = type(RUP.replace_with_closer()).__name__
    print("ReplaceUnassignedPositions() raises %s; replace_with_closer() returns %s"
          % (blob["default_ctor_error"], blob["closer_factory_returns"]))

    rng = np.random.default_rng(POSITION_SEED)
    for name, (lab, cen, cell, sm, mm, refp) in cases.items():
        K = len(cen)
        mob_atoms = np.where(mm)[0]
        at = ase.Atoms(positions=refp, numbers=np.where(mm, 3, 8), cell=cell)
        real, upos = real_trajectory(lab, cen, cell, mm, refp, rng)
        confs = np.linspace(0.0, 1.0, lab.size).reshape(lab.shape)
        if name in own:
            for k, v in zip(("labels", "centers", "cell", "static_mask", "mobile_mask", "ref_positions"),
                            (lab, cen, cell, sm, mm, refp)):
                blob["%s/in_%s" % (name, k)] = v
        blob[name + "/unknown_positions"] = upos

        def make_st():
            sn = SiteNetwork(at, sm, mm)
            sn.centers = cen.copy()
            sn.add_site_attribute("score", np.arange(K) * 0.5, computed=False)
            sn.add_edge_attribute("weight", np.arange(K * K, dtype=np.float64).reshape(K, K), computed=True)
            st = SiteTrajectory(sn, lab.copy(), confidences=confs)
            st.set_real_traj(real)
            return st

        st = make_st()
        out = RUP(RUP.replace_with_last_known).run(st)
        assert out is not st and np.array_equal(st.traj, lab)
        blob[name + "/last"] = out.traj.copy()
        blob[name + "/kept_plain"] = np.bool_(out.site_network.has_attribute("score"))
        blob[name + "/kept_computed"] = np.bool_(out.site_network.has_attribute("weight"))
        blob[name + "/confidences_kept"] = np.bool_(out.confidences is not None and np.shares_memory(out.confidences, confs)
                                                    and np.array_equal(out.confidences, confs))
        blob[name + "/real_traj_kept"] = np.bool_(out.real_trajectory is not None and np.shares_memory(out.real_trajectory, real)
                                                  and out.real_trajectory.shape == real.shape)
        blob[name + "/next"] = RUP(RUP.replace_with_next_known).run(make_st()).traj.copy()

        calls = []

        def recording(st_, mob, before, start, after, end):
            assert st_ is rec_st
            i = len(calls)
            calls.append((mob, before, start, after, end))
            if i % 2 == 0:
                return (3 * i) % K
            return ((start + np.arange(end - start)) % K) + 0.0

        rec_st = make_st()
        blob[name + "/recorded"] = RUP(recording).run(rec_st).traj.copy()
        blob[name + "/calls"] = np.array(calls, dtype=np.int64).reshape(-1, 5)

        pbcc = PBCCalculator(cell)
        margins = [np.inf]

        def closer(st_, mob, before, start, after, end):
            if before == SiteTrajectory.SITE_UNKNOWN or after == SiteTrajectory.SITE_UNKNOWN:
                return SiteTrajectory.SITE_UNKNOWN
            fill = np.empty(end - start, dtype=np.int64)
            two = st_.site_network.centers[[before, after]]
            for i in range(end - start):
                d = pbcc.distances(st_.real_trajectory[start + i, mob_atoms[mob]], two)
                if before != after:
                    margins.append(abs(d[0] - d[1]))
                fill[i] = before if d[0] < d[1] else after
            return fill

        blob[name + "/closer"] = RUP(closer).run(make_st()).traj.copy()
        blob[name + "/closer_margin"] = np.float64(min(margins))
        assert min(margins) >= MARGIN, "%s: a decided frame is a tie within %g A; choose another POSITION_SEED" % (name, MARGIN)
        print("%-16s F=%d M=%d K=%d: %d runs, %d frames decided (margin %.3g A); kept plain %s computed %s confidences %s"
              % (name, lab.shape[0], lab.shape[1], K, len(calls), len(margins) - 1, min(margins),
                 bool(blob[name + "/kept_plain"]), bool(blob[name + "/kept_computed"]), bool(blob[name + "/confidences_kept"])))
    path = os.path.join(GOLDEN, "replace_unassigned_known_answers.npz")
    np.savez_compressed(path, **blob)
    print("replace_unassigned_known_answers %.1f KB" % (os.path.getsize(path) / 1024.0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
