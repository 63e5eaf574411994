"""TEST INFRASTRUCTURE ONLY - inputs and references for dynamic lattice mapping with maps that are not the identity.

Take a trajectory whose static atoms stay within the movement threshold and permute the static atoms of every frame, with
another permutation in every frame.  The reference's mapping (landmark/helpers.pyx:60-64) undoes the permutation, so the
rows of the permuted frames WITH mapping are the rows of the unpermuted frames WITHOUT it - two references, neither of
them the code under test: the oracle with mapping on the permuted frames, the oracle without mapping on the unpermuted
ones.  ``tests/test_dynmap_ref.py`` asserts that the two agree bit for bit for every input below (no argmin went to a
neighbour), ``tests/test_gpu_dynamic_mapping.py`` holds the kernels against both.
"""
import functools
import types

import numpy as np

SEED, PERM_SEED = 19, 5

# (cfg, M, F, permutation mode, fill kernel): the smallest shapes that reach each path of the kernels that read the map
ROW_CASES = [
    ("C2", 64, 12, "all", 3),        # diagonal cell, S = 512 > 256: the strided loops of k_lattice_map run twice
    ("C2", 64, 12, "mixed", 3),
    ("C2", 64, 12, "rotate", 3),
    ("C1d", 4, 40, "all", 3),        # diagonal cell, several frames per workgroup (asserted by the GPU test)
    ("C1b", 4, 40, "rotate", 3),     # triclinic cell, V = 4, D = 324
    ("C5", 160, 6, "all", 3),        # ragged V = 4 / 6
    ("C2t", 64, 6, "mixed", 3),      # general cell at S = 512
    ("C3", 448, 4, "all", 3),        # S = 1088: no multiple of 256
    ("C2", 64, 12, "all", 1),        # k_fill_rows<true, false>
]
OPERATOR_CASES = [("C1d", 4, 300, "all"), ("C1b", 4, 300, "all")]

# the tight / loose split: two static atoms (lattice sites >= 256) far beyond the jitter, below static_movement_threshold
SPLIT_SHOVES = ((2, 300, (0.6, 0.0, 0.0)), (7, 411, (0.0, -0.45, 0.4)))


def permute_statics(frames, sidx, seed, mode):
    """``(pf, perms)``: ``pf[f, sidx] = frames[f, sidx[perms[f]]]``, every other atom as it was.

    ``"all"``: a fresh random permutation in every frame.  ``"mixed"``: the identity in the frames with ``f % 3 == 0``,
    random otherwise (consecutive frames of a workgroup have different maps, the displacement sample sees some valid
    frames).  ``"rotate"``: ``roll(arange(S), f + 1)`` - never the identity, another map in every frame, and a wrong frame
    index gives an atom that is in range but wrong."""
    frames = np.asarray(frames)
    sidx = np.asarray(sidx)
    S = len(sidx)
    rng = np.random.default_rng(seed)
    perms = np.empty((len(frames), S), dtype=np.int64)
    for f in range(len(frames)):
        if mode == "all":
            perms[f] = rng.permutation(S)
        elif mode == "mixed":
            perms[f] = np.arange(S) if f % 3 == 0 else rng.permutation(S)
        elif mode == "rotate":
            perms[f] = np.roll(np.arange(S), f + 1)
        else:
            raise KeyError(mode)
    pf = np.array(frames, dtype=np.float64, order="C")
    for f in range(len(frames)):
        pf[f, sidx] = frames[f, sidx[perms[f]]]
    return pf, perms


def matched_dmax(oracle, cell, ref_static, frames, sidx):
    """Per frame the largest distance from a static atom to its OWN lattice position, on the unpermuted frames: what
    ``frame_dmax`` (k_lattice_map) must hold for the permuted ones."""
    wrapped = oracle.wrap_points(cell, np.asarray(frames)[:, sidx])
    out = np.zeros(len(wrapped))
    for f in range(len(wrapped)):
        for li in range(len(sidx)):
            out[f] = max(out[f], oracle.distances(cell, ref_static[li], wrapped[f, li][None, :])[0])
    return out


def expected_delta(dmax_own, static_thr=1.0):
    """The bound that ensure_tight_table / sample_static_dmax (csrc/fill.hip) derive from the own-index displacement of
    every frame, restated here with the host's constants (1.15, 0.02, every frame sampled below 2048 frames): frames
    beyond the threshold - the permuted ones - are left out; none left gives the floor.  Used by tests/test_dynmap_ref.py
    alone, to show that the split input has a margin; the GPU test takes delta from the context."""
    ok = dmax_own[dmax_own <= static_thr]
    return min((ok.max() if len(ok) else 0.0) * 1.15 + 0.02, static_thr)


def shove_for_split(frames, sidx):
    for f, s, d in SPLIT_SHOVES:
        frames[f, sidx[s]] += np.asarray(d)


@functools.lru_cache(maxsize=None)
def case(cfg, M, F, mode, shove=False):
    """One input, made once per process and left alone: the synthetic trajectory (seed 19), its statics permuted
    (seed 5) after the optional shoves, and the basis as the oracle computes it."""
    from oracle import oracle
    from sitator_amd import synth
    host = synth.config_host(cfg)
    frames, sm, mm, ref = synth.make_trajectory(host, M, F, seed=SEED)
    sidx, midx = np.where(sm)[0], np.where(mm)[0]
    if shove:
        shove_for_split(frames, sidx)
    pf, perms = permute_statics(frames, sidx, PERM_SEED, mode)
    ref_static = ref[sm]
    verts, vcd = oracle.site_vertex_distances(host.cell, host.centers, host.vertices, ref_static)
    c = types.SimpleNamespace(cfg=cfg, host=host, cell=host.cell, frames=frames, pf=pf, perms=perms, sm=sm, mm=mm, ref=ref,
                              sidx=sidx, midx=midx, ref_static=ref_static, verts=verts, vcd=vcd, S=len(sidx), M=M, F=F)
    for a in (frames, pf, perms, verts, vcd, ref_static):
        a.flags.writeable = False
    return c


def oracle_fill(c, frames, **kw):
    """The oracle's ``(rows, n_all_zero)`` of ``frames`` on the basis of case ``c`` (``check_for_zeros=False``)."""
    from oracle import oracle
    kw.setdefault("check_for_zeros", False)
    return oracle.fill(c.cell, oracle.wrap_points(c.cell, frames), c.sidx, c.midx, c.ref_static, c.verts, c.vcd, **kw)


@functools.lru_cache(maxsize=None)
def references(cfg, M, F, mode, shove=False):
    """``(rows, n_all_zero)`` twice: the oracle with mapping on the permuted frames, without on the unpermuted ones."""
    c = case(cfg, M, F, mode, shove)
    mapped = oracle_fill(c, c.pf, dynamic_lattice_mapping=True)
    plain = oracle_fill(c, c.frames)
    mapped[0].flags.writeable = False
    plain[0].flags.writeable = False
    return mapped, plain


# ---- the error contract of k_lattice_map at S > 256 ----------------------------------------------------------------------

ERROR_CASES = [("C2", 64, 8), ("C3", 448, 8)]
PUSH = np.array([1.5, 0.0, 0.0])          # beyond static_movement_threshold = 1.0, short of the neighbouring site (>= 3.25 A away)


@functools.lru_cache(maxsize=None)
def threshold_case(cfg, M, F):
    """Frame 3: the atoms of lattice sites S - 3 and S - 4 beyond the threshold; frame 6: the atom of site 1.  The first
    offender in the reference's order is (3, S - 4)."""
    c = case(cfg, M, F, "all")
    bad = c.frames.copy()
    bad[3, c.sidx[c.S - 3]] += PUSH
    bad[3, c.sidx[c.S - 4]] += PUSH
    bad[6, c.sidx[1]] += PUSH
    pf, perms = permute_statics(bad, c.sidx, PERM_SEED, "all")
    pf.flags.writeable = False
    return c, pf, perms


def unassigned_sites(S):
    """(a, b): two lattice sites >= 256 that are no neighbours."""
    return S - 7, 300


@functools.lru_cache(maxsize=None)
def unassigned_case(cfg, M, F):
    """Frame 4: static atom a sits on top of atom b (0.3 A beside it).  Nobody's nearest atom is a: with a loose threshold
    the frame has an unassigned atom (its index in the PERMUTED order is ``where(perms[4] == a)``); with the default
    threshold lattice site a is a threshold error as well, which the reference reports first."""
    c = case(cfg, M, F, "all")
    a, b = unassigned_sites(c.S)
    bad = c.frames.copy()
    bad[4, c.sidx[a]] = bad[4, c.sidx[b]] + np.array([0.3, 0.0, 0.0])
    pf, perms = permute_statics(bad, c.sidx, PERM_SEED, "all")
    pf.flags.writeable = False
    return c, pf, perms, a
