"""Shared by tests/test_clamp_ref.py, tests/test_clamp_point.py (CPU) and tests/test_gpu_clamped.py (GPU): a numpy
restatement of ``GenerateClampedTrajectory`` written for this project (every sum left to right, numpy's elementwise
multiply / add / floor / sqrt: IEEE operations without contraction), the two margins that make its image decision safe,
designed inputs, and the goldens of the TRUE reference (tests/golden/clamped_known_answers.npz)."""
import numpy as np

from tests import golden_util as G

MARGIN = 1e-9            # Angstrom (image distances) / cell units (crystal coordinates next to an integer)
TRICLINIC = np.array([[7.0, 0.0, 0.0], [1.5, 6.5, 0.0], [-1.0, 0.8, 8.0]])
ORTHO = np.array([[6.0, 0.0, 0.0], [0.0, 7.5, 0.0], [0.0, 0.0, 9.0]])
COMBOS = [(False, False), (False, True), (True, False), (True, True)]          # (wrap, pass_through_unassigned)

UNASSIGNED_MSG = ("The mobile atoms indicated for clamping are unassigned at some point during the trajectory and "
                  "`pass_through_unassigned` is set to False. Try `assign_to_last_known_site()`?")


# ---- the arithmetic -------------------------------------------------------------------------------------------------------

def cell_matrices(cell):
    """(cm, ci) as the reference's PBCCalculator makes them (and ``HipContext``): cell.T and numpy's inverse of it."""
    cell = np.asarray(cell, dtype=np.float64)
    return np.ascontiguousarray(cell.T), np.ascontiguousarray(np.linalg.inv(cell.T))


def _mat(m, p):
    p = np.asarray(p, dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([(m[d, 0] * x + m[d, 1] * y) + m[d, 2] * z for d in range(3)], axis=-1)


def to_cell(cell, p):
    return _mat(cell_matrices(cell)[1], p)


def to_real(cell, b):
    return _mat(cell_matrices(cell)[0], b)


def wrap(cell, p):
    """(wrapped points, floor of their crystal coordinates)."""
    b = to_cell(cell, p)
    fl = np.floor(b)
    return to_real(cell, b - fl), fl


def images(cell):
    """[27, 3]: (i - 1) cell[0] + (j - 1) cell[1] + (k - 1) cell[2], i outermost."""
    cell = np.asarray(cell, dtype=np.float64)
    out = np.empty((27, 3))
    for i in range(3):
        for j in range(3):
            for k in range(3):
                for d in range(3):
                    out[9 * i + 3 * j + k, d] = (float(i - 1) * cell[0, d] + float(j - 1) * cell[1, d]) + float(k - 1) * cell[2, d]
    return out


def image_distances(cell, ref, pt):
    """[..., 27]: the distance of every image of ``pt`` to ``ref`` as ``min_image`` computes it."""
    img = images(cell)
    out = np.empty(np.shape(ref)[:-1] + (27,))
    for m in range(27):
        b = (pt + img[m]) - ref
        b = b * b
        out[..., m] = np.sqrt((b[..., 0] + b[..., 1]) + b[..., 2])
    return out


def clamp_points(cell, centers, labels, positions):
    """wrap = False for assigned labels: ``labels[...]`` in [0, K), ``positions[..., 3]`` -> the nearest image of the centre."""
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    w, fl = wrap(cell, positions)
    wrapped_centers, _ = wrap(cell, centers)
    dist = image_distances(cell, w, wrapped_centers[labels])
    m = np.argmin(dist, axis=-1)                                   # the first minimum, as the strict < of the loop
    mic = np.stack([m // 9 - 1, m // 3 % 3 - 1, m % 3 - 1], axis=-1)
    pt_in_image = fl.astype(np.int64) + mic
    return to_real(cell, to_cell(cell, centers)[labels] + pt_in_image.astype(np.float64))


def margins(cell, centers, labels, positions):
    """(gap between the two smallest image distances, distance of a floored crystal coordinate to an integer): the
    smallest over the assigned entries (inf: none)."""
    labels = np.asarray(labels)
    sel = labels >= 0
    if not np.any(sel):
        return np.inf, np.inf
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    pos, lab = np.asarray(positions)[sel], labels[sel]
    w, _ = wrap(cell, pos)
    wc, _ = wrap(cell, centers)
    dist = np.sort(image_distances(cell, w, wc[lab]), axis=-1)
    crystal = np.concatenate([to_cell(cell, pos).ravel(), to_cell(cell, centers[np.unique(lab)]).ravel()])
    return float(np.min(dist[:, 1] - dist[:, 0])), float(np.min(np.abs(crystal - np.round(crystal))))


def clamp_mobile(cell, centers, labels, positions, wrap_mode, pass_through):
    """The all-mobile operator: labels [F, M], positions [F, M, 3] (or None where none is needed) -> [F, M, 3]."""
    labels = np.asarray(labels)
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    unknown = labels == -1
    if np.any(unknown) and not pass_through:
        raise RuntimeError(UNASSIGNED_MSG)
    if np.any(labels >= len(centers)):
        raise IndexError("index %d is out of bounds for axis 0 with size %d" % (labels.max(), len(centers)))
    if np.any(labels < -1):
        raise ValueError("a label below -1")
    out = np.empty(labels.shape + (3,))
    known = ~unknown
    if wrap_mode:
        out[known] = centers[labels[known]]
    else:
        out[known] = clamp_points(cell, centers, labels[known], np.asarray(positions)[known])
    if np.any(unknown):
        out[unknown] = np.asarray(positions)[unknown]
    return out


def clamp(cell, structure_positions, mobile_mask, centers, labels, real, clamp_mask, wrap_mode, pass_through):
    """The operator on a structure with static atoms in any order: the label column of a mobile atom is its rank among the
    mobile atoms.  ``real``: [F, A, 3] or None."""
    mobile_mask = np.asarray(mobile_mask, dtype=bool)
    A = len(mobile_mask)
    clamp_mask = np.ones(A, dtype=bool) if clamp_mask is None else np.asarray(clamp_mask, dtype=bool)
    labels = np.asarray(labels)
    F = len(labels)
    out = np.empty((F, A, 3))
    if not np.all(clamp_mask):
        out[:, ~clamp_mask] = real[:, ~clamp_mask]
    out[:, clamp_mask & ~mobile_mask] = np.asarray(structure_positions)[clamp_mask & ~mobile_mask]
    sel = clamp_mask & mobile_mask
    if np.any(sel):
        cols = (np.cumsum(mobile_mask) - 1)[sel]
        out[:, sel] = clamp_mobile(cell, centers, labels[:, cols], None if real is None else real[:, sel], wrap_mode, pass_through)
    return out


# ---- designed inputs -----------------------------------------------------------------------------------------------------

def designed(cell, F, M, K, seed, n_unknown=0):
    """(centers [K, 3] up to half a cell outside the unit cell, labels [F, M], positions [F, M, 3] up to three cells away in
    both directions) with both margins >= MARGIN (the seed is stepped until they hold)."""
    while True:
        rng = np.random.default_rng(seed)
        centers = rng.uniform(-0.5, 1.5, size=(K, 3)) @ cell
        positions = rng.uniform(-3.0, 4.0, size=(F, M, 3)) @ cell
        labels = rng.integers(0, K, size=(F, M))
        if n_unknown:
            flat = rng.choice(F * M, size=min(n_unknown, F * M), replace=False)
            labels.reshape(-1)[flat] = -1
        if min(margins(cell, centers, labels, positions)) >= MARGIN:
            return centers, labels.astype(np.int64), positions
        seed += 1000


def structure(M, n_static, layout, seed):
    """(mobile_mask [A], structure positions [A, 3] in the triclinic cell): ``layout`` first / last / interleaved says where
    the M mobile atoms stand among the n_static static ones."""
    A = M + n_static
    mobile = np.zeros(A, dtype=bool)
    if layout == "first":
        mobile[:M] = True
    elif layout == "last":
        mobile[n_static:] = True
    else:
        rng = np.random.default_rng(seed)
        mobile[rng.choice(A, size=M, replace=False)] = True
    return mobile, np.random.default_rng(seed + 1).uniform(size=(A, 3)) @ TRICLINIC


def embed(mobile_mask, structure_positions, mobile_positions, seed):
    """A real trajectory [F, A, 3]: the mobile atoms at ``mobile_positions`` (in rank order), the others near their
    structure positions."""
    F = len(mobile_positions)
    rng = np.random.default_rng(seed)
    real = structure_positions[None] + rng.normal(scale=0.05, size=(F,) + structure_positions.shape)
    real[:, mobile_mask] = mobile_positions
    return real


def network(cell, structure_positions, mobile_mask, centers):
    from sitator_amd import SiteNetwork, Structure
    mobile_mask = np.asarray(mobile_mask, dtype=bool)
    sn = SiteNetwork(Structure(np.asarray(structure_positions), cell), ~mobile_mask, mobile_mask)
    sn.centers = np.array(centers, copy=True)
    return sn


def trajectory(cell, structure_positions, mobile_mask, centers, labels, real):
    from sitator_amd import SiteTrajectory
    st = SiteTrajectory(network(cell, structure_positions, mobile_mask, centers), np.asarray(labels))
    if real is not None:
        st.set_real_traj(real)
    return st


# ---- the goldens -----------------------------------------------------------------------------------------------------------

class ClampGoldens(object):
    """tests/golden/clamped_known_answers.npz (tools/make_clamp_goldens.py documents the layout)."""

    def __init__(self):
        self.z = G.load("clamped_known_answers")
        self.names = [str(n) for n in self.z["names"]]

    def inputs(self, name):
        return {k: self.z["%s/in_%s" % (name, k)] for k in ("cell", "centers", "positions", "ref_positions", "labels",
                                                            "labels_unassigned", "partial_mask")}

    def outputs(self, name):
        """[(labels key, wrap, pass_through, clamp mask or None, with real trajectory, expected array)]"""
        out = []
        for key in ("labels", "labels_unassigned"):
            for w, p in COMBOS:
                k = "%s/out_%s_w%dp%d" % (name, key, w, p)
                if k in self.z.files:
                    out.append((key, w, p, None, True, self.z[k]))
        out.append(("labels_unassigned", False, True, self.z[name + "/in_partial_mask"], True, self.z[name + "/out_partial"]))
        out.append(("labels", True, False, None, False, self.z[name + "/out_no_real"]))
        return out
