"""numpy restatement of ``VanHoveCorrelation`` (``DESIGN.md`` section 21; the decisions of ``sitator_amd/csrc/vanhove_plan.h``
said once more, independently): the same float64 operations in the same order, the bin by ``np.searchsorted`` on the squared
edges, and the overflow entry.  The unwrapping of the self part is that of ``tests/msd_ref.py``."""
import numpy as np

from tests import msd_ref as R

THREADS, WAVE, WAVES = 256, 64, 4
MAX_BINS, MAX_ATOMS = 2048, 1 << 20
TARGET_PAIRS, MAX_PAIRS = 1 << 20, 1 << 31
MAX_FRAC = 1 << 36
SELF_RUN = 4096
MARGIN = 1.0 - 2.0 ** -30


def n_origins(F, tau, stride):
    return (F - 1 - tau) // stride + 1


def hmin(cell):
    """The smallest perpendicular height as the library takes it: 1 / |row of inverse(cell^T)|."""
    ci = np.linalg.inv(np.ascontiguousarray(np.asarray(cell, dtype=np.float64).T))
    return float(np.min(1.0 / np.sqrt(ci[:, 0] * ci[:, 0] + ci[:, 1] * ci[:, 1] + ci[:, 2] * ci[:, 2])))


def rmax_ok(r_max, h):
    return bool(r_max > 0.0 and np.isfinite(h) and h > 0.0 and r_max <= 0.5 * h * MARGIN)


def edges2(r_max, n_bins):
    e = np.arange(n_bins, dtype=np.float64) * (r_max / n_bins)
    return np.concatenate([e * e, [r_max * r_max]])


def bin_of(r2, e2):
    """Bin ``k`` holds ``e2[k] <= r2 < e2[k + 1]``; everything else - NaN, infinity, ``r2 >= e2[-1]`` - is ``n_bins``."""
    n_bins = len(e2) - 1
    k = np.searchsorted(e2, r2, "right") - 1
    return np.where((k < 0) | (k > n_bins), n_bins, k)


def histogram(r2, e2):
    return np.bincount(bin_of(np.asarray(r2).reshape(-1), e2), minlength=len(e2)).astype(np.uint64)


def cell_matrices(cell):
    cm = np.ascontiguousarray(np.asarray(cell, dtype=np.float64).T)
    return cm, np.linalg.inv(cm)                                   # what the context is given


def fractional(x, ci):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(ci[a, 0] * x[..., 0] + ci[a, 1] * x[..., 1]) + ci[a, 2] * x[..., 2] for a in range(3)], axis=-1)


def image_r2(ds, cm):
    """Squared length of the minimum image of the fractional differences ``ds [..., 3]``."""
    with np.errstate(invalid="ignore", over="ignore"):
        ds = ds - np.rint(ds)
        d = [(ds[..., 0] * cm[i, 0] + ds[..., 1] * cm[i, 1]) + ds[..., 2] * cm[i, 2] for i in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def distinct(x, cell, a, b, same, lags, stride, r_max, n_bins):
    """uint64 ``[n_lags, n_bins + 1]`` of the frames ``x [F, A, 3]`` as they are."""
    x = np.asarray(x, dtype=np.float64)
    cm, ci = cell_matrices(cell)
    e2 = edges2(r_max, n_bins)
    s = fractional(x, ci)
    sa, sb = s[:, a], s[:, b]
    keep = ~np.eye(len(a), dtype=bool) if same else None
    out = np.zeros((len(lags), n_bins + 1), dtype=np.uint64)
    F = len(x)
    step = max(1, 4000000 // (len(a) * len(b) * 3))
    for l, tau in enumerate(lags):
        ts = np.arange(0, F - tau, stride)
        for i in range(0, len(ts), step):
            t = ts[i:i + step]
            with np.errstate(invalid="ignore"):
                ds = sb[t + tau][:, None, :, :] - sa[t][:, :, None, :]
            r2 = image_r2(ds, cm)
            out[l] += histogram(r2[:, keep] if same else r2, e2)
    return out


def self_part(x, cell, a, lags, stride, r_max, n_bins, unwrap=True):
    """``(uint64 [n_lags, n_bins + 1], max_residual)``: the displacements of the atoms ``a`` of ``x [F, A, 3]``."""
    sel = np.ascontiguousarray(np.asarray(x, dtype=np.float64)[:, a])
    if unwrap:
        y, res = R.series(sel, cell), R.unwrap(sel, cell)[2]
    else:
        y, res = np.ascontiguousarray(sel.transpose(1, 2, 0)), 0.0
    e2 = edges2(r_max, n_bins)
    out = np.zeros((len(lags), n_bins + 1), dtype=np.uint64)
    F = len(sel)
    for l, tau in enumerate(lags):
        t = np.arange(0, F - tau, stride)
        with np.errstate(invalid="ignore", over="ignore"):
            d = y[:, :, t + tau] - y[:, :, t]
            r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        out[l] = histogram(r2, e2)
    return out, res


# ---- the plan -----------------------------------------------------------------------------------------------------------

def split(n_a, n_b):
    """``(origins per workgroup, atoms of b per workgroup, tiles of b, pairs per workgroup)`` of the distinct kernel."""
    item, chunks = n_a * WAVE, (n_b + WAVE - 1) // WAVE
    items = min(max(TARGET_PAIRS // item, WAVES), MAX_PAIRS // item)
    run, span = (1, items * WAVE) if chunks >= items else (items // chunks, chunks * WAVE)
    return run, span, (n_b + span - 1) // span, run * n_a * span


def window(F, n_a, n_b, cap):
    """Frames whose fractional coordinates fit ``cap``; ``None`` below one."""
    w = (cap - 512) // ((n_a + n_b) * 24) if cap > 512 else 0
    return None if w < 1 else min(F, w, MAX_FRAC // max(n_a, n_b))


def self_batch(F, n_a, unwrap, cap):
    atom = 3 * (R.round256(F * 8) + (R.round256(F * 4) + R.round256(R.n_chunks(F) * 8) if unwrap else 0))
    b = (cap - 768) // atom if cap > 768 else 0
    return None if b < 1 else min(b, R.MAX_BATCH, n_a)


def lds_bytes(n_bins, copies):
    return (n_bins + 1) * 8 + (((n_bins + 1) * 4 * copies + 7) & ~7) + WAVES * 3 * WAVE * 8
