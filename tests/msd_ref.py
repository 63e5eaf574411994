"""numpy restatement of ``MeanSquaredDisplacement`` (``DESIGN.md`` section 20; the decisions of ``sitator_amd/csrc/msd_plan.h``
said once more, independently): the unwrapping, the direct sums in ``np.longdouble``, an emulation of the all-lag path
(zero-padded ``np.fft``, prefix sums of the squares in the order the header fixes), the plan's arithmetic, and the test inputs."""
import numpy as np

SIGMA = 0.05
THREADS, GROUP = 256, 4
CHUNK = THREADS * GROUP
IMAGE_LIMIT = 2.0 ** 30
MAX_BATCH = 16384

# rows are the cell vectors; every perpendicular height is at least 3
ORTHO = np.array([[4.0, 0.0, 0.0], [0.0, 3.5, 0.0], [0.0, 0.0, 5.0]])
HEX = np.array([[4.0, 0.0, 0.0], [-2.0, 2.0 * np.sqrt(3.0), 0.0], [0.0, 0.0, 3.25]])
TRICLINIC = np.array([[4.5, 0.3, -0.2], [1.1, 3.9, 0.4], [-0.7, 0.9, 4.2]])
CELLS = {"ortho": ORTHO, "hex": HEX, "triclinic": TRICLINIC}


def heights(cell):
    """The perpendicular heights of the cell: volume over the area of every face."""
    vol = abs(np.linalg.det(cell))
    return np.array([vol / np.linalg.norm(np.cross(cell[(i + 1) % 3], cell[(i + 2) % 3])) for i in range(3)])


def random_walk(n_frames, n_atoms, seed, sigma=SIGMA, drift=None):
    """``[n_frames, n_atoms, 3]``: Gaussian steps from a fixed seed (as ``tests/vibfreq_ref.py``), ``drift`` ``[3]`` per frame."""
    rng = np.random.default_rng(seed)
    steps = rng.normal(scale=sigma, size=(n_frames, n_atoms, 3))
    if drift is not None:
        steps += np.asarray(drift, dtype=np.float64)[None, None, :]
    return np.ascontiguousarray(10.0 * rng.random((1, n_atoms, 3)) + np.cumsum(steps, axis=0))


def fractional(x, cell):
    return x @ np.linalg.inv(cell)


def wrap_into(x, cell):
    """``(wrapped positions, floor of the fractional coordinates)``: what an MD code that keeps atoms in the cell writes."""
    frac = fractional(x, cell)
    fl = np.floor(frac)
    return np.ascontiguousarray((frac - fl) @ cell), fl.astype(np.int64)


# ---- the unwrapping ---------------------------------------------------------------------------------------------------

def image(f):
    """``(n, residual)`` of fractional steps ``f``: round half to even; 0 and no residual (-1) where ``f`` is not finite or
    beyond 2^30."""
    f = np.asarray(f, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(f) < IMAGE_LIMIT
    safe = np.where(ok, f, 0.0)
    n = np.rint(safe)
    return np.where(ok, n, 0.0).astype(np.int32), np.where(ok, np.abs(safe - n), -1.0)


def unwrap(x, cell):
    """``(x_u [F, n, 3], images int32 [n, F, 3], max_residual)`` of positions ``x [F, n, 3]`` under ``cell``."""
    x = np.asarray(x, dtype=np.float64)
    cm = np.ascontiguousarray(np.asarray(cell, dtype=np.float64).T)
    ci = np.linalg.inv(cm)                                        # what the context is given
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[1:] - x[:-1]
        f = np.stack([(ci[a, 0] * d[..., 0] + ci[a, 1] * d[..., 1]) + ci[a, 2] * d[..., 2] for a in range(3)], axis=-1)
    n, res = image(f)
    shift = np.concatenate([np.zeros((1,) + n.shape[1:], dtype=np.int32), -n])
    N = np.cumsum(shift, axis=0, dtype=np.int32)                  # [F, n, 3]
    Nf = N.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        moved = np.stack([x[..., a] + ((Nf[..., 0] * cm[a, 0] + Nf[..., 1] * cm[a, 1]) + Nf[..., 2] * cm[a, 2]) for a in range(3)], axis=-1)
    none = np.all(N == 0, axis=-1, keepdims=True)
    xu = np.where(none, x, moved)
    return xu, np.ascontiguousarray(N.transpose(1, 0, 2)), float(max(res.max(), 0.0)) if res.size else 0.0


def series(x, cell=None):
    """``y [n, 3, F]``: ``x_u[t] - x_u[0]`` (``cell=None``: no unwrapping)."""
    xu = np.asarray(x, dtype=np.float64) if cell is None else unwrap(x, cell)[0]
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray((xu - xu[:1]).transpose(1, 2, 0))


def collective_series(y):
    """``Y [1, 3, F]``: the atoms of ``y [n, 3, F]`` added in order."""
    Y = y[0].copy()
    for i in range(1, len(y)):
        Y = Y + y[i]
    return Y[None]


# ---- the sums themselves ----------------------------------------------------------------------------------------------

def msd_direct(y, lags):
    """``(msd [n, 3, n_lags], r4 [n, n_lags])`` in ``np.longdouble``, by the definition; lag 0 is 0."""
    y = np.asarray(y, dtype=np.longdouble)
    n, _, F = y.shape
    msd = np.zeros((n, 3, len(lags)), dtype=np.longdouble)
    r4 = np.zeros((n, len(lags)), dtype=np.longdouble)

    def some(which):
        for l in which:
            tau = int(lags[l])
            if tau == 0:
                continue
            sq = y[:, :, tau:] - y[:, :, :F - tau]
            np.multiply(sq, sq, out=sq)
            msd[:, :, l] = np.sum(sq, axis=2) / (F - tau)
            q = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
            np.multiply(q, q, out=q)
            r4[:, l] = np.sum(q, axis=1) / (F - tau)

    if len(lags) * F * n < 4000000:
        some(range(len(lags)))
    else:
        # every lag is a sum of its own: the lags dealt out to a few threads (numpy's loops run without the interpreter lock)
        from concurrent.futures import ThreadPoolExecutor
        workers = 8
        with ThreadPoolExecutor(workers) as pool:
            list(pool.map(some, [range(w, len(lags), workers) for w in range(workers)]))
    return msd, r4


def sum_squares(y):
    """``sum_t y[t]^2`` per series, ``[n, 3]``, in ``np.longdouble``: the unit of the all-lag bound."""
    y = np.asarray(y, dtype=np.longdouble)
    return np.sum(y * y, axis=2)


# ---- the all-lag path --------------------------------------------------------------------------------------------------

def n_chunks(F):
    return (F + CHUNK - 1) // CHUNK


def prefix_squares(y):
    """``P [F + 1]`` of one series, ``P[k] = sum_{t<k} y[t]^2``, in the order ``msd_plan.h`` fixes: chunks of 1024; inside a
    chunk groups of four consecutive elements summed one after the other, a Hillis-Steele scan of the 256 group totals, the
    chunk totals added up one after the other; an element is ``offset + (groups before + local)``."""
    y = np.asarray(y, dtype=np.float64)
    F = len(y)
    nc = n_chunks(F)
    q = np.zeros(nc * CHUNK)
    q[:F] = y * y
    q = q.reshape(nc, THREADS, GROUP)
    local = np.empty_like(q)
    local[..., 0] = q[..., 0]
    for i in range(1, GROUP):
        local[..., i] = local[..., i - 1] + q[..., i]
    g = local[..., GROUP - 1].copy()                              # [nc, 256]
    d = 1
    while d < THREADS:
        nxt = g.copy()
        nxt[:, d:] = g[:, :-d] + g[:, d:]
        g = nxt
        d *= 2
    before = np.concatenate([np.zeros((nc, 1)), g[:, :-1]], axis=1)
    offset = np.zeros(nc)
    run = 0.0
    for c in range(nc):
        offset[c] = run
        run = g[c, -1] if c == 0 else run + g[c, -1]
    incl = offset[:, None, None] + (before[:, :, None] + local)
    P = np.zeros(F + 1)
    P[1:] = incl.reshape(-1)[:F]
    return P


def s1(P, F, tau):
    tau = np.asarray(tau)
    return (P[F - tau] + (P[F] - P[tau])) / (F - tau).astype(np.float64)


def padded_length(F):
    m = 1
    while (1 << m) < 2 * F - 1:
        m += 1
    return 1 << m


def msd_fft_emulation(y, n_lags):
    """The all-lag path of one series in numpy: the same algorithm class (float64 power-of-two transform of the
    zero-padded series, ``|X|^2``, inverse; S1 from ``prefix_squares``), not the same operations."""
    y = np.asarray(y, dtype=np.float64)
    F = len(y)
    M = padded_length(F)
    X = np.fft.fft(y, M)
    acf = np.fft.ifft(X.real * X.real + X.imag * X.imag).real[:n_lags]
    tau = np.arange(n_lags)
    out = s1(prefix_squares(y), F, tau) - 2.0 * acf / (F - tau)
    out[0] = 0.0
    return out


# ---- the plan -----------------------------------------------------------------------------------------------------------

def round256(v):
    return (v + 255) // 256 * 256


def atom_bytes(F, n_lags, direct):
    """Workspace of one atom (``msd_plan``): per series y, the images, P, the chunk totals, the transform's points, the
    results; the fourth moment is a fourth row of results."""
    out = round256(n_lags * 8)
    per = round256(F * 8) + round256(F * 4) + (0 if direct else round256((F + 1) * 8)) + round256(n_chunks(F) * 8) \
        + (0 if direct else padded_length(F) * 16) + out
    return 3 * per + (out if direct else 0)


def fixed_bytes(F, collective):
    return 3 * round256(F * 8) if collective else 0


def batch(F, n_sel, n_lags, direct, collective, cap):
    """``(atoms per batch, batches)``; ``None`` where the cap is below one atom."""
    b = (cap - fixed_bytes(F, collective)) // atom_bytes(F, n_lags, direct)
    if cap < fixed_bytes(F, collective) or b < 1:
        return None
    b = min(b, MAX_BATCH, n_sel)
    return b, (n_sel + b - 1) // b
