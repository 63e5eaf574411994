"""The numpy restatement of sitator_amd/csrc/scattering_plan.h and of the sums of scattering.hip: the same
float64 operations in the same order - every ``*``, ``+`` and ``-`` below is one rounded operation, as under -ffp-contract=off -
so that the device's raw sums are compared with ``array_equal``; and, independent of it, an ``np.longdouble`` evaluation straight
from the definition with the library's exponential, to which the restatement is held by the error model ``term_bound``."""
import numpy as np

from tests import vanhove_ref as V

THREADS = 256
MAX_H = 32
MAX_Q = 1 << 16
MAX_QBATCH = 1 << 15
MAX_ATOMS = 1 << 20
MAX_F = 1 << 29
BLOCK = 128
QTILE = 256
TILE_MAX = 64
TILE_LDS = 24576
LAG_TILE = 8
RUN = 32
MAX_LAGS_LAUNCH = 65535
MAX_FRAC = 1 << 36
DEFAULT_WORKSPACE = 1 << 30

U = 2.0 ** -53

# the correctly rounded doubles of pi^n / n!, the literals of scattering_plan.h
COS_COEFFS = [float.fromhex(v) for v in (
    "0x1.0000000000000p+0", "0x1.3bd3cc9be45dep+2", "0x1.03c1f081b5ac4p+2", "0x1.55d3c7e3cbffap+0", "0x1.e1f506891babbp-3",
    "0x1.a6d1f2a204a8cp-6", "0x1.f9d38a3763cc3p-10", "0x1.b6e24f44b128fp-14", "0x1.20c62c2f2d7f5p-18", "0x1.2a0c591af8314p-23")]
SIN_COEFFS = [float.fromhex(v) for v in (
    "0x1.921fb54442d18p+1", "0x1.4abbce625be53p+2", "0x1.466bc6775aae2p+1", "0x1.32d2cce62bd86p-1", "0x1.50783487ee782p-4",
    "0x1.e3074fde8871fp-8", "0x1.e8f434d018d63p-12", "0x1.6fadb9f155744p-16", "0x1.aaec32af93359p-21")]

# ---- the error model -------------------------------------------------------------------------------
# |sc_sincos2pi(f) - exp(2 pi i f)| <= E_SINCOS u: 1.69 u measured over 3 x 10^6 arguments, 1.02 u at the designed ones
# (test_scattering_ref.py measures both again); the bound keeps a factor of 1.48 over it.  A complex product of rounded
# operations is within sqrt(5) u of the exact one
# (Brent, Percival and Zimmermann 2007).  To first order, moduli being 1: |dP_m| <= m E_SINCOS u + (m - 1) sqrt(5) u, and the term
# is two more products: u (C0 + C1 (|h| + |k| + |l|)), the second-order part covered by the factor 1 + 2^-20.
E_SINCOS = 2.5
C0 = 2.0 * np.sqrt(5.0)
C1 = E_SINCOS + np.sqrt(5.0)


def term_bound(q_int):
    """The forward bound of the modulus of the error of one term, per q vector."""
    n = np.abs(np.asarray(q_int, dtype=np.int64)).sum(axis=-1)
    return U * (C0 + C1 * n) * (1.0 + 2.0 ** -20)


def sum_bound(q_int, n_terms):
    """Of a sum of ``n_terms`` terms added one after the other: the terms' bounds and (n - 1) u times the sum of the moduli."""
    return n_terms * term_bound(q_int) + (n_terms - 1) * U * n_terms * (1.0 + 2.0 ** -20)


def coherent_bound(q_int, n_a, n_b, n_origins_):
    """Of sum_t rho_b conj(rho_a): each rho is within its ``sum_bound`` and at most its atom count in modulus, a product adds
    sqrt(5) u of its modulus, and the sum over the origins (any order) at most (N - 1) u times the sum of the moduli."""
    product = n_a * sum_bound(q_int, n_b) + n_b * sum_bound(q_int, n_a) + np.sqrt(5.0) * U * n_a * n_b
    return (n_origins_ * product + (n_origins_ - 1) * U * n_origins_ * n_a * n_b) * (1.0 + 2.0 ** -20)


# ---- the phase, the sine and cosine, the powers, the term -----------------------------------------------------------------------

def reduce(s):
    with np.errstate(invalid="ignore"):
        return s - np.rint(s)


def frac(x, ci):
    """``f [..., 3]`` of positions ``x [..., 3]``."""
    return reduce(V.fractional(np.asarray(x, dtype=np.float64), ci))


def sincos2pi(f):
    """``(cos 2 pi f, sin 2 pi f)`` as ``sc_sincos2pi``: NaN in both unless ``|f| <= 1``."""
    f = np.asarray(f, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(f) <= 1.0
        g = 2.0 * np.where(ok, f, 0.0)
        k = np.rint(2.0 * g)
        r = g - k * 0.5
        z = r * r
        pc = np.full(f.shape, COS_COEFFS[-1])
        for a in COS_COEFFS[-2::-1]:
            pc = a - z * pc
        ps = np.full(f.shape, SIN_COEFFS[-1])
        for a in SIN_COEFFS[-2::-1]:
            ps = a - z * ps
        ps = r * ps
    m = k.astype(np.int64) & 3
    c = np.choose(m, [pc, -ps, -pc, ps])
    s = np.choose(m, [ps, pc, -ps, -pc])
    return np.where(ok, c, np.nan), np.where(ok, s, np.nan)


def cmul(ar, ai, br, bi):
    with np.errstate(invalid="ignore"):
        return ar * br - ai * bi, ar * bi + ai * br


def powers(c, s, H):
    """``(re, im) [..., H + 1]``: P_0 = 1 (NaN where E is), P_m = E P_{m-1}."""
    re, im = [np.where(np.isnan(c), np.nan, 1.0)], [np.zeros_like(c)]
    for _ in range(H):
        r, i = cmul(c, s, re[-1], im[-1])
        re.append(r)
        im.append(i)
    return np.stack(re, axis=-1), np.stack(im, axis=-1)


def h_max(q_int):
    q = np.asarray(q_int, dtype=np.int64).reshape(-1, 3)
    return [int(v) for v in np.abs(q).max(axis=0)]


def tables(f, q_int):
    """The three power tables of ``f [..., 3]``, as far as the q list reads them."""
    H = h_max(q_int)
    out = []
    for a in range(3):
        c, s = sincos2pi(f[..., a])
        out.append(powers(c, s, H[a]))
    return out


def term(tabs, q_int):
    """``(re, im) [..., n_q]``: (P^0_h P^1_k) P^2_l, a negative index taking the conjugate."""
    q = np.asarray(q_int, dtype=np.int64).reshape(-1, 3)
    parts = []
    for a in range(3):
        re, im = tabs[a]
        idx = np.abs(q[:, a])
        parts.append((re[..., idx], np.where(q[:, a] < 0, -im[..., idx], im[..., idx])))
    m_re, m_im = cmul(parts[0][0], parts[0][1], parts[1][0], parts[1][1])
    return cmul(m_re, m_im, parts[2][0], parts[2][1])


def delta(f_later, f_origin):
    with np.errstate(invalid="ignore"):
        d = f_later - f_origin
        return d - np.rint(d)


# ---- origins, blocks ------------------------------------------------------------------------------------------------------------

def n_origins(F, tau, stride):
    return (F - 1 - tau) // stride + 1


def n_blocks(n_or):
    return (n_or + BLOCK - 1) // BLOCK


def tree(v):
    """``sc_tree`` along axis 1 of ``v [blocks, BLOCK, ...]``."""
    v = np.array(v)
    d = BLOCK // 2
    with np.errstate(invalid="ignore"):
        while d >= 1:
            v[:, :d] = v[:, :d] + v[:, d:2 * d]
            d //= 2
    return v[:, 0]


def add_blocks(p):
    """The blocks ``p [blocks, ...]`` added one after the other from +0."""
    acc = np.zeros(p.shape[1:])
    with np.errstate(invalid="ignore"):
        for b in range(len(p)):
            acc = acc + p[b]
    return acc


# ---- the sums ---------------------------------------------------------------------------------------------------------------------

def density(f_sel, q_int):
    """``(re, im) [F, n_q]`` of ``f_sel [F, n, 3]``: the atoms added one after the other from +0."""
    n_q = len(np.asarray(q_int).reshape(-1, 3))
    re, im = np.zeros((f_sel.shape[0], n_q)), np.zeros((f_sel.shape[0], n_q))
    with np.errstate(invalid="ignore"):
        for i in range(f_sel.shape[1]):
            tr, ti = term(tables(f_sel[:, i], q_int), q_int)
            re, im = re + tr, im + ti
    return re, im


def _padded(v, n_or):
    nb = n_blocks(n_or)
    out = np.zeros((nb * BLOCK,) + v.shape[1:])
    out[:n_or] = v
    return out.reshape((nb, BLOCK) + v.shape[1:])


def coherent_sums(x, cell, a, b, q_int, lags, stride):
    """complex128 ``[n_lags, n_q]``: sum over the origins of rho_b(t + tau) conj(rho_a(t)) in the plan's order."""
    x = np.asarray(x, dtype=np.float64)
    ci = V.cell_matrices(cell)[1]
    F = len(x)
    ar, ai = density(frac(x[:, a], ci), q_int)
    br, bi = (ar, ai) if b is None else density(frac(x[:, b], ci), q_int)
    out = np.zeros((len(lags), ar.shape[1]), dtype=np.complex128)
    for x_l, tau in enumerate(int(v) for v in lags):
        n_or = n_origins(F, tau, stride)
        t = np.arange(n_or) * stride
        with np.errstate(invalid="ignore"):
            re = br[t + tau] * ar[t] + bi[t + tau] * ai[t]
            im = bi[t + tau] * ar[t] - br[t + tau] * ai[t]
        out[x_l] = add_blocks(tree(_padded(re, n_or))) + 1j * add_blocks(tree(_padded(im, n_or)))
    return out


def self_sums(x, cell, a, q_int, lags, stride):
    """complex128 ``[n_lags, n_q]``: sum over the origins and the atoms of the term of the reduced displacement; within a block
    one after the other, origin by origin and atom by atom; lag 0 exactly ``origins x n_a``."""
    x = np.asarray(x, dtype=np.float64)
    ci = V.cell_matrices(cell)[1]
    F, n_a = len(x), len(a)
    f = frac(x[:, a], ci)
    n_q = len(np.asarray(q_int).reshape(-1, 3))
    out = np.zeros((len(lags), n_q), dtype=np.complex128)
    for x_l, tau in enumerate(int(v) for v in lags):
        n_or = n_origins(F, tau, stride)
        if tau == 0:
            out[x_l] = float(n_or * n_a)
            continue
        t = np.arange(n_or) * stride
        tr, ti = term(tables(delta(f[t + tau], f[t]), q_int), q_int)          # [n_or, n_a, n_q]
        nb, whole = n_blocks(n_or), n_or // BLOCK
        tr, ti = _padded(tr, n_or).reshape(nb, BLOCK * n_a, n_q), _padded(ti, n_or).reshape(nb, BLOCK * n_a, n_q)
        re, im = np.zeros((nb, n_q)), np.zeros((nb, n_q))
        last = (n_or - whole * BLOCK) * n_a                                   # entries of a ragged last block
        with np.errstate(invalid="ignore"):
            for e in range(BLOCK * n_a):
                m = nb if (whole == nb or e < last) else whole
                re[:m] = re[:m] + tr[:m, e]
                im[:m] = im[:m] + ti[:m, e]
        out[x_l] = add_blocks(re) + 1j * add_blocks(im)
    return out


def sums(x, cell, a, b, same, q_int, lags, stride):
    """``(self, coherent)`` raw sums as ``sit_scattering`` returns them."""
    return self_sums(x, cell, a, q_int, lags, stride), coherent_sums(x, cell, a, None if same else b, q_int, lags, stride)


# ---- the independent evaluation -----------------------------------------------------------------------------------------------------

LD_PI = np.longdouble(4) * np.arctan(np.longdouble(1))


def exact_unit(phase):
    """``exp(2 pi i phase)`` in ``np.longdouble`` with the library's sine and cosine, the whole turns taken off first."""
    phase = np.asarray(phase, dtype=np.longdouble)
    phase = phase - np.rint(phase)
    return np.cos(2 * LD_PI * phase), np.sin(2 * LD_PI * phase)


def exact_term(f, q_int):
    """``(re, im) [..., n_q]`` in ``np.longdouble`` for the float64 ``f [..., 3]`` as given."""
    q = np.asarray(q_int, dtype=np.int64).reshape(-1, 3).astype(np.longdouble)
    f = np.asarray(f, dtype=np.float64).astype(np.longdouble)
    return exact_unit(f[..., None, 0] * q[:, 0] + f[..., None, 1] * q[:, 1] + f[..., None, 2] * q[:, 2])


# ---- the plan ---------------------------------------------------------------------------------------------------------------------

def round_up(v, m):
    return (v + m - 1) // m * m


def plan(F, n_a, n_b, same, n_q, H, n_lags, stride, self_part, coherent_part, cap=0):
    """``sc_plan``: a dict, or ``None`` where it refuses."""
    if not (1 <= F <= MAX_F) or n_lags < 1 or stride < 1 or not (1 <= n_q <= MAX_Q) or any(h < 0 or h > MAX_H for h in H):
        return None
    if n_a < 1 or n_b < 1 or n_a > MAX_ATOMS or n_b > MAX_ATOMS or (same and n_a != n_b) or not (self_part or coherent_part) or cap < 0:
        return None
    cap = cap if cap > 0 else DEFAULT_WORKSPACE
    p = dict(n_sel=1 if same else 2, n_cols=n_a if same else n_a + n_b, row=sum(H) + 3)
    p["tile"] = min(TILE_LDS // (p["row"] * 16), TILE_MAX)
    p["lds_bytes"] = max(p["tile"] * p["row"] * 16, LAG_TILE * BLOCK * 16)
    p["n_blocks"] = n_blocks(n_origins(F, 0, stride))
    q_series = p["n_sel"] * F * 16 if coherent_part else 0
    q_lag = p["n_blocks"] * 16
    frame = 3 * p["n_cols"] * 8 if coherent_part else 0
    slack = 1024
    if cap < slack + q_series + q_lag + frame:
        return None
    avail = cap - slack
    window = F if frame else 0
    if frame:
        window = min(window, (avail - q_series - q_lag) // frame)
        if window * frame > avail // 4:
            window = max(avail // 4 // frame, 1)
        window = min(window, MAX_FRAC // p["n_cols"])
    left = avail - window * frame
    qb = min(left // (q_series + q_lag), n_q, MAX_QBATCH)
    left -= qb * q_series
    p.update(window=window, q_batch=qb, n_q_batches=(n_q + qb - 1) // qb, lags_per_launch=min(left // (qb * q_lag), n_lags, MAX_LAGS_LAUNCH))
    # the three pieces of the work area, each from the next multiple of 256 on, and the end rounded up likewise
    used = 0
    for size in (window * 3 * p["n_cols"] * 8 if coherent_part else 0, p["n_sel"] * qb * F * 16 if coherent_part else 0,
                 p["lags_per_launch"] * p["n_blocks"] * qb * 16):
        used = round_up(used, 256) + round_up(size, 16)
    p["workspace"] = round_up(used, 256)
    return p
