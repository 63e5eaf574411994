"""References and seeded generators for tests/test_gpu_reductions.py (no test lives here).

The exact accumulators (csrc/sit_internal.h, the comment above exact_fixed; sharding.exact_sum_across): one term p - a
float64 product formed by ONE IEEE multiply - enters as the integer sign(p) * floor(|p| * 2^80); an accumulator is the
sum of its terms modulo 2^128, kept as two unsigned 64-bit words (hi, lo).  The model below never looks at a mantissa:
the four base-2^32 digits of floor(|p| * 2^80) are floor(|p| * 2^(80 - 32 k)) mod 2^32, and scaling by a power of two,
floor and fmod are exact in float64; the digits are summed per accumulator in int64 and the carries resolved at the end.
`fix_fraction` is the same definition in rational arithmetic, for the CPU test of the model."""
import math
from fractions import Fraction

import numpy as np

RUN_R, RUN_S, WRS_S = 64, 12, 16           # cluster.hip: frames per run, slots of k_gram_runs / k_weighted_row_sums_runs
WG_ROWS = 16384                            # sites.hip: rows per workgroup of k_site_wmax_lds / k_site_first_lds
WIDTHS = (0, 1, 12, 13, 16, 17, 24)

_M32 = 0xffffffff


def fix_fraction(p):
    """sign(p) * floor(|p| * 2^80) with rationals (NaN and 0 give 0)."""
    p = float(p)
    if p != p or p == 0.0:
        return 0
    f = Fraction(p)
    n = abs(f) * (1 << 80)
    n = n.numerator // n.denominator
    return -n if f < 0 else n


def exact_limbs(acc, p, n_acc):
    """(hi, lo) uint64[n_acc]: accumulator acc[i] += fix(p[i]) for every term, modulo 2^128."""
    acc = np.asarray(acc, dtype=np.int64).ravel()
    p = np.asarray(p, dtype=np.float64).ravel()
    keep = (p == p) & (p != 0.0)
    acc, p = acc[keep], p[keep]
    hi = np.zeros(n_acc, dtype=np.uint64)
    lo = np.zeros(n_acc, dtype=np.uint64)
    if len(p) == 0:
        return hi, lo
    assert acc.min() >= 0 and acc.max() < n_acc
    a = np.abs(p)
    assert a.max() < 2.0 ** 47, "outside the accumulators' documented range"
    sgn = np.where(p < 0, -1, 1).astype(np.int64)
    uniq, inv = np.unique(acc, return_inverse=True)
    assert len(p) < (1 << 30)                              # digit sums stay far inside int64
    carry = np.zeros(len(uniq), dtype=np.int64)
    digits = []
    for k in range(4):
        dig = np.fmod(np.floor(np.ldexp(a, 80 - 32 * k)), 4294967296.0).astype(np.int64)
        s = np.zeros(len(uniq), dtype=np.int64)
        np.add.at(s, inv, sgn * dig)
        s += carry
        digits.append((s & _M32).astype(np.uint64))        # python-style: the digit is non-negative ...
        carry = s >> 32                                    # ... and the carry floors (borrows for negative sums)
    lo[uniq] = digits[0] | (digits[1] << np.uint64(32))    # what the last carry would add is a multiple of 2^128
    hi[uniq] = digits[2] | (digits[3] << np.uint64(32))
    return hi, lo


def limbs_to_int(hi, lo):
    """Signed python integer of one accumulator (two's complement of 128 bits)."""
    v = (int(hi) << 64) | int(lo)
    return v - (1 << 128) if v >> 127 else v


def add_limbs(parts):
    """Sum of several (hi, lo) pairs modulo 2^128, in python integers."""
    his, los = [np.asarray(h).ravel() for h, _ in parts], [np.asarray(l).ravel() for _, l in parts]
    n = len(his[0])
    hi = np.zeros(n, dtype=np.uint64)
    lo = np.zeros(n, dtype=np.uint64)
    nz = np.zeros(n, dtype=bool)
    for h, l in zip(his, los):
        nz |= (h != 0) | (l != 0)
    for q in np.nonzero(nz)[0]:
        v = sum((int(h[q]) << 64) | int(l[q]) for h, l in zip(his, los)) & ((1 << 128) - 1)
        hi[q], lo[q] = v >> 64, v & ((1 << 64) - 1)
    return hi.reshape(np.shape(parts[0][0])), lo.reshape(np.shape(parts[0][1]))


def rounded_values(hi, lo):
    """The correctly rounded float64 of every accumulator / 2^80: python's int / int rounds the true quotient once."""
    hi, lo = np.asarray(hi), np.asarray(lo)
    out = np.zeros(hi.shape)
    flat = out.reshape(-1)
    h, l = hi.reshape(-1), lo.reshape(-1)
    for q in np.nonzero((h != 0) | (l != 0))[0]:
        flat[q] = limbs_to_int(h[q], l[q]) / (1 << 80)
    return out


def ulp_distance(got, ref):
    """max over the entries of |got - ref| / ulp(ref) (0 where both are 0; inf where only ref is)."""
    got, ref = np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    worst = 0.0
    for q in np.nonzero(got != ref)[0]:
        worst = max(worst, abs(got[q] - ref[q]) / math.ulp(ref[q]) if ref[q] != 0.0 else math.inf)
    return worst


# ---- the terms of the two reductions ----------------------------------------------------------------------------------

def padded_rows(X):
    """(nnz[N], idx[N, W], val[N, W]): the non-zeros of every row in ascending dimension, padded with (-1, 0)."""
    X = np.asarray(X)
    nz = X != 0
    nnz = nz.sum(axis=1)
    W = max(int(nnz.max()) if len(X) else 0, 1)
    idx = np.full((len(X), W), -1, dtype=np.int64)
    val = np.zeros((len(X), W))
    r, d = np.nonzero(nz)                                   # row-major: ascending d inside a row
    e = np.arange(len(r)) - np.concatenate([[0], np.cumsum(nnz)])[r]
    idx[r, e] = d
    val[r, e] = X[r, d]
    return nnz, idx, val


def gram_reference(X):
    """(hi, lo)[D, D] and seen[D] of X^T X: every ordered pair of a row's non-zeros is a term v1 * v2."""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    nnz, idx, val = padded_rows(X)
    W = idx.shape[1]
    step = max(1, 2000000 // (W * W))
    accs, prods = [], []
    for r0 in range(0, N, step):
        i, v = idx[r0:r0 + step], val[r0:r0 + step]
        m = (i[:, :, None] >= 0) & (i[:, None, :] >= 0)
        accs.append((i[:, :, None] * D + i[:, None, :])[m])
        prods.append((v[:, :, None] * v[:, None, :])[m])
    hi, lo = exact_limbs(np.concatenate(accs) if accs else [], np.concatenate(prods) if prods else [], D * D)
    return hi.reshape(D, D), lo.reshape(D, D), np.count_nonzero(X, axis=0).astype(np.int64)


def gram_term_count(X):
    return int((np.count_nonzero(X, axis=1).astype(np.int64) ** 2).sum())


def row_sums_reference(X, labels, confs, K, weighted):
    """(hi, lo)[K * D + K]: sums[k, d] += w * X[n, d] and, behind them, wsum[k] += w over the rows labelled 0 <= k < K."""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    lab = np.asarray(labels).reshape(-1)
    w = np.asarray(confs, dtype=np.float64).reshape(-1) if weighted else np.ones(N)
    rows = np.nonzero((lab >= 0) & (lab < K))[0]
    r, d = np.nonzero(X[rows])
    acc = np.concatenate([lab[rows][r] * D + d, K * D + lab[rows]])
    p = np.concatenate([w[rows][r] * X[rows][r, d], w[rows]])
    return exact_limbs(acc, p, K * D + K)


# ---- generated rows, labels and weights for the reductions ----------------------------------------------------------------

# (F, M, D, K, values): F in {2, 63, 64, 65, 129, 1000} and M in {1, 3, 64, 300}, each at least once
REDUCTION_CASES = [(2, 300, 40, 7, "uniform"), (63, 3, 40, 5, "signed"), (64, 64, 64, 9, "dyadic"), (65, 1, 40, 4, "signed"),
                   (129, 64, 48, 12, "uniform"), (1000, 3, 40, 6, "dyadic"), (1000, 1, 36, 5, "signed"),
                   (65, 300, 64, 20, "signed")]
TINY_DIMS = 4                                            # "signed": the last dimensions hold values around 2^-30 only


def make_reduction_case(F, M, D, K, values, seed=0):
    """X[F * M, D], labels[F, M], confs[F, M].  Row (f, j) is ion j in frame f.  An ion draws its landmarks from a pool
    of its own (30 wide for every third ion, which in 64 frames meets more than 16 of them; 14 otherwise) and a width
    from WIDTHS; its labels follow one of five patterns per run of 64 frames (a new site every frame, one site, two
    alternating sites, dwells broken by -1 and by labels >= K, random).  `values`: "uniform" in (0, 1]; "dyadic", 30-bit
    integers times 2^-77 .. 2^-13, so that products span 2^-96 .. 2^36 (below 2^-80 a term is dropped, below 2^-27
    truncated) while sums of thousands of them stay inside the accumulators' 2^47; "signed" in [-1, 1] plus, on the last
    TINY_DIMS dimensions, a few signed powers of two around 2^-30, whose products add up to small negative sums.
    A tenth of the weights is exactly 0, a tenth exactly 1."""
    rng = np.random.default_rng(seed)
    X = np.zeros((F * M, D))
    lab = np.empty((F, M), dtype=np.int64)
    nd = D - TINY_DIMS if values == "signed" else D
    for j in range(M):
        pool = rng.permutation(nd)[:30 if j % 3 == 0 else 14]
        for f in range(F):
            w = min(int(rng.choice(WIDTHS, p=(0.2, 0.6, 0.04, 0.04, 0.04, 0.04, 0.04))), len(pool))
            dims = rng.choice(pool, size=w, replace=False)
            if values == "uniform":
                v = 1.0 - rng.random(w)                                         # (0, 1]
            elif values == "dyadic":
                v = np.ldexp(rng.integers(1 << 29, 1 << 30, size=w).astype(np.float64), rng.integers(-77, -12, size=w))   # 2^-48 .. 2^18
            else:
                v = rng.uniform(-1.0, 1.0, size=w)
                v[v == 0.0] = 0.5
            X[f * M + j, dims] = v
            if values == "signed" and rng.random() < 0.5:                       # tiny signed entries: small negative sums
                t = nd + rng.choice(TINY_DIMS, size=2, replace=False)
                X[f * M + j, t] = np.ldexp(rng.choice([-1.0, 1.0, -1.5, 1.25], size=2), rng.integers(-34, -26, size=2))
        for c in range((F + RUN_R - 1) // RUN_R):
            f0, f1 = c * RUN_R, min(F, (c + 1) * RUN_R)
            n, mode = f1 - f0, (j + c) % 5
            if mode == 0:
                col = (int(rng.integers(K)) + np.arange(n)) % K if K > 1 else np.where(np.arange(n) % 2, 0, -1)
            elif mode == 1:
                col = np.full(n, int(rng.integers(K)))
            elif mode == 2:
                a = int(rng.integers(K))
                col = np.where(np.arange(n) % 2, a, (a + 1) % K)
            elif mode == 3:
                col = np.repeat(rng.integers(K, size=n), rng.integers(1, 9, size=n))[:n]
                bad = rng.random(n)
                col = np.where(bad < 0.15, -1, np.where(bad < 0.3, K + rng.integers(0, 3, size=n), col))
            else:
                col = rng.integers(K, size=n)
            lab[f0:f1, j] = col
    confs = rng.random((F, M))
    pick = rng.random((F, M))
    confs[pick < 0.1] = 0.0
    confs[pick > 0.9] = 1.0
    if values == "dyadic":
        confs = np.where(pick < 0.1, 0.0, np.where(pick > 0.9, 1.0, np.ldexp(1.0 + rng.integers(0, 8, size=(F, M)) / 8.0,
                                                                               rng.integers(-17, 10, size=(F, M)))))
    return X, lab, confs


def reduction_features(X, lab, confs, K):
    """What the arrays hold, found without the generator's bookkeeping."""
    F, M = lab.shape
    out = set()
    nnz = np.count_nonzero(X, axis=1)
    for w in WIDTHS:
        if np.any(nnz == w):
            out.add("width_%d" % w)
    nzrow = X != 0
    for j in range(M):
        for f0 in range(0, F, RUN_R):
            rows = np.arange(f0, min(F, f0 + RUN_R)) * M + j
            col = lab[f0:f0 + RUN_R, j]
            if nzrow[rows].any(axis=0).sum() > WRS_S:
                out.add("ion_meets_more_than_16_landmarks_in_a_run")
            ok = (col >= 0) & (col < K)
            if len(col) >= 2:
                if np.all(col[1:] != col[:-1]) and ok.all() and len(np.unique(col)) > 2:
                    out.add("label_changes_every_frame")
                if np.all(col == col[0]) and ok[0]:
                    out.add("label_constant_for_the_run")
                if len(col) >= 4 and len(np.unique(col)) == 2 and np.all(col[2:] == col[:-2]) and col[0] != col[1] and ok.all():
                    out.add("label_alternates_between_two_sites")
            # a wide row that does not fit the slots left by the rows before it, on the same valid site
            for a in range(1, len(col)):
                if ok[a] and col[a] == col[a - 1] and nnz[rows[a]] > 0 and nnz[rows[a - 1]] > 0:
                    if (nzrow[rows[a]] | nzrow[rows[a - 1]]).sum() > WRS_S:
                        out.add("slots_overflow_inside_a_row")
    if np.any(lab == -1):
        out.add("label_-1")
    if np.any(lab >= K):
        out.add("label_beyond_K")
    valid = (lab >= 0) & (lab < K)
    if np.any(confs[valid] == 0.0):
        out.add("weight_0")
    if np.any(confs[valid] == 1.0):
        out.add("weight_1")
    v = np.abs(X[X != 0])
    if len(v) and np.all((X[X != 0] > 0) & (v <= 1.0)):
        out.add("values_in_(0,1]")
    if np.any(X < 0):
        out.add("negative_values")
    _, idx, val = padded_rows(X)
    prod = np.abs(val[:, :, None] * val[:, None, :])[(idx[:, :, None] >= 0) & (idx[:, None, :] >= 0)]
    if len(prod):
        if np.any(prod < 2.0 ** -80):
            out.add("product_below_2^-80")
        if np.any((prod >= 2.0 ** -80) & (prod < 2.0 ** -27)):
            out.add("product_truncated_below_2^-27")
        if prod.min() < 2.0 ** -90 and prod.max() > 2.0 ** 30:
            out.add("products_from_2^-90_to_2^30")
    return out


def expected_reduction_features(F, M, values):
    want = {"label_-1", "label_beyond_K", "weight_0", "weight_1"} if F * M >= 600 and F >= 63 else set()
    if F * M >= 600:
        want |= {"width_%d" % w for w in WIDTHS}
    if F >= 64:
        want.add("ion_meets_more_than_16_landmarks_in_a_run")
    if F >= 63:
        want.add("label_changes_every_frame")                 # ion 0 in its first run
    if (M >= 2 and F >= 2) or F >= 129:
        want.add("label_constant_for_the_run")                # ion 1 in its first run, ion 0 in its second
    if (M >= 3 and F >= 4) or F >= 192:
        want.add("label_alternates_between_two_sites")
    if F >= 1000 or F * M >= 4000:
        want.add("slots_overflow_inside_a_row")
    if values == "uniform":
        want.add("values_in_(0,1]")
    if values == "signed":
        want |= {"negative_values", "product_truncated_below_2^-27"}
    if values == "dyadic" and F * M >= 600:
        want |= {"product_below_2^-80", "product_truncated_below_2^-27", "products_from_2^-90_to_2^30"}
    return want


def make_narrow_rows(N, D, seed, width=3):
    """Many narrow uniform rows (the row-parallel Gram kernel with several accumulator copies needs 32768 of them)."""
    rng = np.random.default_rng(seed)
    X = np.zeros((N, D))
    for e in range(width):
        keep = rng.random(N) < 0.7
        X[np.nonzero(keep)[0], rng.integers(D, size=int(keep.sum()))] = 1.0 - rng.random(int(keep.sum()))
    return X


# ---- best match -------------------------------------------------------------------------------------------------------

def sparse_products_argmax(X, c):
    """(row, |dot|, x2 of that row): the dot product leaves the row's exact zeros out (the device stores the non-zeros
    only, so 0 * NaN never arises), numpy's argmax (first maximum, first NaN) picks the row."""
    with np.errstate(invalid="ignore"):
        proj = np.abs(np.where(X != 0, X * c[None, :], 0.0).sum(axis=1))
    row = int(np.argmax(proj))
    return row, proj[row], float((X[row] * X[row]).sum())


def make_match_rows(N, D, seed, free_dims=0):
    """Rows and a centre on the grid of 2^-10 below 1 (every partial sum of at most 24 products is exact in any order):
    up to 24 non-zeros a row, one row in nine empty.  The last `free_dims` dimensions stay zero in every row."""
    rng = np.random.default_rng(seed)
    X = np.zeros((N, D))
    nd = D - free_dims
    widths = rng.integers(0, min(24, nd) + 1, size=N)
    widths[rng.random(N) < 1 / 9.0] = 0
    for w in np.unique(widths):
        if w == 0:
            continue
        rows = np.nonzero(widths == w)[0]
        dims = np.argsort(rng.random((len(rows), nd)), axis=1)[:, :w]
        vals = rng.integers(1, 512, size=dims.shape) * rng.choice([-1.0, 1.0], size=dims.shape) / 1024.0
        X[rows[:, None], dims] = vals
    c = rng.integers(1, 1024, size=D) * rng.choice([-1.0, 1.0], size=D) / 1024.0
    return X, c


def champion_row(c, dims):
    """The row over `dims` (at most 24 of them are used) no other grid row can beat: 1023/1024 with the sign of c."""
    dims = np.asarray(dims)
    dims = dims[np.argsort(-np.abs(c[dims]), kind="stable")[:24]]
    r = np.zeros(len(c))
    r[dims] = np.sign(c[dims]) * 1023.0 / 1024.0
    return r


def tie_pairs(N):
    """(name, first row, second row) of the planted ties the shape has room for."""
    want = [("same_wave", 3, 40), ("two_waves_of_a_block", 10, 200), ("rows_255_256", 255, 256),
            ("first_and_last_block", 5, N - 5), ("row_0_and_row_N-1", 0, N - 1)]
    return [(n, a, b) for n, a, b in want if 0 <= a < b < N and (n != "first_and_last_block" or b // 256 > 0)]


def dot_bound(x, c):
    """Forward error bound of a float64 dot product of the row's nnz non-zero terms, any order: (nnz + 1) u sum|v c|."""
    t = np.abs(x.astype(np.longdouble) * c.astype(np.longdouble))
    return (np.count_nonzero(x) + 1) * np.longdouble(2.0 ** -53) * t.sum()


# ---- site anchors and sums --------------------------------------------------------------------------------------------

def _frac_margin(cell, pts):
    u = np.asarray(pts) @ np.linalg.inv(cell)
    fr = u - np.floor(u)
    return np.minimum(fr, 1.0 - fr).min(axis=-1)


def sorted_sites(lab, K):
    """(order, start[K + 1]): the valid rows in site order (row order inside a site)."""
    lab = np.asarray(lab).reshape(-1)
    valid = np.nonzero((lab >= 0) & (lab < K))[0]
    order = valid[np.argsort(lab[valid], kind="stable")]
    return order, np.searchsorted(lab[order], np.arange(K + 1))


def anchors_reference(orc, cell, pos, lab, confs, K, weighted, frame0=0):
    """(wmax, first_row, anchor points) as PBCCalculator.average chooses them: np.argmax over the site's rows."""
    F, M = np.shape(lab)
    pw = orc.wrap_points(cell, np.asarray(pos).reshape(-1, 3))
    w_all = np.asarray(confs, dtype=np.float64).reshape(-1) if weighted else np.ones(F * M)
    order, start = sorted_sites(lab, K)
    wmax = np.full(K, -1.0)
    first = np.full(K, -1, dtype=np.int64)
    anchors = np.full((K, 3), np.nan)
    for k in range(K):
        rows = order[start[k]:start[k + 1]]
        if len(rows):
            a = int(np.argmax(w_all[rows]))
            wmax[k], first[k], anchors[k] = w_all[rows[a]], rows[a] + frame0 * M, pw[rows[a]]
    return wmax, first, anchors


def shifted_points(orc, cell, pos, lab, K, anchors):
    """(rows, q): the valid rows and q = wrap(wrap(p) + (centroid - anchor of the row's site))."""
    lab = np.asarray(lab).reshape(-1)
    cen = orc.pbc_constants(cell)[2]
    rows = np.nonzero((lab >= 0) & (lab < K))[0]
    pw = orc.wrap_points(cell, np.asarray(pos).reshape(-1, 3)[rows])
    return rows, pw, pw + (cen[None, :] - np.asarray(anchors)[lab[rows]])


def sums_reference(orc, cell, pos, lab, confs, K, weighted, anchors):
    """(sums[K, 4] in long double, tolerance[K, 4]).  The tolerance is (n_k + 2) u sum|w q| per component (a sum of n_k
    rounded products in any order) plus 8 u max|cell| sum w for the wraps: the point is wrapped twice, each time three
    3-term dot products with the inverse cell, a subtraction and three 3-term dot products with the cell - an absolute
    error of a few u max|cell| per component and wrap, which 8 u max|cell| per point covers when the device and the
    reference round a wrap differently at all (they evaluate the same expressions in the same order).  Measured on an
    MI355X: the largest error was 0.12 of this tolerance over the cases of the test file, 0.008 at 4.2e6 rows."""
    lab = np.asarray(lab).reshape(-1)
    rows, _, shifted = shifted_points(orc, cell, pos, lab, K, anchors)
    q = orc.wrap_points(cell, shifted).astype(np.longdouble)
    w = (np.asarray(confs, dtype=np.float64).reshape(-1)[rows] if weighted else np.ones(len(rows))).astype(np.longdouble)
    order = np.argsort(lab[rows], kind="stable")
    start = np.searchsorted(lab[rows][order], np.arange(K + 1))
    terms = np.concatenate([w[:, None], w[:, None] * q], axis=1)[order]
    sums = np.zeros((K, 4), dtype=np.longdouble)
    mags = np.zeros((K, 4), dtype=np.longdouble)
    for k in range(K):
        if start[k + 1] > start[k]:
            sums[k] = terms[start[k]:start[k + 1]].sum(axis=0)
            mags[k] = np.abs(terms[start[k]:start[k + 1]]).sum(axis=0)
    n = np.diff(start).astype(np.longdouble)
    u = np.longdouble(2.0 ** -53)
    tol = (n[:, None] + 2) * u * mags
    tol[:, 1:] += 8 * u * np.abs(cell).max() * mags[:, :1]
    return sums, tol


def centres_from_sums(orc, cell, centroid, sums, anchors):
    """landmark._site_centers: mean of the shifted points, shifted back and wrapped."""
    with np.errstate(invalid="ignore", divide="ignore"):
        centers = np.asarray(sums[:, 1:] / sums[:, :1], dtype=np.float64) - (np.asarray(centroid)[None, :] - anchors)
    ok = ~np.isnan(centers).any(axis=1)
    centers[ok] = orc.wrap_points(cell, centers[ok])
    return centers


def make_site_case(orc, cell, F, M, K, seed, weighted=True):
    """positions[F, M, 3] (not wrapped: some lie outside the cell), labels[F, M], confs[F, M].  A third of the sites sit
    within 0.004 of a cell face in one direction, so their members straddle it; confidences are multiples of 1/64 (ties
    everywhere) with the value 1 planted twice on two sites - once inside one block of 16384 rows, once in two blocks;
    rows 256..511 all sit on site 0; the last site has no rows; some labels are -1 or >= K.  Points whose fractional
    coordinates (their own, or those of the point shifted about its site's anchor) come within 1e-6 of a cell face are
    drawn again until none is left."""
    rng = np.random.default_rng(seed)
    N = F * M
    cfrac = rng.uniform(0.05, 0.95, size=(K, 3))
    face = np.arange(K) % 3 == 0
    cfrac[face, rng.integers(3, size=int(face.sum()))] = rng.choice([0.004, 0.996], size=int(face.sum()))
    lab = rng.integers(K, size=N)
    if K > 2:
        lab[lab == K - 1] = 0
    bad = rng.random(N)
    lab[bad < 0.03] = -1
    lab[(bad >= 0.03) & (bad < 0.05)] = K + rng.integers(0, 3, size=int(((bad >= 0.03) & (bad < 0.05)).sum()))
    if N >= 512:
        lab[256:512] = 0
    confs = rng.integers(1, 64, size=N) / 64.0
    for site, (r1, r2) in ((1 % K, (5, 700)), (2 % K, (100, WG_ROWS + 50))):
        if r2 < N:
            lab[[r1, r2]] = site
            confs[[r1, r2]] = 1.0

    def draw(n_rows, labs):
        fr = rng.uniform(0.0, 1.0, size=(n_rows, 3))
        v = (labs >= 0) & (labs < K)
        fr[v] = cfrac[labs[v]] + np.clip(rng.normal(0.0, 0.02, size=(int(v.sum()), 3)), -0.08, 0.08)
        return fr @ cell

    pos = draw(N, lab)
    for _ in range(50):
        _, _, anchors = anchors_reference(orc, cell, pos, lab.reshape(F, M), confs, K, weighted)
        rows, _, shifted = shifted_points(orc, cell, pos, lab, K, anchors)
        close = _frac_margin(cell, pos) < 1e-6
        close[rows] |= _frac_margin(cell, shifted) < 1e-6
        if not close.any():
            break
        pos[close] = draw(int(close.sum()), lab[close])
    else:
        raise AssertionError("points near a cell face keep coming back")
    return pos.reshape(F, M, 3), lab.reshape(F, M), confs.reshape(F, M)


def face_margin(orc, cell, pos, lab, confs, K, weighted):
    """The smallest distance (in fractional coordinates) of any point, raw or shifted about its anchor, to a cell face."""
    _, _, anchors = anchors_reference(orc, cell, pos, lab, confs, K, weighted)
    rows, _, shifted = shifted_points(orc, cell, pos, lab, K, anchors)
    m = _frac_margin(cell, np.asarray(pos).reshape(-1, 3)).min()
    return min(m, _frac_margin(cell, shifted).min()) if len(rows) else m


def site_features(lab, confs, K):
    lab, confs = np.asarray(lab).reshape(-1), np.asarray(confs).reshape(-1)
    out = set()
    order, start = sorted_sites(lab, K)
    for k in range(K):
        rows = order[start[k]:start[k + 1]]
        if len(rows) == 0:
            out.add("site_without_rows")
            continue
        top = rows[confs[rows] == confs[rows].max()]
        if len(top) >= 2:
            blocks = top // WG_ROWS
            out.add("maximal_weight_twice_in_one_block" if blocks[0] == blocks[1] else "maximal_weight_first_in_two_blocks")
    if np.any(lab == -1):
        out.add("label_-1")
    if np.any(lab >= K):
        out.add("label_beyond_K")
    for c in range(len(lab) // 256):
        chunk = lab[c * 256:(c + 1) * 256]
        if chunk[0] >= 0 and chunk[0] < K and np.all(chunk == chunk[0]):
            out.add("chunk_of_256_rows_on_one_site")
    return out
