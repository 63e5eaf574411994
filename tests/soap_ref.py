"""Two independent yardsticks for the SOAP power spectrum of DESIGN.md section 17 (the GTO construction of Himanen et al. 2020 with
the radial basis, the density and the feature order fixed there).

``quadrature`` integrates the definition directly - a radial Gauss-Legendre rule times a Gauss product rule on the sphere, with
``scipy.special.sph_harm_y`` - and uses no closed form.  ``restate`` is a plain numpy restatement of the closed form that finds the
periodic images by brute force over a box that provably covers the cutoff; it uses none of the plan's ranges.  Both return
``(p, B)``: the features and the same sums with every term replaced by its absolute value."""
import math

import numpy as np
from scipy.special import sph_harm_y

DEFAULTS = dict(cutoff=3.0, l_max=6, n_max=6, atom_sigma=0.4, crossover=False, cutoff_transition_width=0.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def radial_tables(cutoff, n_max, l_max):
    """alpha [l_max + 1, n_max] and the Loewdin root beta [l_max + 1, n_max, n_max] of the inverse overlap."""
    rn = np.linspace(1.0, cutoff, n_max)
    alpha = np.array([-np.log(1e-3 / rn ** l) / rn ** 2 for l in range(l_max + 1)])
    beta = np.empty((l_max + 1, n_max, n_max))
    for l in range(l_max + 1):
        S = 0.5 * math.gamma(l + 1.5) * (alpha[l][:, None] + alpha[l][None, :]) ** -(l + 1.5)
        w, v = np.linalg.eigh(S)
        beta[l] = (v * w ** -0.5) @ v.T
    return alpha, beta


def y_real(l, m, theta, phi):
    """Real orthonormal spherical harmonics without the Condon-Shortley phase: m > 0 cos, m < 0 sin."""
    if m == 0:
        return sph_harm_y(l, 0, theta, phi).real
    if m > 0:
        return math.sqrt(2.0) * (-1) ** m * sph_harm_y(l, m, theta, phi).real
    return math.sqrt(2.0) * (-1) ** m * sph_harm_y(l, -m, theta, phi).imag


def heights(cell):
    cell = np.asarray(cell, dtype=np.float64)
    vol = abs(np.linalg.det(cell))
    return np.array([vol / np.linalg.norm(np.cross(cell[(a + 1) % 3], cell[(a + 2) % 3])) for a in range(3)])


def switch(d, cutoff, t):
    d = np.asarray(d, dtype=np.float64)
    if not t > 0:
        return np.ones_like(d)
    return np.where(d <= cutoff - t, 1.0, 0.5 * (1.0 + np.cos(np.pi * (d - cutoff + t) / t)))


def neighbours(cell, static_pos, species_idx, center, cutoff):
    """(p [n, 3], species [n]) of every periodic image of every atom of the environment within the cutoff of ``center``: the
    difference is brought to crystal coordinates in [-0.5, 0.5], then every translation |t_a| <= ceil(cutoff / h_a) + 1 is tried."""
    cell = np.asarray(cell, dtype=np.float64)
    static_pos = np.asarray(static_pos, dtype=np.float64).reshape(-1, 3)
    species_idx = np.asarray(species_idx).reshape(-1)
    keep = species_idx >= 0
    if not keep.any():
        return np.zeros((0, 3)), np.zeros(0, dtype=np.int64)
    diff = static_pos[keep] - np.asarray(center, dtype=np.float64)
    frac = diff @ np.linalg.inv(cell)
    frac -= np.round(frac)
    N = np.ceil(cutoff / heights(cell)).astype(int) + 1
    t = np.stack(np.meshgrid(*[np.arange(-n, n + 1) for n in N], indexing="ij"), axis=-1).reshape(-1, 3)
    p = ((frac[:, None, :] + t[None, :, :]) @ cell).reshape(-1, 3)
    z = np.repeat(species_idx[keep], len(t))
    ok = np.einsum("ij,ij->i", p, p) <= cutoff * cutoff
    return p[ok], z[ok]


def feature_table(n_species, n_max, l_max, crossover):
    feats = []
    for z1 in range(n_species):
        for z2 in range(z1, n_species if crossover else z1 + 1):
            for n in range(n_max):
                for m in range(n if z1 == z2 else 0, n_max):
                    for l in range(l_max + 1):
                        feats.append((z1, n, z2, m, l))
    return feats


def power_spectrum(c, feats):
    """c [Z, n, l] -> array over m; the features of ``feats``."""
    return np.array([math.pi * math.sqrt(8.0 / (2 * l + 1)) * float(np.dot(c[z1][n][l], c[z2][m][l])) for z1, n, z2, m, l in feats])


def coefficients(p, z, n_species, par, absolute=False):
    """c[Z][n][l] = array over m of the closed form, summed over the neighbours (p, z)."""
    cutoff, n_max, l_max = par["cutoff"], par["n_max"], par["l_max"]
    a = 1.0 / (2.0 * par["atom_sigma"] ** 2)
    alpha, beta = radial_tables(cutoff, n_max, l_max)
    d = np.linalg.norm(p, axis=1) if len(p) else np.zeros(0)
    theta = np.arccos(np.divide(p[:, 2], d, out=np.ones_like(d), where=d > 0)) if len(p) else d
    phi = np.arctan2(p[:, 1], p[:, 0]) if len(p) else d
    w = switch(d, cutoff, par["cutoff_transition_width"])
    c = [[[np.zeros(2 * l + 1) for l in range(l_max + 1)] for _ in range(n_max)] for _ in range(n_species)]
    for l in range(l_max + 1):
        prim = (math.pi ** 1.5 * a ** l * (alpha[l] + a) ** -(l + 1.5))[None, :] * np.exp(
            -(alpha[l] * a / (alpha[l] + a))[None, :] * (d * d)[:, None])                      # [i, n']
        b = np.abs(beta[l]) if absolute else beta[l]
        radial = prim @ b.T * w[:, None]                                                      # [i, n]
        ylm = np.array([d ** l * y_real(l, m, theta, phi) for m in range(-l, l + 1)]).reshape(2 * l + 1, -1).T   # [i, m]
        if absolute:
            ylm = np.abs(ylm)
        for zz in range(n_species):
            sel = z == zz
            for n in range(n_max):
                c[zz][n][l] = (radial[sel, n][:, None] * ylm[sel]).sum(axis=0)
    return c


def restate(cell, static_pos, species_idx, centers, n_species, par):
    """(p [P, n_dim], B [P, n_dim], terms [P]) from the closed form; terms = neighbours within the cutoff."""
    feats = feature_table(n_species, par["n_max"], par["l_max"], par["crossover"])
    out, bound, terms = [], [], []
    for x in np.asarray(centers, dtype=np.float64).reshape(-1, 3):
        p, z = neighbours(cell, static_pos, species_idx, x, par["cutoff"])
        out.append(power_spectrum(coefficients(p, z, n_species, par), feats))
        bound.append(power_spectrum(coefficients(p, z, n_species, par, absolute=True), feats))
        terms.append(len(p))
    return np.array(out).reshape(len(terms), len(feats)), np.array(bound).reshape(len(terms), len(feats)), np.array(terms)


def quadrature(cell, static_pos, species_idx, center, n_species, par, nr=120, nt=48, nphi=96):
    """(p [n_dim], B [n_dim]) for one centre by integrating g_nl(r) Y_lm rho_Z over a ball that holds every Gaussian's tail."""
    cutoff, n_max, l_max = par["cutoff"], par["n_max"], par["l_max"]
    a = 1.0 / (2.0 * par["atom_sigma"] ** 2)
    alpha, beta = radial_tables(cutoff, n_max, l_max)
    p, z = neighbours(cell, static_pos, species_idx, center, cutoff)
    w = switch(np.linalg.norm(p, axis=1), cutoff, par["cutoff_transition_width"]) if len(p) else np.zeros(0)
    R = cutoff + 9.0 * par["atom_sigma"]
    xr, wr = np.polynomial.legendre.leggauss(nr)
    r, wr = (xr + 1.0) * R / 2.0, wr * R / 2.0
    xt, wt = np.polynomial.legendre.leggauss(nt)
    th = np.arccos(xt)
    ph = np.arange(nphi) * 2.0 * np.pi / nphi
    Rg, Tg, Pg = np.meshgrid(r, th, ph, indexing="ij")
    X, Y, Z = Rg * np.sin(Tg) * np.cos(Pg), Rg * np.sin(Tg) * np.sin(Pg), Rg * np.cos(Tg)
    W = (wr * r * r)[:, None, None] * wt[None, :, None] * (2.0 * np.pi / nphi)
    rho = [sum((w[i] * np.exp(-a * ((X - p[i, 0]) ** 2 + (Y - p[i, 1]) ** 2 + (Z - p[i, 2]) ** 2)) for i in range(len(p)) if z[i] == zz),
               np.zeros_like(X)) for zz in range(n_species)]
    c = [[[np.zeros(2 * l + 1) for l in range(l_max + 1)] for _ in range(n_max)] for _ in range(n_species)]
    cabs = [[[np.zeros(2 * l + 1) for l in range(l_max + 1)] for _ in range(n_max)] for _ in range(n_species)]
    for l in range(l_max + 1):
        g = [sum(beta[l][n][k] * Rg ** l * np.exp(-alpha[l][k] * Rg ** 2) for k in range(n_max)) for n in range(n_max)]
        for m in range(-l, l + 1):
            ylm = y_real(l, m, Tg, Pg)
            for zz in range(n_species):
                for n in range(n_max):
                    f = W * g[n] * ylm * rho[zz]
                    c[zz][n][l][m + l] = f.sum()
                    cabs[zz][n][l][m + l] = np.abs(f).sum()
    feats = feature_table(n_species, n_max, l_max, par["crossover"])
    return power_spectrum(c, feats), power_spectrum(cabs, feats)


def bucket_plan(labels, K, stepsize, averaging=None, avg_descriptors_per_site=None):
    """A line-by-line restatement of SOAP.py:258-320 with a one-hot vector per (frame, ion): (W [R, F * M], desc_to_site [R])."""
    labels = np.asarray(labels)
    F, M = labels.shape
    site_traj = labels[::stepsize]
    frames = np.arange(F)[::stepsize]
    counts = np.zeros(K + 1, dtype=int)
    for frame in site_traj:
        counts[frame] += 1
    counts = counts[:-1]
    if averaging is None:
        averaging = int(np.floor(np.mean(counts) / avg_descriptors_per_site))
    if averaging == 0:
        averaging = 1
    nr_of_descs = counts // averaging
    insufficient = nr_of_descs == 0
    averagings = np.full(len(nr_of_descs), averaging)
    averagings[insufficient] = counts[insufficient]
    nr_of_descs = np.maximum(nr_of_descs, 1)
    descs = np.zeros((int(np.sum(nr_of_descs)), F * M))
    desc_index = np.asarray([np.sum(nr_of_descs[:i]) for i in range(K)])
    max_index = np.asarray([np.sum(nr_of_descs[:i + 1]) for i in range(K)])
    count_of_site = np.zeros(K, dtype=int)
    allowed = np.ones(K, dtype=bool)
    for f, site_traj_t in zip(frames, site_traj):
        to_describe = (site_traj_t != -1) & allowed[site_traj_t]
        if np.any(to_describe):
            sites = site_traj_t[to_describe]
            soaps = np.zeros((len(sites), F * M))
            soaps[np.arange(len(sites)), f * M + np.nonzero(to_describe)[0]] = 1.0
            soaps /= averagings[sites][:, np.newaxis]
            descs[desc_index[sites]] += soaps
            count_of_site[sites] += 1
        full = count_of_site == averagings
        desc_index[full] += 1
        count_of_site[full] = 0
        allowed[max_index == desc_index] = False
    return descs, np.repeat(np.arange(K), nr_of_descs)
