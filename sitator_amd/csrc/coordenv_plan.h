// Every decision of SiteCoordinationEnvironment (the coordination polyhedron of a site and its continuous shape measure), written
// once for the kernels of coordenv.hip and for the host compiler (tests/test_coordenv_plan.py drives it with g++ under ASan /
// UBSan).  Compile without contraction (-ffp-contract=off).  The sphere, the membership answers, the octants, the search radius and
// the neighbour order are those of voronoi_plan.h and are not restated.
//
// The contract.  A site centre c is taken alone with the static lattice and all its periodic images; everything is relative to c.
//
// Cell.  A VERTEX of the site's Voronoi cell is a sphere through c and at least 3 static images that holds no static image
// (vp_classify, tolerance tau, certified against the forward bound of vp_sphere).  A degenerate sphere is one vertex with all its
// members: it is written from the first triple of its members, in enumeration order, that passes the shape floor (ce_shape_ok:
// that of voronoi_plan.h, and |D| against the product of the three lengths as well).  The cell is
// complete at search radius R when every open octant about c holds a neighbour and no empty sphere through c has r > R / 2
// (voronoi_plan.h, completeness (a) and (b)); otherwise the site runs again at the plan's next R.  Status: VS_OK, VS_GROW,
// VS_UNCERTAIN, VS_CAPACITY (neighbours, vertices, members of a sphere, vertices of a face, coordinating images, or R).
//
// Faces.  The face of neighbour j is the polygon of the vertices whose member list holds j, in the bisector plane of q_j.  The
// vertices are ordered by angle about their mean (a pseudo-angle x / (|x| + |y|) in a basis of the plane: divisions only, so the
// host and the device order alike); the solid angle from c is |sum| of the Van Oosterom-Strackee terms of the fan (mean, v_i,
// v_i+1).  Fewer than 3 vertices: 0.  A collinear face has every term 0.  Plain float64 in this fixed order, not certified.
//
// Coordinating images.  d_min the smallest distance of a face neighbour (a neighbour on any vertex), w_max the largest solid angle:
// j coordinates iff d_j / d_min <= distance_cutoff and w_j / w_max >= angle_cutoff.  A ratio within CE_NEAR (1e-9) relative of its
// cutoff sets CF_NEAR_CUTOFF; the comparison still decides.  They are listed in the neighbour order (distance, static index, image).
//
// Shape measure.  q_k the coordinating images (the site is the origin, not re-centred), p_k the vertices of an ideal shape:
//     S = 100 * (1 - t_max^2 / (sum |q|^2 sum |p|^2)),   t_max = max over the n! assignments of the largest eigenvalue of Horn's
// symmetric 4 x 4 matrix of M = sum q_k p_pi(k)^T  (= sigma_1 + sigma_2 + sign(det M) sigma_3).  The eigenvalue comes from
// CE_SWEEPS cyclic Jacobi sweeps: no square root of a small eigenvalue, so the rank-deficient M of the planar shapes keeps its
// digits.  S is clamped at 0.  An assignment may be skipped when 3 |M|_F^2 (1 + CE_BOUND_INFLATE) < incumbent^2: t <= sqrt(3) |M|_F
// (Cauchy-Schwarz on the singular values), the inflation covers the roundings of |M|_F^2 (9 products, 8 sums) and of the
// incumbent, so the maximum is that of the full enumeration.
//
// Result.  The shape of the site's n with the smallest S (library order breaks ties) is its environment if S < max_csm, with
// confidence w_best / sum w, w(S) = (1 - S / max_csm)^2 below max_csm and 0 otherwise; else no shape (-1) and confidence 0.
#pragma once

#include "voronoi_plan.h"

#define CE_BLOCK VP_BLOCK                              // threads of a workgroup of either kernel
#define CE_REC_CAP 128                                 // vertices of a site's cell
#define CE_FACE_CAP 32                                 // vertices of one face
#define CE_COORD_CAP 32                                // coordinating images of a site
#define CE_N_MAX 8                                     // largest n with a shape measure: 8! = 40320 assignments
#define CE_SHAPES 12
#define CE_SHAPES_PER_N 3                              // columns of csm_all
#define CE_SWEEPS 8
#define CE_NEAR 1e-9
#define CE_BOUND_INFLATE 1e-12
#define CE_LDS_BYTES (VP_NBR_CAP * (24 + 3 * 8 + 4 + 8 + 8 + 4 + 4) + CE_REC_CAP * 64 + 256)   // of the cell kernel

#define CF_NEAR_CUTOFF 1

struct CeVertex {
    double u[3];                                       // centre relative to the site
    int32_t nm;
    uint8_t m[VP_MEMBER_CAP];                          // positions in the neighbour list
    int32_t pad;
};

// library order; the table of ce_shape_table is [CE_SHAPES][CE_N_MAX][3], rows beyond n are 0
VP_HD inline int ce_shape_n(int s)
{
    const int n[CE_SHAPES] = {1, 2, 3, 4, 4, 5, 5, 6, 6, 7, 8, 8};
    return s >= 0 && s < CE_SHAPES ? n[s] : 0;
}

// host only: sqrt is correctly rounded, the device reads this table
inline void ce_shape_table(double *t)
{
    for (int k = 0; k < CE_SHAPES * CE_N_MAX * 3; k++) t[k] = 0.0;
    auto set = [&](int s, int k, double x, double y, double z) { double *p = t + (s * CE_N_MAX + k) * 3; p[0] = x; p[1] = y; p[2] = z; };
    const double h3 = sqrt(3.0) / 2.0, i3 = 1.0 / sqrt(3.0);
    set(0, 0, 0, 0, 1);                                                          // S:1
    set(1, 0, 0, 0, 1); set(1, 1, 0, 0, -1);                                     // L:2
    set(2, 0, 1, 0, 0); set(2, 1, -0.5, h3, 0); set(2, 2, -0.5, -h3, 0);         // TL:3
    set(3, 0, i3, i3, i3); set(3, 1, i3, -i3, -i3); set(3, 2, -i3, i3, -i3); set(3, 3, -i3, -i3, i3);       // T:4
    set(4, 0, 1, 0, 0); set(4, 1, 0, 1, 0); set(4, 2, -1, 0, 0); set(4, 3, 0, -1, 0);                       // S:4
    set(5, 0, 0, 0, 1); set(5, 1, 0, 0, -1); set(5, 2, 1, 0, 0); set(5, 3, -0.5, h3, 0); set(5, 4, -0.5, -h3, 0);   // T:5
    set(6, 0, 0, 0, 1); set(6, 1, 1, 0, 0); set(6, 2, 0, 1, 0); set(6, 3, -1, 0, 0); set(6, 4, 0, -1, 0);          // S:5
    set(7, 0, 1, 0, 0); set(7, 1, -1, 0, 0); set(7, 2, 0, 1, 0); set(7, 3, 0, -1, 0); set(7, 4, 0, 0, 1); set(7, 5, 0, 0, -1);  // O:6
    {                                                                            // T:6: r = 2 / sqrt 7, h = sqrt 3 / sqrt 7
        const double r = 2.0 / sqrt(7.0), h = sqrt(3.0) / sqrt(7.0);
        for (int z = 0; z < 2; z++) {
            const double hz = z ? -h : h;
            set(8, 3 * z, r, 0, hz); set(8, 3 * z + 1, -0.5 * r, h3 * r, hz); set(8, 3 * z + 2, -0.5 * r, -h3 * r, hz);
        }
    }
    {                                                                            // PB:7
        const double s5 = sqrt(5.0);
        const double c1 = (s5 - 1.0) / 4.0, s1 = sqrt(10.0 + 2.0 * s5) / 4.0, c2 = -(s5 + 1.0) / 4.0, s2 = sqrt(10.0 - 2.0 * s5) / 4.0;
        set(9, 0, 0, 0, 1); set(9, 1, 0, 0, -1); set(9, 2, 1, 0, 0); set(9, 3, c1, s1, 0); set(9, 4, c2, s2, 0); set(9, 5, c2, -s2, 0);
        set(9, 6, c1, -s1, 0);
    }
    for (int k = 0; k < 8; k++) set(10, k, k & 1 ? -i3 : i3, k & 2 ? -i3 : i3, k & 4 ? -i3 : i3);            // C:8
    {                                                                            // SA:8: edge 1, circumradius 1 / sqrt 2, separation 2^(-1/4)
        const double half = 0.5 / sqrt(sqrt(2.0));
        const double nrm = sqrt(0.5 + half * half), rho = sqrt(0.5) / nrm, e = 0.5 / nrm, z = half / nrm;
        set(11, 0, rho, 0, z); set(11, 1, 0, rho, z); set(11, 2, -rho, 0, z); set(11, 3, 0, -rho, z);
        set(11, 4, e, e, -z); set(11, 5, -e, e, -z); set(11, 6, -e, -e, -z); set(11, 7, e, -e, -z);
    }
}

// the shapes of a coordination number in library order: out[CE_SHAPES_PER_N], -1 padded; returns how many
VP_HD inline int ce_shapes_of(int n, int out[CE_SHAPES_PER_N])
{
    int ns = 0;
    for (int j = 0; j < CE_SHAPES_PER_N; j++) out[j] = -1;
    for (int s = 0; s < CE_SHAPES; s++)
        if (ce_shape_n(s) == n && ns < CE_SHAPES_PER_N) out[ns++] = s;
    return ns;
}

VP_HD inline int64_t ce_factorial(int n)
{
    int64_t f = 1;
    for (int k = 2; k <= n; k++) f *= k;
    return f;
}

// the rank-th permutation of 0 .. n - 1 in lexicographic order (factoradic digits)
VP_HD inline void ce_unrank(int64_t rank, int n, int perm[CE_N_MAX])
{
    int pool[CE_N_MAX];
    for (int k = 0; k < n; k++) pool[k] = k;
    int64_t f = ce_factorial(n - 1);
    for (int k = 0; k < n; k++) {
        const int d = (int)(rank / f);
        rank -= (int64_t)d * f;
        perm[k] = pool[d];
        for (int j = d; j + 1 < n - k; j++) pool[j] = pool[j + 1];
        if (n - 1 - k > 0) f /= (n - 1 - k);
    }
}

// the next permutation in lexicographic order; false after the last
VP_HD inline bool ce_next(int perm[CE_N_MAX], int n)
{
    int i = n - 2;
    while (i >= 0 && perm[i] > perm[i + 1]) i--;
    if (i < 0) return false;
    int j = n - 1;
    while (perm[j] < perm[i]) j--;
    int x = perm[i]; perm[i] = perm[j]; perm[j] = x;
    for (int a = i + 1, b = n - 1; a < b; a++, b--) { x = perm[a]; perm[a] = perm[b]; perm[b] = x; }
    return true;
}

// M[3 a + b] = sum_k q_k[a] p_perm[k][b], k ascending
VP_HD inline void ce_matrix(const double *q, const double *p, const int perm[CE_N_MAX], int n, double M[9])
{
    for (int e = 0; e < 9; e++) M[e] = 0.0;
    for (int k = 0; k < n; k++) {
        const double *qk = q + 3 * k, *pk = p + 3 * perm[k];
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) M[3 * a + b] += qk[a] * pk[b];
    }
}

#define CE_ROT(P, Q)                                                                                     \
    if (a[P][Q] != 0.0) {                                                                                \
        const double th = (a[Q][Q] - a[P][P]) / (2.0 * a[P][Q]);                                         \
        const double tt = (th < 0.0 ? -1.0 : 1.0) / (fabs(th) + sqrt(th * th + 1.0));                    \
        const double cc = 1.0 / sqrt(tt * tt + 1.0), ss = tt * cc;                                       \
        for (int r = 0; r < 4; r++) {                                                                    \
            const double x = a[r][P], y = a[r][Q];                                                       \
            a[r][P] = cc * x - ss * y; a[r][Q] = ss * x + cc * y;                                        \
        }                                                                                                \
        for (int r = 0; r < 4; r++) {                                                                    \
            const double x = a[P][r], y = a[Q][r];                                                       \
            a[P][r] = cc * x - ss * y; a[Q][r] = ss * x + cc * y;                                        \
        }                                                                                                \
        a[P][Q] = 0.0; a[Q][P] = 0.0;                                                                    \
    }

// the largest eigenvalue of Horn's matrix of M: max over proper rotations R of trace(R^T M)
VP_HD inline double ce_horn(const double M[9])
{
    const double xx = M[0], xy = M[1], xz = M[2], yx = M[3], yy = M[4], yz = M[5], zx = M[6], zy = M[7], zz = M[8];
    double a[4][4];
    a[0][0] = (xx + yy) + zz; a[1][1] = (xx - yy) - zz; a[2][2] = (yy - xx) - zz; a[3][3] = (zz - xx) - yy;
    a[0][1] = a[1][0] = yz - zy; a[0][2] = a[2][0] = zx - xz; a[0][3] = a[3][0] = xy - yx;
    a[1][2] = a[2][1] = xy + yx; a[1][3] = a[3][1] = zx + xz; a[2][3] = a[3][2] = yz + zy;
#ifdef __HIPCC__
#pragma unroll 1
#endif
    for (int sweep = 0; sweep < CE_SWEEPS; sweep++) {
        CE_ROT(0, 1) CE_ROT(0, 2) CE_ROT(0, 3) CE_ROT(1, 2) CE_ROT(1, 3) CE_ROT(2, 3)
    }
    double t = a[0][0];
    if (a[1][1] > t) t = a[1][1];
    if (a[2][2] > t) t = a[2][2];
    if (a[3][3] > t) t = a[3][3];
    return t;
}

VP_HD inline double ce_frobenius2(const double M[9])
{
    double f = 0.0;
    for (int e = 0; e < 9; e++) f += M[e] * M[e];
    return f;
}

// the assignment cannot beat the incumbent
VP_HD inline bool ce_skip(const double M[9], double incumbent)
{
    return incumbent > 0.0 && 3.0 * ce_frobenius2(M) * (1.0 + CE_BOUND_INFLATE) < incumbent * incumbent;
}

VP_HD inline double ce_norm2(const double *v, int n)
{
    double s = 0.0;
    for (int k = 0; k < n; k++) s += (v[3 * k] * v[3 * k] + v[3 * k + 1] * v[3 * k + 1]) + v[3 * k + 2] * v[3 * k + 2];
    return s;
}

VP_HD inline double ce_measure(double t_max, double q2, double p2)
{
    const double s = 100.0 * (1.0 - (t_max * t_max) / (q2 * p2));
    return s > 0.0 ? s : 0.0;
}

// the largest t over the assignments [first, first + count) of n vertices; use_bound: skip what cannot beat the incumbent
VP_HD inline double ce_best_t(const double *q, const double *p, int n, int64_t first, int64_t count, int use_bound)
{
    int perm[CE_N_MAX];
    double best = -INFINITY;
    if (count <= 0) return best;
    ce_unrank(first, n, perm);
    for (int64_t k = 0; k < count; k++) {
        double M[9];
        ce_matrix(q, p, perm, n, M);
        if (!(use_bound && ce_skip(M, best))) {
            const double t = ce_horn(M);
            if (t > best) best = t;
        }
        if (!ce_next(perm, n)) break;
    }
    return best;
}

// The shape floor of a site's triple.  vp_shape_ok measures |D| against the permanent, which bounds the roundings of D but is
// itself of the order of a rounding when the site is collinear with two of the atoms or coplanar with all three up to a rounding
// (a hole of an ideal lattice whose coordinates went through one addition: rows that share a zero).  |D| is therefore also
// measured against the product of the three lengths (Hadamard's bound): a quadruple flatter than VP_SHAPE_MIN of that is skipped
// like the other flat ones; its sphere, if it is a vertex at all, is found from its other triples.
VP_HD inline bool ce_shape_ok(const double qa[3], const double qb[3], const double qc[3])
{
    double det, permanent;
    if (!vp_shape_ok(qa, qb, qc, &det, &permanent)) return false;
    const double la = sqrt((qa[0] * qa[0] + qa[1] * qa[1]) + qa[2] * qa[2]);
    const double lb = sqrt((qb[0] * qb[0] + qb[1] * qb[1]) + qb[2] * qb[2]);
    const double lc = sqrt((qc[0] * qc[0] + qc[1] * qc[1]) + qc[2] * qc[2]);
    return fabs(det) >= VP_SHAPE_MIN * ((la * lb) * lc);
}

// one triple (a < b < c) of the neighbour list of a site: what becomes of its sphere (the VC_* of voronoi_plan.h; no VC_DUP by
// ownership: a site shares its cell with nobody)
VP_HD inline int ce_candidate(const double *q, int n, int a, int b, int c, double R, double tau, CeVertex *out)
{
    VpSphere s;
    if (!ce_shape_ok(q + 3 * a, q + 3 * b, q + 3 * c) || !vp_sphere(q + 3 * a, q + 3 * b, q + 3 * c, s)) return VC_SKIP;
    int members[VP_MEMBER_CAP];
    int nm = 0, uncertain = 0, overflow = 0;
    for (int k = 0; k < n; k++) {
        int ans = VM_ON;
        if (k != a && k != b && k != c) {
            const double d = vp_distance(q + 3 * k, s);
            ans = vp_classify(d, s.r, tau, vp_slack(d, s, tau));
        }
        if (ans == VM_INSIDE) return VC_REJECT;
        if (ans == VM_UNCERTAIN) uncertain = 1;
        else if (ans == VM_ON) {
            if (nm < VP_MEMBER_CAP) members[nm++] = k;
            else overflow = 1;
        }
    }
    if (!vp_near(s, R)) return VC_FAR;
    if (uncertain) return VC_UNCERTAIN;
    if (overflow) return VC_CAPACITY;
    for (int x = 0; x < nm; x++)
        for (int y = x + 1; y < nm; y++)
            for (int z = y + 1; z < nm; z++) {
                const int ma = members[x], mb = members[y], mc = members[z];
                if (ma == a && mb == b && mc == c) goto first;
                if (ce_shape_ok(q + 3 * ma, q + 3 * mb, q + 3 * mc)) return VC_DUP;
            }
first:
    if (out) {
        for (int k = 0; k < 3; k++) out->u[k] = s.u[k];
        out->nm = nm;
        out->pad = 0;
        for (int j = 0; j < VP_MEMBER_CAP; j++) out->m[j] = (uint8_t)(j < nm ? members[j] : 0);
    }
    return VC_RECORD;
}

// one Van Oosterom-Strackee term: the signed solid angle of the triangle (a, b, c) seen from the origin
VP_HD inline double ce_triangle(const double a[3], const double b[3], const double c[3])
{
    const double la = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    const double lb = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    const double lc = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    const double ab = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    const double ac = (a[0] * c[0] + a[1] * c[1]) + a[2] * c[2];
    const double bc = (b[0] * c[0] + b[1] * c[1]) + b[2] * c[2];
    const double det = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])) + a[2] * (b[0] * c[1] - b[1] * c[0]);
    const double den = ((la * lb) * lc + ab * lc) + (ac * lb + bc * la);
    if (det == 0.0) return 0.0;
    return 2.0 * atan2(det, den);
}

// monotone in the angle of (x, y), in [0, 4)
VP_HD inline double ce_pseudo_angle(double x, double y)
{
    const double r = fabs(x) + fabs(y);
    if (!(r > 0.0)) return 0.0;
    const double p = x / r;
    return y >= 0.0 ? 1.0 - p : 3.0 + p;
}

// the solid angle of the face of neighbour j (at qj) among the vertices rec[nrec]; *touched: j is on some vertex; *overflow: more
// than CE_FACE_CAP vertices
VP_HD inline double ce_face_angle(const double qj[3], const CeVertex *rec, int nrec, int j, int *touched, int *overflow)
{
    uint8_t vid[CE_FACE_CAP];
    double key[CE_FACE_CAP];
    int nv = 0;
    *touched = 0;
    for (int r = 0; r < nrec; r++) {
        bool has = false;
        for (int k = 0; k < rec[r].nm; k++) has = has || rec[r].m[k] == j;
        if (!has) continue;
        *touched = 1;
        if (nv < CE_FACE_CAP) vid[nv++] = (uint8_t)r;
        else *overflow = 1;
    }
    if (nv < 3) return 0.0;
    double mean[3] = {0.0, 0.0, 0.0};
    for (int v = 0; v < nv; v++)
        for (int k = 0; k < 3; k++) mean[k] += rec[vid[v]].u[k];
    for (int k = 0; k < 3; k++) mean[k] /= (double)nv;
    int ax = 0;                                                      // a basis of the plane: e1 = qj x axis, e2 = qj x e1
    if (fabs(qj[1]) < fabs(qj[ax])) ax = 1;
    if (fabs(qj[2]) < fabs(qj[ax])) ax = 2;
    double e[3] = {0.0, 0.0, 0.0}, e1[3], e2[3];
    e[ax] = 1.0;
    e1[0] = qj[1] * e[2] - qj[2] * e[1]; e1[1] = qj[2] * e[0] - qj[0] * e[2]; e1[2] = qj[0] * e[1] - qj[1] * e[0];
    e2[0] = qj[1] * e1[2] - qj[2] * e1[1]; e2[1] = qj[2] * e1[0] - qj[0] * e1[2]; e2[2] = qj[0] * e1[1] - qj[1] * e1[0];
    const double s1 = fabs(e1[0]) + fabs(e1[1]) + fabs(e1[2]), s2 = fabs(e2[0]) + fabs(e2[1]) + fabs(e2[2]);
    for (int v = 0; v < nv; v++) {
        const double *u = rec[vid[v]].u;
        const double d0 = u[0] - mean[0], d1 = u[1] - mean[1], d2 = u[2] - mean[2];
        const double x = ((d0 * e1[0] + d1 * e1[1]) + d2 * e1[2]) / s1, y = ((d0 * e2[0] + d1 * e2[1]) + d2 * e2[2]) / s2;
        const double kv = ce_pseudo_angle(x, y);
        int at = v;                                                  // insertion, stable: ties keep the vertex order
        const uint8_t id = vid[v];
        while (at > 0 && key[at - 1] > kv) { key[at] = key[at - 1]; vid[at] = vid[at - 1]; at--; }
        key[at] = kv; vid[at] = id;
    }
    double sum = 0.0;
    for (int v = 0; v < nv; v++) sum += ce_triangle(mean, rec[vid[v]].u, rec[vid[v + 1 < nv ? v + 1 : 0]].u);
    return fabs(sum);
}

// does a face neighbour at distance d with solid angle w coordinate the site; *near: a ratio within CE_NEAR of its cutoff
VP_HD inline bool ce_select(double d, double d_min, double w, double w_max, double dcut, double acut, double *nd, double *na, int *near)
{
    *nd = d / d_min;
    *na = w_max > 0.0 ? w / w_max : 0.0;
    if (fabs(*nd - dcut) <= CE_NEAR * dcut || fabs(*na - acut) <= CE_NEAR * acut) *near = 1;
    return *nd <= dcut && *na >= acut;
}

VP_HD inline double ce_weight(double S, double max_csm)
{
    if (!(S < max_csm)) return 0.0;
    const double x = 1.0 - S / max_csm;
    return x * x;
}

// csm[ns] of the shapes of one n in library order -> the position of the environment (-1: none), its confidence
VP_HD inline int ce_decide(const double *csm, int ns, double max_csm, double *confidence, double *best_csm)
{
    int best = -1;
    double sum = 0.0;
    *confidence = 0.0;
    *best_csm = NAN;
    for (int j = 0; j < ns; j++) {
        if (best < 0 || csm[j] < csm[best]) best = j;
        sum += ce_weight(csm[j], max_csm);
    }
    if (best < 0) return -1;
    *best_csm = csm[best];
    if (!(csm[best] < max_csm) || !(sum > 0.0)) return -1;
    *confidence = ce_weight(csm[best], max_csm) / sum;
    return best;
}

// what the cell kernel leaves for a site
struct CeSite {
    int32_t status, flags, n, nbr;                     // nbr: the true neighbour count, also beyond the cap
    int32_t pos[CE_COORD_CAP];                         // positions in the neighbour list
    double nd[CE_COORD_CAP], na[CE_COORD_CAP];
};

// The cell kernel, one candidate after the other: q[n][3] the neighbour list of a site in order.  rec: room for CE_REC_CAP.
inline void ce_site_serial(const double *q, int n, double R, double tau, double dcut, double acut, CeVertex *rec, CeSite &out)
{
    int octants = 0, uncertain = 0, capacity = 0, n_far = 0, nrec = 0;
    out.flags = 0; out.n = 0;
    for (int k = 0; k < n; k++) {
        const int o = vp_octant(q + 3 * k);
        if (o >= 0) octants |= 1 << o;
    }
    for (int a = 0; a < n; a++)
        for (int b = a + 1; b < n; b++) {
            int found = 0;
            for (int c = b + 1; c < n; c++) {
                CeVertex v;
                const int kind = ce_candidate(q, n, a, b, c, R, tau, &v);
                if (kind == VC_FAR) n_far++;
                else if (kind == VC_UNCERTAIN) uncertain = 1;
                else if (kind == VC_CAPACITY) capacity = 1;
                else if (kind == VC_RECORD) {
                    if (found < VP_PAIR_FOUND && nrec < CE_REC_CAP) { rec[nrec++] = v; found++; }
                    else capacity = 1;
                }
            }
        }
    out.status = vp_status(0, capacity, octants, n_far, uncertain);
    if (out.status != VS_OK) return;
    std::vector<double> w((size_t)n + 1), d((size_t)n + 1);
    std::vector<int> touched((size_t)n + 1);
    double d_min = INFINITY, w_max = 0.0;
    for (int j = 0; j < n; j++) {
        int over = 0;
        w[(size_t)j] = ce_face_angle(q + 3 * j, rec, nrec, j, &touched[(size_t)j], &over);
        d[(size_t)j] = sqrt((q[3 * j] * q[3 * j] + q[3 * j + 1] * q[3 * j + 1]) + q[3 * j + 2] * q[3 * j + 2]);
        if (over) capacity = 1;
        if (touched[(size_t)j]) {
            if (d[(size_t)j] < d_min) d_min = d[(size_t)j];
            if (w[(size_t)j] > w_max) w_max = w[(size_t)j];
        }
    }
    for (int j = 0; j < n; j++) {
        if (!touched[(size_t)j]) continue;
        double nd, na;
        int near = 0;
        const bool in = ce_select(d[(size_t)j], d_min, w[(size_t)j], w_max, dcut, acut, &nd, &na, &near);
        if (near) out.flags |= CF_NEAR_CUTOFF;
        if (!in) continue;
        if (out.n < CE_COORD_CAP) { out.pos[out.n] = j; out.nd[out.n] = nd; out.na[out.n] = na; out.n++; }
        else capacity = 1;
    }
    if (capacity) { out.status = VS_CAPACITY; out.n = 0; out.flags = 0; }
}
