// Every decision of the periodic site graph of DiffusionPathwayAnalysis (network/DiffusionPathwayAnalysis.py:175-228), written
// once for the kernels of pathways.hip and for the host compiler (tests/test_pathway_graph.py runs a serial driver of the same
// rules with g++ under ASan / UBSan on the reference's goldens).  On top of cp_images / cp_min_image (clamp_point.h), so the
// image decision is the one that is pinned bit for bit there; compile without contraction (-ffp-contract=off).
//
// The graph.  The 3 x 3 x 3 supercell has n_images * K nodes, node = image * K + site, the images in the order of
// itertools.product(range(-1, 2), repeat = 3): image 9 i + 3 j + k is (i - 1, j - 1, k - 1) and the home image is 13.  A
// connected pair (from, to) carries the code 100 i + 10 j + k of the image of `to` nearest `from` (PBCCalculator.min_image,
// util/PBCCalculator.pyx:262-316: the first strictly smaller distance in the order of its loops).  Code 111: the edge stays
// inside every image.  Otherwise, from source image s it goes to image s + (digits - 1) and is dropped when a component of that
// leaves [-1, 1] (:218-224).  With n_images == 1 the graph is the plain K-node graph and every listed edge is (from, to).
//
// The labelling.  label[v] starts as v and only ever decreases to the index of a node of v's component, so every label
// chain v, label[v], label[label[v]], ... descends and ends at a node that is its own label (a root).  A round HOOKS every
// edge whose ends carry different labels - the larger label's node takes the smaller label if that is below its own (an
// atomic minimum: the order of arrival cannot matter) - and then COMPRESSES every node onto the end of its chain (pointer
// jumping, a bounded number of steps).  A round whose hook pass finds every edge with equal labels at both ends is the fixed
// point: all nodes of a component then share one label r, r is its own label, and since no label exceeds its node the
// component's lowest node is its own label too: r is the lowest node index of the component, whatever the order of arrival.
#pragma once

#include "clamp_point.h"

#define PG_MAX_SITES 16384          // K x K masks and codes: 256 MB and 1 GB at the limit
#define PG_HOME_IMAGE 13
#define PG_INTERNAL_CODE 111
#define PG_JUMP_CAP 64              // label-chain steps a node takes in one compress pass; the rest waits for the next round

// image index 9 i + 3 j + k -> the reference's return value 100 i + 10 j + k (PBCCalculator.pyx:316)
CP_HD inline int pg_code_of_image(int m) { return 100 * (m / 9) + 10 * (m / 3 % 3) + m % 3; }

// the code of the connected pair (from, to): min_image(pos[from], buf = pos[to]) (DiffusionPathwayAnalysis.py:200-201)
CP_HD inline int pg_pair_code(const double img[27][3], const double from[3], const double to[3])
{
    return pg_code_of_image(cp_min_image(img, from, to));
}

// PBCCalculator.pyx:305-314: the point moved to that image, pt[d] += (i - 1) cell[0, d] + (j - 1) cell[1, d] + (k - 1) cell[2, d]
CP_HD inline int pg_min_image(const double img[27][3], const double ref[3], double pt[3])
{
    const int m = cp_min_image(img, ref, pt);
    for (int d = 0; d < 3; d++) pt[d] += img[m][d];
    return pg_code_of_image(m);
}

CP_HD inline int pg_node(int image, int site, int K) { return image * K + site; }

// the image an edge of `code` reaches from image `src`, -1 where it leaves the supercell (DiffusionPathwayAnalysis.py:218-224)
CP_HD inline int pg_target_image(int code, int src)
{
    const int t0 = src / 9 + (code / 100 % 10 - 1), t1 = src / 3 % 3 + (code / 10 % 10 - 1), t2 = src % 3 + (code % 10 - 1);
    if (t0 < 0 || t0 > 2 || t1 < 0 || t1 > 2 || t2 < 0 || t2 > 2) return -1;
    return 9 * t0 + 3 * t1 + t2;
}

// implicit edge (listed edge, source image) -> its two nodes; false: dropped
CP_HD inline bool pg_edge_nodes(int n_images, int K, int from, int to, int code, int src, int *u, int *v)
{
    int dst = src;
    if (n_images > 1 && code != PG_INTERNAL_CODE) dst = pg_target_image(code, src);
    if (dst < 0) return false;
    *u = pg_node(src, from, K);
    *v = pg_node(dst, to, K);
    return true;
}

// the hook rule: the labels at the two ends of an edge -> the node whose label is lowered and the value it may take
CP_HD inline bool pg_hook(int lu, int lv, int *node, int *value)
{
    if (lu == lv) return false;
    *node = lu > lv ? lu : lv;
    *value = lu > lv ? lv : lu;
    return true;
}

// the compress rule: the end of v's label chain, or where PG_JUMP_CAP steps lead; `label(x)` reads the label of node x
template <class Label> CP_HD inline int pg_compress(Label label, int v)
{
    int p = label(v);
    for (int s = 0; s < PG_JUMP_CAP; s++) {
        const int g = label(p);
        if (g == p) break;
        p = g;
    }
    return p;
}
