"""Writes tests/golden/voronoi_known_answers.npz: for every generic fixture of tests/voronoi_ref.py the inputs (cell, static
positions) and qhull's answer - ``scipy.spatial.Voronoi`` over a 5 x 5 x 5 block of periodic images: the node centres that lie
in the cell and, per node, the static indices of the atoms whose Voronoi regions meet there (CSR); and under ``ref/`` for every
fixture, the ideal lattices too, the answer of the numpy restatement (nodes in its order, statuses, rounds) with the exact
rational centre and radius of every node's first record, which tests/test_voronoi_ref.py recomputes and compares.  Data only, so
that the GPU tests need neither scipy nor the restatement's minute on the void fixture.  Follows tests/make_vibfreq_golden.py: run it by hand when a fixture changes,

    python -m tests.make_voronoi_golden

There is no Zeo++ answer in this file: that binary cannot be run here."""
import numpy as np

from tests import voronoi_ref as VR


def main():
    out = {"names": np.array(sorted(VR.GENERIC))}
    for name in sorted(VR.GENERIC):
        cell, pos = VR.fixture(name)
        centers, verts = VR.qhull_nodes(cell, pos, block=2)
        out[name + "/cell"] = cell
        out[name + "/pos"] = pos
        out[name + "/centers"] = centers
        out[name + "/offsets"] = np.concatenate([[0], np.cumsum([len(v) for v in verts])]).astype(np.int64)
        out[name + "/indices"] = np.array([i for v in verts for i in v], dtype=np.int32)
        print("%s: %d atoms, %d nodes" % (name, len(pos), len(verts)))
    for name in sorted(VR.GENERIC) + sorted(VR.IDEAL):
        cell, pos = VR.fixture(name)
        a, k = VR.answer(name), "ref/" + name + "/"
        assert (a["status"] == VR.OK).all() and a["merge_status"] == VR.OK, name
        exact = [VR.exact_node(cell, pos, atom, quad) for atom, quad in a["quad"]]
        out[k + "centers"], out[k + "radii"] = a["centers"], a["radii"]
        out[k + "exact_centers"] = np.array([e[0] for e in exact]).reshape(-1, 3)
        out[k + "exact_radii"] = np.array([e[1] for e in exact])
        out[k + "offsets"] = np.concatenate([[0], np.cumsum([len(v) for v in a["vertices"]])]).astype(np.int64)
        out[k + "indices"] = np.array([i for v in a["vertices"] for i in v], dtype=np.int32)
        out[k + "status"], out[k + "nbr_count"] = a["status"], a["nbr_count"]
        out[k + "rounds"], out[k + "final_radius"], out[k + "records"] = a["rounds"], a["final_radius"], a["records"]
        print("ref %s: %d nodes, %d rounds" % (name, len(a["vertices"]), a["rounds"]))
    np.savez_compressed(VR.GOLDEN, **out)


if __name__ == "__main__":
    main()
