"""GPU: DiffusionPathwayAnalysis, sit_pathway_components and PBCCalculator.min_image against the TRUE reference's goldens
(tests/golden/pathway_known_answers.npz) and, on inputs the goldens do not hold, against the restatement those goldens pin
(tests/pathway_ref.py).  Everything is compared with exact equality: image codes, component numbers, both attributes, the
pathway count and the directions."""
import numpy as np
import pytest

from tests import golden_util as G
from tests import pathway_ref as PR

pytestmark = pytest.mark.gpu

PG = PR.PathwayGoldens()
MAX_SITES = 16384


def network(cell, centers, n_ij=None):
    from sitator_amd import SiteNetwork, Structure
    sm = np.array([True, False])
    sn = SiteNetwork(Structure(np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]), cell), sm, ~sm)
    sn.centers = np.array(centers, copy=True)
    if n_ij is not None:
        sn.add_edge_attribute("n_ij", np.array(n_ij, copy=True))
    return sn


def run_operator(cell, centers, n_ij, kw):
    """What a golden case stores, from the operator."""
    from sitator_amd import DiffusionPathwayAnalysis
    periodic = kw.get("true_periodic_pathways", True)
    sn = network(cell, centers, n_ij)
    dpa = DiffusionPathwayAnalysis(**kw)
    out = dpa.run(sn, return_count=True, return_direction=periodic)
    assert out[0] is sn and len(out) == (3 if periodic else 2)
    rows, offsets = PR.directions_arrays(out[2] if periodic else [])
    return {"site": np.asarray(sn.site_diffusion_pathway), "edge": np.asarray(sn.edge_diffusion_pathway), "count": out[1],
            "dir_rows": rows, "dir_offsets": offsets, "rounds": dpa.rounds}


def assert_operator_equal(got, exp):
    assert got["site"].dtype == np.int64 and got["edge"].dtype == np.int64
    assert np.array_equal(got["site"], exp["site"])
    assert np.array_equal(got["edge"], exp["edge"])
    assert got["count"] == int(exp["count"])
    assert np.array_equal(got["dir_offsets"], exp["dir_offsets"])
    assert np.array_equal(got["dir_rows"], exp["dir_rows"])


@pytest.fixture(scope="module")
def contexts():
    """One device context per cell for the raw entry points."""
    from sitator_amd import _lib
    made = {}

    def get(cell):
        key = np.asarray(cell, dtype=np.float64).tobytes()
        if key not in made:
            made[key] = _lib.HipContext(cell)
        return made[key]
    yield get
    for ctx in made.values():
        ctx.close()


@pytest.mark.parametrize("name", PG.names)
def test_operator_equals_the_reference(name):
    cell, centers, n_ij, kw = PG.inputs(name)
    assert_operator_equal(run_operator(cell, centers, n_ij, kw), PG.expected(name))


@pytest.mark.parametrize("name", PG.names)
def test_components_and_codes_equal_the_reference(contexts, name):
    cell, centers, n_ij, kw = PG.inputs(name)
    exp = PG.expected(name)
    conn = PR.connectivity(n_ij, kw.get("connectivity_threshold", 1))
    n_images = 27 if kw.get("true_periodic_pathways", True) else 1
    root, rounds, codes = contexts(cell).pathway_components(conn, centers, n_images, codes=True)
    assert np.array_equal(codes, exp["codes"])
    assert np.array_equal(root[root], root) and (root <= np.arange(len(root))).all()
    assert np.array_equal(PR.ranked(root), exp["labels"])
    assert (rounds == 0) == (not conn.any()) and rounds < max(len(root), 1)
    # the same call again, without the codes: the same roots
    again, _, none = contexts(cell).pathway_components(conn, centers, n_images)
    assert none is None and np.array_equal(again, root)


@pytest.mark.parametrize("name", PG.names)
def test_min_image_on_the_connected_pairs(contexts, name):
    cell, centers, n_ij, kw = PG.inputs(name)
    src, dst = np.nonzero(PR.connectivity(n_ij, kw.get("connectivity_threshold", 1)))
    if len(src) == 0:
        moved, codes = contexts(cell).min_image(np.zeros((0, 3)), np.zeros((0, 3)))
        assert moved.shape == (0, 3) and codes.shape == (0,)
        return
    given = centers[dst].copy()
    moved, codes = contexts(cell).min_image(centers[src], given)
    assert np.array_equal(given, centers[dst])                   # the batch call copies; PBCCalculator works in place
    assert np.array_equal(codes, PG.expected(name)["codes"][src, dst])
    exp_moved, exp_codes = PR.min_image(cell, centers[src], centers[dst])
    assert np.array_equal(moved, exp_moved) and np.array_equal(codes, exp_codes)


@pytest.mark.parametrize("n", [1, 3, 5])
def test_min_image_of_a_few_pairs(contexts, n):
    """Counts at which every piece of the call's scratch layout ends off a 16-byte boundary."""
    rng = np.random.default_rng(40 + n)
    ref, pts = rng.random((n, 3)) @ PR.TRICLINIC, rng.random((n, 3)) @ PR.TRICLINIC
    moved, codes = contexts(PR.TRICLINIC).min_image(ref, pts)
    exp_moved, exp_codes = PR.min_image(PR.TRICLINIC, ref, pts)
    assert np.array_equal(moved, exp_moved) and np.array_equal(codes, exp_codes)


def test_pbc_calculator_min_image_in_place_and_ties(contexts):
    from sitator_amd import PBCCalculator
    pbcc = PBCCalculator(PR.CUBIC, _ctx=contexts(PR.CUBIC))
    # exactly half a cell apart: both images are equally far and the first of the loop wins
    for ref, pt, code, moved in (([2.5, 5, 5], [7.5, 5, 5], 11, [-2.5, 5, 5]), ([7.5, 5, 5], [2.5, 5, 5], 111, [2.5, 5, 5]),
                                 ([0, 0, 0], [5, 5, 5], 0, [-5, -5, -5]), ([5, 5, 5], [0, 0, 0], 111, [0, 0, 0]),
                                 ([1, 1, 1], [9, 1, 9.5], 10, [-1, 1, -0.5])):
        buf = np.array(pt, dtype=np.float64)
        got = pbcc.min_image(np.array(ref, dtype=np.float64), buf)
        assert isinstance(got, int) and got == code
        assert np.array_equal(buf, np.array(moved, dtype=np.float64))
        exp_moved, exp_code = PR.min_image(PR.CUBIC, [ref], [pt])
        assert exp_code[0] == code and np.array_equal(exp_moved[0], buf)


@pytest.mark.parametrize("K,cell,seed,kw", [
    (40, "cubic", 11, {}), (63, "triclinic", 12, {}), (64, "cubic", 13, {"connectivity_threshold": 2}),
    (65, "triclinic", 14, {"connectivity_threshold": 0.004}), (127, "cubic", 15, {}), (128, "triclinic", 16, {}),
    (129, "cubic", 17, {"true_periodic_pathways": False, "minimum_n_sites": 3}), (130, "triclinic", 18, {}),
    (3, "triclinic", 19, {}), (3, "cubic", 20, {"true_periodic_pathways": False})])   # every scratch piece ends off a 16-byte boundary
def test_fuzz_against_the_restatement(contexts, K, cell, seed, kw):
    cell = PR.CUBIC if cell == "cubic" else PR.TRICLINIC
    centers, n_ij = PR.random_network(cell, K, seed)
    exp = PR.analyse(cell, centers, n_ij, **kw)
    assert_operator_equal(run_operator(cell, centers, n_ij, kw), exp)
    n_images = 27 if kw.get("true_periodic_pathways", True) else 1
    root, _, codes = contexts(cell).pathway_components(exp["conn"], centers, n_images, codes=True)
    assert np.array_equal(codes, exp["codes"]) and np.array_equal(PR.ranked(root), exp["labels"])


@pytest.mark.parametrize("name,n_pathways", [("c1_hex_scgrid", 1), ("c1b_tri_bcctet", 0), ("bcc_ortho", 0)])
def test_pipeline_from_jump_analysis(name, n_pathways):
    """JumpAnalysis -> DiffusionPathwayAnalysis on the labels of merge_known_answers.npz; the reference finds one pathway
    of all 22 sites in c1_hex_scgrid and none in the other two."""
    from sitator_amd import DiffusionPathwayAnalysis, JumpAnalysis, SiteNetwork, SiteTrajectory, Structure
    z = G.load("merge_known_answers")
    sn = SiteNetwork(Structure(z[name + "/ref_positions"], z[name + "/cell"]), z[name + "/static_mask"], z[name + "/mobile_mask"])
    sn.centers = np.array(z[name + "/centers"], copy=True)
    st = SiteTrajectory(sn, z[name + "/labels"].copy())
    JumpAnalysis().run(st)
    out_sn, count, dirs = DiffusionPathwayAnalysis().run(st.site_network, return_count=True, return_direction=True)
    assert out_sn is st.site_network and count == n_pathways == len(dirs)
    exp = PR.analyse(z[name + "/cell"], z[name + "/centers"], np.asarray(sn.n_ij))
    assert np.array_equal(sn.site_diffusion_pathway, exp["site"]) and np.array_equal(sn.edge_diffusion_pathway, exp["edge"])
    assert np.array_equal(PR.directions_arrays(dirs)[0], exp["dir_rows"])
    if name == "c1_hex_scgrid":
        assert sn.n_sites == 22 and (sn.site_diffusion_pathway == 0).all()
    else:
        assert (sn.site_diffusion_pathway == DiffusionPathwayAnalysis.NO_PATHWAY).all()


def test_snake_settles_in_few_rounds():
    """257 sites in one closed path around x, indices permuted: the supercell component is a chain of 771 nodes.  The
    bound is a condition on the scheme, not a measurement: plain label propagation needs rounds of the order of the chain's
    length, any pointer-jumping scheme a small multiple of its logarithm."""
    cell, centers, n_ij = PR.snake()
    exp = PR.analyse(cell, centers, n_ij)
    got = run_operator(cell, centers, n_ij, {})
    assert_operator_equal(got, exp)
    assert exp["count"] == 1 and (exp["site"] == 0).all()
    print("snake: %d rounds for %d nodes" % (got["rounds"], 27 * len(centers)))
    assert 0 < got["rounds"] < 27 * len(centers) // 8


def test_error_paths(contexts):
    from sitator_amd import DiffusionPathwayAnalysis
    cell, centers, n_ij, _ = PG.inputs("chain_x")
    with pytest.raises(ValueError, match="n_ij"):
        DiffusionPathwayAnalysis().run(network(cell, centers))
    with pytest.raises(TypeError):
        DiffusionPathwayAnalysis(connectivity_threshold="1").run(network(cell, centers, n_ij))
    with pytest.raises(ValueError, match="return_direction"):
        DiffusionPathwayAnalysis(true_periodic_pathways=False).run(network(cell, centers, n_ij), return_direction=True)
    # more sites than the limit: refused before anything is read (the untouched pages of these arrays are never made)
    K = MAX_SITES + 1
    with pytest.raises(ValueError, match="16384"):
        contexts(cell).pathway_components(np.zeros((K, K), dtype=np.uint8), np.zeros((K, 3)), 27)
    with pytest.raises(ValueError, match="n_images"):
        contexts(cell).pathway_components(np.zeros((3, 3), dtype=np.uint8), centers, 9)
    # an attribute that is already there is not overwritten, as in the reference
    sn = network(cell, centers, n_ij)
    DiffusionPathwayAnalysis().run(sn)
    with pytest.raises(KeyError):
        DiffusionPathwayAnalysis().run(sn)
