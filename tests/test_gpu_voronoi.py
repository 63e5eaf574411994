"""GPU: ``sit_voronoi_nodes`` and ``VoronoiSiteGenerator.run`` against the numpy restatement (tests/voronoi_ref.py; its answers
are stored in tests/golden/voronoi_known_answers.npz and recomputed by tests/test_voronoi_ref.py) and against qhull's answer in
the same file.  There is no Zeo++ golden: that binary cannot be run here.

Vertex sets, the node count, the statuses, the rounds of the search radius, the neighbour counts and the order of the nodes are
compared exactly; centres and radii against the exact rational ones within ``voronoi_ref.CENTER_TOL`` (64 times the error the
host probe measured over the generic fixtures), the nodes of the ideal lattices against their closed-form centres within
``mu = 16 tau``.  The shapes are the smallest at which the kernels can go wrong: one atom (every neighbour an own image), two
atoms, the degenerate 8-, 6- and 24-atom spheres, atom counts around the wave width, a triclinic and a small triclinic cell with
atoms given several cells outside, a void that makes the driver grow the search radius, a neighbour count at the cap and over it."""
import numpy as np
import pytest

from sitator_amd import synth
from tests import voronoi_ref as VR

pytestmark = pytest.mark.gpu

MU = VR.MU_FACTOR * VR.TAU


@pytest.fixture(scope="module")
def contexts():
    from sitator_amd import _lib
    made = []

    def get(cell):
        made.append(_lib.HipContext(cell))
        return made[-1]
    yield get
    for ctx in made:
        ctx.close()


def mic_norm(d, cell):
    return np.linalg.norm(synth.mic_displacement(d, cell), axis=1)


@pytest.mark.parametrize("name", sorted(VR.GENERIC) + sorted(VR.IDEAL))
def test_nodes_are_the_restatements(contexts, name):
    cell, pos = VR.fixture(name)
    ref = VR.stored(name)
    got = contexts(cell).voronoi_nodes(pos, VR.TAU)
    info = got["info"]
    print(name, info)
    assert np.array_equal(got["status"], ref["status"]) and np.all(got["status"] == VR.OK)
    assert info["rounds"] == ref["rounds"] and info["merge_status"] == VR.OK and info["records"] == ref["records"]
    assert np.array_equal(got["nbr_count"], ref["nbr_count"]) and info["max_neighbours"] == ref["nbr_count"].max()
    assert abs(info["final_radius"] - ref["final_radius"]) <= 1e-12 * ref["final_radius"]
    assert [v.tolist() for v in got["vertices"]] == ref["vertices"]           # the same nodes in the same order
    assert all(v.tolist() == sorted(set(v.tolist())) for v in got["vertices"])
    dc = mic_norm(got["centers"] - ref["exact_centers"], cell).max()
    dr = np.abs(got["radii"] - ref["exact_radii"]).max()
    print("largest |centre - exact| %.3g, |radius - exact| %.3g" % (dc, dr))
    frac = got["centers"] @ VR.cell_inverse(cell).T
    assert np.all((frac > -1e-12) & (frac < 1.0 + 1e-12))                      # wrapped into the cell
    if name in VR.GENERIC:
        assert dc <= VR.CENTER_TOL and dr <= VR.CENTER_TOL
        g, k = VR.golden(), name + "/"
        off = g[k + "offsets"]
        qhull = sorted(tuple(g[k + "indices"][off[j]:off[j + 1]].tolist()) for j in range(len(off) - 1))
        assert sorted(tuple(v.tolist()) for v in got["vertices"]) == qhull   # qhull's nodes, as vertex sets
        assert np.array_equal(g[k + "pos"], pos)
    else:
        assert dc <= MU and dr <= MU
    if name == "sc_void":
        assert info["rounds"] > 1 and max(len(v) for v in got["vertices"]) == 24
    if name == "sc1":
        assert [v.tolist() for v in got["vertices"]] == [[0]]
    # a second computation (another context: a context keeps its last result) returns the same bytes
    again = contexts(cell).voronoi_nodes(pos, VR.TAU)
    for key in ("centers", "radii", "status", "nbr_count"):
        assert got[key].tobytes() == again[key].tobytes(), key
    assert [v.tobytes() for v in got["vertices"]] == [v.tobytes() for v in again["vertices"]]


@pytest.mark.parametrize("name", ["sc1", "sc2", "bcc1", "bcc2", "fcc2"])
def test_ideal_lattices_have_their_closed_form_nodes(contexts, name):
    cell, pos = VR.fixture(name)
    got = contexts(cell).voronoi_nodes(pos, VR.TAU)
    want = VR.closed_form(name)
    assert len(got["centers"]) == len(want)
    taken = set()
    for c in got["centers"]:
        d = mic_norm(want - c, cell)
        j = int(d.argmin())
        assert d[j] <= MU and j not in taken
        taken.add(j)
    counts = sorted(len(v) for v in got["vertices"])
    expect = {"sc1": [1], "sc2": [8] * 8, "bcc1": [2] * 12, "bcc2": [4] * 96, "fcc2": [4] * 64 + [6] * 32}[name]
    assert counts == expect


def ball(S, seed):
    """S atoms in a ball of radius 0.1 L in a cubic cell of edge L = 100: every atom has the S - 1 others within the first search
    radius (0.33 L for 257 atoms) and no image (the nearest is 0.8 L away)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(S, 3))
    v *= (10.0 * rng.uniform(0.0, 1.0, S) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    return np.eye(3) * 100.0, v + 50.0


def test_a_neighbour_count_at_the_cap_and_one_over_it(contexts):
    from sitator_amd import SiteNetwork, Structure, VoronoiError, VoronoiSiteGenerator, _lib
    cap = _lib.voronoi_plan(np.eye(3) * 100.0, 257)["neighbour_cap"]
    assert cap == VR.NBR_CAP
    cell, pos = ball(cap + 1, 1)
    assert VR.radius(cell, cap + 1, 0) > 20.0 and VR.radius(cell, cap + 1, 3) < 80.0 < VR.radius(cell, cap + 1, 4)
    got = contexts(cell).voronoi_nodes(pos, VR.TAU)
    done = got["status"] == VR.OK
    # the atoms inside the ball are done in the first round with exactly `cap` neighbours; those on its hull have an empty
    # octant until the radius reaches the images of the ball, which are more than the cap holds
    assert done.any() and np.all(got["nbr_count"][done] == cap)
    assert np.all(got["status"][~done] == VR.CAPACITY) and np.all(got["nbr_count"][~done] > cap)
    inner = int(np.linalg.norm(pos - 50.0, axis=1).argmin())
    assert done[inner]
    assert len(got["centers"]) == 0 and got["info"]["rounds"] == 5           # never a partial network
    cell, pos = ball(cap + 2, 2)
    got = contexts(cell).voronoi_nodes(pos, VR.TAU)
    assert np.all(got["status"] == VR.CAPACITY) and np.all(got["nbr_count"] == cap + 1) and got["info"]["rounds"] == 1
    sn = SiteNetwork(Structure(pos, cell), np.ones(len(pos), dtype=bool), np.zeros(len(pos), dtype=bool))
    with pytest.raises(VoronoiError) as err:
        VoronoiSiteGenerator().run(sn)
    assert err.value.atoms == list(range(cap + 2)) and set(err.value.statuses) == {VR.CAPACITY}


def test_generator_surface():
    from sitator_amd import SiteNetwork, Structure, VoronoiSiteGenerator
    with pytest.raises(NotImplementedError):
        VoronoiSiteGenerator(radial=True)
    cell, pos = VR.fixture("triclinic")
    ref = VR.stored("triclinic")
    A = len(pos) + 3
    allpos = np.concatenate([pos[:5], np.full((3, 3), 1.0), pos[5:]])        # three mobile atoms among the statics
    sm = np.ones(A, dtype=bool)
    sm[5:8] = False
    sn = SiteNetwork(Structure(allpos, cell), sm, ~sm)
    gen = VoronoiSiteGenerator(zeopp_path="/nowhere/network")
    out = gen.run(sn)
    assert out is not sn and sn.centers is None
    assert out.vertices == ref["vertices"] and isinstance(out.vertices[0], list) and isinstance(out.vertices[0][0], int)
    assert mic_norm(out.centers - ref["exact_centers"], cell).max() <= VR.CENTER_TOL
    assert gen.last_info["rounds"] == ref["rounds"] and gen.last_info["kernel_ms"] > 0.0


@pytest.mark.parametrize("which", ["sc_grid", "fcc_mixed"])
def test_generated_network_drives_landmark_analysis(which):
    """synth's host with its centres and vertices withheld: the generated network has the host's landmarks, and
    LandmarkAnalysis on it gives the landmark vectors of the run on the host's own basis (rtol 1e-6, the project's float tolerance)."""
    from sitator_amd import LandmarkAnalysis, SiteNetwork, Structure, VoronoiSiteGenerator
    host = synth.config_host("C1d") if which == "sc_grid" else synth.fcc_mixed(G=2, a=5.0)
    frames, sm, mm, ref = synth.make_trajectory(host, 4, 256, seed=3)
    bare = SiteNetwork(Structure(ref, host.cell), sm, mm)
    gen = VoronoiSiteGenerator().run(bare)
    assert gen.n_sites == len(host.centers)
    order = []
    for c in host.centers:
        d = mic_norm(np.asarray(gen.centers) - c, host.cell)
        order.append(int(d.argmin()))
        assert d[order[-1]] <= MU
    assert sorted(order) == list(range(len(host.centers)))
    assert [gen.vertices[k] for k in order] == [sorted(v) for v in host.vertices]
    mine = SiteNetwork(Structure(ref, host.cell), sm, mm)
    mine.centers = np.asarray(gen.centers)[order]
    mine.vertices = [gen.vertices[k] for k in order]
    theirs = SiteNetwork(Structure(ref, host.cell), sm, mm)
    theirs.centers = host.centers
    theirs.vertices = host.vertices
    vectors = []
    for sn in (mine, theirs):
        la = LandmarkAnalysis(verbose=False, device=0)
        la.run(sn, frames)
        vectors.append(np.array(la.landmark_vectors))
    np.testing.assert_allclose(vectors[0], vectors[1], rtol=1e-6, atol=1e-300)
