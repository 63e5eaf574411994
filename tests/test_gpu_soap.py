"""GPU: ``sit_soap_vectors``, ``sit_soap_site_averages`` and the SOAP operators against the numpy restatement of the closed form
(tests/soap_ref.py, pinned to a direct quadrature of the definition by tests/test_soap_ref.py) and against the weight matrices the
TRUE reference's ``SOAPDescriptorAverages`` gave (tests/golden/soap_averages_known_answers.npz).

Every feature must be within ``1e-12 * B`` of the restatement's, ``B`` being the same sums with every term replaced by its absolute
value.  That is derived, not measured: a float64 evaluation of at most about 1e3 operations per term errs by about
``1e3 * 2^-53 * B``, roughly ``1.1e-13 B``; the bound leaves a factor 10 for the device's ``exp``.  The cases keep the terms of a
coefficient (neighbours x n_max) at 1e3 or below (asserted).  The shapes are the smallest at which the kernel can go wrong: S around
the wave width, the workgroup's tile of atoms and the neighbour staging capacity, neighbour lists that are empty, of one, around a
wave and beyond the staging capacity, one workgroup and many."""
import contextlib
import functools

import numpy as np
import pytest

from tests import soap_ref as SR

pytestmark = pytest.mark.gpu

TOL = 1e-12
CUBIC = np.eye(3) * 20.0
TRICLINIC = np.array([[9.1, 0.0, 0.0], [2.3, 8.4, 0.0], [-1.9, 2.7, 8.8]])
SMALL_TRICLINIC = np.array([[2.1, 0.0, 0.0], [0.6, 1.9, 0.0], [-0.3, 0.5, 2.4]])
CELLS = {"cubic": CUBIC, "triclinic": TRICLINIC, "small_triclinic": SMALL_TRICLINIC}


def plan():
    from sitator_amd import _lib
    return _lib.soap_plan(CUBIC, 3.0, 1, 6, 6)


def soap_dict(n_species, par):
    from sitator_amd.site_descriptors import soap_tables
    return soap_tables(n_species, {k: par[k] for k in ("cutoff", "l_max", "n_max", "atom_sigma", "crossover", "cutoff_transition_width")})


# (name, cell, S, neighbours of the first centre (None: as they fall), P, (l_max, n_max), species, crossover, width, outside)
RAW = [
    ("s1_empty", "cubic", 1, 0, 1, (6, 6), 1, False, 0.0, False),
    ("s3_one", "cubic", 3, 1, 1, (6, 6), 1, False, 0.0, False),
    ("s63", "cubic", 63, None, 1, (1, 2), 2, True, 0.0, False),
    ("s64_n64", "cubic", 64, 64, 1, (6, 6), 1, False, 0.0, False),
    ("s65_n65", "cubic", 65, 65, 1, (6, 6), 2, False, 1.0, True),
    ("cap", "cubic", "cap", "cap", 1, (1, 2), 1, False, 0.0, False),
    ("cap+1", "cubic", "cap+1", "cap+1", 1, (6, 6), 3, True, 0.0, True),
    ("tile", "cubic", "tile", None, 1, (0, 1), 1, False, 0.0, False),
    ("tile+1", "cubic", "tile+1", 5, 2, (1, 2), 3, True, 1.0, True),
    ("p300", "triclinic", 40, None, 300, (1, 2), 2, True, 0.0, True),
    ("tri_66", "triclinic", 65, None, 2, (6, 6), 3, False, 1.0, True),
    ("small_s1", "small_triclinic", 1, None, 1, (6, 6), 1, False, 0.0, True),
    ("small_s3", "small_triclinic", 3, None, 2, (1, 2), 3, True, 1.0, False),
    ("l0n1", "small_triclinic", 3, None, 1, (0, 1), 2, False, 0.0, False),
    ("edge", "cubic", 9, 6, 1, (6, 6), 2, True, 0.0, False),
]


@functools.lru_cache(maxsize=None)
def raw_case(name):
    _, cell_name, S, nbrs, P, (l_max, n_max), Z, crossover, width, outside = next(c for c in RAW if c[0] == name)
    pl = plan()
    sizes = {"cap": pl["nbr_cap"], "cap+1": pl["nbr_cap"] + 1, "tile": pl["threads"], "tile+1": pl["threads"] + 1}
    S, nbrs = sizes.get(S, S), sizes.get(nbrs, nbrs)
    cell = CELLS[cell_name]
    cutoff = 3.0 if cell_name != "small_triclinic" else 2.6 * SR.heights(cell).min()
    par = SR.params(cutoff=cutoff, l_max=l_max, n_max=n_max, crossover=crossover, cutoff_transition_width=width)
    rng = np.random.default_rng(len(name) * 1000 + S)
    centers = rng.uniform(0.0, 1.0, (P, 3)) @ cell
    static = rng.uniform(0.0, 1.0, (S, 3)) @ cell
    species = rng.integers(0, Z, S)
    species[:Z] = np.arange(Z)[:S]
    if nbrs is not None:                                         # exactly `nbrs` atoms within the cutoff of the first centre
        centers[0] = [10.0, 10.0, 10.0]
        u = rng.normal(size=(S, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        r = np.where(np.arange(S) < nbrs, rng.uniform(0.0, 0.9 * cutoff, S), rng.uniform(cutoff + 1.0, 9.0, S))
        static = centers[0] + u * r[:, None]
        if name == "edge":
            static[0] = centers[0]                               # the centre exactly on an atom
            static[1] = centers[0] + u[1] * (cutoff - 1e-6)      # an atom just inside the cutoff
            static[2] = centers[0] + u[2] * (cutoff + 1e-6)      # and one just outside
            nbrs -= 1
    else:
        if S >= 3 and cell_name != "small_triclinic":
            centers[0] = static[0]                               # the centre exactly on an atom
        if S > Z + 1:
            species[Z + 1] = -1                                  # an atom of a species that is masked out
    if outside:
        static = static + rng.integers(-2, 3, (S, 3)).astype(np.float64) @ cell
    exp, B, terms = SR.restate(cell, static, species, centers, Z, par)
    return {"cell": cell, "static": static, "species": species, "centers": centers, "Z": Z, "par": par, "exp": exp, "B": B, "terms": terms,
            "nbrs": nbrs}


@pytest.mark.parametrize("name", [c[0] for c in RAW])
def test_vectors_against_restatement(name):
    from sitator_amd import _lib
    c = raw_case(name)
    soap = soap_dict(c["Z"], c["par"])
    assert soap["n_dim"] == c["exp"].shape[1]
    with contextlib.closing(_lib.HipContext(c["cell"])) as ctx:
        out, cnt = ctx.soap_vectors(c["static"], c["species"], c["centers"], soap, nbr_count=True)
        again, _ = ctx.soap_vectors(c["static"], c["species"], c["centers"], soap)
    print("%s: neighbours %d..%d, worst |diff| / B %.3e" % (name, c["terms"].min(), c["terms"].max(),
                                                          np.max(np.abs(out - c["exp"]) / np.where(c["B"] > 0, c["B"], 1.0))))
    assert np.array_equal(cnt, c["terms"])
    if c["nbrs"] is not None:
        assert c["terms"][0] == c["nbrs"]
    assert c["terms"].max() * c["par"]["n_max"] <= 1000          # the term count the bound was derived for
    assert np.all(np.abs(out - c["exp"]) <= TOL * c["B"])
    assert out.tobytes() == again.tobytes()


def test_the_cases_reach_the_shapes_they_name():
    pl = plan()
    reached = {n: raw_case(n)["terms"] for n, *_ in RAW}
    assert reached["s1_empty"][0] == 0 and reached["s3_one"][0] == 1
    assert reached["small_s1"].max() > pl["nbr_cap"] and reached["small_s3"].max() > 2 * pl["nbr_cap"]
    assert raw_case("tile+1")["static"].shape[0] == pl["threads"] + 1
    assert np.max(np.abs(raw_case("p300")["exp"])) > 0


def test_no_centres_and_no_atoms():
    from sitator_amd import _lib
    par = SR.params()
    with contextlib.closing(_lib.HipContext(CUBIC)) as ctx:
        out, _ = ctx.soap_vectors(np.zeros((2, 3)), [0, 0], np.zeros((0, 3)), soap_dict(1, par))
        assert out.shape == (0, 147)
        out, cnt = ctx.soap_vectors(np.zeros((0, 3)), [], np.ones((2, 3)), soap_dict(1, par), nbr_count=True)
        assert np.all(out == 0.0) and np.all(cnt == 0)


def test_errors_of_the_entry_point():
    from sitator_amd import _lib
    static, centers = np.ones((2, 3)), np.ones((1, 3))
    with contextlib.closing(_lib.HipContext(CUBIC)) as ctx:
        for bad, what in ((dict(l_max=9), "l_max"), (dict(n_max=9), "n_max")):
            with pytest.raises(RuntimeError, match=what):
                ctx.soap_vectors(static, [0, 0], centers, soap_dict(1, SR.params(**bad)))
        with pytest.raises(RuntimeError, match="species"):
            ctx.soap_vectors(static, [0, 0], centers, soap_dict(5, SR.params()))
        with pytest.raises(RuntimeError):
            _lib.soap_plan(CUBIC, 3.0, 5, 6, 6)
        soap = soap_dict(1, SR.params())
        with pytest.raises(ValueError):
            ctx.soap_vectors(static, [0, 1], centers, soap)              # a species index beyond the environment
        with pytest.raises(ValueError, match="finite"):
            ctx.soap_vectors(static * np.array([[1.0], [np.nan]]), [0, 0], centers, soap)
        with pytest.raises(ValueError, match="finite"):
            ctx.soap_vectors(static, [0, 0], centers * np.inf, soap)
        with pytest.raises(ValueError):
            ctx.soap_vectors(static, [0, 0], centers, dict(soap, cutoff=20.0 * 256))
        out, _ = ctx.soap_vectors(static, [0, 0], centers, soap)         # the context is still usable
        assert np.isfinite(out).all()


# ---- SOAPDescriptorAverages on the reference's weight matrices -------------------------------------------------------------------

GOLDEN = np.load(SR.__file__.replace("soap_ref.py", "golden/soap_averages_known_answers.npz"))
AVG_CELL = np.eye(3) * 7.0


@functools.lru_cache(maxsize=None)
def averages_input(M):
    """Frames in which the static atoms are displaced differently in every frame, for the goldens' labels of M ions."""
    name = next(str(n) for n in GOLDEN["cases"] if GOLDEN[str(n) + "/labels"].shape[1] == M)
    mobile = GOLDEN[name + "/mobile_mask"]
    F = GOLDEN[name + "/labels"].shape[0]
    rng = np.random.default_rng(77 + M)
    base = rng.uniform(0.0, 7.0, (len(mobile), 3))
    real = base[None] + rng.normal(scale=0.35, size=(F, len(mobile), 3))
    real[:, mobile] = rng.uniform(-3.0, 10.0, (F, M, 3))
    numbers = np.where(mobile, 3, np.where(np.arange(len(mobile)) % 2 == 0, 8, 14))
    return real, mobile, numbers


@pytest.mark.parametrize("name", [str(n) for n in GOLDEN["cases"]])
def test_site_averages_on_the_golden_cases(name):
    from sitator_amd import _lib
    labels, K, W = GOLDEN[name + "/labels"], int(GOLDEN[name + "/n_sites"]), GOLDEN[name + "/W"]
    F, M = labels.shape
    real, mobile, numbers = averages_input(M)
    static_idx, mobile_idx = np.where(~mobile)[0], np.where(mobile)[0]
    species = np.where(numbers[static_idx] == 8, 0, 1)
    soap = soap_dict(2, SR.params(l_max=3, n_max=3, crossover=True))
    kw = dict(stepsize=int(GOLDEN[name + "/stepsize"]), averaging=int(GOLDEN[name + "/averaging"]) or None,
              avg_descriptors_per_site=int(GOLDEN[name + "/avg_descriptors_per_site"]) or None)
    with contextlib.closing(_lib.HipContext(AVG_CELL)) as ctx:
        ctx.set_assignments(labels)
        version = ctx.labels_version
        descs, counts, nr, info = ctx.soap_site_averages(K, static_idx, species, mobile_idx, soap, positions=real, **kw)
        again = ctx.soap_site_averages(K, static_idx, species, mobile_idx, soap, positions=real, **kw)[0]
        chunked, _, _, info2 = ctx.soap_site_averages(K, static_idx, species, mobile_idx, soap, positions=real,
                                                      workspace_bytes=2 * (real[0].nbytes + min(M, K) * soap["n_dim"] * 8), **kw)
        assert ctx.labels_version == version and np.array_equal(ctx.assignments()[0].reshape(labels.shape), labels)
        V = np.concatenate([ctx.soap_vectors(real[f, static_idx], species, real[f, mobile_idx], soap)[0] for f in range(F)])
        V0 = ctx.soap_vectors(real[0, static_idx], species, real[:, mobile_idx].reshape(-1, 3), soap)[0]
    assert np.array_equal(np.repeat(np.arange(K), nr), GOLDEN[name + "/desc_to_site"])
    assert descs.shape == (len(W), soap["n_dim"]) and info["contributors"] == np.count_nonzero(W)
    scale = np.max(np.abs(V))
    print("%s: |descs - W V| %.3e, |descs - W V0| %.3e, max |p| %.3e" % (name, np.max(np.abs(descs - W @ V)), np.max(np.abs(descs - W @ V0)), scale))
    assert np.max(np.abs(descs - W @ V)) <= TOL * scale
    assert np.max(np.abs(descs - W @ V0)) > 1e-3 * scale          # reading frame 0's host lattice everywhere cannot pass
    assert descs.tobytes() == again.tobytes() == chunked.tobytes() and info2["chunks"] > info["chunks"]


def test_site_averages_refuse_bad_labels():
    from sitator_amd import _lib
    real, mobile, numbers = averages_input(3)
    labels = GOLDEN["m3_step1_avg1/labels"].copy()
    soap = soap_dict(1, SR.params(l_max=1, n_max=2))
    static_idx, mobile_idx = np.where(~mobile)[0], np.where(mobile)[0]
    with contextlib.closing(_lib.HipContext(AVG_CELL)) as ctx:
        with pytest.raises(ValueError, match="assignments"):
            ctx.soap_site_averages(4, static_idx, np.zeros(len(static_idx)), mobile_idx, soap, averaging=1, positions=real)
        labels[5, 1] = 7
        ctx.set_assignments(labels)
        with pytest.raises(IndexError):
            ctx.soap_site_averages(4, static_idx, np.zeros(len(static_idx)), mobile_idx, soap, averaging=1, positions=real)
        with pytest.raises(ValueError, match="resident frames"):
            ctx.soap_site_averages(8, static_idx, np.zeros(len(static_idx)), mobile_idx, soap, averaging=1)
        with pytest.raises(ValueError, match="workspace"):
            ctx.soap_site_averages(8, static_idx, np.zeros(len(static_idx)), mobile_idx, soap, averaging=1, positions=real, workspace_bytes=8)


# ---- the operators -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def analysis():
    from sitator_amd import LandmarkAnalysis, SiteNetwork, Structure, synth
    host = synth.config_host("C1")
    frames, sm, mm, ref = synth.make_trajectory(host, 4, 120, seed=23, p_hop=1.0 / 30)
    numbers = np.where(mm, 3, np.where(np.arange(len(mm)) % 2 == 0, 8, 15))
    sn = SiteNetwork(Structure(ref, host.cell, numbers), sm, mm)
    sn.centers = host.centers
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False)
    st = la.run(sn, frames)
    return la, st, frames, numbers


def direct(sn, centers, soap_params, environment):
    """What sit_soap_vectors returns for these centres in the static structure of ``sn``."""
    from sitator_amd import _lib
    from sitator_amd.site_descriptors import soap_tables
    numbers = sn.static_structure.get_atomic_numbers()
    idx = np.full(len(numbers), -1)
    for k, z in enumerate(environment):
        idx[numbers == z] = k
    with contextlib.closing(_lib.HipContext(np.asarray(sn.structure.cell, dtype=np.float64))) as ctx:
        return ctx.soap_vectors(sn.static_structure.positions, idx, centers, soap_tables(len(environment), soap_params))[0]


def test_centers_and_sampled_centers():
    from sitator_amd import GenerateAroundSites, NAvgsPerSite, PBCCalculator, SOAPCenters, SOAPSampledCenters, device_soap_backend
    la, st, frames, numbers = analysis()
    sn = st.site_network
    params = {"l_max": 3, "n_max": 3, "crossover": True}
    backend = device_soap_backend(params)
    descs, to_site = SOAPCenters(3, backend=backend).get_descriptors(sn)
    assert np.array_equal(to_site, np.arange(sn.n_sites)) and np.any(descs != 0.0)
    assert descs.tobytes() == direct(sn, sn.centers, params, [8, 15]).tobytes()
    assert SOAPCenters(None, backend=backend).get_descriptors(st)[0].tobytes() == descs.tobytes()
    only_p, _ = SOAPCenters(3, environment=["P"], backend=backend).get_descriptors(sn)
    assert only_p.tobytes() == direct(sn, sn.centers, params, [15]).tobytes() and only_p.shape[1] < descs.shape[1]
    masked, _ = SOAPCenters(3, soap_mask=("O",), backend=backend).get_descriptors(sn)
    assert masked.tobytes() == direct(sn, sn.centers, params, [8]).tobytes()
    default = SOAPCenters(3).get_descriptors(sn)[0]
    assert default.shape[1] == 2 * 147 and default.tobytes() == direct(sn, sn.centers, {}, [8, 15]).tobytes()

    transform = NAvgsPerSite(2, error_on_insufficient=False)
    sampled = transform.run(st)
    descs, to_site = SOAPSampledCenters(3, backend=backend, sampling_transform=transform).get_descriptors(st)
    assert np.array_equal(to_site, sampled.site_types) and descs.tobytes() == direct(sn, sampled.centers, params, [8, 15]).tobytes()

    np.random.seed(5)
    descs, to_site = SOAPSampledCenters(3, backend=backend, sampling_transform=GenerateAroundSites(3, 0.1)).get_descriptors(sn)
    np.random.seed(5)
    pts = np.asarray(sn.centers).repeat(3, axis=0) + 0.1 * np.random.standard_normal((3 * sn.n_sites, 3))
    pbcc = PBCCalculator(sn.structure.cell)
    pbcc.wrap_points(pts)
    np.random.seed(5)
    around = GenerateAroundSites(3, 0.1).run(sn)
    assert around.centers.tobytes() == pts.tobytes()             # the reference's numpy expression, the same draws
    assert np.array_equal(to_site, np.repeat(np.arange(sn.n_sites), 3)) and np.array_equal(around.site_types, to_site)
    assert descs.tobytes() == direct(sn, pts, params, [8, 15]).tobytes()


def test_descriptor_averages_for_analysis():
    from sitator_amd import SOAPDescriptorAverages, SiteTrajectory, device_soap_backend
    la, st, frames, numbers = analysis()
    backend = device_soap_backend({"l_max": 2, "n_max": 3})
    op = SOAPDescriptorAverages(3, backend=backend, stepsize=2, averaging=5)
    if st.real_trajectory is None:
        st.set_real_traj(frames)
    labels = st._traj.copy()
    version = la._ctx.labels_version
    descs, to_site = op.get_descriptors(st)
    resident, to_site2 = op.get_descriptors_for_analysis(la)
    assert descs.tobytes() == resident.tobytes() and np.array_equal(to_site, to_site2)
    assert op.get_descriptors_for_analysis(la, st)[0].tobytes() == descs.tobytes()
    assert len(descs) == len(to_site) >= st.site_network.n_sites and np.any(descs != 0.0)
    assert la._ctx.labels_version == version and np.array_equal(st._traj, labels)
    per_site = SOAPDescriptorAverages(3, backend=backend, avg_descriptors_per_site=3)
    a, b = per_site.get_descriptors(st), per_site.get_descriptors_for_analysis(la)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    foreign = SiteTrajectory(st.site_network, labels)
    foreign.set_real_traj(frames)
    with pytest.raises(ValueError, match="does not share"):
        op.get_descriptors_for_analysis(la, foreign)
    assert op.get_descriptors(foreign)[0].tobytes() == descs.tobytes()
    with pytest.raises(ValueError):
        op.get_descriptors(SiteTrajectory(st.site_network, labels))      # no real trajectory


def test_descriptor_averages_refuse_frame_shards():
    from sitator_amd import LandmarkAnalysis, SOAPDescriptorAverages, SiteNetwork, Structure, synth
    host = synth.config_host("C1")
    frames, sm, mm, ref = synth.make_trajectory(host, 4, 100, seed=3, p_hop=1.0 / 50)
    sn = SiteNetwork(Structure(ref, host.cell, np.where(mm, 3, 8)), sm, mm)
    sn.centers = host.centers
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False, devices=[0, 0])
    la.run(sn, frames)
    with pytest.raises(NotImplementedError):
        SOAPDescriptorAverages(3, averaging=2).get_descriptors_for_analysis(la)
