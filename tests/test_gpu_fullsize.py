"""GPU, BASELINE.json full size (config C2: 100 000 frames x 64 mobile ions = 6.4e6 landmark vectors):
size-independent properties, oracle parity on a random sample of frames, the whole run against the oracle's stream, and
the label-trajectory operators on the run's labels against the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c2_full():
    from sitator_amd import LandmarkAnalysis, SiteNetwork, Structure, synth
    host = synth.config_host("C2")
    gen = synth.TrajectoryGenerator(host, 64, seed=2)
    ref = gen.reference_positions()
    frames = gen.generate(100000)
    sn = SiteNetwork(Structure(ref, host.cell), gen.static_mask, gen.mobile_mask)
    sn.centers = host.centers
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False)
    st = la.run(sn, frames)
    return host, gen, ref, frames, sn, la, st


def test_full_size_outputs_are_consistent(c2_full):
    host, gen, ref, frames, sn, la, st = c2_full
    assert st.traj.shape == (100000, 64) and st.traj.dtype == np.int64
    K = st.site_network.n_sites
    assert K >= 64 and st.traj.max() == K - 1 and st.traj.min() >= -1
    # every kept site passed the min_samples filter; confidences of assigned rows are >= the assignment threshold
    counts = np.bincount(st.traj[st.traj >= 0], minlength=K)
    assert counts.min() >= 1
    m = st.traj >= 0
    assert st.confidences[m].min() >= 0.8 and st.confidences[m].max() <= 1.0 + 1e-12
    assert np.all(st.confidences[~m] == 0.0)
    # at most one ion per site and frame (the occupancy check passed), re-derived on the host
    assert la.n_multiple_assignments == 0 and la.avg_mobile_per_site == 1.0
    srt = np.sort(st.traj, axis=1)
    assert not np.any((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0))
    # site centres lie inside the cell
    frac = np.asarray(st.site_network.centers) @ np.linalg.inv(host.cell)
    assert frac.min() >= -1e-9 and frac.max() < 1 + 1e-9


def test_full_size_sample_matches_oracle(c2_full, oracle):
    """Landmark vectors and labels of 40 random frames vs the CPU oracle (same centres)."""
    host, gen, ref, frames, sn, la, st = c2_full
    rng = np.random.default_rng(5)
    pick = np.sort(rng.choice(100000, size=40, replace=False))
    wrapped = oracle.wrap_points(host.cell, frames[pick])
    verts, vcd = oracle.site_vertex_distances(host.cell, host.centers, host.vertices, ref[gen.static_mask])
    exp, _ = oracle.fill(host.cell, wrapped, np.where(gen.static_mask)[0], np.where(gen.mobile_mask)[0],
                         ref[gen.static_mask], verts, vcd)
    for i, f in enumerate(pick):
        mine = la._ctx.rows_dense(int(f) * 64, 64)
        assert np.array_equal(mine != 0, exp[i * 64:(i + 1) * 64] != 0)
        np.testing.assert_allclose(mine, exp[i * 64:(i + 1) * 64], rtol=1e-6, atol=0)
    lab, conf = oracle.predict(exp, np.asarray(la.cluster_centers_), 0.8, True)
    assert np.array_equal(lab.reshape(40, 64), st.traj[pick])
    mm = lab >= 0
    np.testing.assert_allclose(conf[mm], st.confidences[pick].reshape(-1)[mm], rtol=1e-6)


def test_full_size_two_shards_equal_one_pass(c2_full):
    """Frame sharding: two contexts chained through the clustering state give the single-pass labels."""
    from sitator_amd import _lib
    from sitator_amd.dotprod_classifier import DotProdClassifier, LandmarkVectors
    from sitator_amd.sharding import Comm
    host, gen, ref, frames, sn, la, st = c2_full

    class Chain(Comm):            # two "ranks" executed one after the other in this process
        size = 1

    ctxs = []
    for lo, hi in ((0, 50000), (50000, 100000)):
        c = _lib.HipContext(host.cell)
        verts = np.full((512, 8), -1, dtype=np.int64)
        for k, v in enumerate(host.vertices):
            verts[k] = v
        vcd = c.site_vertex_distances(host.centers, ref[gen.static_mask], verts)
        c.set_basis(ref[gen.static_mask], verts, vcd, 1.5, 30, 1.0)
        c.set_frames(frames[lo:hi], np.where(gen.static_mask)[0], np.where(gen.mobile_mask)[0], frame0=lo)
        assert c.fill()[0] == 0
        ctxs.append(c)
    ctxs[0].fit_reset()
    ctxs[0].fit_push_stored_rows(0.45)
    cen, cnt = ctxs[0].fit_get_state()
    ctxs[1].fit_set_state(cen, cnt)
    ctxs[1].fit_push_stored_rows(0.45)
    cen, cnt = ctxs[1].fit_get_state()
    # iterations >= 2 on one context (replicated on every rank in a real run)
    last = len(cen)
    for _ in range(9):
        ctxs[0].fit_reset()
        ctxs[0].fit_push_dense_rows(cen, cnt, 0.45)
        cen, cnt = ctxs[0].fit_get_state()
        if len(cen) == last:
            break
        last = len(cen)
    clf = DotProdClassifier(threshold=0.45, min_samples=0.01 / 64)
    clf.set_cluster_centers(cen)
    normed = cen / np.linalg.norm(cen, axis=1)[:, None]
    counts = np.zeros(len(cen), dtype=np.int64)
    for c in ctxs:
        c.set_centers(normed, True)
        counts += c.predict(0.8, fetch=False)[2]
    keep = counts >= max(int(np.floor(0.01 / 64 * counts.sum())), 1)
    normed = normed[keep]
    labels = []
    for c in ctxs:
        c.set_centers(normed, True)
        labels.append(c.predict(0.8)[0])
    assert np.array_equal(np.concatenate(labels).reshape(100000, 64), st.traj)


def test_c2_full_size_run_equals_the_oracle_stream(c2_full, oracle):
    """The whole C2 run at its stated size against the ORACLE, not against the product's other paths: the oracle fills
    the 100 000 frames (256-frame blocks on a thread pool), streams the 6.4e6 sparse rows through its CSR fit (serial by
    nature) and assigns them per block.  Labels, sizes and the all-zero count must be identical, fitted centres and
    confidences within the float bar of the 12 288-frame test, site centres within the sharded golden test's bar, the
    occupancy statistics equal."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    from tests.test_gpu_parity import RTOL
    host, gen, ref, frames, sn, la, st = c2_full
    F, M = st.traj.shape
    sidx, midx = np.where(gen.static_mask)[0], np.where(gen.mobile_mask)[0]
    verts, vcd = oracle.site_vertex_distances(host.cell, host.centers, host.vertices, ref[sidx])
    D = len(host.centers)
    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as ex:
        parts = oracle.fill_csr_blocks(host.cell, frames, sidx, midx, ref[sidx], verts, vcd,
                                       check_for_zeros=la.check_for_zero_landmarks, block=256, map_fn=ex.map)
        out = oracle.cluster_dotprod_csr_blocks([p[0] for p in parts], D, {}, 0.01 / M, map_fn=ex.map)
    n_zero = sum(p[1] for p in parts)
    del parts
    labels = out["cluster-labels"].reshape(F, M)
    confs = out["cluster-confs"].reshape(F, M)
    K = len(out["cluster-size"])
    assert la.n_all_zero_lvecs == n_zero
    assert np.mean(labels < 0) > 0, "the run must hold unassigned samples"
    assert np.array_equal(st.traj, labels), "site indices must be identical to the oracle's"
    assert st.site_network.n_sites == K
    assert np.array_equal(np.bincount(st.traj[st.traj >= 0], minlength=K), out["cluster-size"])
    np.testing.assert_allclose(np.asarray(la.cluster_centers_), out["cluster-representative-lvecs"], rtol=1e-9, atol=1e-300)
    m = labels >= 0
    np.testing.assert_allclose(st.confidences[m], confs[m], rtol=RTOL)
    # site centres (real-weighted, LandmarkAnalysis.py:278-287): the oracle's average of every site's wrapped mobile
    # positions, weighted by the oracle's confidences; rows grouped by label once, in row order
    mob = oracle.wrap_points(host.cell, frames[:, midx]).reshape(-1, 3)
    flat = labels.reshape(-1)
    order = np.argsort(flat, kind="stable")
    bounds = np.searchsorted(flat[order], np.arange(K + 1))
    w = confs.reshape(-1)
    exp_centers = np.empty((K, 3))
    for s in range(K):
        rows = order[bounds[s]:bounds[s + 1]]
        exp_centers[s] = oracle.average(host.cell, mob[rows], w[rows])
    np.testing.assert_allclose(np.asarray(st.site_network.centers), exp_centers, rtol=1e-6, atol=1e-8)
    n_multi, avg = oracle.check_multiple_occupancy(labels, K, 1)
    assert la.n_multiple_assignments == n_multi and la.avg_mobile_per_site == avg


def test_c2_full_size_label_trajectory_layer_equals_the_oracle(c2_full, oracle):
    """The label-trajectory operators (JumpAnalysis, jumps, assign_to_last_known_site, occupancies, running windowed
    mode) on the full-size C2 labels - 391 frame chunks of the device scans - against the oracle.  Every operator runs
    on a fresh trajectory around a copy of the labels (assign_to_last_known_site rewrites its labels in place and the
    fixture is shared)."""
    from sitator_amd import JumpAnalysis, SmoothSiteTrajectory
    from tests.test_next_tier import JA, _eq, _st
    host, gen, ref, frames, sn, la, st = c2_full
    lab0 = np.array(st.traj, copy=True)
    F, M = lab0.shape
    K = st.site_network.n_sites
    # JumpAnalysis: the site / edge attributes, and the raw accumulators (n_problems is only logged by the operator)
    exp = oracle.jump_analysis(lab0, K)
    got = JumpAnalysis().run(_st(lab0.copy(), K))
    for a in JA:
        assert _eq(getattr(got.site_network, a), exp[a]), a
    n_ij, tsum, tn, total, nprob, _, _ = _st(lab0.copy(), K)._device().jump_analysis(K)
    assert np.array_equal(n_ij, exp["n_ij"]) and np.array_equal(total, exp["total_corrected_residences"])
    assert np.array_equal(tsum, exp["time_sum"]) and np.array_equal(tn, exp["time_n"])
    assert nprob == exp["n_problems"]
    assert exp["n_ij"].sum() - np.trace(exp["n_ij"]) > 1000, "the run must hold jumps"
    # jumps
    assert list(_st(lab0.copy(), K).jumps()) == oracle.jumps(lab0)
    # assign_to_last_known_site
    for thr in (1, 3):
        s2 = _st(lab0.copy(), K)
        res = s2.assign_to_last_known_site(frame_threshold=thr)
        t, (mx, avg, re) = oracle.assign_to_last_known_site(lab0, thr)
        assert np.array_equal(s2.traj, t)
        assert res["max_time_unknown"] == mx and res["total_reassigned"] == re
        assert res["avg_time_unknown"] == pytest.approx(avg, rel=1e-15, abs=0)
    # occupancies
    occ = _st(lab0.copy(), K).compute_site_occupancies()
    assert np.array_equal(occ, np.true_divide(np.bincount(lab0[lab0 >= 0], minlength=K), F))
    # running windowed mode on three frame bands (the oracle's loop is too slow for 6.4e6 labels); the window is local,
    # so the oracle sees every band with a margin of wleft + wright frames and the interior is compared
    mid = 256 * (F // 512)
    bands = [(0, 320), (mid - 160, mid + 160), (F - 320, F)]
    for thr, factor, repl in ((3, 2.1, True), (5, 2.1, False)):
        w = factor * thr
        wl, wr = int(np.floor(w / 2)), int(np.ceil(w / 2))
        sm = SmoothSiteTrajectory(window_threshold_factor=factor, remove_unoccupied_sites=False,
                                  set_unassigned_under_threshold=repl)
        out = sm.run(_st(lab0.copy(), K), thr).traj
        for lo, hi in bands:
            a, b = max(lo - wl - wr, 0), min(hi + wl + wr, F)
            e = oracle.running_windowed_mode(lab0[a:b], wl, wr, thr, K, repl)
            assert np.array_equal(out[lo:hi], e[lo - a:hi - a]), (thr, lo)
    assert np.array_equal(st.traj, lab0), "the fixture's labels must be untouched"


@pytest.mark.parametrize("cfg,M,F", [("C3", 448, 250000), ("C4", 256, 125000)])
def test_full_length_properties_and_sampled_oracle(oracle, cfg, M, F):
    """BASELINE configs[2] at its stated size: LLZO-like cell, 448 mobile ions, 250 000 frames = 1.12e8 landmark
    vectors (9.2 GB of frames, resident in HBM), and one rank's share of configs[3] (1 000 000 frames over 8 GPUs:
    125 000 frames x 256 ions, 6.9 GB).  Size-independent properties, and landmark vectors / labels of a random
    sample of frames against the CPU oracle."""
    import psutil
    from sitator_amd import LandmarkAnalysis, SiteNetwork, Structure, synth
    if psutil.virtual_memory().available < 30 * 2 ** 30:
        pytest.skip("needs ~20 GB of host memory for the trajectory")
    host = synth.config_host(cfg)
    gen = synth.TrajectoryGenerator(host, M, seed=3, threads=16)
    ref = gen.reference_positions()
    frames = gen.generate(F)
    sn = SiteNetwork(Structure(ref, host.cell), gen.static_mask, gen.mobile_mask)
    sn.centers = host.centers
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False)
    st = la.run(sn, frames)
    assert st.traj.shape == (F, M) and st.traj.dtype == np.int64
    K = st.site_network.n_sites
    assert K >= M and st.traj.max() == K - 1 and st.traj.min() >= -1
    m = st.traj >= 0
    assert 0 < np.mean(~m) < 0.05, "hops leave a small unassigned fraction"
    assert st.confidences[m].min() >= 0.8 and np.all(st.confidences[~m] == 0.0)
    assert la.n_multiple_assignments == 0 and la.avg_mobile_per_site == 1.0
    counts = np.bincount(st.traj[m], minlength=K)
    assert counts.min() >= 1 and np.array_equal(st.compute_site_occupancies(), np.true_divide(counts, F))
    njumps = sum(1 for _ in st.jumps())
    assert njumps > 1000
    # sampled parity
    rng = np.random.default_rng(8)
    pick = np.sort(rng.choice(F, size=12, replace=False))
    wrapped = oracle.wrap_points(host.cell, frames[pick])
    sidx, midx = np.where(gen.static_mask)[0], np.where(gen.mobile_mask)[0]
    verts, vcd = oracle.site_vertex_distances(host.cell, host.centers, host.vertices, ref[gen.static_mask])
    exp, _ = oracle.fill(host.cell, wrapped, sidx, midx, ref[gen.static_mask], verts, vcd)
    for i, f in enumerate(pick):
        mine = la._ctx.rows_dense(int(f) * M, M)
        assert np.array_equal(mine != 0, exp[i * M:(i + 1) * M] != 0)
        np.testing.assert_allclose(mine, exp[i * M:(i + 1) * M], rtol=1e-6, atol=0)
    lab, conf = oracle.predict(exp, np.asarray(la.cluster_centers_), 0.8, True)
    assert np.array_equal(lab.reshape(len(pick), M), st.traj[pick])
    mm = lab >= 0
    np.testing.assert_allclose(conf[mm], st.confidences[pick].reshape(-1)[mm], rtol=1e-6)


def test_c5_share_with_markov_clustering_and_jump_detection(oracle):
    """One rank's share of BASELINE configs[4] at its stated size: the LGPS-like ragged host, 160 mobile ions, 62 500
    frames = 1e7 landmark vectors of 5-13 entries, the FULL pipeline: Markov clustering of the landmarks
    (landmark/cluster/mcl.py:43-131; `max_mobile_per_site=2`: with the plugin's defaults the reference itself raises
    MultipleOccupancyError on this host - a golden), assignment, site centres, occupancy, jump detection.
    Size-independent properties, landmark vectors and labels of sampled frames against the oracle (same centres), the
    jumps re-derived on the host."""
    from sitator_amd import LandmarkAnalysis, SiteNetwork, Structure, synth
    M, F = 160, 62500
    host = synth.config_host("C5")
    gen = synth.TrajectoryGenerator(host, M, seed=5, threads=16)
    ref = gen.reference_positions()
    frames = gen.generate(F)
    sn = SiteNetwork(Structure(ref, host.cell), gen.static_mask, gen.mobile_mask)
    sn.centers = host.centers
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False, clustering_algorithm="mcl", max_mobile_per_site=2)
    st = la.run(sn, frames)
    assert st.traj.shape == (F, M) and st.traj.dtype == np.int64
    K = st.site_network.n_sites
    assert K >= M // 2 and st.traj.max() == K - 1 and st.traj.min() >= -1
    m = st.traj >= 0
    assert 0 < np.mean(~m) < 0.2
    assert st.confidences[m].min() >= 0.7 and np.all(st.confidences[~m] == 0.0)       # the plugin's assignment threshold
    counts = np.bincount(st.traj[m], minlength=K)
    assert counts.min() >= 1 and np.array_equal(st.compute_site_occupancies(), np.true_divide(counts, F))
    # at most two ions per site and frame; the reported statistics re-derived on the host for a block of frames
    srt = np.sort(st.traj[:2000], axis=1)
    assert not np.any((srt[:, 2:] == srt[:, :-2]) & (srt[:, 2:] >= 0))
    # every landmark group became a site: vertices of a site = union of its landmarks' vertices
    assert len(st.site_network.vertices) == K
    # jump detection (SiteTrajectory.py:307-373) against a host replay of the forward fill
    jumps = np.array(list(st.jumps()), dtype=np.int64).reshape(-1, 4)
    last = st.traj[0].copy()
    exp_j = []
    for f in range(1, 4000):
        cur = st.traj[f]
        known = cur >= 0
        jumped = known & (cur != last)                  # a first known site after an unknown start counts (:357-361)
        for a in np.where(jumped)[0]:
            exp_j.append((f, a, last[a], cur[a]))
        last = np.where(known, cur, last)
    head = jumps[jumps[:, 0] < 4000]
    assert len(jumps) > 500 and sorted(map(tuple, head)) == sorted(exp_j)
    # sampled parity: rows against the oracle's fill, labels against the oracle's predict with the plugin's centres
    rng = np.random.default_rng(9)
    pick = np.sort(rng.choice(F, size=16, replace=False))
    wrapped = oracle.wrap_points(host.cell, frames[pick])
    sidx, midx = np.where(gen.static_mask)[0], np.where(gen.mobile_mask)[0]
    verts, vcd = oracle.site_vertex_distances(host.cell, host.centers, host.vertices, ref[gen.static_mask])
    exp, _ = oracle.fill(host.cell, wrapped, sidx, midx, ref[gen.static_mask], verts, vcd)
    for i, f in enumerate(pick):
        mine = la._ctx.rows_dense(int(f) * M, M)
        assert np.array_equal(mine != 0, exp[i * M:(i + 1) * M] != 0)
        np.testing.assert_allclose(mine, exp[i * M:(i + 1) * M], rtol=1e-6, atol=0)
    asg = la._landmark_vectors.assignment
    assert asg["normed"] is False and len(asg["centers"]) == K
    lab, conf = oracle.predict(exp, asg["centers"], asg["threshold"], False)
    assert np.array_equal(lab.reshape(len(pick), M), st.traj[pick])
    mm = lab >= 0
    np.testing.assert_allclose(conf[mm], st.confidences[pick].reshape(-1)[mm], rtol=1e-6)
