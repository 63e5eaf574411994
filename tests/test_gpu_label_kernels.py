"""The label-trajectory kernels (dynamics.hip: jump scan, JumpAnalysis, assign_to_last_known_site, running windowed mode;
sites.hip: occupancy check, site counts) on adversarial label arrays at edge shapes, against the oracle.

The device scans cut the frames into chunks of 256 (LS_CHUNK of label_scan.h; tests/test_label_scan.py runs the same
chunk algebra on the CPU at other lengths) and carry one state per ion from chunk to chunk and from
frame shard to frame shard; the ions sit in groups of 64 lanes, and k_ja_accumulate strides over the ions of a frame
256 at a time.  The generator below plants, on purpose, what those cuts can get wrong: dwells and unknown streaks that
span whole chunks, streaks that start or end on a chunk boundary, a first known label after a boundary-crossing streak
that is a jump against the carried-in site, jumps on the first and last frame of a chunk, ions never known, and several
ions making the same jump in one frame, more than 256 columns apart.  `test_generated_arrays_hold_every_feature` checks
(with detectors that do not share code with the generator) that every feature the shape has room for is there."""
import numpy as np
import pytest

CH = 256                                             # LS_CHUNK of the device scans

# (F, M): every F in {1, 2, 255, 256, 257, 769, 3000} and every M in {1, 63, 64, 65, 300, 448} at least once
SHAPES = [(1, 65), (2, 1), (255, 64), (256, 63), (257, 300), (769, 448), (3000, 1), (3000, 65), (3000, 448)]
MODE_LIMIT = 100000                                  # F x M above this: the oracle's running-mode loop sees bands only
FAR_IONS = (290, 440)                                # > 256 columns away from the ions 10-12


def n_sites(M):
    return max(12, M // 2 + 5)


def make_labels(F, M, seed=0):
    """A seeded [F, M] int64 label array over K = n_sites(M) sites: random dwells (a few longer than two chunks) and
    unknown stretches, then the planted features at fixed ions and frames (each only where the shape has room)."""
    K = n_sites(M)
    rng = np.random.default_rng(seed)
    lab = np.empty((F, M), dtype=np.int64)
    for j in range(M):
        f = 0
        while f < F:
            if rng.random() < 0.1:
                L, v = int(rng.geometric(0.25)), -1
            else:
                L = int(rng.integers(520, 700)) if rng.random() < 0.04 else int(rng.geometric(1 / 40.0))
                v = int(rng.integers(K))
            lab[f:f + L, j] = v
            f += L

    def other(*not_these):
        while True:
            s = int(rng.integers(K))
            if s not in not_these:
                return s

    def put(j, lo, hi, v):
        if j < M and lo < F and hi > 0:
            lab[max(lo, 0):min(hi, F), j] = v

    def streak(j, s, L):
        """-1 over [s, s + L) on ion j, a known site before it and a different one after it (a jump after the streak)."""
        if j >= M or s >= F:
            return
        a = other()
        put(j, s - 3, s, a)
        put(j, s, s + L, -1)
        put(j, s + L, s + L + 4, other(a))

    # ion 0: the highest site dwelling 600 frames, a jump on the last frame of chunk 2 (767) and on the first frame of
    # chunk 4 (1024), a 600-frame streak over the boundaries 1280 and 1536 ending in a jump (the carry's jump case)
    a = K - 1
    b = other(a)
    put(0, 0, 600, a)
    put(0, 600, 767, b)
    c = other(b)
    put(0, 767, 1024, c)
    d = other(c)
    put(0, 1024, 1100, d)
    put(0, 1100, 1700, -1)
    put(0, 1700, 1760, other(d))
    # ion 1: unknown from frame 0 for more than a chunk; ion 2: never known
    put(1, 0, 300, -1)
    put(1, 300, 340, other())
    put(2, 0, F, -1)
    # ion 3: streaks of 1, 2, 3 early (short arrays have them too)
    for s, L in ((10, 1), (20, 2), (30, 3)):
        streak(3, s, L)
    streak(4, 1, 255)                   # frames 1..255: ends on a chunk's last frame
    streak(5, 256, 256)                 # 256..511: starts on a boundary, ends on a chunk's last frame
    streak(6, 255, 257)                 # 255..511: crosses 256; the first known label (512) is a jump
    for s, L in ((256, 1), (510, 2), (766, 3)):
        streak(7, s, L)                 # on a boundary / ending on a chunk's last frame / across 768
    streak(8, 300, 700)                 # > 512 over the boundaries 512 and 768; the first known label (1000) jumps
    # ion 9: jumps on the last frame of chunk 0 and the first frame of chunk 1
    e = other()
    put(9, 200, 255, e)
    g = other(e)
    put(9, 255, 256, g)
    put(9, 256, 300, other(g))
    # the same jump (a -> b) in one frame by several ions, >256 columns apart, after dwells of different lengths (the
    # jump times differ: numpy's fancy-index += keeps the last duplicate's)
    fj = 700 if F > 700 else F - 1
    group = [j for j in (10, 11, 12) + FAR_IONS if j < M]
    if fj >= 1 and len(group) >= 3:
        a = other()
        b = other(a)
        for i, j in enumerate(group):
            dwell = 5 + 4 * i
            put(j, fj - dwell - 3, fj - dwell, other(a))
            put(j, fj - dwell, fj, a)
            put(j, fj, fj + 5, b)
    return lab, K


# ---- feature detectors (independent of the placement above) ------------------------------------------------------

def _runs(col, value=None):
    """Maximal runs of equal values in a column: (start, length, value)."""
    if len(col) == 0:
        return []
    edges = np.nonzero(np.diff(col))[0] + 1
    starts = np.concatenate([[0], edges])
    lens = np.diff(np.concatenate([starts, [len(col)]]))
    return [(int(s), int(L), int(col[s])) for s, L in zip(starts, lens) if value is None or col[s] == value]


def features(lab, K):
    F, M = lab.shape
    out = set()
    if lab.max() == K - 1:
        out.add("label_K-1")
    for j in range(M):
        col = lab[:, j]
        known = np.nonzero(col >= 0)[0]
        if len(known) == 0:
            out.add("never_known")
        elif known[0] > CH:
            out.add("unknown_from_0_beyond_a_chunk")
        for s, L, v in _runs(col):
            if v >= 0 and L > 2 * CH:
                out.add("dwell_beyond_two_chunks")
            if v == -1 and s > 0 and s + L < F:                    # a streak with known labels on both sides
                for want in (1, 2, 3, 255, 256, 257):
                    if L == want:
                        out.add("streak_%d" % want)
                if L > 2 * CH:
                    out.add("streak_beyond_512")
                if s % CH == 0:
                    out.add("streak_starts_on_boundary")
                if (s + L - 1) % CH == CH - 1:
                    out.add("streak_ends_on_chunk_end")
                e = s + L                                          # the first known label after it
                if e // CH > s // CH and col[e] != col[s - 1]:
                    out.add("jump_after_boundary_crossing_streak")
        f = np.arange(1, F)
        jumped = f[(col[1:] >= 0) & (col[:-1] >= 0) & (col[1:] != col[:-1])]
        if np.any(jumped % CH == 0):
            out.add("jump_on_first_frame_of_chunk")
        if np.any(jumped % CH == CH - 1):
            out.add("jump_on_last_frame_of_chunk")
    for f in range(1, F):
        prev, cur = lab[f - 1], lab[f]
        jm = (prev >= 0) & (cur >= 0) & (prev != cur)
        if jm.sum() < 3:
            continue
        pairs = prev[jm] * K + cur[jm]
        ions = np.nonzero(jm)[0]
        for p in np.unique(pairs):
            who = ions[pairs == p]
            if len(who) >= 3:
                out.add("same_jump_by_3_ions")
                if who.max() - who.min() > CH:
                    out.add("same_jump_ions_beyond_256_apart")
    return out


# (feature, [(min F, min M), ...]): present whenever the shape reaches one of the alternatives
EXPECTED = [
    ("label_K-1", [(1, 1)]),
    ("never_known", [(1, 3)]),
    ("unknown_from_0_beyond_a_chunk", [(301, 2)]),
    ("dwell_beyond_two_chunks", [(601, 1)]),
    ("streak_1", [(34, 4)]), ("streak_2", [(34, 4)]), ("streak_3", [(34, 4)]),
    ("streak_255", [(257, 5)]), ("streak_256", [(513, 6)]), ("streak_257", [(513, 7)]),
    ("streak_beyond_512", [(1001, 9), (1701, 1)]),
    ("streak_starts_on_boundary", [(258, 8), (513, 6)]),
    ("streak_ends_on_chunk_end", [(257, 5)]),
    ("jump_after_boundary_crossing_streak", [(513, 7), (1701, 1)]),
    ("jump_on_first_frame_of_chunk", [(257, 10), (1025, 1)]),
    ("jump_on_last_frame_of_chunk", [(257, 10), (768, 1)]),
    ("same_jump_by_3_ions", [(2, 13)]),
    ("same_jump_ions_beyond_256_apart", [(2, 291)]),
]


def expected_features(F, M):
    return {name for name, alts in EXPECTED if any(F >= f and M >= m for f, m in alts)}


@pytest.mark.parametrize("F,M", SHAPES)
def test_generated_arrays_hold_every_feature(F, M):
    lab, K = make_labels(F, M, seed=F * 1000 + M)
    assert lab.shape == (F, M) and lab.dtype == np.int64 and lab.min() >= -1 and lab.max() <= K - 1
    missing = expected_features(F, M) - features(lab, K)
    assert not missing, missing
    if F >= 3000 and M >= 448:
        assert expected_features(F, M) == {name for name, _ in EXPECTED}, "the largest shape must hold them all"
    if F >= 3000 and M >= 9:
        # the reference's max_time_unknown is the maximum of the LAST frame that had one above the threshold, not the
        # largest of all: the array must tell the two apart
        _, (mx, _, _) = _oracle().assign_to_last_known_site(lab, 3)
        assert mx < _longest_closed_unknown(lab)


def _longest_closed_unknown(lab):
    F, M = lab.shape
    best = 0
    for j in range(M):
        for s, L, v in _runs(lab[:, j]):
            if v == -1 and s + L < F:
                best = max(best, L)
    return best


def _oracle():
    from oracle import oracle
    oracle.lib()
    return oracle


# ---- GPU ----------------------------------------------------------------------------------------------------------

def _ctx(lab, frame0=0):
    from sitator_amd import _lib
    c = _lib.HipContext(np.eye(3) * 10.0)
    c.set_assignments(np.ascontiguousarray(lab), frame0=frame0)
    return c


def _sources(jl, F, M):
    """jump_sources' [F, M] array from a jump list."""
    from sitator_amd import _lib
    src = np.full((F, M), _lib.HipContext.JUMP_NONE, dtype=np.int64)
    for f, a, fr, _ in jl:
        src[f, a] = fr
    return src


def _splits(F):
    return sorted({s for s in (256, 300, F - 1) if 0 < s < F})


@pytest.mark.gpu
@pytest.mark.parametrize("F,M", SHAPES)
def test_jump_analysis_accumulators_and_shard_carry(oracle, F, M):
    lab, K = make_labels(F, M, seed=F * 1000 + M)
    exp = oracle.jump_analysis(lab, K)
    c = _ctx(lab)
    n_ij, tsum, tn, total, nprob, lout, tout = c.jump_analysis(K)
    assert np.array_equal(n_ij, exp["n_ij"])
    assert np.array_equal(tsum, exp["time_sum"])
    assert np.array_equal(tn, exp["time_n"])
    assert np.array_equal(total, exp["total_corrected_residences"])
    assert nprob == exp["n_problems"]
    for s in _splits(F):
        c1, c2 = _ctx(lab[:s]), _ctx(lab[s:], frame0=s)
        p1 = c1.jump_analysis(K)
        p2 = c2.jump_analysis(K, p1[5], p1[6])
        assert np.array_equal(p1[0] + p2[0], n_ij), s
        assert np.array_equal(p1[1] + p2[1], tsum), s
        assert np.array_equal(p1[2] + p2[2], tn), s
        assert np.array_equal(p1[3] + p2[3], total), s
        assert p1[4] + p2[4] == nprob, s
        assert np.array_equal(p2[5], lout) and np.array_equal(p2[6], tout), s


@pytest.mark.gpu
@pytest.mark.parametrize("F,M", SHAPES)
def test_jump_analysis_operator(oracle, F, M):
    from sitator_amd import JumpAnalysis
    from tests.test_next_tier import JA, _eq, _st
    lab, K = make_labels(F, M, seed=F * 1000 + M)
    exp = oracle.jump_analysis(lab, K)
    st = JumpAnalysis().run(_st(lab, K))
    for a in JA:
        assert _eq(getattr(st.site_network, a), exp[a]), a


@pytest.mark.gpu
@pytest.mark.parametrize("F,M", SHAPES)
def test_assign_to_last_known_site_and_shard_carry(oracle, F, M):
    from tests.test_next_tier import _st
    lab, K = make_labels(F, M, seed=F * 1000 + M)
    for thr in (1, 3, 256):
        t, (mx, avg, re) = oracle.assign_to_last_known_site(lab, thr)
        st = _st(lab, K)
        res = st.assign_to_last_known_site(frame_threshold=thr)
        assert np.array_equal(st.traj, t), thr
        assert res["max_time_unknown"] == mx and res["total_reassigned"] == re, thr
        assert res["avg_time_unknown"] == pytest.approx(avg, rel=1e-15, abs=0), thr
        labels, fmax, st3, lout, tout = _ctx(lab).assign_last_known(thr)
        assert np.array_equal(labels, t)
        for s in _splits(F):
            c1, c2 = _ctx(lab[:s]), _ctx(lab[s:], frame0=s)
            a1 = c1.assign_last_known(thr)
            a2 = c2.assign_last_known(thr, a1[3], a1[4])
            assert np.array_equal(np.concatenate([a1[0], a2[0]]), t), (thr, s)
            assert np.array_equal(np.concatenate([a1[1], a2[1]]), fmax), (thr, s)
            assert np.array_equal(a1[2] + a2[2], st3), (thr, s)
            assert np.array_equal(a2[3], lout) and np.array_equal(a2[4], tout), (thr, s)


@pytest.mark.gpu
@pytest.mark.parametrize("F,M", SHAPES)
@pytest.mark.parametrize("unknown_as_jump", [False, True])
def test_jumps_and_shard_carry(oracle, F, M, unknown_as_jump):
    lab, K = make_labels(F, M, seed=F * 1000 + M)
    exp = oracle.jumps(lab, unknown_as_jump=unknown_as_jump)
    c = _ctx(lab)
    rec, last = c.jump_list(unknown_as_jump)
    assert [tuple(r) for r in rec.tolist()] == exp
    src, last2 = c.jump_sources(unknown_as_jump)
    assert np.array_equal(src, _sources(exp, F, M)) and np.array_equal(last, last2)
    for s in _splits(F):
        c1, c2 = _ctx(lab[:s]), _ctx(lab[s:], frame0=s)
        r1, l1 = c1.jump_list(unknown_as_jump)
        r2, l2 = c2.jump_list(unknown_as_jump, l1)
        r2[:, 0] += s
        assert [tuple(r) for r in np.concatenate([r1, r2]).tolist()] == exp, s
        assert np.array_equal(l2, last), s
        s2, _ = c2.jump_sources(unknown_as_jump, l1)
        s1, _ = c1.jump_sources(unknown_as_jump)
        assert np.array_equal(np.concatenate([s1, s2]), src), s


@pytest.mark.gpu
@pytest.mark.parametrize("with_halo", [False, True])
def test_forward_scans_of_a_context_without_frames(with_halo):
    """F = 0: no chunk, so only the carry kernels run; they hand the carried-in state (or the start state) on unchanged."""
    K, M = 5, 3
    c = _ctx(np.empty((0, M), dtype=np.int64))
    last = np.array([2, -1, 4], dtype=np.int64) if with_halo else None
    other = np.array([7, 1, 300], dtype=np.int64) if with_halo else None
    for unknown_as_jump in (False, True):
        rec, lout = c.jump_list(unknown_as_jump, last)
        src, lout2 = c.jump_sources(unknown_as_jump, last)
        assert rec.shape == (0, 4) and src.shape == (0, M) and src.dtype == np.int64
        assert np.array_equal(lout, last if with_halo else [-1] * M) and np.array_equal(lout2, lout)
    n_ij, tsum, tn, total, nprob, lout, tout = c.jump_analysis(K, last, other)
    assert not n_ij.any() and not tsum.any() and not tn.any() and not total.any() and nprob == 0
    assert n_ij.shape == (K, K) and total.shape == (K,)
    assert np.array_equal(lout, last if with_halo else [-1] * M) and np.array_equal(tout, other if with_halo else [1] * M)
    labels, fmax, st3, lout, tout = c.assign_last_known(3, last, other)
    assert labels.shape == (0, M) and fmax.shape == (0,) and not st3.any()
    assert np.array_equal(lout, last if with_halo else [-1] * M) and np.array_equal(tout, other if with_halo else [0] * M)


@pytest.mark.gpu
@pytest.mark.parametrize("F,M", SHAPES)
def test_running_windowed_mode(oracle, F, M):
    """Both values of replace_no_winner_unknown, windows clipped at both ends, and the counts output; above MODE_LIMIT
    the oracle sees a band at each end (with a margin: the window is local) and a set of ions around the lane groups."""
    lab, K = make_labels(F, M, seed=F * 1000 + M)
    c = _ctx(lab)
    if F * M <= MODE_LIMIT:
        cols, bands = np.arange(M), [(0, F)]
    else:
        cols = np.array([j for j in (0, 1, 6, 8, 10, 63, 64, 65, 255, 256, 257, 290, 447) if j < M])
        bands = [(0, 300), (F - 300, F)]
    for thr, factor, repl in ((3, 2.1, True), (3, 2.1, False), (5, 2.1, True), (10, 2.1, False)):
        w = factor * thr
        wl, wr = int(np.floor(w / 2)), int(np.ceil(w / 2))
        out, counts = c.running_mode(wl, wr, thr, repl, n_sites=K)
        assert np.array_equal(counts, np.bincount(out[out >= 0], minlength=K))
        for lo, hi in bands:
            a, b = max(lo - wl - wr, 0), min(hi + wl + wr, F)
            e = oracle.running_windowed_mode(lab[a:b][:, cols], wl, wr, thr, K, repl)
            assert np.array_equal(out[lo:hi][:, cols], e[lo - a:hi - a]), (thr, repl, lo)


def make_occupancy_labels(F, M, K, offenders, seed=0):
    """Every frame a random one-to-one placement of the ions on the K >= M sites (some unknown); then, per
    (frame, site, ions), those ions put together on that site."""
    rng = np.random.default_rng(seed)
    lab = np.empty((F, M), dtype=np.int64)
    for f in range(F):
        lab[f] = rng.permutation(K)[:M]
    lab[rng.random((F, M)) < 0.05] = -1
    for f, s, ions in offenders:
        row = lab[f]
        row[row == s] = -1                      # the site's own occupant (if any) leaves
        row[list(ions)] = s
    return lab


@pytest.mark.gpu
@pytest.mark.parametrize("F,M", [(769, 448), (3000, 65), (257, 300)])
@pytest.mark.parametrize("max_per_site", [1, 2])
def test_occupancy_check_first_offender_and_statistics(oracle, F, M, max_per_site):
    """The first offender is the lowest frame, then the lowest site, whatever block of 64 frames or group of ions
    holds it; frame0 shifts the reported frame; without offenders the statistics equal the oracle's."""
    from sitator_amd import _lib
    K = M + 20
    n = max_per_site + 1
    far = [0, M - 1] + list(range(1, n - 1))            # ions more than 256 apart where M allows
    late = [(F - 1, 3, far), (F - 1, 1, list(range(5, 5 + n))), (F // 2, 7, list(range(20, 20 + n)))]
    first = (70, K - 1, far)                            # in the second 64-frame block
    same_frame_lower_site = (first[0], 2, list(range(30, 30 + n)))
    for offenders, want in ((late, (F // 2, 7)), (late + [first], (first[0], K - 1)),
                            (late + [first, same_frame_lower_site], (first[0], 2))):
        lab = make_occupancy_labels(F, M, K, offenders, seed=F + M)
        with pytest.raises(oracle.OracleError) as ei:
            oracle.check_multiple_occupancy(lab, K, max_per_site)
        assert (ei.value.frame, ei.value.site) == want
        for frame0 in (0, 1000):
            rc, _, _, _, err = _ctx(lab, frame0=frame0).check_occupancy(K, max_per_site)
            assert rc == _lib.E_MULTIPLE_OCCUPANCY and (err.frame, err.index) == (frame0 + want[0], want[1])
    # no offender: doubles below the limit only (max_per_site 2), or none at all
    doubles = [(f, s, [f % M, (f + M // 2) % M]) for f, s in ((5, 1), (64, 2), (200, 3)) if f < F] \
        if max_per_site == 2 else []
    lab = make_occupancy_labels(F, M, K, doubles, seed=F + M + 1)
    n_multi, avg = oracle.check_multiple_occupancy(lab, K, max_per_site)
    rc, n_multi2, total, nsites, _ = _ctx(lab).check_occupancy(K, max_per_site)
    assert rc == _lib.OK and n_multi2 == n_multi and total / nsites == avg
    assert n_multi == len(doubles)


@pytest.mark.gpu
@pytest.mark.parametrize("F,M", SHAPES)
def test_site_counts(F, M):
    lab, K = make_labels(F, M, seed=F * 1000 + M)
    assert np.array_equal(_ctx(lab).site_counts(K), np.bincount(lab[lab >= 0], minlength=K))


# ---- the staged copies of labels and positions (transfer.hip), at a size that goes round the ring --------------------------

@pytest.fixture
def small_ring(monkeypatch):
    """Ring chunks of 64 KB and every read-back staged: a copy of a megabyte laps the 16 slots."""
    monkeypatch.setenv("SITATOR_RING_CHUNK_KB", "64")
    monkeypatch.setenv("SITATOR_STAGED_D2H_MB", "0")


@pytest.mark.gpu
@pytest.mark.parametrize("F,M", [(601, 256), (3, 5)])
def test_labels_and_confidences_read_back_bit_for_bit(small_ring, F, M):
    """[601, 256]: 1 230 848 bytes per array = 19 chunks of 64 KB, more than one lap, the last one partial; [3, 5] is
    the control below one chunk."""
    rng = np.random.default_rng(F)
    lab = rng.integers(-1, 50, size=(F, M))
    lab[0, 0] = lab[-1, -1] = -1
    conf = rng.uniform(size=(F, M))
    c = _ctx(lab)
    c.set_assignments(lab, conf)
    got_lab, got_conf, _ = c.assignments()
    assert np.array_equal(got_lab.reshape(F, M), lab)
    assert np.array_equal(got_conf.view(np.uint64).reshape(F, M), conf.view(np.uint64))
    c.close()


@pytest.mark.gpu
def test_host_positions_pass_through_the_clamp_bit_for_bit(small_ring):
    """Every role -1 and no wrapping: the output is the input.  [601, 100, 3] is 1 442 400 bytes = 23 chunks of 64 KB, up
    through copy_to_device and back through the staged copy_to_host."""
    F, M, A = 601, 256, 100
    rng = np.random.default_rng(7)
    c = _ctx(rng.integers(-1, 50, size=(F, M)))
    pos = rng.normal(scale=20.0, size=(F, A, 3))
    out = c.clamp_trajectory(np.full(A, -1), np.zeros((A, 3)), np.zeros((0, 3)), False, False, positions=pos)
    assert np.array_equal(out.view(np.uint64), pos.view(np.uint64))
    c.close()
