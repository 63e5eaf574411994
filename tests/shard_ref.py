"""Shared by tests/test_shard_chains.py (CPU, a numpy stand-in for the device) and tests/test_gpu_shard_chains.py (GPU):
operators and chains of operators on FRAME SHARDS - a ``SiteTrajectory`` per rank over a contiguous block of the frames,
with a communicator - against the same calls on the whole array on one rank.

* ``designed()``: a small label array in which every hand-over between ranks decides something (``designed_features``
  finds each case again from the array alone), with cuts for 2, 3 and 5 ranks; the five-rank cut has a rank without
  frames and one shorter than every smoothing window.
* ``random_case(seed)``: a seeded family of shapes, cuts and labels.
* ``run_ranks``: a thread and a trajectory per rank; it never waits for ever.
* ``check_*``: the comparisons, everything with exact equality (all quantities are integers or quotients of the same
  integers)."""
import threading

import numpy as np

from tests.cooccupancy_ref import plain_network
from tests.test_next_tier import JA, _eq

CUTS = {2: [0, 40, 96], 3: [0, 40, 70, 96], 5: [0, 40, 40, 43, 70, 96]}
SMOOTH_MODES = ((3, 2.1, True), (3, 2.1, False), (5, 2.1, True), (10, 2.1, False))     # threshold, factor, set unassigned
# 1, 3, 40 and one more: the unknown streak of four frames that straddles frame 70 ends after it and is longer than 1 and
# 3, so at those thresholds the last frame above the threshold is the last rank's; at 4 it lies before frame 70 (and at 40
# there is a single streak above the threshold)
ASSIGN_THRESHOLDS = (1, 3, 4, 40)
RULE_THRESHOLD = 4
SEEDS = tuple(range(12))
JOIN_TIMEOUT = 120.0          # seconds for all ranks of one run together; a run takes a fraction of a second


# ---- inputs ------------------------------------------------------------------------------------------------------------

def designed(F=96, M=7, K=14):
    """(labels[96, 7], K = 14, cuts).  Ion by ion (sites in brackets):

    0 [0, 1]    on 0, unknown over 38..43 (across frame 40; all of rank 2 of the five-rank cut), then on 1: the source of
                the jump at 44 is known on rank 0 only; 1 -> 0 at 80 and 0 -> 1 at 88 (what the threshold merge joins)
    1 [2, 3]    2 -> 3 exactly at frame 40; unknown over 69, 70, 71 (three frames across 70), then on 2
    2 [4, 5]    unknown over 20..29 (ten frames, ends at 30) and over 50..55 (six frames, ends at 56); 4 -> 5 exactly at
                frame 70; on ion 1's site in frame 60 (site 3) and in frame 75 (site 2): the double occupancies
    3 [6]       on 6, unknown from frame 37 to the end: all of [40, 70) and of every later rank
    4 [8, 9]    never known before frame 44; unknown over 68..71 (four frames across 70), then on 9 (last rank only)
    5           never known
    6 [10..13]  on 11, on 10 for exactly 39, 40, 41, on 12, on 13 for 69 and 70 only, on 12 again

    Site 7 is never visited."""
    assert (F, M, K) == (96, 7, 14)
    lab = np.full((F, M), -1, dtype=np.int64)
    lab[0:38, 0], lab[44:80, 0], lab[80:88, 0], lab[88:, 0] = 0, 1, 0, 1
    lab[0:40, 1], lab[40:69, 1], lab[72:, 1] = 2, 3, 2
    lab[0:20, 2], lab[30:50, 2], lab[56:70, 2], lab[70:, 2] = 4, 4, 4, 5
    lab[60, 2], lab[75, 2] = 3, 2
    lab[0:37, 3] = 6
    lab[44:68, 4], lab[72:, 4] = 8, 9
    lab[0:39, 6], lab[39:42, 6], lab[42:69, 6], lab[69:71, 6], lab[71:, 6] = 11, 10, 12, 13, 12
    return lab, K, {n: list(c) for n, c in CUTS.items()}


def random_case(seed):
    """(labels[F, M], K, cut): F in 60..200, M in 1..7, K in 4..16, 2..4 ranks.  The cuts are drawn from 1..F with
    repetition: neighbouring cuts may be equal (a rank without frames) and may equal F (trailing ranks without frames,
    what ``shard_frames`` gives a short trajectory); rank 0 always holds a frame, as it does there.  Every ion dwells on
    random sites for geometric times (mean 12 frames); about 8 % of the labels are unknown, in runs (mean 3 frames)."""
    rng = np.random.default_rng(1000 + seed)
    F, M, K = int(rng.integers(60, 201)), int(rng.integers(1, 8)), int(rng.integers(4, 17))
    n = int(rng.integers(2, 5))
    cut = [0] + sorted(int(c) for c in rng.integers(1, F + 1, size=n - 1)) + [F]
    lab = np.empty((F, M), dtype=np.int64)
    for j in range(M):
        f = 0
        while f < F:
            L = int(rng.geometric(1 / 12.0))
            lab[f:f + L, j] = rng.integers(K)
            f += L
        f = int(rng.geometric(1 / 35.0))
        while f < F:
            L = int(rng.geometric(1 / 3.0))
            lab[f:f + L, j] = -1
            f += L + int(rng.geometric(1 / 35.0))
    return lab, K, cut


def has_known_cut(lab, cut):
    """Some cut with frames on both sides at which some ion is known in the frame before it and in the frame after."""
    return any(0 < c < len(lab) and ((lab[c - 1] >= 0) & (lab[c] >= 0)).any() for c in cut[1:-1])


def _runs(col):
    """Maximal runs of equal values: (start, length, value)."""
    edges = np.nonzero(np.diff(col))[0] + 1
    starts = np.concatenate([[0], edges])
    lens = np.diff(np.concatenate([starts, [len(col)]]))
    return [(int(s), int(L), int(col[s])) for s, L in zip(starts, lens)]


def _closed_streaks(lab):
    """(end frame, length) of every unknown run that a known label ends, all ions."""
    return [(s + L, L) for j in range(lab.shape[1]) for s, L, v in _runs(lab[:, j]) if v == -1 and s + L < len(lab)]


def designed_features(lab, K, oracle):
    """The names of the designed cases found in ``lab`` - by detectors that share nothing with ``designed``."""
    F, M = lab.shape
    out = set()
    for j in range(M):
        col = lab[:, j]
        known = np.nonzero(col >= 0)[0]
        if len(known) == 0:
            out.add("never_known")
            continue
        if known[0] >= 40:
            out.add("never_known_before_40")
        if not (col[40:70] >= 0).any() and (col[:40] >= 0).any():
            out.add("silent_through_40_70")
        for c in (40, 70):
            if col[c - 1] >= 0 and col[c] >= 0 and col[c - 1] != col[c]:
                out.add("jump_at_%d" % c)
        for s, L, v in _runs(col):
            if v != -1 or s == 0 or s + L >= F:
                continue
            if s < 40 < s + L and col[s - 1] != col[s + L]:
                out.add("streak_across_40_between_different_sites")
            if s <= 40 and s + L >= 43 and col[s - 1] != col[s + L]:
                out.add("streak_over_all_of_40_43")
            if s < 70 < s + L and L in (3, 4):
                out.add("streak_%d_across_70" % L)
    # max_time_unknown at RULE_THRESHOLD: the last frame at which a streak above the threshold ends lies before frame 70,
    # its value is below that of an earlier, longer streak, and rank 0 of the three-rank cut has such a frame at a LOCAL
    # number above that frame's local number in rank 1 (frame numbers that start at 0 on every rank pick another value)
    over = sorted(e for e in _closed_streaks(lab) if e[1] > RULE_THRESHOLD)
    if over:
        end, _ = over[-1]
        value = max(L for e, L in over if e == end)
        answer = oracle.assign_to_last_known_site(lab, RULE_THRESHOLD)[1][0]
        rank0 = [(e, L) for e, L in over if e < 40]
        if 40 <= end < 70 and answer == value and any(L > value and e < end for e, L in over) \
                and rank0 and rank0[-1][0] > end - 40 and rank0[-1][1] != value:
            out.add("max_time_unknown_rule")
    double = [f for f in range(F) if np.unique(lab[f][lab[f] >= 0], return_counts=True)[1].max(initial=0) > 1]
    if double and 40 <= double[0] < 70 and double[-1] >= 70:
        out.add("double_occupancy_in_two_ranks_none_in_the_first")
        if double[-1] - 70 < double[0] - 40:
            out.add("later_double_occupancy_has_the_lower_local_frame")
    visited = np.unique(lab[lab >= 0])
    if any((lab[70:] == s).any() and not (lab[:70] == s).any() for s in visited):
        out.add("site_of_the_last_rank_only")
    if len(np.setdiff1d(np.arange(K - 1), visited)):
        out.add("site_never_visited_below_the_last")
    # smoothing at (threshold 3, factor 2.1): windows of [f - 3, f + 4)
    whole = oracle.running_windowed_mode(lab, 3, 4, 3, K, True)
    pieces = np.concatenate([oracle.running_windowed_mode(lab[a:b], 3, 4, 3, K, True) for a, b in ((0, 40), (40, 70), (70, F))])
    for j in range(M):
        col = lab[:, j]
        if col[38] != col[39] and col[39] == col[40] == col[41] != col[42] and col[39] >= 0:
            if (whole[39:42, j] == col[39]).all() and not (pieces[39:42, j] == col[39]).all():
                out.add("dwell_39_41_survives_only_with_both_sides")
        s = col[69]
        if s >= 0 and col[70] == s and (lab == s).sum() == 2 and not (whole == s).any():
            out.add("blip_69_70_on_its_own_site_smoothed_away")
    return out


DESIGNED_FEATURES = {
    "never_known", "never_known_before_40", "silent_through_40_70", "jump_at_40", "jump_at_70",
    "streak_across_40_between_different_sites", "streak_over_all_of_40_43", "streak_3_across_70", "streak_4_across_70",
    "max_time_unknown_rule", "double_occupancy_in_two_ranks_none_in_the_first",
    "later_double_occupancy_has_the_lower_local_frame", "site_of_the_last_rank_only", "site_never_visited_below_the_last",
    "dwell_39_41_survives_only_with_both_sides", "blip_69_70_on_its_own_site_smoothed_away"}


# ---- the harness ---------------------------------------------------------------------------------------------------------

def trajectory(lab, K, lo=0, hi=None, comm=None):
    """A ``SiteTrajectory`` over frames lo:hi of ``lab``; with ``comm`` a frame shard whose first frame is ``lo``."""
    from sitator_amd import SiteTrajectory
    hi = len(lab) if hi is None else hi
    return SiteTrajectory(plain_network(lab.shape[1], K), lab[lo:hi], _comm=comm, _frame0=lo)


def run_ranks(work, lab, K, cut, timeout=JOIN_TIMEOUT):
    """``(single, joined, failures)``: ``work(st)`` of the whole array on one rank, and of every rank's shard (frames
    ``cut[r]:cut[r + 1]``) with a thread per rank, in rank order.  A rank that fails releases the others (``abort``) and
    is reported as ``(rank, repr)``; the threads are joined with a time limit, and one that is still alive afterwards is
    reported as a failure too - the caller asserts ``not failures``."""
    import time
    from sitator_amd.sharding import ThreadComm
    single = work(trajectory(lab, K))
    comms = ThreadComm.group(len(cut) - 1)
    joined, failures = [None] * len(comms), []

    def rank(r):
        try:
            joined[r] = work(trajectory(lab, K, cut[r], cut[r + 1], comms[r]))
        except BaseException as e:                               # noqa: BLE001 - reported by the caller
            failures.append((r, repr(e)))
            comms[r].abort()

    threads = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(len(comms))]
    for t in threads:
        t.start()
    deadline = time.monotonic() + timeout
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [r for r, t in enumerate(threads) if t.is_alive()]
    if alive:
        comms[0].abort()                                         # whoever waits at the barrier leaves it
        failures.append((alive, "still running after %.0f s" % timeout))
    return single, joined, failures


def is_shard(st, comm_size, lo):
    return st._comm is not None and st._comm.size == comm_size and st._frame0 == lo


def network_state(sn):
    """What the ranks must agree on: the number of sites, the centres and the six attributes of JumpAnalysis (if set)."""
    state = {"n_sites": int(sn.n_sites), "centers": np.array(sn.centers, copy=True)}
    for a in JA:
        if sn.has_attribute(a):
            state[a] = np.array(getattr(sn, a), copy=True)
    return state


def same_state(a, b):
    return a.keys() == b.keys() and a["n_sites"] == b["n_sites"] and all(_eq(a[k], b[k]) for k in a if k != "n_sites")


def snapshot(st, n_ranks=None, lo=None):
    """(labels, network state[, whether the trajectory is the rank's shard])."""
    snap = {"traj": np.array(st._traj, copy=True), "net": network_state(st.site_network)}
    if n_ranks is not None:
        snap["shard"] = is_shard(st, n_ranks, lo)
    return snap


def assert_joined(single, parts, what=""):
    """The ranks' snapshots against the single-rank one: labels joined in rank order, the network on every rank."""
    assert np.array_equal(np.concatenate([p["traj"] for p in parts]), single["traj"]), what
    for r, p in enumerate(parts):
        assert same_state(p["net"], single["net"]), (what, r)
        assert p.get("shard", True), (what, r, "the derived trajectory lost its communicator or its first frame")


# ---- the checks ------------------------------------------------------------------------------------------------------------

def check_jump_analysis(oracle, lab, K, cut):
    from sitator_amd import JumpAnalysis
    exp = oracle.jump_analysis(lab, K)
    single, joined, failures = run_ranks(lambda st: network_state(JumpAnalysis().run(st).site_network), lab, K, cut)
    assert not failures, failures
    for state in [single] + joined:
        for a in JA:
            assert _eq(state[a], exp[a]), a


def check_jumps(oracle, lab, K, cut, unknown_as_jump):
    exp = oracle.jumps(lab, unknown_as_jump=unknown_as_jump)

    def work(st):
        by_frame = [(f, list(zip(a.tolist(), fr.tolist(), to.tolist())))
                    for f, a, fr, to in st.jumps_by_frame(unknown_as_jump=unknown_as_jump)]
        return list(st.jumps(unknown_as_jump=unknown_as_jump)), by_frame

    single, joined, failures = run_ranks(work, lab, K, cut)
    assert not failures, failures
    assert single[0] == exp
    assert [j for part in joined for j in part[0]] == exp
    by_frame = [x for part in joined for x in part[1]]
    assert [f for f, _ in by_frame] == list(range(1, len(lab)))          # every frame once, in order
    assert [(f,) + j for f, js in by_frame for j in js] == exp
    assert by_frame == single[1]


def check_assign(oracle, lab, K, cut, threshold):
    t, (mx, avg, re) = oracle.assign_to_last_known_site(lab, threshold)

    def work(st):
        res = st.assign_to_last_known_site(frame_threshold=threshold)
        return res, np.array(st._traj, copy=True), list(st.jumps())      # the jumps: the device labels are the new ones

    single, joined, failures = run_ranks(work, lab, K, cut)
    assert not failures, failures
    assert np.array_equal(single[1], t)
    assert single[0] == {"max_time_unknown": mx, "avg_time_unknown": avg, "total_reassigned": re}
    assert np.array_equal(np.concatenate([p[1] for p in joined]), t)
    for p in joined:
        assert p[0] == single[0], (p[0], single[0])
    assert [j for p in joined for j in p[2]] == single[2]


def check_occupancy(oracle, lab, K, cut):
    from sitator_amd import errors

    def work(st):
        try:
            st.check_multiple_occupancy(max_mobile_per_site=1)
            first = None
        except errors.MultipleOccupancyError as e:
            first = (int(e.frame), int(e.site), [int(m) for m in e.mobile_particles])
        try:
            two = st.check_multiple_occupancy(max_mobile_per_site=2)
        except errors.MultipleOccupancyError as e:
            two = ("raised", int(e.frame), int(e.site))
        return first, two, st.compute_site_occupancies()

    single, joined, failures = run_ranks(work, lab, K, cut)
    assert not failures, failures
    try:
        oracle.check_multiple_occupancy(lab, K, 1)
        assert single[0] is None
    except oracle.OracleError as e:
        assert single[0] == (e.frame, e.site, [int(m) for m in e.mobile])
    assert np.array_equal(single[2], np.bincount(lab[lab >= 0], minlength=K) / len(lab))
    for p in joined:
        assert p[0] == single[0], (p[0], single[0])               # frame, site and ions, on every rank
        assert p[1] == single[1], (p[1], single[1])
        assert np.array_equal(p[2], single[2])


def check_smoothing(oracle, lab, K, cut, mode, remove):
    from sitator_amd import SmoothSiteTrajectory, errors
    threshold, factor, set_unassigned = mode
    n = len(cut) - 1

    def work(st):
        before = np.array(st._traj, copy=True)
        try:
            new = SmoothSiteTrajectory(window_threshold_factor=factor, remove_unoccupied_sites=remove,
                                       set_unassigned_under_threshold=set_unassigned).run(st, threshold)
        except errors.InsufficientSitesError as e:
            return ("InsufficientSitesError", e.n_sites, e.n_mobile)
        assert np.array_equal(st._traj, before)
        return snapshot(new, n if st._comm is not None else None, st._frame0)

    single, joined, failures = run_ranks(work, lab, K, cut)
    assert not failures, failures
    if isinstance(single, tuple):
        assert all(p == single for p in joined), (single, joined)
        return
    assert not any(isinstance(p, tuple) for p in joined), [p for p in joined if isinstance(p, tuple)]
    if not remove:
        w = factor * threshold
        exp = oracle.running_windowed_mode(lab, int(np.floor(w / 2)), int(np.ceil(w / 2)), threshold, K, set_unassigned)
        assert np.array_equal(single["traj"], exp) and single["net"]["n_sites"] == K
    assert_joined(single, joined, (mode, remove))


def check_input_labels_stay_resident(oracle, lab, K, cut):
    """After SmoothSiteTrajectory the labels in the INPUT's device context are still the input's: its jumps afterwards
    are the jumps of the unsmoothed labels."""
    from sitator_amd import SmoothSiteTrajectory
    exp = oracle.jumps(lab)

    def work(st):
        first = list(st.jumps())                                  # (the context exists and holds the labels)
        SmoothSiteTrajectory(remove_unoccupied_sites=False).run(st, 3)
        return first, list(st.jumps())

    single, joined, failures = run_ranks(work, lab, K, cut)
    assert not failures, failures
    assert single == (exp, exp)
    assert [j for p in joined for j in p[0]] == exp and [j for p in joined for j in p[1]] == exp


def chain_1(st, n_ranks=None):
    """assign_to_last_known_site(3) -> SmoothSiteTrajectory -> JumpAnalysis -> MergeSitesByThreshold("n_ij") ->
    RemoveUnoccupiedSites -> JumpAnalysis -> jumps(); a snapshot after every step.  The smoothing keeps the unoccupied
    sites, so that the step named after removing them has something to remove."""
    from sitator_amd import JumpAnalysis, MergeSitesByThreshold, RemoveUnoccupiedSites, SmoothSiteTrajectory
    lo = st._frame0
    steps = []

    def keep(name, t, **more):
        steps.append(dict(snapshot(t, n_ranks, lo), name=name, **more))

    res = st.assign_to_last_known_site(frame_threshold=3)
    keep("assign", st, result=res)
    st = SmoothSiteTrajectory(remove_unoccupied_sites=False).run(st, 3)
    keep("smooth", st)
    JumpAnalysis().run(st)
    keep("jump analysis", st)
    st = MergeSitesByThreshold("n_ij", check_types=False).run(st, threshold=1)
    keep("merge", st)
    st, kept = RemoveUnoccupiedSites().run(st, return_kept_sites=True)
    keep("remove", st, kept=kept[0])
    JumpAnalysis().run(st)
    keep("jump analysis 2", st, jumps=list(st.jumps()), occupancies=st.compute_site_occupancies())
    return steps


def chain_2(st, n_ranks=None):
    """ReplaceUnassignedPositions(replace_with_last_known) -> JumpAnalysis."""
    from sitator_amd import JumpAnalysis, ReplaceUnassignedPositions as RUP
    lo = st._frame0
    new = RUP(RUP.replace_with_last_known).run(st)
    steps = [dict(snapshot(new, n_ranks, lo), name="replace")]
    JumpAnalysis().run(new)
    steps.append(dict(snapshot(new, n_ranks, lo), name="jump analysis", jumps=list(new.jumps())))
    return steps


def check_chain(oracle, chain, lab, K, cut):
    n = len(cut) - 1
    single, joined, failures = run_ranks(lambda st: chain(st, n if st._comm is not None else None), lab, K, cut)
    assert not failures, failures
    for i, step in enumerate(single):
        parts = [p[i] for p in joined]
        assert_joined(step, parts, step["name"])
        if "result" in step:
            assert all(p["result"] == step["result"] for p in parts), step["name"]
        if "kept" in step:
            assert all(np.array_equal(p["kept"], step["kept"]) for p in parts), step["name"]
        if "jumps" in step:
            assert [j for p in parts for j in p["jumps"]] == step["jumps"], step["name"]
        if "occupancies" in step:
            assert all(np.array_equal(p["occupancies"], step["occupancies"]) for p in parts), step["name"]
    by_name = {s["name"]: s for s in single}
    if chain is chain_1:
        # the single-rank chain against the oracle where the oracle has the operation, and: both steps do something
        t, _ = oracle.assign_to_last_known_site(lab, 3)
        assert np.array_equal(by_name["assign"]["traj"], t)
        sm = oracle.running_windowed_mode(t, 3, 4, 3, K, True)
        assert np.array_equal(by_name["smooth"]["traj"], sm)
        ja = oracle.jump_analysis(sm, K)
        for a in JA:
            assert _eq(by_name["jump analysis"]["net"][a], ja[a]), a
        assert by_name["merge"]["net"]["n_sites"] < K, "the merge merges nothing"
        assert by_name["remove"]["net"]["n_sites"] < by_name["merge"]["net"]["n_sites"], "the removal removes nothing"
        ja2 = oracle.jump_analysis(by_name["remove"]["traj"], by_name["remove"]["net"]["n_sites"])
        for a in JA:
            assert _eq(by_name["jump analysis 2"]["net"][a], ja2[a]), a
        assert by_name["jump analysis 2"]["jumps"] == oracle.jumps(by_name["remove"]["traj"])
    else:
        from tests import replace_ref
        filled = replace_ref.replace(lab, 0)
        assert np.array_equal(by_name["replace"]["traj"], filled)
        ja = oracle.jump_analysis(filled, K)
        for a in JA:
            assert _eq(by_name["jump analysis"]["net"][a], ja[a]), a
        assert by_name["jump analysis"]["jumps"] == oracle.jumps(filled)
