"""CPU: operators and chains of operators on frame shards (tests/shard_ref.py) with a numpy stand-in for the device.

The stand-in restates the label entry points of ``_lib.HipContext`` that the shard code calls - ``jump_analysis``,
``assign_last_known``, ``running_mode``, ``label_ends`` / ``replace_unassigned``, ``cooccupancy``, ``site_counts`` - as
plain loops over frames and ions with the carried state explicit.  Each restatement is first pinned to the oracle (the
whole array, and two pieces with the carry handed over, at every cut); then the same checks as on the GPU
(tests/test_gpu_shard_chains.py) run through the product's own shard loops, halo exchange and derived trajectories.
The two generator tests at the top need nothing but numpy and the oracle."""
import numpy as np
import pytest

from tests import cooccupancy_ref, replace_ref
from tests import shard_ref as S
from tests.fake_ctx import FakeContext

LAB, K, CUTS = S.designed()
ALL_CUTS = sorted({c for cut in CUTS.values() for c in cut[1:-1]})


# ---- the generators ------------------------------------------------------------------------------------------------------

def test_designed_labels_hold_every_feature(oracle):
    assert LAB.shape == (96, 7) and LAB.dtype == np.int64 and LAB.min() == -1 and LAB.max() == K - 1
    assert CUTS == {2: [0, 40, 96], 3: [0, 40, 70, 96], 5: [0, 40, 40, 43, 70, 96]}
    missing = S.DESIGNED_FEATURES - S.designed_features(LAB, K, oracle)
    assert not missing, missing
    # and the detectors do not see them where they are not: without the frames either side of the cuts
    assert not S.designed_features(np.delete(LAB, np.r_[36:46, 66:76], axis=0), K, oracle) & {
        "jump_at_40", "jump_at_70", "streak_3_across_70", "streak_4_across_70", "dwell_39_41_survives_only_with_both_sides"}


@pytest.mark.parametrize("seed", S.SEEDS)
def test_seeded_cases_have_a_cut_between_known_labels(seed):
    lab, k, cut = S.random_case(seed)
    F, M = lab.shape
    assert 60 <= F <= 200 and 1 <= M <= 7 and 4 <= k <= 16 and 3 <= len(cut) <= 5
    assert cut[0] == 0 and cut[-1] == F and cut[1] > 0 and cut == sorted(cut)
    assert lab.min() == -1 and lab.max() < k
    assert S.has_known_cut(lab, cut)


def test_seeded_family_as_a_whole():
    """About 8 % of all labels are unknown, and some case has a rank without frames."""
    cases = [S.random_case(seed) for seed in S.SEEDS]
    unknown = sum(int((lab == -1).sum()) for lab, _, _ in cases) / sum(lab.size for lab, _, _ in cases)
    assert 0.06 < unknown < 0.10, unknown
    assert any(len(set(cut)) < len(cut) for _, _, cut in cases)


# ---- the stand-in ----------------------------------------------------------------------------------------------------------

class ShardFakeContext(FakeContext):
    ENDS_NONE = replace_ref.NONE

    def _lab(self):
        return self._labels.reshape(self.F, self.M)

    def jump_analysis(self, K, last_known_in=None, time_at_current_in=None):
        """dynamics/JumpAnalysis.py:75-108 frame by frame.  Two ions that do the same thing in one frame count once (the
        reference adds with a fancy index), and the time of the last of them is the one recorded."""
        lab = self._lab()
        F, M = lab.shape
        if last_known_in is None:
            last = [int(v) for v in lab[0]] if F else [-1] * M
            tac = [1] * M
        else:
            last, tac = [int(v) for v in last_known_in], [int(v) for v in time_at_current_in]
        n_ij, tsum = np.zeros((K, K)), np.zeros((K, K))
        tn, total = np.zeros((K, K), dtype=np.int64), np.zeros(K, dtype=np.int64)
        problems = 0
        for f in range(F):
            sites, pairs, times = set(), set(), {}
            for j in range(M):
                cur = int(lab[f, j])
                now = last[j] if cur == -1 else cur
                if max(now, last[j]) >= K:
                    raise IndexError("index %d is out of bounds for axis 0 with size %d" % (max(now, last[j]), K))
                if now < 0 or last[j] < 0:
                    problems += 1
                    tac[j] += 1
                else:
                    sites.add(now)
                    pairs.add((last[j], now))
                    if now != last[j]:
                        times[(last[j], now)] = tac[j]
                        tac[j] = 1
                    else:
                        tac[j] += 1
                if cur != -1:
                    last[j] = cur
            for s in sites:
                total[s] += 1
            for a, b in pairs:
                n_ij[a, b] += 1
            for (a, b), t in times.items():
                tsum[a, b] += t
                tn[a, b] += 1
        return n_ij, tsum, tn, total, problems, np.array(last, dtype=np.int64), np.array(tac, dtype=np.int64)

    def assign_last_known(self, frame_threshold, last_known_in=None, time_unknown_in=None, out=None):
        """SiteTrajectory.py:235-304 ion by ion; the resident labels become the new ones."""
        lab = self._lab()
        F, M = lab.shape
        new = lab.copy()
        fmax = np.zeros(F, dtype=np.int32)
        st3 = np.zeros(3, dtype=np.int64)
        lout, tout = np.empty(M, dtype=np.int64), np.empty(M, dtype=np.int64)
        for j in range(M):
            last = -1 if last_known_in is None else int(last_known_in[j])
            unknown_for = 0 if time_unknown_in is None else int(time_unknown_in[j])
            for f in range(F):
                if lab[f, j] != -1:
                    last = int(lab[f, j])
                    if unknown_for:
                        fmax[f] = max(fmax[f], unknown_for)
                        st3[0] += unknown_for
                        st3[1] += 1
                    unknown_for = 0
                else:
                    if unknown_for < frame_threshold:
                        new[f, j] = last
                        st3[2] += 1
                    unknown_for += 1
            lout[j], tout[j] = last, unknown_for
        self.labels_version += 1
        self.labels_digest = None
        self._labels = new.reshape(-1).copy()
        if out is not None:
            out[...] = new
            new = out
        return new, fmax, st3, lout, tout

    def running_mode(self, wleft, wright, threshold, replace_unknown, n_sites=0):
        """dynamics/SmoothSiteTrajectory.pyx:79-111: the most frequent label of [f - wleft, f + wright), the lowest one
        (unknown first) among equals, if it occurs ``threshold`` times."""
        lab = self._lab()
        F, M = lab.shape
        out = lab.copy()
        for j in range(M):
            for f in range(F):
                window = [int(v) for v in lab[max(f - wleft, 0):min(f + wright, F), j]]
                best = max(window.count(v) for v in window)
                winner = min(v for v in window if window.count(v) == best)
                if best >= threshold:
                    out[f, j] = winner
                elif replace_unknown:
                    out[f, j] = -1
        if n_sites > 0:
            return out, np.bincount(out[out >= 0], minlength=int(n_sites)).astype(np.int64)
        return out

    def label_ends(self):
        return replace_ref.ends(self._lab())

    def replace_unassigned(self, mode, before_in=None, after_in=None):
        return replace_ref.replace(self._lab(), mode, before_in, after_in)

    def cooccupancy(self, K):
        return cooccupancy_ref.brute_cooccupancy(self._lab(), int(K))


@pytest.fixture
def fake_device(monkeypatch):
    from sitator_amd import _lib, pbc
    monkeypatch.setattr(_lib, "HipContext", ShardFakeContext)
    monkeypatch.setattr(pbc, "HipContext", ShardFakeContext)


def _ctx(lab, frame0=0):
    c = ShardFakeContext(np.eye(3) * 12.0)
    c.set_assignments(np.ascontiguousarray(lab), frame0=frame0)
    return c


def test_the_stand_in_exposes_what_the_device_wrapper_does():
    from sitator_amd import _lib
    for name in ("jump_analysis", "assign_last_known", "running_mode", "label_ends", "replace_unassigned", "cooccupancy",
                 "site_counts", "check_occupancy", "jump_list", "set_assignments", "close", "ENDS_NONE", "JUMP_NONE"):
        assert hasattr(_lib.HipContext, name) and hasattr(ShardFakeContext, name), name
    assert ShardFakeContext.ENDS_NONE == _lib.HipContext.ENDS_NONE and ShardFakeContext.JUMP_NONE == _lib.HipContext.JUMP_NONE


# ---- the restatements against the oracle: whole, and two pieces with the carry handed over -------------------------------------

def _cases():
    return [("designed", LAB, K, ALL_CUTS)] + [("seed%d" % s,) + S.random_case(s)[:2] + (S.random_case(s)[2][1:-1],)
                                                for s in S.SEEDS[:4]]


@pytest.mark.parametrize("name,lab,k,cuts", _cases(), ids=[c[0] for c in _cases()])
def test_restated_jump_analysis(oracle, name, lab, k, cuts):
    exp = oracle.jump_analysis(lab, k)
    whole = _ctx(lab).jump_analysis(k)
    for got, key in zip(whole[:5], ("n_ij", "time_sum", "time_n", "total_corrected_residences", "n_problems")):
        assert np.array_equal(got, exp[key]), key
    for s in cuts:
        p1 = _ctx(lab[:s]).jump_analysis(k)
        p2 = _ctx(lab[s:], frame0=s).jump_analysis(k, p1[5], p1[6])
        for i in range(5):
            assert np.array_equal(p1[i] + p2[i], whole[i]), (s, i)
        assert np.array_equal(p2[5], whole[5]) and np.array_equal(p2[6], whole[6]), s


@pytest.mark.parametrize("name,lab,k,cuts", _cases(), ids=[c[0] for c in _cases()])
def test_restated_assign_last_known(oracle, name, lab, k, cuts):
    for thr in S.ASSIGN_THRESHOLDS:
        t, (mx, avg, re) = oracle.assign_to_last_known_site(lab, thr)
        c = _ctx(lab)
        labels, fmax, st3, lout, tout = c.assign_last_known(thr)
        assert np.array_equal(labels, t) and np.array_equal(c._lab(), t)
        over = np.nonzero(fmax > thr)[0]
        assert (int(fmax[over[-1]]) if len(over) else 0) == mx and st3[2] == re
        assert (st3[0] / st3[1] if st3[1] else 0) == avg
        for s in cuts:
            a1 = _ctx(lab[:s]).assign_last_known(thr)
            a2 = _ctx(lab[s:], frame0=s).assign_last_known(thr, a1[3], a1[4])
            assert np.array_equal(np.concatenate([a1[0], a2[0]]), t), (thr, s)
            assert np.array_equal(np.concatenate([a1[1], a2[1]]), fmax), (thr, s)
            assert np.array_equal(a1[2] + a2[2], st3), (thr, s)
            assert np.array_equal(a2[3], lout) and np.array_equal(a2[4], tout), (thr, s)


@pytest.mark.parametrize("name,lab,k,cuts", _cases(), ids=[c[0] for c in _cases()])
def test_restated_running_mode_jumps_ends_and_counts(oracle, name, lab, k, cuts):
    for thr, factor, repl in S.SMOOTH_MODES:
        wl, wr = int(np.floor(factor * thr / 2)), int(np.ceil(factor * thr / 2))
        out, counts = _ctx(lab).running_mode(wl, wr, thr, repl, n_sites=k)
        assert np.array_equal(out, oracle.running_windowed_mode(lab, wl, wr, thr, k, repl))
        assert np.array_equal(counts, np.bincount(out[out >= 0], minlength=k))
    assert np.array_equal(_ctx(lab).site_counts(k), np.bincount(lab[lab >= 0], minlength=k))
    for uaj in (False, True):
        exp = oracle.jumps(lab, unknown_as_jump=uaj)
        assert [tuple(r) for r in _ctx(lab).jump_list(uaj)[0].tolist()] == exp
        for s in cuts:
            r1, l1 = _ctx(lab[:s]).jump_list(uaj)
            r2, _ = _ctx(lab[s:], frame0=s).jump_list(uaj, l1)
            r2[:, 0] += s
            assert [tuple(r) for r in np.concatenate([r1, r2]).tolist()] == exp, s
    for s in cuts:
        (f1, l1), (f2, l2) = _ctx(lab[:s]).label_ends(), _ctx(lab[s:]).label_ends()
        for rank, piece in ((0, lab[:s]), (1, lab[s:])):
            from sitator_amd.dynamics import shard_halo
            b, a = shard_halo(np.stack([f1, f2]), np.stack([l1, l2]), rank, ShardFakeContext.ENDS_NONE)
            eb, ea = replace_ref.shard_halo_brute(lab, [0, s, len(lab)], rank)
            assert np.array_equal(b, eb) and np.array_equal(a, ea)
            filled = _ctx(piece).replace_unassigned(0, b, a)
            assert np.array_equal(filled, replace_ref.replace(lab, 0)[slice(0, s) if rank == 0 else slice(s, None)])


# ---- the product's shard code on the stand-in ------------------------------------------------------------------------------------

def _inputs():
    out = [("designed/%d" % n, LAB, K, CUTS[n]) for n in sorted(CUTS)]
    return out + [("seed%d" % s,) + S.random_case(s) for s in S.SEEDS]


INPUTS = _inputs()
IDS = [c[0] for c in INPUTS]
DESIGNED = INPUTS[:3]


@pytest.mark.parametrize("name,lab,k,cut", INPUTS, ids=IDS)
def test_jump_analysis_on_shards(fake_device, oracle, name, lab, k, cut):
    S.check_jump_analysis(oracle, lab, k, cut)


@pytest.mark.parametrize("unknown_as_jump", [False, True])
@pytest.mark.parametrize("name,lab,k,cut", INPUTS, ids=IDS)
def test_jumps_on_shards(fake_device, oracle, name, lab, k, cut, unknown_as_jump):
    S.check_jumps(oracle, lab, k, cut, unknown_as_jump)


@pytest.mark.parametrize("threshold", S.ASSIGN_THRESHOLDS)
@pytest.mark.parametrize("name,lab,k,cut", INPUTS, ids=IDS)
def test_assign_to_last_known_site_on_shards(fake_device, oracle, name, lab, k, cut, threshold):
    S.check_assign(oracle, lab, k, cut, threshold)


@pytest.mark.parametrize("name,lab,k,cut", INPUTS, ids=IDS)
def test_occupancy_on_shards(fake_device, oracle, name, lab, k, cut):
    S.check_occupancy(oracle, lab, k, cut)


@pytest.mark.parametrize("remove", [False, True])
@pytest.mark.parametrize("mode", S.SMOOTH_MODES)
@pytest.mark.parametrize("name,lab,k,cut", INPUTS, ids=IDS)
def test_smoothing_on_shards(fake_device, oracle, name, lab, k, cut, mode, remove):
    S.check_smoothing(oracle, lab, k, cut, mode, remove)


@pytest.mark.parametrize("name,lab,k,cut", DESIGNED, ids=IDS[:3])
def test_smoothing_leaves_the_inputs_labels_resident(fake_device, oracle, name, lab, k, cut):
    S.check_input_labels_stay_resident(oracle, lab, k, cut)


@pytest.mark.parametrize("chain", [S.chain_1, S.chain_2], ids=["chain1", "chain2"])
@pytest.mark.parametrize("name,lab,k,cut", DESIGNED, ids=IDS[:3])
def test_chains_on_shards(fake_device, oracle, name, lab, k, cut, chain):
    S.check_chain(oracle, chain, lab, k, cut)


def test_a_rank_that_fails_is_reported_and_nobody_waits(fake_device):
    """The harness itself: rank 1 raises before its first exchange, the others are released and the failure is named."""
    def work(st):
        if st._comm is not None and st._comm.rank == 1:
            raise ValueError("rank 1 leaves")
        return st.compute_site_occupancies()

    _, joined, failures = S.run_ranks(work, LAB, K, CUTS[3])
    assert (1, "ValueError('rank 1 leaves')") in failures and len(failures) == 3 and joined[1] is None


def test_a_partial_slice_is_a_plain_trajectory(fake_device):
    from sitator_amd.sharding import ThreadComm
    st = S.trajectory(LAB, K, 40, 70, ThreadComm.group(3)[1])
    assert S.is_shard(st, 3, 40) and S.is_shard(st[:], 3, 40) and S.is_shard(st.copy(), 3, 40)
    part = st[2:5]
    assert part._comm is None and part._frame0 == 0 and part.n_frames == 3
