"""Shared by tests/test_replace_unassigned.py (CPU) and tests/test_gpu_replace_unassigned.py (GPU): a numpy brute force of
``ReplaceUnassignedPositions`` (per ion, for every frame, search backwards and forwards), designed label sets, the
goldens of the TRUE reference (tests/golden/replace_unassigned_known_answers.npz) and a frame-shard driver."""
import numpy as np

from tests import golden_util as G

NONE = -(1 << 63)
MARGIN = 1e-9            # Angstrom; CPU and GPU distances agree to 5e-14, a decided frame may not be a nearer tie than this


# ---- brute force -----------------------------------------------------------------------------------------------------

def before_after(labels, before_in=None, after_in=None):
    """(before, after), each [F, M]: for EVERY frame the nearest label != -1 at an earlier / a later frame of the ion,
    failing that the carried-in value, failing that -1."""
    labels = np.asarray(labels)
    F, M = labels.shape
    before = np.empty((F, M), dtype=np.int64)
    after = np.empty((F, M), dtype=np.int64)
    for j in range(M):
        for f in range(F):
            b = -1 if before_in is None else before_in[j]
            for g in range(f - 1, -1, -1):
                if labels[g, j] != -1:
                    b = labels[g, j]
                    break
            a = -1 if after_in is None else after_in[j]
            for g in range(f + 1, F):
                if labels[g, j] != -1:
                    a = labels[g, j]
                    break
            before[f, j], after[f, j] = b, a
    return before, after


def replace(labels, mode, before_in=None, after_in=None):
    side = before_after(labels, before_in, after_in)[mode]
    return np.where(np.asarray(labels) == -1, side, labels)


def ends(labels):
    labels = np.asarray(labels)
    first = np.full(labels.shape[1], NONE, dtype=np.int64)
    last = np.full(labels.shape[1], NONE, dtype=np.int64)
    for j in range(labels.shape[1]):
        known = labels[:, j][labels[:, j] != -1]
        if len(known):
            first[j], last[j] = known[0], known[-1]
    return first, last


def runs(labels, before_in=None, after_in=None, frame0=0):
    """(records[n, 6], n_positions): (ion, start, end, before, after, pos_offset), ion-major and by start."""
    labels = np.asarray(labels)
    F, M = labels.shape
    before, after = before_after(labels, before_in, after_in)
    rec, npos = [], 0
    for j in range(M):
        f = 0
        while f < F:
            if labels[f, j] != -1:
                f += 1
                continue
            e = f
            while e < F and labels[e, j] == -1:
                e += 1
            b, a = before[f, j], after[e - 1, j]
            decide = b >= 0 and a >= 0 and b != a
            rec.append((j, frame0 + f, frame0 + e, b, a, npos if decide else -1))
            if decide:
                npos += e - f
            f = e
    return np.array(rec, dtype=np.int64).reshape(-1, 6), npos


def positions_of(records, mobile_positions, frame0=0):
    """[n_positions, 3]: the positions ``replace_closer`` wants, from ``mobile_positions[F, M, 3]``."""
    out = [mobile_positions[s - frame0:e - frame0, j] for j, s, e, _, _, off in records if off >= 0]
    return np.concatenate(out).reshape(-1, 3) if out else np.zeros((0, 3))


def closer(oracle, cell, labels, centers, mobile_positions, before_in=None, after_in=None):
    """(labels filled by the closer-site rule, smallest |d_before - d_after| over the decided frames), the distances by
    the CPU oracle's restatement of the reference's shift-and-wrap distance."""
    labels = np.asarray(labels)
    before, after = before_after(labels, before_in, after_in)
    out = labels.copy()
    margin = np.inf
    for f, j in zip(*np.nonzero(labels == -1)):
        b, a = before[f, j], after[f, j]
        if b < 0 or a < 0:
            continue
        if b == a:
            out[f, j] = b
            continue
        d = oracle.distances(cell, mobile_positions[f, j], centers[[b, a]])
        margin = min(margin, abs(d[0] - d[1]))
        out[f, j] = b if d[0] < d[1] else a
    return out, margin


def shard_halo_brute(labels, cut, rank):
    """What holds before the first and after the last frame of shard ``rank`` (frames cut[rank]:cut[rank + 1]): by
    searching the WHOLE label array."""
    labels = np.asarray(labels)
    M = labels.shape[1]
    b = np.full(M, -1, dtype=np.int64)
    a = np.full(M, -1, dtype=np.int64)
    for j in range(M):
        for g in range(cut[rank] - 1, -1, -1):
            if labels[g, j] != -1:
                b[j] = labels[g, j]
                break
        for g in range(cut[rank + 1], len(labels)):
            if labels[g, j] != -1:
                a[j] = labels[g, j]
                break
    return b, a


# ---- designed inputs ---------------------------------------------------------------------------------------------------

K_DESIGNED = 7
CELL = np.array([[7.0, 0.0, 0.0], [1.5, 6.5, 0.0], [-1.0, 0.8, 8.0]])        # triclinic


def designed_labels(F, M, seed):
    """[F, M] labels over ``K_DESIGNED`` sites, about half of them -1: every frame an ion keeps what it has with
    probability 0.7, otherwise it becomes unknown (probability 0.5) or draws a site."""
    rng = np.random.default_rng(seed)
    lab = np.empty((F, M), dtype=np.int64)
    state = np.where(rng.uniform(size=M) < 0.5, -1, rng.integers(0, K_DESIGNED, size=M))
    for f in range(F):
        again = rng.uniform(size=M) >= 0.7
        fresh = np.where(rng.uniform(size=M) < 0.5, -1, rng.integers(0, K_DESIGNED, size=M))
        state = np.where(again, fresh, state)
        lab[f] = state
    return lab


def designed_geometry(F, M, seed):
    """(centres[K_DESIGNED, 3], mobile positions[F, M, 3]) uniform in ``CELL``."""
    rng = np.random.default_rng(seed + 1000)
    return rng.uniform(size=(K_DESIGNED, 3)) @ CELL, rng.uniform(size=(F, M, 3)) @ CELL


def halos(M, seed):
    rng = np.random.default_rng(seed + 2000)
    return (np.where(rng.uniform(size=M) < 0.3, -1, rng.integers(0, K_DESIGNED, size=M)),
            np.where(rng.uniform(size=M) < 0.3, -1, rng.integers(0, K_DESIGNED, size=M)))


def plain_network(n_mobile, centers, cell=CELL):
    """Two static atoms FIRST, then the mobile ones: mobile atom j is atom j + 2 of the structure."""
    from sitator_amd import SiteNetwork, Structure
    sm = np.array([True, True] + [False] * n_mobile)
    sn = SiteNetwork(Structure(np.zeros((n_mobile + 2, 3)), cell), sm, ~sm)
    sn.centers = np.array(centers, copy=True)
    return sn


def real_trajectory(mobile_positions, n_static=2):
    F, M = mobile_positions.shape[:2]
    real = np.zeros((F, M + n_static, 3))
    real[:, n_static:] = mobile_positions
    return real


# ---- the goldens ---------------------------------------------------------------------------------------------------------

class ReplaceGoldens(object):
    """tests/golden/replace_unassigned_known_answers.npz; the inputs of the cases that are not ``own`` come from
    merge_known_answers.npz."""

    FIELDS = ("labels", "centers", "cell", "static_mask", "mobile_mask", "ref_positions")

    def __init__(self):
        self.z = G.load("replace_unassigned_known_answers")
        self.src = G.load("merge_known_answers")
        self.names = [str(n) for n in self.z["names"]]
        self.own = [str(n) for n in self.z["own"]]

    def inputs(self, name):
        if name in self.own:
            return {k: self.z["%s/in_%s" % (name, k)] for k in self.FIELDS}
        return {k: self.src["%s/%s" % (name, k)] for k in self.FIELDS}

    def mobile_positions(self, name):
        """[F, M, 3] by the generator's rule: a known entry stands on the centre of its site, the unknown ones are
        stored."""
        i = self.inputs(name)
        lab = i["labels"]
        unknown = lab == -1
        pos = i["centers"][np.where(unknown, 0, lab)]
        pos[unknown] = self.z[name + "/unknown_positions"]
        return pos

    def real_trajectory(self, name):
        i = self.inputs(name)
        real = np.broadcast_to(i["ref_positions"], (len(i["labels"]),) + i["ref_positions"].shape).copy()
        real[:, np.where(i["mobile_mask"])[0]] = self.mobile_positions(name)
        return real

    def confidences(self, name):
        lab = self.inputs(name)["labels"]
        return np.linspace(0.0, 1.0, lab.size).reshape(lab.shape)

    def trajectory(self, name):
        """The SiteTrajectory the generator ran the reference on: two attributes, confidences, a real trajectory."""
        from sitator_amd import SiteNetwork, SiteTrajectory, Structure
        i = self.inputs(name)
        sn = SiteNetwork(Structure(i["ref_positions"], i["cell"]), i["static_mask"], i["mobile_mask"])
        sn.centers = np.array(i["centers"], copy=True)
        K = sn.n_sites
        sn.add_site_attribute("score", np.arange(K) * 0.5, computed=False)
        sn.add_edge_attribute("weight", np.arange(K * K, dtype=np.float64).reshape(K, K), computed=True)
        st = SiteTrajectory(sn, i["labels"].copy(), confidences=self.confidences(name))
        st.set_real_traj(self.real_trajectory(name))
        return st


class Recorder(object):
    """The generator's recording callable: call i returns the scalar (3 i) % K when i is even, a float array when odd."""

    def __init__(self, st, K):
        self.st, self.K, self.calls = st, K, []

    def __call__(self, st, mob, before, start, after, end):
        assert st is self.st
        i = len(self.calls)
        self.calls.append((mob, before, start, after, end))
        if i % 2 == 0:
            return (3 * i) % self.K
        return ((start + np.arange(end - start)) % self.K) + 0.0


def check_golden_case(RG, name, margin_oracle=None):
    """Runs all four strategies and the default constructor on a golden case and compares everything the file records."""
    from sitator_amd import ReplaceUnassignedPositions as RUP
    z = RG.z
    lab = RG.inputs(name)["labels"]
    assert str(z["default_ctor_error"]) == "NameError" and str(z["closer_factory_returns"]) == "NoneType"
    if margin_oracle is not None:
        i = RG.inputs(name)
        _, margin = closer(margin_oracle, i["cell"], lab, i["centers"], RG.mobile_positions(name))
        assert margin >= MARGIN and float(z[name + "/closer_margin"]) >= MARGIN
    for fn, key in ((RUP.replace_with_last_known, "last"), (RUP.replace_with_next_known, "next"),
                    (RUP.replace_with_closer(), "closer"), (None, "last")):
        st = RG.trajectory(name)
        real, confs = st.real_trajectory, st.confidences
        out = (RUP() if fn is None else RUP(fn)).run(st)
        assert out is not st and out.traj.dtype == np.int64
        assert np.array_equal(out.traj, z["%s/%s" % (name, key)]), key
        assert np.array_equal(st._traj, lab) and st.site_network.has_attribute("score")          # the input is untouched
        assert out.site_network.has_attribute("score") == bool(z[name + "/kept_plain"])
        assert out.site_network.has_attribute("weight") == bool(z[name + "/kept_computed"])
        assert bool(z[name + "/confidences_kept"]) and np.shares_memory(out.confidences, confs)
        assert np.array_equal(out.confidences, confs)
        assert bool(z[name + "/real_traj_kept"]) and np.shares_memory(out.real_trajectory, real)
        assert out.real_trajectory.shape == real.shape
        assert out.site_network is not st.site_network
        assert np.array_equal(np.asarray(out.site_network.centers), np.asarray(st.site_network.centers))
    # the protocol of any other callable: arguments, order, a scalar and a float-array return
    st = RG.trajectory(name)
    rec = Recorder(st, st.site_network.n_sites)
    out = RUP(rec).run(st)
    assert np.array_equal(np.array(rec.calls, dtype=np.int64).reshape(-1, 5), z[name + "/calls"])
    assert np.array_equal(out.traj, z[name + "/recorded"]) and out.traj.dtype == np.int64
    # the closer-site callable called as a plain callable, run by run, gives what the device path gives
    st = RG.trajectory(name)
    plain = RUP.replace_with_closer()
    out = RUP(lambda *a: plain(*a)).run(st)
    assert np.array_equal(out.traj, z[name + "/closer"])


# ---- frame shards ----------------------------------------------------------------------------------------------------------

def sharded_case():
    """(labels[90, 6], centres, mobile positions, cuts): rank 1 of the three-shard cut (frames 40..69) holds NO known
    label of ion 2, ion 3 is never known, ion 4 is unknown from frame 35 to frame 74 (over both cuts)."""
    lab = designed_labels(90, 6, seed=11)
    lab[40:70, 2] = -1
    lab[:, 3] = -1
    lab[35:75, 4] = -1
    lab[34, 4], lab[75, 4] = 1, 5
    centers, pos = designed_geometry(90, 6, seed=11)
    return lab, centers, pos, {2: [0, 40, 90], 3: [0, 40, 70, 90]}


def run_sharded(lab, centers, pos, cut, custom=False):
    """(single-rank results, per-rank results in rank order, exceptions); a result: the label arrays of the three
    built-in strategies (``custom``: of a callable of the caller's)."""
    import threading
    from sitator_amd import ReplaceUnassignedPositions as RUP, SiteTrajectory
    from sitator_amd.sharding import ThreadComm
    real = real_trajectory(pos)

    def work(lo, hi, comm):
        def st():
            t = SiteTrajectory(plain_network(lab.shape[1], centers), lab[lo:hi], _comm=comm)
            t.set_real_traj(real[lo:hi])
            return t
        if custom:
            return [RUP(lambda st_, mob, b, s, a, e: b).run(st()).traj]
        return [RUP(fn).run(st()).traj for fn in (RUP.replace_with_last_known, RUP.replace_with_next_known,
                                                  RUP.replace_with_closer())]

    single = work(0, len(lab), None)
    comms = ThreadComm.group(len(cut) - 1)
    joined, failures = [None] * len(comms), []

    def rank(r):
        try:
            joined[r] = work(cut[r], cut[r + 1], comms[r])
        except BaseException as e:                               # noqa: BLE001 - reported by the caller
            failures.append((r, type(e).__name__))
            comms[r].abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(len(comms))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return single, joined, failures
