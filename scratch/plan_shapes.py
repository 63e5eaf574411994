"""The launch shapes k_fill3 takes: scratch/plan_shapes.py [C2 C3 C4 C5]   (everything goes to stderr)
For C2-C5 as bench.py builds them - plain, SITATOR_FUSE=0, SITATOR_FUSE=1, with and without dynamic mapping - under every
launch-shape override of tests/test_gpu_kernels.py, test_gpu_fill_slots.py and test_gpu_fill_d1e.py (all of them at C2 and
C5, whose 64 and 160 ions those tests use; the waves and the slot form at C3 and C4): the line SITATOR_DEBUG_SHAPE=1 prints
and sit_info's shape fields after every fill (SITATOR_FILL_AUTOTUNE=0), then one fill with the autotune on ("k_fill3
trial:" lines).  SHAPES_MODE=sweep / tune runs one half only; SITATOR_LIB picks another build.
    scratch/plan_shapes.py --compact LOG     that log as one line per setting (profiles/r08_plan_shapes*.txt):
    tag dyn setting | mode nw fpb rcap iw tt mcap lds fused slot_width | mode ...
tests/test_fill3_plan.py replays profiles/r08_plan_shapes_parent.txt against the planner."""
import sys, os, re

FRAMES = {"C2": 100000, "C3": 250000, "C4": 125000, "C5": 62500}
FIELDS = ("waves_per_workgroup", "frames_per_workgroup", "survivors_per_wave", "task_table_per_wave", "assignment_fused", "fill_slot_width")
P = "SITATOR_"


def E(**kw):
    return {P + k: str(v) for k, v in kw.items()}


def each(bases, shapes):
    return [dict(b, **s) for b in bases for s in shapes]


SHAPES = [{}, E(FILL_WAVES=16), E(F3_SLOT=0), E(FILL_WAVES=8)]               # test_gpu_fill_d1e.SHAPES
SLOTS = [E(F3_SLOT=0), E(F3_SLOT=1)]                                          # test_gpu_fill_slots._fill_both
STOP = [E(DEBUG_STOP=9)]                                                      # test_gpu_fill_d1e._census
ONE_WINDOW = E(FILL_IW=64, FILL_FPB=1, FILL_WAVES=4, FILL_TCAP=512)
IW_FPB1 = [E(FILL_IW=i, FILL_FPB=1) for i in (4, 8, 12, 16, 20, 32, 64)]
# test_gpu_kernels
ENVS = [{}, E(F3_FORCE_EXACT=1), E(F3_CHEAP=0), E(F3_SKIPWRAP=0), E(FILL_RCAP=8), E(FILL_RCAP=16), E(FILL_WAVES=4), E(FILL_WAVES=8)]
ENVS += [E(FILL_WAVES=w, FILL_FPB=f, FILL_RCAP=r, FILL_IW=i, FILL_CONTIG=c, FILL_TCAP=t) for w, f, r, i, c, t in
         ((4, 1, 48, 16, 2, 128), (8, 2, 8, 5, 1, 64), (16, 3, 64, 64, 0, 512), (4, 4, 16, 33, 2, 256))]
# test_gpu_fill_slots
ENVS += each([{}, E(FILL_RCAP=8, FILL_TCAP=64), E(FILL_FPB=1), E(FILL_WAVES=8), E(FILL_WAVES=16)] + IW_FPB1, SLOTS)
# test_gpu_fill_d1e
ENVS += each([ONE_WINDOW], [{}, E(F3_SLOT=0), E(FILL_TCAP=128)] + STOP) + each(IW_FPB1, SHAPES + STOP)
ENVS += each([E(FILL_RCAP=r, FILL_FPB=1) for r in (8, 16, 24)] + [E(FILL_TCAP=64, FILL_IW=64, FILL_FPB=1), E(FILL_TCAP=64, FILL_IW=64, FILL_FPB=1, FILL_RCAP=16)] +
             [E(F3_FORCE_EXACT=1), E(F3_FORCE_EXACT=1, FILL_RCAP=16), E(F3_FORCE_EXACT=1, FILL_IW=4, FILL_FPB=1)], SHAPES)
ENVS += [E(DEBUG_STOP=10)]                                                    # scratch/phase_times.py
ENVS = [e for n, e in enumerate(ENVS) if e not in ENVS[:n]]
FEW = [{}, E(FILL_WAVES=4), E(FILL_WAVES=8), E(FILL_WAVES=16)] + SLOTS        # C3, C4
DYN = [{}, E(F3_SLOT=1), E(DEBUG_STOP=9), E(FILL_WAVES=8)]
KEYS = sorted({k for e in ENVS for k in e} | {P + "FUSE", P + "FILL_AUTOTUNE"})


def name(env):
    return " ".join("%s=%s" % (k[len(P):], env[k]) for k in sorted(env)) or "(defaults)"


def compact(path):
    """one line per (configuration, dynamic mapping, setting) of this script's list, in its order; the facts lines as they are"""
    got, order, facts, cur, shape = {}, [], [], None, None
    for line in open(path):
        m = re.match(r"## (\w+) (\w+) dyn=(\d) env (.*)", line)
        if line.startswith("facts "):
            facts.append(line.rstrip())
        elif m:
            cur, shape = m.groups(), None
        elif line.startswith("k_fill3 shape:"):
            shape = re.findall(r"\d+", line.split(":", 1)[1])
        elif line.startswith("info rc ") and cur:
            info = dict(re.findall(r"(\w+)=(-?\d+)", line))
            assert line.split()[2] == "0" and shape, line
            assert shape[:3] + [shape[4]] == [info[k] for k in FIELDS[:4]], (cur, line)         # sit_info is the launch's shape
            modes, entry = got.setdefault((cur[0], cur[2], cur[3]), []), "%s %s %s %s" % (cur[1], " ".join(shape), info[FIELDS[4]], info[FIELDS[5]])
            assert entry in modes or not any(m.split()[0] == cur[1] for m in modes), (cur, modes)     # the same setting again: the same shape
            if entry not in modes:
                modes.append(entry)
            cur = None
    print("\n".join(f for f in facts if f.split()[1] in FRAMES))
    for tag in ("C2", "C3", "C4", "C5"):
        for dyn, envs in (("0", ENVS if tag in ("C2", "C5") else FEW), ("1", DYN)):
            for env in envs:
                modes = got.get((tag, dyn, name(env)))
                print("%s %s %s | %s" % (tag, dyn, name(env), " | ".join(modes)) if modes else "# not in this log: %s %s %s" % (tag, dyn, name(env)))


if sys.argv[1:2] == ["--compact"]:
    compact(sys.argv[2])
    sys.exit(0)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("SITATOR_PROGRESSBAR", "false")
import numpy as np
from sitator_amd import _lib, synth, LandmarkAnalysis, SiteNetwork, Structure


def say(s):
    sys.stderr.write(s + "\n"); sys.stderr.flush()


def basis(ctx, host, ref_static):
    V = max(len(v) for v in host.vertices)
    verts = np.full((len(host.vertices), V), -1, dtype=np.int64); vcd = np.full(verts.shape, np.nan)
    for k, v in enumerate(host.vertices):
        verts[k, :len(v)] = v; vcd[k, :len(v)] = ctx.distances(host.centers[k], ref_static[np.asarray(v)])
    ctx.set_basis(ref_static, verts, vcd, 1.5, 30, 1.0)


def one(ctx, tag, env, mode, dyn=False):
    for k in KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ[P + "FILL_AUTOTUNE"] = "0"
    kw = {}
    if mode in ("fused", "unfused"):
        os.environ[P + "FUSE"] = "1" if mode == "fused" else "0"
        kw = dict(assign=True, predict_threshold=0.8, store_rows=False)
    say("## %s %s dyn=%d env %s" % (tag, mode, dyn, name(env)))
    rc, nz, err = ctx.fill(dyn, False, False, **kw)
    info = ctx.info()
    say("info rc %d %s" % (rc, " ".join("%s=%s" % (k, int(info[k])) for k in FIELDS)))


def sweep(ctx, tag):
    for env in (ENVS if tag in ("C2", "C5") else FEW):
        for mode in ("plain", "unfused", "fused"):
            # (the ablation builds leave no rows worth assigning - the phase-clock build with the assignment behind it ends in a
            # HIP error: as in the tests and phase_times.py, they run on their own)
            if mode == "plain" or P + "DEBUG_STOP" not in env:
                one(ctx, tag, env, mode)
    for env in DYN:
        one(ctx, tag, env, "plain", dyn=True)
        if P + "DEBUG_STOP" not in env:
            one(ctx, tag, env, "fused", dyn=True)


def facts(ctx, tag, S, M, host):
    i = ctx.info()
    say("facts %s S %d M %d vmax %d W %d W_tight %d mean_loose %.17g mean_tight %.17g delta %.17g" % (
        tag, S, M, max(len(v) for v in host.vertices), i["row_width"], i["tight_width"], i["mean_candidates_loose"], i["mean_candidates_tight"], i["delta"]))


os.environ[P + "DEBUG_SHAPE"] = "1"
MODE = os.environ.get("SHAPES_MODE", "both")
for cfg in sys.argv[1:] or ["C2", "C3", "C4", "C5"]:
    F = FRAMES[cfg]
    host = synth.config_host(cfg); M = synth.CONFIG_MOBILE[cfg]
    gen = synth.TrajectoryGenerator(host, M, seed=synth.CONFIG_SEED.get(cfg, 2), threads=16)
    ref = gen.reference_positions()
    frames = gen.generate(F)
    sn = SiteNetwork(Structure(ref, host.cell), gen.static_mask, gen.mobile_mask); sn.centers = host.centers; sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False)
    os.environ[P + "FILL_AUTOTUNE"] = "0"
    os.environ.pop(P + "DEBUG_SHAPE")
    la.run(sn, np.ascontiguousarray(frames[:20000]))
    os.environ[P + "DEBUG_SHAPE"] = "1"
    centers = np.asarray(la.cluster_centers_)
    ctx = _lib.HipContext(host.cell)
    basis(ctx, host, ref[gen.static_mask])
    ctx.set_frames(frames, np.where(gen.static_mask)[0], np.where(gen.mobile_mask)[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        ctx.set_centers(centers / np.linalg.norm(centers, axis=1)[:, None], True)
    say("# %s: %d frames as bench.py builds them" % (cfg, F))
    one(ctx, cfg, {}, "plain")
    facts(ctx, cfg, int(gen.static_mask.sum()), M, host)
    if MODE != "tune":
        sweep(ctx, cfg)
    if MODE == "sweep":
        del ctx, frames, la
        continue
    # the autotune: the candidate pairs tried, in order (the winner is timed: not compared)
    for k in KEYS:
        os.environ.pop(k, None)
    os.environ[P + "FILL_AUTOTUNE"] = "1"
    say("## %s autotune on" % cfg)
    rc, nz, err = ctx.fill(False, False, False)
    say("autotune rc %d" % rc)
    del ctx, frames, la
say("done")
