"""Warm calls of IntermediateScattering / StructureFactor .compute_for_analysis at the benchmark's C2 size (100 000 frames, 64 mobile
ions, 512 static atoms) after run(): 1 call discarded, 7 timed, median and range of the Python call's wall time, (origin, atom, q)
terms per second; beside the numpy restatement on one core of this machine on a cut of the same input, whose sums must be the
device's bytes."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sitator_amd import IntermediateScattering, LandmarkAnalysis, SiteNetwork, Structure, StructureFactor, q_vectors, synth  # noqa: E402
from sitator_amd import _lib_scattering  # noqa: E402
from tests import scattering_ref as S  # noqa: E402

F, cfg = 100000, "C2"
host = synth.config_host(cfg)
M = synth.CONFIG_MOBILE[cfg]
gen = synth.TrajectoryGenerator(host, M, seed=synth.CONFIG_SEED[cfg], threads=16)
ref = gen.reference_positions()
frames = gen.generate(F)
sn = SiteNetwork(Structure(ref, host.cell), gen.static_mask, gen.mobile_mask)
sn.centers = host.centers
sn.vertices = host.vertices
la = LandmarkAnalysis(verbose=False, device=0, clustering_algorithm="dotprod")
la.run(sn, frames)
cell = np.asarray(host.cell, dtype=np.float64)
n_static = int(np.sum(gen.static_mask))
# the half-space q set up to the |q| at which it first holds 250 vectors or more: about one tile of q
q_max = 2.0 * np.pi / np.linalg.norm(cell, axis=1).max()
while len(q_vectors(cell, q_max)) < 250:
    q_max *= 1.05
q = q_vectors(cell, q_max)
H = S.h_max(q)
lags = np.unique(np.round(np.logspace(0, np.log10(F // 2), 64)).astype(np.int64))
out = {"frames": F, "mobile": M, "static": n_static, "q_max": q_max, "n_q": int(len(q)), "h_max": H, "n_lags": int(len(lags))}
print(out, flush=True)


def timed(fn, repeats=7):
    fn()                                                             # warm: code objects, pool buffers
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)                          # the call ends in a stream synchronise
    return r, ts


def origins(stride):
    return int(sum(S.n_origins(F, int(t), stride) for t in lags))


def record(name, fn, terms, plan):
    res, ts = timed(fn)
    med = float(np.median(ts))
    out[name] = {"seconds": [round(t, 5) for t in ts], "min": min(ts), "max": max(ts), "median": med, "terms": terms,
                 "terms_per_second": terms / med, "plan": plan}
    print(name, out[name], flush=True)
    return res


def plan_of(n_a, n_b, same, n_lags, stride, self_part, coherent_part):
    return _lib_scattering.scattering_plan(F, n_a, n_b, len(q), H, n_lags, stride, same, self_part, coherent_part)


for stride in (1, 10):
    record("self_stride_%d" % stride,
           lambda: IntermediateScattering(q, lags, origin_stride=stride, coherent_part=False).compute_for_analysis(la),
           origins(stride) * M * len(q), plan_of(M, M, True, len(lags), stride, True, False))
for stride in (1, 10):
    # the density modes of every frame, then one product per (origin, q)
    record("coherent_stride_%d" % stride,
           lambda: IntermediateScattering(q, lags, origin_stride=stride, self_part=False).compute_for_analysis(la),
           F * M * len(q), plan_of(M, M, True, len(lags), stride, False, True))
sf = record("structure_factor_mobile_static", lambda: StructureFactor(q).compute_for_analysis(la, mask_b="static"),
            F * (M + n_static) * len(q), plan_of(M, n_static, False, 1, 1, False, True))
out["largest_partial_S"] = float(np.abs(sf.S).max())

# the numpy restatement on the first 600 frames at three of the lags: one thread
sub = np.ascontiguousarray(frames[:600])
mobile = np.where(gen.mobile_mask)[0]
few = np.array([1, 10, 100])
t0 = time.perf_counter()
ref_self = S.self_sums(sub, cell, mobile, q, few, 1)
t = time.perf_counter() - t0
terms = int(sum(S.n_origins(600, int(tau), 1) for tau in few)) * M * len(q)
out["numpy_self"] = {"frames": 600, "lags": [int(v) for v in few], "seconds": t, "terms": terms, "terms_per_second": terms / t}
print("numpy", out["numpy_self"], flush=True)
t0 = time.perf_counter()
ref_coherent = S.coherent_sums(sub, cell, mobile, None, q, few, 1)
out["numpy_coherent_seconds"] = time.perf_counter() - t0
dev = IntermediateScattering(q, few).compute(sub, cell, gen.mobile_mask)
out["device_equals_numpy"] = bool(dev.self_sums.tobytes() == ref_self.tobytes() and dev.coherent_sums.tobytes() == ref_coherent.tobytes())
print("device equals numpy:", out["device_equals_numpy"], flush=True)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "scattering_bench.json", "w"), indent=1)
