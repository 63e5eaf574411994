"""Warm calls of VanHoveCorrelation / RadialDistribution .compute_for_analysis at the benchmark's C2 size (100 000 frames, 64 mobile
ions) after run(): 1 call discarded, 7 timed, median and range of the Python call's wall time, pairs per second; each distinct call
with one LDS histogram per workgroup and with one per wave (SITATOR_VANHOVE_HIST_COPIES); beside the numpy restatement on this
machine's CPUs at a size it finishes."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sitator_amd import LandmarkAnalysis, RadialDistribution, SiteNetwork, Structure, VanHoveCorrelation, synth  # noqa: E402
from tests import vanhove_ref as V  # noqa: E402

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
S = int(np.sum(gen.static_mask))
r_max, n_bins = 0.5 * V.hmin(cell) * V.MARGIN, 300
lags = np.unique(np.round(np.logspace(0, np.log10(F // 2), 64)).astype(np.int64))
out = {"frames": F, "mobile": M, "static": S, "r_max": r_max, "n_bins": n_bins, "n_lags": int(len(lags))}


def timed(fn, repeats=7):
    fn()                                                             # warm: code objects, pool buffers
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)                          # the call ends in a stream synchronise
    return r, ts


def origins(stride):
    return int(sum(V.n_origins(F, int(t), stride) for t in lags))


def record(name, fn, pairs):
    res, ts = timed(fn)
    med = float(np.median(ts))
    out[name] = {"seconds": [round(t, 5) for t in ts], "min": min(ts), "max": max(ts), "median": med, "pairs": pairs, "pairs_per_second": pairs / med}
    print(name, out[name], flush=True)
    return res


for copies in ("1", "4"):
    os.environ["SITATOR_VANHOVE_HIST_COPIES"] = copies
    tag = "" if copies == "1" else "_per_wave_histograms"
    for stride in (1, 10):
        record("distinct_stride_%d%s" % (stride, tag),
               lambda: VanHoveCorrelation(lags, r_max, n_bins, origin_stride=stride, self_part=False).compute_for_analysis(la),
               origins(stride) * M * (M - 1))
    rdf = record("rdf_mobile_static%s" % tag, lambda: RadialDistribution(r_max, n_bins).compute_for_analysis(la), F * M * S)
    record("rdf_mobile_static_narrow%s" % tag, lambda: RadialDistribution(0.25 * r_max, 16).compute_for_analysis(la), F * M * S)
    record("self_stride_1%s" % tag, lambda: VanHoveCorrelation(lags, r_max, n_bins, distinct_part=False).compute_for_analysis(la), origins(1) * M)
os.environ["SITATOR_VANHOVE_HIST_COPIES"] = "1"
for stride in (1, 10):
    vh = record("both_parts_stride_%d" % stride, lambda: VanHoveCorrelation(lags, r_max, n_bins, origin_stride=stride).compute_for_analysis(la),
                origins(stride) * M * M)
out["max_residual"] = vh.max_residual
out["share_of_pairs_within_r_max"] = float(1.0 - rdf.counts[-1] / rdf.counts.sum())
out["largest_bin_share_of_the_rdf"] = float(rdf.counts[:-1].max() / rdf.counts.sum())

# the numpy restatement on the first 2000 frames at 8 of the lags: one thread
sub = np.ascontiguousarray(frames[:2000])
mobile = np.where(gen.mobile_mask)[0]
few = lags[lags < 1000][::4][:8]
t0 = time.perf_counter()
ref_counts = V.distinct(sub, cell, mobile, mobile, True, few, 1, r_max, n_bins)
t = time.perf_counter() - t0
pairs = int(sum(V.n_origins(2000, int(tau), 1) for tau in few)) * M * (M - 1)
out["numpy_distinct"] = {"frames": 2000, "lags": [int(v) for v in few], "seconds": t, "pairs": pairs, "pairs_per_second": pairs / t}
print("numpy", out["numpy_distinct"], flush=True)
dev = VanHoveCorrelation(few, r_max, n_bins, self_part=False).compute(sub, cell, gen.mobile_mask)
out["device_equals_numpy"] = bool(np.array_equal(dev.distinct_counts, ref_counts))
print("device equals numpy:", out["device_equals_numpy"], flush=True)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "vanhove_bench.json", "w"), indent=1)
