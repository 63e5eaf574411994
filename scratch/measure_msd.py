"""One warm call of MeanSquaredDisplacement.compute_for_analysis at the benchmark's C2 size (100 000 frames, 64 mobile ions): all
lags to F // 2, 64 log-spaced direct lags, and the same call of AverageVibrationalFrequency, beside the numpy restatement of
the all-lag path on this machine's CPUs (SITATOR_LIB: another build of the library, for A/B runs in turns)."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sitator_amd import AverageVibrationalFrequency, LandmarkAnalysis, MeanSquaredDisplacement, SiteNetwork, Structure, synth  # noqa: E402
from tests import msd_ref as R  # noqa: E402

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
out = {"frames": F, "mobile": M, "atoms": int(frames.shape[1])}


def timed(fn, repeats=7):
    fn()                                                             # warm: code objects, pool buffers, root table
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)                          # the call ends in a stream synchronise
    return r, ts


lags = np.unique(np.round(np.logspace(0, np.log10(F // 2), 64)).astype(np.int64))
for name, op in [("all_lags", MeanSquaredDisplacement()), ("all_lags_collective", MeanSquaredDisplacement(collective=True)),
                 ("all_lags_to_1000", MeanSquaredDisplacement(max_lag=1000)),
                 ("direct_%d_lags" % len(lags), MeanSquaredDisplacement(lags=lags)), ("all_lags_no_unwrap", MeanSquaredDisplacement(unwrap=False))]:
    res, ts = timed(lambda: op.compute_for_analysis(la))
    out[name] = {"seconds": [round(t, 5) for t in ts], "min": min(ts), "median": float(np.median(ts)), "max_residual": res.max_residual,
                 "n_lags": int(len(res.lags))}
    print(name, out[name], flush=True)
    if name == "all_lags":
        dev = res
    if name.startswith("direct"):
        direct = res

avg, ts = timed(lambda: AverageVibrationalFrequency().compute_for_analysis(la))
out["speed_spectrum"] = {"seconds": [round(t, 5) for t in ts], "min": min(ts), "median": float(np.median(ts)), "avg_frequency": float(avg)}
print("speed_spectrum", out["speed_spectrum"], flush=True)
# the two device paths against each other at the direct lags, in the units of the all-lag bound
sel = np.ascontiguousarray(frames[:, gen.mobile_mask])
y = R.series(sel, np.asarray(host.cell, dtype=np.float64))
unit = np.asarray(R.sum_squares(y), dtype=np.float64)
diff = np.abs(dev.msd_axes[:, lags, :] - direct.msd_axes) * (F - lags)[None, :, None] / unit[:, None, :]
out["fft_vs_direct_in_units_of_sum_y2"] = float(diff.max())
print("fft vs direct", diff.max(), flush=True)

# the numpy restatement of the all-lag path: one thread, then 16
n_lags = F // 2 + 1


def one(i):
    return [R.msd_fft_emulation(y[i, a], n_lags) for a in range(3)]


t0 = time.perf_counter()
yy = R.series(sel, np.asarray(host.cell, dtype=np.float64))
t_series = time.perf_counter() - t0
t0 = time.perf_counter()
emu = [one(i) for i in range(4)]
t_one = (time.perf_counter() - t0) / 4 * M
t0 = time.perf_counter()
with ThreadPoolExecutor(16) as pool:
    emu = list(pool.map(one, range(M)))
t_16 = time.perf_counter() - t0
emu = np.array(emu).transpose(0, 2, 1)
out["numpy"] = {"gather_unwrap_series_seconds": t_series, "fft_one_thread_seconds_extrapolated": t_one, "fft_16_threads_seconds": t_16}
out["device_vs_numpy_in_units_of_sum_y2"] = float(np.max(np.abs(emu - dev.msd_axes) * (F - np.arange(n_lags))[None, :, None] / unit[:, None, :]))
print(out["numpy"], out["device_vs_numpy_in_units_of_sum_y2"], flush=True)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "msd_bench.json", "w"), indent=1)
