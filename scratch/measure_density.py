"""Warm calls of IonicDensity.compute_for_analysis / compute_for_trajectory at the benchmark's C2 size (100 000 frames, 64 mobile
ions) after run(): 1 call discarded, 7 timed, median and range of the Python call's wall time, entries (frame, ion) per second and
bytes of positions read per second; the count alone in the direct and in the aggregated form on a grid of about 0.2 A voxels, the
count with a Gaussian smoothing of sigma 0.3 A, the count split by the labels; beside the numpy restatement on one core of this
machine on a cut of the same input, whose counts must be the device's bytes."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sitator_amd import IonicDensity, LandmarkAnalysis, SiteNetwork, Structure, gaussian_stencil, synth  # noqa: E402
from sitator_amd import _lib_density  # noqa: E402
from tests import density_ref as R  # noqa: E402

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
st = la.run(sn, frames)
cell = np.asarray(host.cell, dtype=np.float64)
grid = IonicDensity(spacing=0.2).grid_for(cell)
mobile = np.where(gen.mobile_mask)[0]
entries = F * M
out = {"frames": F, "mobile": M, "atoms": int(frames.shape[1]), "grid": list(grid), "voxels": int(np.prod(grid)), "entries": entries,
       "plan": _lib_density.density_plan(F, frames.shape[1], M, grid, host=False)}
print(out, flush=True)


def timed(fn, repeats=7):
    fn()                                                             # warm: code objects, pool buffers
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)                          # the call ends in a stream synchronise
    return r, ts


def record(name, fn, **extra):
    res, ts = timed(fn)
    med = float(np.median(ts))
    out[name] = dict({"seconds": [round(t, 5) for t in ts], "min": min(ts), "max": max(ts), "median": med,
                      "entries_per_second": entries / med, "position_bytes_per_second": entries * 24 / med}, **extra)
    print(name, out[name], flush=True)
    return res


direct = record("count_form_1", lambda: IonicDensity(grid=grid, form=1).compute_for_analysis(la))
table = record("count_form_2", lambda: IonicDensity(grid=grid, form=2).compute_for_analysis(la))
auto = record("count_form_0", lambda: IonicDensity(grid=grid).compute_for_analysis(la))
out["forms_equal"] = bool(direct.counts.tobytes() == table.counts.tobytes() == auto.counts.tobytes())
out["occupied_voxels"] = int((table.counts > 0).sum())
out["largest_count"] = int(table.counts.max())
# the same kernels on a grid of one voxel: every entry on one key, no array of counts to bring back
record("count_form_1_one_voxel", lambda: IonicDensity(grid=(1, 1, 1), form=1).compute_for_analysis(la))
record("count_form_2_one_voxel", lambda: IonicDensity(grid=(1, 1, 1), form=2).compute_for_analysis(la))
taps, w = gaussian_stencil(cell, grid, 0.3)
sm = record("count_and_smoothing_sigma_0.3", lambda: IonicDensity(grid=grid, sigma=0.3).compute_for_analysis(la), n_taps=int(len(taps)),
            halo=R.halo(taps, grid))
split = record("for_trajectory_assigned", lambda: IonicDensity(grid=grid).compute_for_trajectory(la, st))
out["planes_add_up"] = bool(np.array_equal(split.counts.sum(axis=0, keepdims=True), table.counts))
out["unassigned_entries"] = int(split.counts[1].sum())
peaks = sm.peaks(0.05)
out["peaks_of_the_smoothed_grid"] = int(len(peaks[0]))

# the numpy restatement on the first 2000 frames: one thread
n_sub = 2000
sub = np.ascontiguousarray(frames[:n_sub])
t0 = time.perf_counter()
ref_counts = R.counts(sub, cell, mobile, grid)[0]
t = time.perf_counter() - t0
out["numpy_count"] = {"frames": n_sub, "seconds": t, "entries_per_second": n_sub * M / t}
print("numpy", out["numpy_count"], flush=True)
dev = IonicDensity(grid=grid).compute(sub, cell, gen.mobile_mask)
out["device_equals_numpy"] = bool(dev.counts.tobytes() == ref_counts.tobytes())
print("device equals numpy:", out["device_equals_numpy"], flush=True)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "density_bench.json", "w"), indent=1)
