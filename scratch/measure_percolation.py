"""DensityPercolation at the benchmark's C2 size: the smoothed density (sigma 0.3 A) of the 64 mobile ions over 100 000 frames on the
grid of about 0.2 A voxels (160 x 176 x 192), 26 neighbours.  Warm calls, 1 discarded, 7 timed, median and range of the Python call's
wall time: the levels (``percolation()``) in both labelling forms, the components at t_1 in both forms (rounds, seam records), beside
the serial driver of the same rules (scratch/percolation_serial.cpp, -O2, one core of this machine) on the same grid, whose labels and
levels must be the device's bytes.  Usage: measure_percolation.py OUT.json [frames]"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sitator_amd import IonicDensity, LandmarkAnalysis, SiteNetwork, Structure, synth  # noqa: E402
from sitator_amd import _lib_percolation  # noqa: E402

F, cfg = int(sys.argv[2]) if len(sys.argv) > 2 else 100000, "C2"
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
dens = IonicDensity(spacing=0.2, sigma=0.3).compute_for_analysis(la)
grid = dens._plane(None)
ctx = la._ctx
out = {"frames": F, "mobile": M, "grid": list(grid.shape), "voxels": int(grid.size), "connectivity": 26,
       "positive_voxels": int((grid > 0).sum()), "plan": _lib_percolation.percolation_plan(grid.shape, 26)}
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
    out[name] = dict({"seconds": [round(t, 5) for t in ts], "min": min(ts), "max": max(ts), "median": float(np.median(ts))}, **extra)
    return res


levels = {}
for form in (1, 2):
    t, r, info = record("levels_form_%d" % form, lambda: _lib_percolation.percolation_levels(ctx, grid, 26, form))
    out["levels_form_%d" % form].update(passes=info[0], rounds_of_the_last_pass=info[1], seam_records_of_the_last_pass=info[2],
                                        seconds_per_pass=out["levels_form_%d" % form]["median"] / max(info[0], 1))
    levels[form] = (t, r)
    print("levels form", form, out["levels_form_%d" % form], t, r, flush=True)
out["levels"] = [float(v) for v in levels[2][0]]
out["levels_hex"] = [float(v).hex() for v in levels[2][0]]
out["ranks_at_levels"] = [int(v) for v in levels[2][1]]
out["forms_give_equal_levels"] = bool(levels[1][0].tobytes() == levels[2][0].tobytes() and np.array_equal(levels[1][1], levels[2][1]))
res = dens.percolation(ctx=ctx)
out["barriers_kT_0.0257"] = [float(v) for v in res.barriers(0.0257)]
out["dimensionality"] = res.dimensionality

t1 = float(levels[2][0][0]) if levels[2][0][0] > 0 else float(grid[grid > 0].min())
labels = {}
for form in (1, 2):
    lab, rec, info = record("components_at_t1_form_%d" % form, lambda: _lib_percolation.percolation_components(ctx, grid, t1, 26, form))
    out["components_at_t1_form_%d" % form].update(rounds=info[0], seam_records=info[1], distinct_seam_records=info[3], components=int(len(rec)),
                                                  largest=int(rec[:, 1].max()), max_rank=int(rec[:, 2].max()))
    labels[form] = lab
    print("components form", form, out["components_at_t1_form_%d" % form], flush=True)
    # the labelling and the seam pass alone: no label array, no component record brought back
    record("components_at_t1_form_%d_no_labels" % form, lambda: _lib_percolation.percolation_components(ctx, grid, t1, 26, form, want_labels=False))
out["forms_give_equal_labels"] = bool(labels[1].tobytes() == labels[2].tobytes())
# what every call pays beside its labelling: the upload of the grid, the sizes, the roots - a level above the maximum has an empty set
record("components_of_an_empty_set", lambda: _lib_percolation.percolation_components(ctx, grid, np.inf, 26, 1, want_labels=False))

# the serial driver on one core
bin_dir = os.path.join(ROOT, "scratch", "_bin")
os.makedirs(bin_dir, exist_ok=True)
exe = os.path.join(bin_dir, "percolation_serial")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "sitator_amd", "csrc"),
                       os.path.join(ROOT, "scratch", "percolation_serial.cpp"), "-o", exe])
with tempfile.TemporaryDirectory() as td:
    src, dst = os.path.join(td, "grid.bin"), os.path.join(td, "labels.bin")
    with open(src, "wb") as fh:
        fh.write(np.array(list(grid.shape) + [26], dtype=np.int64).tobytes())
        fh.write(np.array([t1]).tobytes())
        fh.write(np.ascontiguousarray(grid).tobytes())
    serial = json.loads(subprocess.run((["taskset", "-c", "0"] if shutil.which("taskset") else []) + [exe, src, dst], stdout=subprocess.PIPE, check=True).stdout)
    serial_labels = np.fromfile(dst, dtype=np.int32).reshape(grid.shape)
out["serial_driver"] = serial
out["device_labels_equal_the_driver"] = bool(serial_labels.tobytes() == labels[2].tobytes())
out["device_levels_equal_the_driver"] = bool([float.fromhex(h) for h in serial["levels_hex"]] == out["levels"] and serial["ranks"] == out["ranks_at_levels"])
print("serial", serial, out["device_labels_equal_the_driver"], out["device_levels_equal_the_driver"], flush=True)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "percolation_bench.json", "w"), indent=1)
