"""EnergyLandscape at the benchmark's C2 host: its 512 static atoms on the grid of about 0.2 A voxels, rc = 6 A and 12 A, and the 4 A
triclinic cell of the tests (5 atoms) at 0.05 A with rc = 2.2 smallest heights.  Warm calls, 1 discarded, 7 timed, alternating the
two forms, median and range of the Python call's wall time (it ends in a stream synchronise and includes the copy back of the
energies); a device-to-host copy of as many doubles into pageable memory is timed on its own.  Beside them the restatement of
tests/landscape_ref.py on one core, on a sample of voxels, whose bytes must be the device's.  Counted terms: the mean number of
images within rc of a point, S (4 pi rc^3 / 3) / V_cell, times the voxels.  Usage: measure_landscape.py OUT.json"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sitator_amd import EnergyLandscape, calculators, synth, _lib, _lib_landscape  # noqa: E402
from tests import barrier_ref as BR, landscape_ref as LR  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12           # FLOP/s: half the FP32 vector peak of the MI355X (157.3 TFLOP/s)
FLOP_PER_CANDIDATE, FLOP_PER_COUNTED = 11, 8        # 6 subtractions, 3 products, 2 sums; then a quotient, 4 products, 2 differences, 1 sum
REPEATS = 7
out = {}


def case(name, cell, pos, sigma, rc, spacing, restate=24):
    calc = calculators.LennardJones(epsilon=1.0, sigma=sigma, rc=rc)
    numbers = np.zeros(len(pos), dtype=np.int64)
    grid = EnergyLandscape(calc, spacing=spacing).grid_for(cell)
    V = int(np.prod(grid))
    rec = {"grid": list(grid), "voxels": V, "atoms": len(pos), "rc": rc,
           "counted_terms_expected": V * len(pos) * 4.0 / 3.0 * np.pi * rc ** 3 / abs(np.linalg.det(cell))}
    eps, sig = calc.parameters_for(numbers)
    with _lib.HipContext(cell) as ctx:
        calls = {form: (lambda form=form: _lib_landscape.landscape_energies(ctx, pos, eps, sig, rc, grid, form)) for form in (1, 2)}
        results, times = {}, {1: [], 2: []}
        for form in (1, 2):
            calls[form]()                                            # warm: code objects, pool buffers
        for _ in range(REPEATS):
            for form in (1, 2):                                      # alternating
                t0 = time.perf_counter()
                results[form] = calls[form]()
                times[form].append(time.perf_counter() - t0)
        hip = C.CDLL("libamdhip64.so")                               # the runtime the library is linked against
        hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], \
            [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
        dev, landing = C.c_void_p(), np.empty(V)
        assert hip.hipMalloc(C.byref(dev), V * 8) == 0 and hip.hipMemcpy(dev, landing.ctypes.data, V * 8, 1) == 0
        copies = []
        for _ in range(REPEATS + 1):
            t0 = time.perf_counter()
            assert hip.hipMemcpy(landing.ctypes.data, dev, V * 8, 2) == 0        # device to host, done on return
            copies.append(time.perf_counter() - t0)
        hip.hipFree(dev)
        rec["copy_back_seconds"] = {"median": float(np.median(copies[1:])), "min": min(copies[1:]), "max": max(copies[1:])}
    rec["forms_give_equal_bytes"] = bool(results[1][0].tobytes() == results[2][0].tobytes())
    for form in (1, 2):
        ts, info = times[form], results[form][1]
        med = float(np.median(ts))
        kernel = max(med - rec["copy_back_seconds"]["median"], 1e-9)
        evaluations = info[3] * (256 if form == 2 else 1)           # a list entry is run by every voxel of its tile
        flop = evaluations * FLOP_PER_CANDIDATE + rec["counted_terms_expected"] * FLOP_PER_COUNTED
        rec["form_%d" % form] = {"seconds": [round(t, 5) for t in ts], "median": med, "min": min(ts), "max": max(ts), "tiles": info[1],
                                 "list_chunks_of_the_longest_tile": info[2], "candidate_terms": info[3],
                                 "median_less_copy_seconds": kernel, "candidate_terms_per_second": evaluations / kernel,
                                 "counted_terms_per_second": rec["counted_terms_expected"] / kernel,
                                 "share_of_fp64_vector_peak": flop / kernel / FP64_VECTOR_PEAK}
    vox = np.random.default_rng(7).choice(V, size=restate, replace=False)
    t0 = time.perf_counter()
    counted = sum(LR.energy(cell, pos, eps, sig, rc, LR.center(cell, grid, LR.unflatten(grid, int(v))))[1] for v in vox)
    want = LR.energies(cell, pos, eps, sig, rc, grid, vox)
    dt = (time.perf_counter() - t0) / 2.0
    rec["restatement"] = {"voxels": restate, "counted_terms": int(counted), "seconds": dt, "counted_terms_per_second": counted / dt,
                          "bytes_equal_the_device": bool(want.tobytes() == results[1][0].reshape(-1)[vox].tobytes())}
    rec["finite_fraction"] = float(np.isfinite(results[1][0]).mean())
    out[name] = rec
    print(name, json.dumps(rec), flush=True)


host = synth.config_host("C2")
cell = np.asarray(host.cell, dtype=np.float64)
static = np.asarray(host.static_pos, dtype=np.float64)
case("C2_rc6", cell, static, 2.0, 6.0, 0.2)
case("C2_rc12", cell, static, 2.0, 12.0, 0.2, restate=8)
small = BR.SMALL_TRICLINIC
pos5 = np.random.default_rng(3).random((5, 3)) @ small
case("triclinic4_rc2.2h", small, pos5, 1.0, 2.2 * BR.heights(small).min(), 0.05, restate=24)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "landscape_bench.json", "w"), indent=1)
