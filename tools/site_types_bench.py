"""Times the device side of ``SiteTypeAnalysis`` on the ``SOAPDescriptorAverages`` rows of the frames a ``LandmarkAnalysis.run``
left on the GPU and writes ``profiles/site_types_bench.json``: ``sit_pca_covariance``, ``sit_pca_project``, ``sit_dpc_graph`` (the
kernel milliseconds from HIP events, and the wall time of the call with its copies) and ``sit_dpc_assign``, then the whole
operator; and for scale, on every k-th row - an N at which the dense restatement (tests/dpc_ref.py) still fits - the same
``sit_dpc_graph`` next to the restatement's wall time.  There is no other implementation to time and no threshold: the numbers
are a record.  Run from the repository root:

    python tools/site_types_bench.py [--config C2] [--frames N] [--averaging 100] [--cutoff 5.0] [--small 4000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class Fixed(object):
    def __init__(self, dvecs, to_site):
        self.dvecs, self.to_site = dvecs, to_site

    def get_descriptors(self, stn, **kwargs):
        return self.dvecs, self.to_site


def timed(fn, *args, repeat=3):
    best, out = None, None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn(*args)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--averaging", type=int, default=100)
    ap.add_argument("--cutoff", type=float, default=5.0, help="on the C2 host (a 4 A grid) no atom lies within the default 3.0 of an ion")
    ap.add_argument("--small", type=int, default=4000, help="rows of the comparison with the dense restatement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "site_types_bench.json"))
    args = ap.parse_args()
    from sitator_amd import (LandmarkAnalysis, SiteNetwork, SiteTypeAnalysis, SOAPDescriptorAverages, Structure, _lib,
                             device_soap_backend, synth)
    from sitator_amd.site_descriptors import pca_from_covariance
    from tests import dpc_ref as DR
    host = synth.config_host(args.config)
    M = synth.CONFIG_MOBILE[args.config]
    F = args.frames or synth.CONFIG_FRAMES[args.config]
    gen = synth.TrajectoryGenerator(host, M, seed=synth.CONFIG_SEED[args.config], threads=16)
    ref = gen.reference_positions()
    frames = gen.generate(F)
    print("frames made", flush=True)
    sn = SiteNetwork(Structure(ref, host.cell, np.where(gen.mobile_mask, 3, 8)), gen.static_mask, gen.mobile_mask)
    sn.centers = host.centers
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False)
    st = la.run(sn, frames)
    print("landmark analysis done: %d sites" % st.site_network.n_sites, flush=True)
    soap = SOAPDescriptorAverages(3, averaging=args.averaging, backend=device_soap_backend({"cutoff": args.cutoff}))
    dvecs, to_site = soap.get_descriptors_for_analysis(la)
    dvecs = np.ascontiguousarray(dvecs)
    N, D = dvecs.shape
    print("descriptors: %d rows of %d" % (N, D), flush=True)
    record = {"what": "the device side of SiteTypeAnalysis on SOAPDescriptorAverages rows; wall seconds are the best of 3 calls, copies included",
              "config": synth.CONFIG_TEXT.get(args.config, args.config), "frames": int(F), "averaging": args.averaging,
              "cutoff": args.cutoff, "rows": int(N), "features": int(D)}

    ctx = _lib.HipContext(host.cell)
    (mean, cov), t_cov = timed(ctx.pca_covariance, dvecs)
    t0 = time.perf_counter()
    pca = pca_from_covariance(mean, cov, N, 0.9, 2)
    t_eigh = time.perf_counter() - t0
    Y, t_proj = timed(ctx.pca_project, dvecs, pca.mean_, pca.components_)
    record["pca"] = {"covariance_wall_seconds": round(t_cov, 4), "eigh_host_seconds": round(t_eigh, 4), "project_wall_seconds": round(t_proj, 4),
                     "components": int(pca.n_components_), "explained_variance_ratio": [float(v) for v in pca.explained_variance_ratio_]}
    print(json.dumps(record["pca"]), flush=True)
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        ks, rho, delta, nbr, info = ctx.dpc_graph(Y, 0.02)
        runs.append({"wall_seconds": round(time.perf_counter() - t0, 4), "kernel_ms": round(info["kernel_ms"], 3)})
        print(json.dumps(runs[-1]), flush=True)
    best = min(runs, key=lambda r: r["kernel_ms"])
    record["dpc_graph"] = {"points": int(N), "coordinates": int(Y.shape[1]), "pairs": info["pairs"], "kernel_size": float(ks), "runs": runs,
                           "kernel_ms": best["kernel_ms"],
                           # every pair once per select pass (8), twice for the densities, once for delta (the points above only)
                           "distance_evaluations": 11 * info["pairs"],
                           "distance_evaluations_per_second": round(11 * info["pairs"] / (1e-3 * best["kernel_ms"]), 1),
                           "dense_matrix_bytes_of_pydpc": int(8 * N * N)}
    _, t_assign = timed(ctx.dpc_assign, rho, delta, nbr, float(np.median(rho)), float(np.quantile(delta, 0.999)), to_site,
                        st.site_network.n_sites)
    record["dpc_assign_wall_seconds"] = round(t_assign, 4)

    # the dense restatement on every k-th row
    step = max(1, N // max(args.small, 2))
    Ys = np.ascontiguousarray(Y[::step])
    t0 = time.perf_counter()
    dist = DR.distances(Ys)
    dc = DR.kernel_size(dist, 0.02)[0]
    rho_ref = DR.density(dist, dc)
    DR.delta_neighbour(dist, rho_ref)
    t_ref = time.perf_counter() - t0
    (ks_s, rho_s, _, _, info_s), t_small = timed(ctx.dpc_graph, Ys, 0.02)
    record["small"] = {"points": int(len(Ys)), "restatement_wall_seconds": round(t_ref, 3), "device_wall_seconds": round(t_small, 4),
                       "device_kernel_ms": round(info_s["kernel_ms"], 3), "kernel_size_equal": bool(ks_s == dc),
                       "worst_density_difference": float(np.max(np.abs(rho_s - rho_ref) / np.where(rho_ref > 0, rho_ref, 1.0)))}
    ctx.close()
    print(json.dumps(record["small"]), flush=True)

    op = SiteTypeAnalysis(Fixed(dvecs, to_site))
    t0 = time.perf_counter()
    try:
        out = op.run(st)
        record["operator"] = {"wall_seconds": round(time.perf_counter() - t0, 3), "n_types": int(op.n_types), "elbow": int(op._decision_elbow),
                              "unassigned": int(op._n_unassigned), "sites_per_type": [int(v) for v in np.bincount(out.site_types)]}
    except ValueError as e:                                          # the reference's own refusals are a result too
        record["operator"] = {"wall_seconds": round(time.perf_counter() - t0, 3), "error": str(e)}
    with open(args.out, "w") as fh:
        fh.write(json.dumps(record) + "\n")
    print(json.dumps(record))
    return 0


if __name__ == "__main__":
    sys.exit(main())
