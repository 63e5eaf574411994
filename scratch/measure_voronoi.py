"""VoronoiSiteGenerator.run on the static lattices of configs C2 and C3 (warm process, repeated), and qhull on the 27-image block
on the host for the same inputs (profiles/voronoi_bench.json).  Usage: python scratch/measure_voronoi.py OUT.json"""
import json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
from sitator_amd import SiteNetwork, Structure, VoronoiSiteGenerator, synth

def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}

out = {"device": "MI355X", "what": "VoronoiSiteGenerator.run wall (host clock around the call; it ends in a device synchronise and includes "
       "context creation, copies and the host merge) and kernel milliseconds (HIP events around the neighbour and sphere kernels), "
       "after 3 warm-up calls in the same process; qhull: scipy.spatial.Voronoi over the 3x3x3 image block on the host CPU", "configs": {}}
for name in ("C2", "C3"):
    host = synth.config_host(name)
    S = len(host.static_pos)
    sn = SiteNetwork(Structure(host.static_pos, host.cell), np.ones(S, dtype=bool), np.zeros(S, dtype=bool))
    gen = VoronoiSiteGenerator()
    for _ in range(3):
        res = gen.run(sn)
    wall, kern = [], []
    for _ in range(15):
        t = time.perf_counter(); res = gen.run(sn); wall.append((time.perf_counter() - t) * 1e3); kern.append(gen.last_info["kernel_ms"])
    ok = res.n_sites == len(host.centers) and sorted(map(tuple, res.vertices)) == sorted(tuple(sorted(v)) for v in host.vertices)
    from scipy.spatial import Voronoi
    shifts = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64) @ host.cell
    pts = (host.static_pos[None] + shifts[:, None]).reshape(-1, 3)
    q = []
    for _ in range(5):
        t = time.perf_counter(); Voronoi(pts); q.append((time.perf_counter() - t) * 1e3)
    out["configs"][name] = {"S": S, "nodes": int(res.n_sites), "nodes_are_the_hosts_landmarks": bool(ok), "info": gen.last_info,
                            "run_wall_ms": stats(wall), "kernel_ms": stats(kern), "qhull_27_images_host_ms": stats(q)}
    print(name, json.dumps(out["configs"][name]), flush=True)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "voronoi_bench.json", "w"), indent=1)
