"""SiteCoordinationEnvironment.run on the static lattices and landmark sites of configs C2 and C3 (warm process, 3 calls discarded,
then 15): wall time and the two kernels' milliseconds (profiles/coordenv_bench.json).
Usage: python scratch/measure_coordenv.py OUT.json"""
import collections, json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
from sitator_amd import SiteCoordinationEnvironment, SiteNetwork, Structure, synth

def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}

out = {"device": "MI355X", "what": "SiteCoordinationEnvironment.run wall (host clock around the call; it ends in a device synchronise and "
       "includes context creation, copies and the host bookkeeping) and the milliseconds of k_coordenv_cell (all rounds) and k_coordenv_csm "
       "(HIP events), after 3 warm-up calls in the same process", "configs": {}}
for name in ("C2", "C3"):
    host = synth.config_host(name)
    S = len(host.static_pos)
    sn = SiteNetwork(Structure(host.static_pos, host.cell), np.ones(S, dtype=bool), np.zeros(S, dtype=bool))
    sn.centers = host.centers
    op = SiteCoordinationEnvironment()
    for _ in range(3):
        op.run(sn)
    wall, cell, csm = [], [], []
    for _ in range(15):
        t = time.perf_counter(); op.run(sn); wall.append((time.perf_counter() - t) * 1e3)
        cell.append(op.last_info["cell_ms"]); csm.append(op.last_info["csm_ms"])
    out["configs"][name] = {"S": S, "sites": int(sn.n_sites), "environments": dict(collections.Counter(sn.coordination_environments.tolist())),
                            "info": op.last_info, "run_wall_ms": stats(wall), "cell_kernel_ms": stats(cell), "csm_kernel_ms": stats(csm)}
    print(name, json.dumps(out["configs"][name]), flush=True)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "coordenv_bench.json", "w"), indent=1)
