"""Records tests/golden/vibfreq_known_answers.npz: what the reference's AverageVibrationalFrequency returns on a handful of
small inputs.  Run by hand where a checkout of the reference is at hand, never by a test:

    python tests/make_vibfreq_golden.py /path/to/sitator

The reference's file imports numpy alone, so it is loaded by its path; the package (and what it drags in) is not."""
import importlib.util
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import vibfreq_ref as V  # noqa: E402

# name: (frames, atoms, seed, mask, min_frequency, max_frequency (None: inf), return_stdev)
CASES = {
    "defaults_n_odd": (34, 4, 11, [True, True, True, True], 0, None, False),
    "band_n_even": (33, 4, 12, [True, True, True, True], 0.05, 0.3, False),
    "stdev_defaults": (34, 5, 13, [True, True, True, True, True], 0, None, True),
    "index_mask_skips_atoms_band_stdev": (101, 7, 14, [5, 0, 3], 0.05, 0.3, True),
    "bool_mask_skips_atoms": (258, 6, 15, [False, True, True, False, True, False], 0, None, False),
    "narrow_band_stdev": (200, 3, 16, [True, False, True], 0.1, 0.12, True),
}


def main(reference_root):
    path = os.path.join(reference_root, "sitator", "dynamics", "AverageVibrationalFrequency.py")
    spec = importlib.util.spec_from_file_location("reference_avf", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {"names": np.array(json.dumps(list(CASES)))}
    for name, (F, A, seed, mask, fmin, fmax, stdev) in CASES.items():
        traj = V.random_walk(F, A, seed)
        mask = np.asarray(mask)
        op = mod.AverageVibrationalFrequency(min_frequency=fmin, max_frequency=np.inf if fmax is None else fmax)
        res = op.compute_avg_vibrational_freq(traj.copy(), mask, return_stdev=stdev)
        out[name + "/traj"] = traj
        out[name + "/mask"] = mask
        out[name + "/kwargs"] = np.array(json.dumps(dict(min_frequency=fmin, max_frequency=fmax, return_stdev=stdev)))
        out[name + "/expected"] = np.atleast_1d(np.asarray(res, dtype=np.float64))
    np.savez_compressed(V.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (V.GOLDEN, os.path.getsize(V.GOLDEN)))


if __name__ == "__main__":
    main(sys.argv[1])
