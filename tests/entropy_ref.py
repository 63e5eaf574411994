"""numpy restatement of ``ConfigurationalEntropy`` and of the residences it reads (``total_corrected_residences`` of
``JumpAnalysis``), and the small label arrays tests/golden/entropy_known_answers.npz was recorded on
(tests/make_entropy_golden.py ran the reference's own file over them)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "entropy_known_answers.npz")


def residences(labels, n_sites):
    """Frames an ion was at each site, a frame without a site counting for the ion's last known one."""
    labels = np.asarray(labels, dtype=np.int64)
    total = np.zeros(n_sites, dtype=np.int64)
    last = labels[0].copy()
    for frame in labels:
        now = np.where(frame < 0, last, frame)
        known = (now >= 0) & (last >= 0)
        np.add.at(total, now[known], 1)
        last = np.where(frame >= 0, frame, last)
    return total


def entropy(total, n_frames, site_types=None):
    """S~ from the residences: over the site types when given, else over the sites (no overshoot handling)."""
    total = np.asarray(total, dtype=np.float64)
    if site_types is None:
        N, n = np.ones(len(total)), total / n_frames
    else:
        kinds, N = np.unique(site_types, return_counts=True)
        n = np.array([total[site_types == k].sum() / n_frames for k in kinds])
    p = n / N
    keep = (p > 0.0) & (p < 1.0)
    return -float(np.sum(N[keep] * (p[keep] * np.log(p[keep]) + (1.0 - p[keep]) * np.log(1.0 - p[keep])))) / float(n.sum())


def _walk(frames, ions, sites, seed, hold=0.7, unknown=0.15):
    """Ions hopping between distinct sites, staying with probability `hold`, unassigned with probability `unknown`."""
    rng = np.random.default_rng(seed)
    at = rng.permutation(sites)[:ions]
    out = np.empty((frames, ions), dtype=np.int64)
    for f in range(frames):
        for i in range(ions):
            if rng.uniform() > hold:
                free = [s for s in range(sites) if s not in at]
                if free:
                    at[i] = free[rng.integers(len(free))]
        out[f] = np.where(rng.uniform(size=ions) < unknown, -1, at)
    return out


# name: (labels [frames, ions], n_sites, site_types or None, acceptable_overshoot)
def cases():
    crowded = np.zeros((16, 3), dtype=np.int64)                       # three ions on site 0 and one type of one site: P_2 = 3
    two = np.stack([np.zeros(40, dtype=np.int64), np.where(np.arange(40) % 8 == 7, 2, 1)], axis=1)
    return {
        "by_site": (_walk(64, 8, 20, 1), 20, None, 0.0),
        "by_site_few_frames": (_walk(5, 2, 6, 2), 6, None, 0.0),
        "by_site_first_frame_unknown": (np.concatenate([-np.ones((2, 4), dtype=np.int64), _walk(30, 4, 9, 3)]), 9, None, 0.0),
        "by_type": (_walk(64, 8, 20, 4), 20, np.arange(20) % 3, 0.0),
        "by_type_unsorted_labels": (_walk(48, 5, 12, 5), 12, np.array([7, 7, 2, 2, 2, 9, 9, 9, 9, 2, 7, 9]), 0.0),
        "by_type_one_type": (_walk(32, 3, 7, 6), 7, np.zeros(7, dtype=np.int64), 0.0),
        "by_site_full_site": (two, 3, None, 0.0),                     # site 0 always occupied: its term is 0
        "by_site_overshoot_raises": (crowded, 2, None, 0.0),
        "by_site_overshoot_not_forgiven": (crowded, 2, None, 1.5),
        "by_site_overshoot_forgiven": (crowded, 2, None, 2.5),
        "by_type_overshoot_raises": (crowded, 2, np.array([0, 1]), 0.5),
        "by_type_overshoot_forgiven": (np.concatenate([crowded, two[:8, :1].repeat(3, axis=1) + 1]), 2, np.array([4, 4]), 0.75),
    }
