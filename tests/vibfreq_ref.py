"""numpy restatement of ``AverageVibrationalFrequency`` (reference ``sitator/dynamics/AverageVibrationalFrequency.py:30-61``),
step by step, with every intermediate the device path can be compared on; the test inputs; and the reader of
``tests/golden/vibfreq_known_answers.npz`` (results of the reference's own class, recorded by ``make_vibfreq_golden.py``)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vibfreq_known_answers.npz")
SIGMA = 0.05


def random_walk(n_frames, n_atoms, seed, sigma=SIGMA, scale=None):
    """``[n_frames, n_atoms, 3]``: every atom a random walk with Gaussian steps (power in every bin: the ratio of the two
    band sums is well conditioned).  ``scale``: per-atom factors on the steps."""
    rng = np.random.default_rng(seed)
    steps = rng.normal(scale=sigma, size=(n_frames, n_atoms, 3))
    if scale is not None:
        steps *= np.asarray(scale, dtype=np.float64)[None, :, None]
    return np.ascontiguousarray(10.0 * rng.random((1, n_atoms, 3)) + np.cumsum(steps, axis=0))


def band(n, min_frequency=0, max_frequency=np.inf):
    """``(freqs, fmask)`` of a transform of length ``n``: steps 2 and 3."""
    freqs = np.fft.rfftfreq(n)
    return freqs, (freqs > min_frequency) & (freqs < max_frequency)


def restatement(traj, mask, min_frequency=0, max_frequency=np.inf):
    """The five steps; a dict of ``speeds`` [n_sel, n], ``freqs``, ``fmask``, ``spectrum`` [n_sel, n // 2 + 1],
    ``band_power`` and ``avg`` per atom, ``mean`` and ``std`` over the atoms."""
    traj = np.asarray(traj)
    d = traj[1:, mask] - traj[:-1, mask]                                       # 1: no periodic wrap
    speeds = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    freqs, fmask = band(speeds.shape[0], min_frequency, max_frequency)         # 2, 3
    assert np.any(fmask), "Trajectory too short?"
    spectrum = np.stack([np.fft.rfft(speeds[:, a]) for a in range(speeds.shape[1])])
    ps = np.abs(spectrum) ** 2                                                 # 4
    band_power = np.array([np.sum(p[fmask]) for p in ps])
    avg = np.array([np.sum(freqs[fmask] * p[fmask]) for p in ps]) / band_power
    return dict(speeds=np.ascontiguousarray(speeds.T), freqs=freqs, fmask=fmask, spectrum=spectrum, band_power=band_power,
                avg=avg, mean=np.mean(avg), std=np.std(avg))                   # 5


class VibGoldens(object):
    """The cases of the golden file: ``case(name)`` -> ``(traj, mask, kwargs, expected)``; ``expected`` is what the
    reference's ``compute_avg_vibrational_freq`` returned, as an array of one (or, with ``return_stdev``, two) values."""

    def __init__(self, path=GOLDEN):
        z = np.load(path)
        self.names = json.loads(str(z["names"]))
        self._z = {k: z[k] for k in z.files}

    def case(self, name):
        kwargs = json.loads(str(self._z[name + "/kwargs"]))
        if kwargs["max_frequency"] is None:
            kwargs["max_frequency"] = np.inf
        return self._z[name + "/traj"], self._z[name + "/mask"], kwargs, self._z[name + "/expected"]
