"""Potentials the device evaluates itself.  ``MergeSitesByBarrier`` of the reference takes any ASE calculator and names
``ase.calculators.lj.LennardJones`` as the kind it means (``network/MergeSitesByBarrier.py:32-33``); here the calculator is a
description of the potential, and the energies come from ``sit_barrier_energies`` (``csrc/barrier.hip``).
"""
import numbers

import numpy as np


class LennardJones(object):
    """A truncated and shifted 12-6 potential of the mobile species with every coordinating atom.

    :param epsilon, sigma: a positive real, or a dict ``{atomic number of the coordinating atom: value}``.
    :param rc: the cutoff; ``None``: three times the largest ``sigma``.

    With ``d`` the distance of the mobile atom to a coordinating atom of species ``s`` (or to one of its periodic images),
    ``s6 = (sigma_s**2 / d**2)**3`` and ``phi_s(d) = 4 * epsilon_s * s6 * (s6 - 1) - e0_s`` for ``d**2 <= rc**2``, else 0;
    ``e0_s`` is the same expression at ``d = rc``, so the potential is continuous at the cutoff.  ``d = 0`` gives ``+inf``.
    This is defined here and not by ASE (whose ``LennardJones`` has one ``epsilon`` / ``sigma`` for all pairs).
    """

    def __init__(self, epsilon=1.0, sigma=1.0, rc=None):
        self.epsilon = self._checked("epsilon", epsilon)
        self.sigma = self._checked("sigma", sigma)
        if rc is None:
            rc = 3.0 * (max(self.sigma.values()) if isinstance(self.sigma, dict) else self.sigma)
        if not isinstance(rc, numbers.Real) or not (0.0 < float(rc) < np.inf):
            raise ValueError("LennardJones: `rc` must be a positive real, not %r" % (rc,))
        self.rc = float(rc)

    @staticmethod
    def _checked(name, value):
        if isinstance(value, dict):
            if not value:
                raise ValueError("LennardJones: `%s` is an empty dict" % name)
            out = {}
            for number, v in value.items():
                if not isinstance(number, numbers.Integral):
                    raise ValueError("LennardJones: the keys of `%s` are atomic numbers, not %r" % (name, number))
                out[int(number)] = LennardJones._checked(name, v)
            return out
        if isinstance(value, bool) or not isinstance(value, numbers.Real) or not (0.0 < float(value) < np.inf):
            raise ValueError("LennardJones: `%s` must be a positive real or a dict of them, not %r" % (name, value))
        return float(value)

    def _per_atom(self, name, value, atomic_numbers):
        if not isinstance(value, dict):
            return np.full(len(atomic_numbers), value, dtype=np.float64)
        missing = sorted(set(atomic_numbers.tolist()) - set(value))
        if missing:
            raise ValueError("LennardJones: no `%s` for the coordinating atoms of atomic number %s" % (name, missing))
        return np.array([value[z] for z in atomic_numbers.tolist()], dtype=np.float64)

    def parameters_for(self, atomic_numbers):
        """``(epsilon [S], sigma [S])`` of coordinating atoms with these atomic numbers; a species without a value raises
        ``ValueError``."""
        atomic_numbers = np.asarray(atomic_numbers, dtype=np.int64).reshape(-1)
        return self._per_atom("epsilon", self.epsilon, atomic_numbers), self._per_atom("sigma", self.sigma, atomic_numbers)
