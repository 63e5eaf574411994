"""ctypes binding of the landscape entry points of ``libsitator_hip.so`` (declared in ``include/sitator_hip_landscape.h``, the sixth
header of the library): a signature table of its own, set on the object ``_lib.load()`` returns, and module-level functions that
take a ``HipContext``.  The five other tables and the methods of ``HipContext`` stay as they are."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import _d, _i, _f64, _triple, _dp, _ip, _vp, i64

# every symbol include/sitator_hip_landscape.h declares: (restype, argtypes)
SIGNATURES = {
    "sit_landscape_energies": (C.c_int, [_vp, _dp, _dp, _dp, i64, C.c_double, _ip, C.c_int, _dp, _ip]),
    "sit_landscape_plan": (C.c_int, [_dp, C.c_double, _ip, C.c_int, _ip]),
}

PLAN_KEYS = ["tile0", "tile1", "tile2", "threads", "lds_bytes", "list_capacity", "tiles", "form", "n0", "n1", "n2", "wide0", "wide1",
             "wide2", "voxels", "atom_tile"]
MAX_GRID = 1024
MAX_VOXELS = 1 << 27


def bind(lib):
    """Sets ``argtypes`` / ``restype`` of the two symbols on ``lib`` (once) and returns it."""
    return _lib.bind_signatures(lib, "_landscape_bound", SIGNATURES)


def landscape_plan(cell, rc, grid, form=0):
    """The plan of ``landscape_energies`` for ``cell`` (rows are the cell vectors), the cutoff ``rc`` and a grid ``(n0, n1, n2)``
    (``sit_landscape_plan``): the tile of voxels of a workgroup, its threads and LDS bytes, the records of a chunk of a tile's list,
    the tiles, the form that 0 resolves to, ``translations`` - ``|t_a|`` of the direct form - and ``list_translations`` - those of the
    list of a full tile.  Whatever the call would refuse of these arguments: ``ValueError``."""
    lib = bind(_lib.load())
    cell, g = _f64(cell).reshape(3, 3), _triple(grid, "grid")
    rc_, plan = _lib._plan(PLAN_KEYS, lambda out: lib.sit_landscape_plan(_d(cell), float(rc), _i(g), int(form), out))
    if rc_ != _lib.OK:
        raise ValueError("landscape_plan: an axis outside [1, 1024], more than 2^27 voxels, a form outside {0, 1, 2}, a degenerate cell, "
                         "or rc not positive or beyond 255 perpendicular heights of the cell")
    plan["translations"] = _lib._translations(plan)
    plan["list_translations"] = (plan.pop("wide0"), plan.pop("wide1"), plan.pop("wide2"))
    return plan


def landscape_energies(ctx, static_pos, eps, sigma, rc, grid, form=0):
    """``(energies float64 [n0, n1, n2], info)`` of ``sit_landscape_energies`` on the context ``ctx``, whose cell is the cell: the
    energy of a probe ion at every voxel centre among the atoms ``static_pos`` ``[S, 3]`` with ``eps`` / ``sigma`` ``[S]`` and all
    their periodic images under the truncated and shifted 12-6 potential; ``info`` = (form taken, tiles, list chunks of the longest
    tile, candidate terms).  Anything that does not fit raises ``ValueError``."""
    lib = bind(ctx.lib)
    static_pos = _f64(static_pos).reshape(-1, 3)
    eps, sigma = _f64(eps).reshape(-1), _f64(sigma).reshape(-1)
    if not len(eps) == len(static_pos) == len(sigma):
        raise ValueError("one epsilon and one sigma per static atom are needed")
    g = _triple(grid, "grid")
    if any(v < 1 or v > MAX_GRID for v in g) or int(np.prod(g)) > MAX_VOXELS:                          # before the output is made
        raise ValueError("sit_landscape_energies: an axis of the grid holds 1 to 1024 voxels, and 2^27 voxels at most")
    energies = np.empty(tuple(int(v) for v in g), dtype=np.float64)
    info = np.zeros(4, dtype=np.int64)
    ctx._check(lib.sit_landscape_energies(ctx._h, _d(static_pos), _d(eps), _d(sigma), len(static_pos), float(rc), _i(g), int(form),
                                          _d(energies), _i(info)))
    return energies, tuple(int(v) for v in info)
