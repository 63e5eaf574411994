"""CPU-only: what tests/test_density_binding.py does for the fourth header, for the fifth one, include/sitator_hip_percolation.h,
and the table of ``sitator_amd/_lib_percolation.py``: the library exports the three symbols, table and header agree in names and
arity, the five tables are disjoint and the first four headers do not name the new symbols, and the module's calls go through a stub
that converts every argument with ``argtypes[i].from_param`` - the context is the stub context of tests/test_binding_calls.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sitator_amd import _lib, _lib_density, _lib_percolation, _lib_scattering, _lib_vanhove
from sitator_amd._lib import HipContext
from sitator_amd._lib_percolation import SIGNATURES
from tests import percolation_ref as R
from tests.test_binding_calls import Stub, make_ctx, f

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sit_percolation_components", "sit_percolation_levels", "sit_percolation_plan"]
EARLIER = ("sitator_hip.h", "sitator_hip_vanhove.h", "sitator_hip_scattering.h", "sitator_hip_density.h")


def header_text(name):
    return open(os.path.join(ROOT, "include", name)).read()


def header_declarations(name="sitator_hip_percolation.h"):
    """``{symbol: number of parameters}`` of a header."""
    text = re.sub(r"/\*.*?\*/", "", header_text(name), flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\b(sit_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


class PercolationStub(Stub):
    """The stub of test_binding_calls.py with the three symbols of the fifth table beside those of the first."""

    def __getattr__(self, name):
        if name not in SIGNATURES:
            return Stub.__getattr__(self, name)
        res, argtypes = SIGNATURES[name]

        def call(*args):
            assert len(args) == len(argtypes), "%s: %d arguments, %d declared" % (name, len(args), len(argtypes))
            for k, (t, a) in enumerate(zip(argtypes, args)):
                try:
                    t.from_param(a)
                except (TypeError, C.ArgumentError) as e:
                    raise AssertionError("%s: argument %d (%r) is no %s: %s" % (name, k, a, t.__name__, e))
            self.calls.append((name, args))
            if name in self.effects:
                self.effects[name](args)
            rc = self.rc.get(name, 0)
            return rc.pop(0) if isinstance(rc, list) else rc
        return call


@pytest.fixture
def stub():
    return PercolationStub()


@pytest.fixture
def ctx(stub):
    c = make_ctx(stub)
    yield c
    c._h = None


def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib_percolation.bind(_lib.load())


def test_library_exports_the_symbols_and_the_table_is_the_header():
    lib = built()
    decl = header_declarations()
    assert sorted(decl) == sorted(SIGNATURES) == NAMES
    for name, nparams in decl.items():
        fn = getattr(lib, name)
        assert len(SIGNATURES[name][1]) == nparams == len(fn.argtypes) and fn.restype is C.c_int, name
    assert (decl["sit_percolation_components"], decl["sit_percolation_levels"], decl["sit_percolation_plan"]) == (11, 8, 4)


def test_the_five_tables_are_disjoint_and_the_first_four_headers_stay_as_they_are():
    tables = [set(_lib.SIGNATURES), set(_lib_vanhove.SIGNATURES), set(_lib_scattering.SIGNATURES), set(_lib_density.SIGNATURES), set(SIGNATURES)]
    for i in range(5):
        for j in range(i):
            assert not tables[i] & tables[j]
    for name in ("percolation_components", "percolation_levels", "percolation_plan", "density_components", "density_percolation"):
        assert not hasattr(HipContext, name)
    for earlier in EARLIER:
        assert "sit_percolation" not in header_text(earlier) and "sitator_hip_percolation" not in header_text(earlier)
    assert sorted(header_declarations("sitator_hip_density.h")) == ["sit_density", "sit_density_peaks", "sit_density_plan"]
    fifth = header_text("sitator_hip_percolation.h")
    assert '#include "sitator_hip.h"' in fifth and "SIT_ABI_VERSION" not in fifth


def test_components_marshals_every_argument(stub, ctx):
    grid = f(4, 5, 6)

    def effect(args):
        if args[6] is not None:
            args[6]._arr[...] = 3
        out = C.cast(args[8], C.POINTER(C.c_int64))
        for k in range(24):
            out[k] = 100 + k
        C.cast(args[9], C.POINTER(C.c_int64))[0] = 2
        args[10]._arr[:] = [5, 17, 2, 9]
    stub.effects["sit_percolation_components"] = effect
    labels, rec, info = _lib_percolation.percolation_components(ctx, grid, 0.25, connectivity=18, form=1)
    (args,) = stub.of("sit_percolation_components")
    assert stub.names() == ["sit_percolation_components"]
    assert args[1]._arr.shape == (4, 5, 6) and args[1]._arr.dtype == np.float64 and list(args[2]._arr) == [4, 5, 6]
    assert args[3:6] == (0.25, 18, 1) and args[6]._arr is labels and args[7] == 1 << 16
    assert labels.shape == (4, 5, 6) and labels.dtype == np.int32 and np.all(labels == 3)
    assert rec.shape == (2, 12) and rec.dtype == np.int64 and rec.reshape(-1).tolist() == list(range(100, 124)) and info == (5, 17, 2, 9)
    labels, rec, _ = _lib_percolation.percolation_components(ctx, grid.astype(np.float32), -np.inf, want_labels=False)
    args = stub.of("sit_percolation_components")[-1]
    assert labels is None and args[6] is None and args[3] == -np.inf and args[4:6] == (26, 0) and args[1]._arr.dtype == np.float64
    for bad in (np.zeros((2, 2)), np.zeros((2, 2, 2, 2)), np.zeros(5)):
        with pytest.raises(ValueError, match="3-D"):
            _lib_percolation.percolation_components(ctx, bad, 0.0)
        with pytest.raises(ValueError, match="3-D"):
            _lib_percolation.percolation_levels(ctx, bad)


def test_components_capacity_protocol(stub, ctx):
    """As ``HipContext._records``: asked for with room for 2^16, and where there are more, again with room for all."""
    total = (1 << 16) + 3

    def effect(args):
        cap = args[7]
        out = C.cast(args[8], C.POINTER(C.c_int64))
        for k in range(min(cap, total)):
            out[12 * k] = 2 * k
            out[12 * k + 1] = 1
        C.cast(args[9], C.POINTER(C.c_int64))[0] = total
    stub.effects["sit_percolation_components"] = effect
    _, rec, _ = _lib_percolation.percolation_components(ctx, f(64, 64, 32), 0.5, connectivity=6)
    calls = stub.of("sit_percolation_components")
    assert [c[7] for c in calls] == [1 << 16, total] and rec.shape == (total, 12) and rec.flags.c_contiguous
    assert np.array_equal(rec[:, 0], 2 * np.arange(total)) and np.all(rec[:, 1] == 1)


def test_levels_marshals_every_argument(stub, ctx):
    def effect(args):
        args[5]._arr[:] = [0.5, 0.25, 0.0]
        args[6]._arr[:] = [2, 2, 0]
        args[7]._arr[:] = [40, 3, 12, 2]
    stub.effects["sit_percolation_levels"] = effect
    grid = f(3, 4, 5)
    levels, ranks, info = _lib_percolation.percolation_levels(ctx, grid, connectivity=6, form=2)
    (args,) = stub.of("sit_percolation_levels")
    assert args[1]._arr.shape == (3, 4, 5) and list(args[2]._arr) == [3, 4, 5] and args[3:5] == (6, 2)
    assert args[5]._arr is levels and levels.dtype == np.float64 and levels.tolist() == [0.5, 0.25, 0.0]
    assert args[6]._arr is ranks and ranks.dtype == np.int32 and ranks.tolist() == [2, 2, 0] and info == (40, 3, 12, 2)


def test_a_wrong_dtype_fails_in_from_param(stub, ctx):
    argtypes = SIGNATURES["sit_percolation_components"][1]
    good = np.zeros(3, dtype=np.int64)
    argtypes[2].from_param(_lib._ptr(good))
    for k, bad in ((1, np.zeros(3, dtype=np.int64)), (2, np.zeros(3)), (6, np.zeros(3, dtype=np.int64)), (8, np.zeros(3, dtype=np.int32)),
                   (10, np.zeros(4))):
        with pytest.raises((TypeError, C.ArgumentError)):
            argtypes[k].from_param(_lib._ptr(bad))
    with pytest.raises(AssertionError, match="argument 6"):
        stub.sit_percolation_components(ctx._h, _lib._ptr(np.zeros(3)), _lib._ptr(good), 0.5, 26, 0, _lib._ptr(np.zeros(3)), 4, _lib._ptr(good),
                                        C.byref(C.c_int64(0)), _lib._ptr(good))
    with pytest.raises(AssertionError, match="arguments"):
        stub.sit_percolation_levels(ctx._h)
    assert stub.calls == []


def test_status_codes_become_exceptions(stub, ctx):
    stub.message = b"sit_percolation_components: connectivity is 6, 18 or 26"
    stub.rc["sit_percolation_components"] = _lib.E_INVALID
    with pytest.raises(ValueError, match="6, 18 or 26"):
        _lib_percolation.percolation_components(ctx, f(2, 2, 2), 0.5, connectivity=7)
    stub.rc["sit_percolation_components"] = _lib.E_HIP
    with pytest.raises(RuntimeError, match="libsitator_hip"):
        _lib_percolation.percolation_components(ctx, f(2, 2, 2), 0.5)
    stub.rc["sit_percolation_levels"] = _lib.E_INVALID
    stub.message = b"sit_percolation_levels: more than 2^27 voxels"
    with pytest.raises(ValueError, match="2\\^27"):
        _lib_percolation.percolation_levels(ctx, f(2, 2, 2))
    stub.rc["sit_percolation_levels"] = _lib.E_CAPACITY
    with pytest.raises(RuntimeError):
        _lib_percolation.percolation_levels(ctx, f(2, 2, 2))


def test_plan_function(stub, monkeypatch):
    monkeypatch.setattr(_lib, "_lib", stub)

    def effect(args):
        p = C.cast(args[3], C.POINTER(C.c_int64))
        for k in range(12):
            p[k] = 100 + k
    stub.effects["sit_percolation_plan"] = effect
    plan = _lib_percolation.percolation_plan((5, 6, 7), connectivity=18, form=2)
    assert list(plan) == _lib_percolation.PLAN_KEYS and list(plan.values()) == list(range(100, 112))
    args = stub.of("sit_percolation_plan")[0]
    assert list(args[0]._arr) == [5, 6, 7] and args[1:3] == (18, 2)
    stub.rc["sit_percolation_plan"] = _lib.E_INVALID
    with pytest.raises(ValueError, match="percolation_plan"):
        _lib_percolation.percolation_plan((0, 6, 7))
    with pytest.raises(ValueError, match="per axis"):
        _lib_percolation.percolation_plan((5, 6))


def test_plan_of_the_library_is_the_restatement():
    """No GPU is needed for the plan: the library's answer is the restatement's."""
    built()
    for n in ((1, 1, 1), (2, 3, 5), (17, 16, 33), (64, 48, 40), (160, 176, 192), (1024, 1024, 128)):
        for connectivity in (6, 18, 26):
            for form in (0, 1, 2):
                exp = R.plan(n, connectivity, form)
                plan = _lib_percolation.percolation_plan(n, connectivity, form)
                assert (plan["threads"], plan["tile0"], plan["tile1"], plan["tile2"]) == (R.THREADS,) + R.TILE
                assert (plan["lds_bytes"], plan["tiles"], plan["form"], plan["seam_records_max"], plan["workspace"], plan["voxels"],
                        plan["blocks"]) == (exp["lds_bytes"], exp["n_tiles"], exp["form"], exp["seam_max"], exp["workspace"], exp["V"], exp["blocks"])
                assert plan["record_words"] == _lib_percolation.RECORD_WORDS == 12
    for bad in (dict(grid=(1025, 1, 1)), dict(grid=(0, 1, 1)), dict(grid=(1024, 1024, 129)), dict(grid=(4, 4, 4), connectivity=8),
                dict(grid=(4, 4, 4), form=3)):
        with pytest.raises(ValueError):
            _lib_percolation.percolation_plan(**bad)
        assert R.plan(bad["grid"], bad.get("connectivity", 26), bad.get("form", 0)) is None


def test_results_on_made_up_records():
    """The result classes are host code: ranks, masks, masses, barriers."""
    from sitator_amd.percolation import ComponentsResult, PercolationResult
    grid = np.zeros((2, 2, 3))
    labels = np.full((2, 2, 3), -1, dtype=np.int32)
    labels[0, 0, :], labels[1, 1, 1] = 0, 10
    grid[0, 0, :], grid[1, 1, 1] = [1.0, 2.0, 4.0], 0.5
    rec = np.array([[0, 3, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0], [10, 1, 0] + [0] * 9], dtype=np.int64)
    cell = np.diag([2.0, 3.0, 5.0])
    r = ComponentsResult(grid, cell, 0.5, 26, labels, rec, (4, 2, 1, 1))
    assert r.roots.tolist() == [0, 10] and r.sizes.tolist() == [3, 1] and r.rank.tolist() == [1, 0] and r.basis.shape == (2, 3, 3)
    assert r.directions[0].tolist() == [[0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]] and r.mass.tolist() == [7.0, 0.5]
    assert np.array_equal(r.percolating(1), labels == 0) and not r.percolating(2).any() and (r.rounds, r.seam_records) == (4, 2)
    p = PercolationResult(np.array([0.5, 0.25, 0.0]), np.array([2, 2, 0], dtype=np.int32), (40, 3, 12, 2), 4.0)
    assert p.dimensionality == 2 and p.passes == 40
    b = p.barriers(0.025)
    assert b[0] == -0.025 * np.log(0.5 / 4.0) and b[1] == -0.025 * np.log(0.25 / 4.0) and b[2] == np.inf
