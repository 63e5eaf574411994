"""CPU-only: what tests/test_scattering_binding.py does for the third header, for the fourth one, include/sitator_hip_density.h,
and the table of ``sitator_amd/_lib_density.py``: the library exports the three symbols, table and header agree in names and arity,
the four tables are disjoint and the first three headers do not name the new symbols, and the module's calls go through a stub
that converts every argument with ``argtypes[i].from_param`` - the context is the stub context of tests/test_binding_calls.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sitator_amd import _lib, _lib_density, _lib_scattering, _lib_vanhove
from sitator_amd._lib import HipContext
from sitator_amd._lib_density import SIGNATURES
from tests import density_ref as R
from tests.test_binding_calls import Stub, make_ctx, F, A, MOBILE, f

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sit_density", "sit_density_peaks", "sit_density_plan"]


def header_text(name):
    return open(os.path.join(ROOT, "include", name)).read()


def header_declarations():
    """``{symbol: number of parameters}`` of include/sitator_hip_density.h."""
    text = re.sub(r"/\*.*?\*/", "", header_text("sitator_hip_density.h"), flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\b(sit_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


class DensityStub(Stub):
    """The stub of test_binding_calls.py with the three symbols of the fourth table beside those of the first."""

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
    return DensityStub()


@pytest.fixture
def ctx(stub):
    c = make_ctx(stub)
    yield c
    c._h = None


def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib_density.bind(_lib.load())


def test_library_exports_the_symbols_and_the_table_is_the_header():
    lib = built()
    decl = header_declarations()
    assert sorted(decl) == sorted(SIGNATURES) == NAMES
    for name, nparams in decl.items():
        fn = getattr(lib, name)
        assert len(SIGNATURES[name][1]) == nparams == len(fn.argtypes) and fn.restype is C.c_int, name
    assert (decl["sit_density"], decl["sit_density_peaks"], decl["sit_density_plan"]) == (19, 7, 13)


def test_the_four_tables_are_disjoint_and_the_first_three_headers_stay_as_they_are():
    tables = [set(_lib.SIGNATURES), set(_lib_vanhove.SIGNATURES), set(_lib_scattering.SIGNATURES), set(SIGNATURES)]
    for i in range(4):
        for j in range(i):
            assert not tables[i] & tables[j]
    for name in ("density", "density_peaks", "density_plan"):
        assert not hasattr(HipContext, name)
    for first in ("sitator_hip.h", "sitator_hip_vanhove.h", "sitator_hip_scattering.h"):
        assert "sit_density" not in header_text(first) and "sitator_hip_density" not in header_text(first)
    fourth = header_text("sitator_hip_density.h")
    assert '#include "sitator_hip.h"' in fourth and "SIT_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", fourth, flags=re.S)


def test_the_call_marshals_every_argument(stub, ctx):
    ctx._deferred, ctx.labels_version, ctx.labels_digest = 1, 5, (5, "digest")

    def effect(args):
        args[16]._arr[...] = 7
        if args[17] is not None:
            args[17]._arr[...] = 0.5
        args[18]._arr[:] = [11, 3]
    stub.effects["sit_density"] = effect
    counts, smoothed, taken, skipped = _lib_density.density(ctx, MOBILE, (2, 3, 5), frame_stride=2, form=1, workspace_bytes=4096)
    (args,) = stub.of("sit_density")
    assert stub.names() == ["sit_density"]                         # no labels: no deferred pass is collected
    assert (ctx._deferred, ctx.labels_version, ctx.labels_digest) == (1, 5, (5, "digest"))
    assert args[1] is None and (args[2], args[3]) == (F, A)        # the resident frames
    assert list(args[4]._arr) == MOBILE and args[5] == len(MOBILE) and args[6] == 2 and list(args[7]._arr) == [2, 3, 5]
    assert args[8] is None and args[9:11] == (0, 1) and args[11] is None and args[12] is None and args[13:16] == (0, 1, 4096)
    assert args[16]._arr is counts and counts.shape == (1, 2, 3, 5) and counts.dtype == np.uint64 and np.all(counts == 7)
    assert args[17] is None and smoothed is None and (taken, skipped) == (11, 3)
    # a host array, taps and classes
    pos = f(F, 3, 3)
    taps, w = [[0, 0, 0], [1, 0, -1]], [0.75, 0.25]
    ctx._deferred = 0
    counts, smoothed, _, _ = _lib_density.density(ctx, [0, 1, 2], (4, 4, 4), positions=pos, site_class=[0, 1, 0, 2], n_classes=4, taps=taps, weights=w)
    args = stub.of("sit_density")[-1]
    assert args[1]._arr.shape == (F, 3, 3) and (args[2], args[3]) == (F, 3)
    assert args[8]._arr.dtype == np.int32 and list(args[8]._arr) == [0, 1, 0, 2] and args[9:11] == (4, 4)
    assert args[11]._arr.dtype == np.int64 and args[11]._arr.tolist() == taps and list(args[12]._arr) == w and args[13] == 2
    assert counts.shape == smoothed.shape == (4, 4, 4, 4) and smoothed.dtype == np.float64 and np.all(smoothed == 0.5)
    assert args[17]._arr is smoothed
    for bad in (dict(grid=(2, 3)), dict(grid=(2, 3, 4, 5)), dict(taps=[[1, 2]], weights=[1.0]), dict(taps=[[1, 2, 3]], weights=[1.0, 2.0]),
                dict(grid=(1025, 1, 1)), dict(n_classes=17), dict(grid=(1024, 1024, 1024))):
        kw = dict(dict(grid=(2, 2, 2)), **bad)
        with pytest.raises(ValueError):
            _lib_density.density(ctx, [0], kw.pop("grid"), **kw)


def test_a_wrong_dtype_fails_in_from_param(stub, ctx):
    argtypes = SIGNATURES["sit_density"][1]
    good = np.zeros(3, dtype=np.int64)
    argtypes[4].from_param(_lib._ptr(good))
    for k, bad in ((4, np.zeros(3)), (8, np.zeros(3, dtype=np.int64)), (1, np.zeros(3, dtype=np.int64)), (16, np.zeros(3, dtype=np.int64)),
                   (17, np.zeros(3, dtype=np.uint64)), (12, np.zeros(3, dtype=np.int32))):
        with pytest.raises((TypeError, C.ArgumentError)):
            argtypes[k].from_param(_lib._ptr(bad))
    with pytest.raises(AssertionError, match="argument 16"):       # and the stub says which argument
        stub.sit_density(ctx._h, None, F, A, _lib._ptr(good), 3, 1, _lib._ptr(good), None, 0, 1, None, None, 0, 0, 0, _lib._ptr(np.zeros(3)), None,
                         _lib._ptr(good))
    with pytest.raises(AssertionError, match="arguments"):
        stub.sit_density(ctx._h)
    assert stub.calls == []


def test_status_codes_become_exceptions(stub, ctx):
    stub.message = b"sit_density: frame_stride is below 1"
    stub.rc["sit_density"] = _lib.E_INVALID
    with pytest.raises(ValueError, match="below 1"):
        _lib_density.density(ctx, MOBILE, (2, 2, 2), frame_stride=0)
    stub.message = b"index 9 is out of bounds for axis 0 with size 4"
    with pytest.raises(IndexError, match="out of bounds"):
        _lib_density.density(ctx, MOBILE, (2, 2, 2), site_class=[0, 0, 0, 0], n_classes=2)
    stub.rc["sit_density"] = _lib.E_HIP
    with pytest.raises(RuntimeError, match="libsitator_hip"):
        _lib_density.density(ctx, MOBILE, (2, 2, 2))
    stub.rc["sit_density_peaks"] = _lib.E_INVALID
    stub.message = b"sit_density_peaks: more than 2^27 voxels"
    with pytest.raises(ValueError, match="2\\^27"):
        _lib_density.density_peaks(ctx, np.zeros((2, 2, 2)), 0.0)
    with pytest.raises(ValueError, match="3-D"):
        _lib_density.density_peaks(ctx, np.zeros((2, 2)), 0.0)


def test_peaks_capacity_protocol(stub, ctx):
    """As ``HipContext._records``: asked for with room for 2^16, and where there are more, again with room for all."""
    total = (1 << 16) + 5

    def effect(args):
        cap = args[4]
        out = C.cast(args[5], C.POINTER(C.c_int64))
        for k in range(min(cap, total)):
            out[k] = 2 * k
        C.cast(args[6], C.POINTER(C.c_int64))[0] = total
    stub.effects["sit_density_peaks"] = effect
    grid = f(64, 64, 32)
    v = _lib_density.density_peaks(ctx, grid, 0.25)
    calls = stub.of("sit_density_peaks")
    assert [c[4] for c in calls] == [1 << 16, total] and calls[0][3] == 0.25 and list(calls[0][2]._arr) == [64, 64, 32]
    assert calls[0][1]._arr.shape == (64, 64, 32) and v.dtype == np.int64 and v.flags.c_contiguous
    assert np.array_equal(v, 2 * np.arange(total))


def test_plan_function(stub, monkeypatch):
    monkeypatch.setattr(_lib, "_lib", stub)

    def effect(args):
        p = C.cast(args[12], C.POINTER(C.c_int64))
        for k in range(20):
            p[k] = 100 + k
    stub.effects["sit_density_plan"] = effect
    plan = _lib_density.density_plan(100, 9, 4, (5, 6, 7), frame_stride=3, K=8, n_classes=3, n_taps=27, halo=(1, 1, 2), form=2, host=False,
                                     workspace_bytes=1 << 20)
    assert list(plan) == _lib_density.PLAN_KEYS and list(plan.values()) == list(range(100, 120))
    args = stub.of("sit_density_plan")[0]
    assert args[:4] == (100, 9, 4, 3) and list(args[4]._arr) == [5, 6, 7] and args[5:8] == (8, 3, 27) and list(args[8]._arr) == [1, 1, 2]
    assert args[9:12] == (2, 0, 1 << 20)
    stub.rc["sit_density_plan"] = _lib.E_INVALID
    with pytest.raises(ValueError, match="density_plan"):
        _lib_density.density_plan(100, 9, 4, (0, 6, 7))
    with pytest.raises(ValueError, match="per axis"):
        _lib_density.density_plan(100, 9, 4, (5, 6))


@pytest.mark.parametrize("cap", [0, 1 << 22, 64 * 140 * 24])
def test_plan_of_the_library_is_the_restatement(cap):
    """No GPU is needed for the plan: the library's answer is the restatement's."""
    built()
    for F_, A_, n_sel, grid, stride, K, nc, n_taps, halo, form, host in (
            (100000, 576, 64, (50, 50, 50), 1, 0, 1, 0, (0, 0, 0), 0, False), (389, 140, 130, (17, 16, 33), 3, 40, 3, 27, (1, 1, 1), 2, True),
            (389, 140, 130, (64, 48, 40), 1, 0, 1, 925, (6, 6, 6), 1, True), (100000, 576, 64, (64, 48, 40), 1, 0, 1, 9, (31, 0, 0), 0, True)):
        exp = R.plan(F_, A_, n_sel, grid, stride, K, nc, n_taps, halo, form, host, cap)
        if exp is None:
            with pytest.raises(ValueError):
                _lib_density.density_plan(F_, A_, n_sel, grid, stride, K, nc, n_taps, halo, form, host, cap)
            continue
        plan = _lib_density.density_plan(F_, A_, n_sel, grid, stride, K, nc, n_taps, halo, form, host, cap)
        assert (plan["threads"], plan["table_slots"], plan["probe_limit"], plan["frames_per_run"]) == (R.THREADS, R.SLOTS, R.PROBE, R.RUN)
        assert (plan["tile0"], plan["tile1"], plan["tile2"]) == R.TILE and [plan["ext0"], plan["ext1"], plan["ext2"]] == exp["ext"]
        assert plan["lds_bytes"] == exp["lds_bytes"] <= 65536 and plan["smooth_lds_bytes"] == exp["smooth_lds"] <= R.SMOOTH_LDS
        assert (plan["runs"], plan["window"], plan["n_windows"], plan["workspace"], plan["frames_taken"], plan["voxels"], plan["cells"]) == (
            exp["runs"], exp["window"], exp["n_windows"], exp["workspace"], exp["taken"], exp["V"], exp["cells"])
        assert plan["form"] == exp["form"] and (form == 0 or plan["form"] == form) and plan["workspace"] <= (cap or R.DEFAULT_WORKSPACE)
    with pytest.raises(ValueError):
        _lib_density.density_plan(100, 3, 3, (1025, 1, 1))
    with pytest.raises(ValueError):
        _lib_density.density_plan(100, 3, 3, (4, 4, 4), workspace_bytes=100)
    assert _lib_density.density_plan(100, 3, 3, (4, 4, 4), workspace_bytes=100, host=False)["workspace"] == 0
