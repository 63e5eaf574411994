"""CPU-only: what tests/test_vanhove_binding.py does for the second header, for the third one, include/sitator_hip_scattering.h,
and the table of ``sitator_amd/_lib_scattering.py``: the library exports both symbols, table and header agree in names and arity,
the three tables are disjoint and the first two headers do not name the new symbols, and the module's calls go through a stub
that converts every argument with ``argtypes[i].from_param`` - the context is the stub context of tests/test_binding_calls.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sitator_amd import _lib, _lib_scattering, _lib_vanhove
from sitator_amd._lib import HipContext
from sitator_amd._lib_scattering import SIGNATURES
from tests import scattering_ref as S
from tests.test_binding_calls import Stub, make_ctx, F, A, MOBILE, f

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sit_scattering", "sit_scattering_plan"]


def header_text(name):
    return open(os.path.join(ROOT, "include", name)).read()


def header_declarations():
    """``{symbol: number of parameters}`` of include/sitator_hip_scattering.h."""
    text = re.sub(r"/\*.*?\*/", "", header_text("sitator_hip_scattering.h"), flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\b(sit_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


class ScatteringStub(Stub):
    """The stub of test_binding_calls.py with the two symbols of the third table beside those of the first."""

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
            return self.rc.get(name, 0)
        return call


@pytest.fixture
def stub():
    return ScatteringStub()


@pytest.fixture
def ctx(stub):
    c = make_ctx(stub)
    yield c
    c._h = None


def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib_scattering.bind(_lib.load())


def test_library_exports_both_symbols_and_the_table_is_the_header():
    lib = built()
    decl = header_declarations()
    assert sorted(decl) == sorted(SIGNATURES) == NAMES
    for name, nparams in decl.items():
        fn = getattr(lib, name)
        assert len(SIGNATURES[name][1]) == nparams == len(fn.argtypes) and fn.restype is C.c_int, name
    assert (decl["sit_scattering"], decl["sit_scattering_plan"]) == (17, 12)


def test_the_three_tables_are_disjoint_and_the_first_two_headers_stay_as_they_are():
    tables = [set(_lib.SIGNATURES), set(_lib_vanhove.SIGNATURES), set(SIGNATURES)]
    assert not tables[0] & tables[2] and not tables[1] & tables[2] and not tables[0] & tables[1]
    assert not hasattr(HipContext, "scattering") and not hasattr(HipContext, "scattering_plan")
    for first in ("sitator_hip.h", "sitator_hip_vanhove.h"):
        assert "sit_scattering" not in header_text(first) and "scattering" not in header_text(first)
    third = header_text("sitator_hip_scattering.h")
    assert '#include "sitator_hip.h"' in third and "SIT_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", third, flags=re.S)


def test_the_call_marshals_every_argument(stub, ctx):
    ctx._deferred, ctx.labels_version, ctx.labels_digest = 1, 5, (5, "digest")

    def effect(args):
        if args[15] is not None:
            args[15]._arr[...] = 1.0 + 2.0j
        if args[16] is not None:
            args[16]._arr[...] = -3.0j
    stub.effects["sit_scattering"] = effect
    q = [[0, 0, 0], [1, -2, 32], [-32, 0, 5], [2, 2, 2]]
    ss, cs = _lib_scattering.scattering(ctx, MOBILE, [0, 1, 2], q, [0, 1, 4], origin_stride=2, workspace_bytes=4096)
    (args,) = stub.of("sit_scattering")
    assert stub.names() == ["sit_scattering"]                     # no deferred pass is collected
    assert (ctx._deferred, ctx.labels_version, ctx.labels_digest) == (1, 5, (5, "digest"))
    assert args[1] is None and (args[2], args[3]) == (F, A)       # the resident frames
    assert list(args[4]._arr) == MOBILE and args[5] == len(MOBILE) and list(args[6]._arr) == [0, 1, 2] and args[7] == 3 and args[8] == 0
    assert args[9]._arr.shape == (4, 3) and args[9]._arr.dtype == np.int64 and args[9]._arr.tolist() == q and args[10] == 4
    assert list(args[11]._arr) == [0, 1, 4] and args[12:15] == (3, 2, 4096)
    assert args[15]._arr is ss and args[16]._arr is cs and ss.shape == cs.shape == (3, 4) and ss.dtype == cs.dtype == np.complex128
    assert np.all(ss == 1.0 + 2.0j) and np.all(cs == -3.0j)       # the library sees pairs of doubles
    # a host array, one selection, a part left out
    pos = f(F, 3, 3)
    ss, cs = _lib_scattering.scattering(ctx, [0, 1, 2], [0, 1, 2], q, [0], positions=pos, same=True, self_part=False)
    args = stub.of("sit_scattering")[-1]
    assert args[1]._arr.shape == (F, 3, 3) and (args[2], args[3], args[8]) == (F, 3, 1)
    assert ss is None and args[15] is None and args[16]._arr is cs
    ss, cs = _lib_scattering.scattering(ctx, [0], [1], q, [0], coherent_part=False)
    assert cs is None and stub.of("sit_scattering")[-1][16] is None and ss.shape == (1, 4)
    for bad in ([1, 2, 3], [[1, 2]], [[[1, 2, 3]]]):
        with pytest.raises(ValueError, match="triples"):
            _lib_scattering.scattering(ctx, [0], [1], bad, [0])


def test_a_wrong_dtype_fails_in_from_param(stub, ctx):
    argtypes = SIGNATURES["sit_scattering"][1]
    good = np.zeros(3, dtype=np.int64)
    argtypes[4].from_param(_lib._ptr(good))
    for k, bad in ((4, np.zeros(3)), (9, np.zeros(3, dtype=np.int32)), (1, np.zeros(3, dtype=np.int64)), (15, np.zeros(3, dtype=np.int64)),
                   (16, np.zeros(3, dtype=np.uint64))):
        with pytest.raises((TypeError, C.ArgumentError)):
            argtypes[k].from_param(_lib._ptr(bad))
    with pytest.raises(AssertionError, match="argument 9"):       # and the stub says which argument
        stub.sit_scattering(*([ctx._h, None, F, A, _lib._ptr(good), 3, _lib._ptr(good), 3, 0, _lib._ptr(np.zeros(3)), 1, _lib._ptr(good), 3, 1, 0,
                               None, None]))
    with pytest.raises(AssertionError, match="arguments"):
        stub.sit_scattering(ctx._h)
    assert stub.calls == []


def test_status_codes_become_exceptions(stub, ctx):
    stub.message = b"sit_scattering: an index of a q vector is beyond 32"
    stub.rc["sit_scattering"] = _lib.E_INVALID
    with pytest.raises(ValueError, match="beyond 32"):
        _lib_scattering.scattering(ctx, MOBILE, MOBILE, [[33, 0, 0]], [0], same=True)
    stub.rc["sit_scattering"] = _lib.E_HIP
    with pytest.raises(RuntimeError, match="libsitator_hip"):
        _lib_scattering.scattering(ctx, MOBILE, MOBILE, [[1, 0, 0]], [0], same=True)


def test_plan_function(stub, monkeypatch):
    monkeypatch.setattr(_lib, "_lib", stub)

    def effect(args):
        p = C.cast(args[11], C.POINTER(C.c_int64))
        for k in range(12):
            p[k] = 100 + k
    stub.effects["sit_scattering_plan"] = effect
    plan = _lib_scattering.scattering_plan(100, 3, 4, 20, [1, 2, 3], 2, origin_stride=3, self_part=False, workspace_bytes=1 << 20)
    assert list(plan) == _lib_scattering.PLAN_KEYS and list(plan.values()) == list(range(100, 112))
    args = stub.of("sit_scattering_plan")[0]
    assert args[:5] == (100, 3, 4, 0, 20) and list(args[5]._arr) == [1, 2, 3] and args[6:11] == (2, 3, 0, 1, 1 << 20)
    stub.rc["sit_scattering_plan"] = _lib.E_INVALID
    with pytest.raises(ValueError, match="scattering_plan"):
        _lib_scattering.scattering_plan(100, 3, 4, 20, [33, 0, 0], 2)
    with pytest.raises(ValueError, match="per axis"):
        _lib_scattering.scattering_plan(100, 3, 4, 20, [1, 2], 2)


@pytest.mark.parametrize("cap", [0, 1 << 22, 200000])
def test_plan_of_the_library_is_the_restatement(cap):
    """No GPU is needed for the plan: the library's answer is the restatement's."""
    built()
    for F_, n_a, n_b, same, n_q, H, n_lags, stride, sp, cp in ((100000, 64, 64, True, 257, [6, 6, 6], 59, 1, True, True),
                                                                (97, 5, 70, False, 300, [3, 4, 32], 4, 3, False, True),
                                                                (129, 130, 130, True, 40, [32, 32, 32], 3, 1, True, False)):
        exp = S.plan(F_, n_a, n_b, same, n_q, H, n_lags, stride, sp, cp, cap)
        if exp is None:
            with pytest.raises(ValueError):
                _lib_scattering.scattering_plan(F_, n_a, n_b, n_q, H, n_lags, stride, same, sp, cp, cap)
            continue
        plan = _lib_scattering.scattering_plan(F_, n_a, n_b, n_q, H, n_lags, stride, same, sp, cp, cap)
        assert (plan["threads"], plan["max_index"], plan["origins_per_block"], plan["lags_per_workgroup"]) == (S.THREADS, S.MAX_H, S.BLOCK, S.LAG_TILE)
        assert plan["tile_entries"] == exp["tile"] and plan["lds_bytes"] == exp["lds_bytes"] < 65536 and plan["n_blocks"] == exp["n_blocks"]
        assert (plan["q_batch"], plan["n_q_batches"], plan["window"], plan["lags_per_launch"], plan["workspace"]) == (
            exp["q_batch"], exp["n_q_batches"], exp["window"], exp["lags_per_launch"], exp["workspace"])
        assert plan["workspace"] <= (cap or S.DEFAULT_WORKSPACE)
    with pytest.raises(ValueError):
        _lib_scattering.scattering_plan(100, 3, 4, 10, [33, 0, 0], 1)
    with pytest.raises(ValueError):
        _lib_scattering.scattering_plan(100, 3, 4, 10, [1, 1, 1], 1, workspace_bytes=100)
