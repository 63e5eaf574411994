"""CPU-only: what tests/test_abi.py and tests/test_binding_calls.py do for include/sitator_hip.h and ``_lib.SIGNATURES``, for the
second header include/sitator_hip_vanhove.h and the table of ``sitator_amd/_lib_vanhove.py``: the library exports both symbols,
table and header agree in names and arity, and the module's calls go through a stub that converts every argument with
``argtypes[i].from_param`` - the context is the stub context of tests/test_binding_calls.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sitator_amd import _lib, _lib_vanhove
from sitator_amd._lib import HipContext
from sitator_amd._lib_vanhove import SIGNATURES
from tests.test_binding_calls import Stub, make_ctx, F, A, MOBILE, f

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_declarations():
    """``{symbol: number of parameters}`` of include/sitator_hip_vanhove.h."""
    text = open(os.path.join(ROOT, "include", "sitator_hip_vanhove.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\b(sit_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


class VanHoveStub(Stub):
    """The stub of test_binding_calls.py with the two symbols of the second table beside those of the first."""

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
    return VanHoveStub()


@pytest.fixture
def ctx(stub):
    c = make_ctx(stub)
    yield c
    c._h = None


def test_library_exports_both_symbols_and_the_table_is_the_header():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib_vanhove.bind(_lib.load())
    decl = header_declarations()
    assert sorted(decl) == sorted(SIGNATURES) == ["sit_vanhove", "sit_vanhove_plan"]
    for name, nparams in decl.items():
        fn = getattr(lib, name)
        assert len(SIGNATURES[name][1]) == nparams == len(fn.argtypes) and fn.restype is C.c_int, name


def test_the_first_table_and_the_context_stay_as_they_are():
    assert not set(SIGNATURES) & set(_lib.SIGNATURES)
    assert not hasattr(HipContext, "vanhove") and not hasattr(HipContext, "vanhove_plan")
    header = open(os.path.join(ROOT, "include", "sitator_hip.h")).read()
    assert "sit_vanhove" not in header
    second = open(os.path.join(ROOT, "include", "sitator_hip_vanhove.h")).read()
    assert '#include "sitator_hip.h"' in second and "SIT_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", second, flags=re.S)


def test_the_call_marshals_every_argument(stub, ctx):
    ctx._deferred, ctx.labels_version, ctx.labels_digest = 1, 5, (5, "digest")
    stub.effects["sit_vanhove"] = lambda args: setattr(args[18]._obj, "value", 0.125)
    sc, dc, res = _lib_vanhove.vanhove(ctx, MOBILE, [0, 1, 2], [0, 1, 4], 2.5, 8, origin_stride=2, workspace_bytes=4096)
    (args,) = stub.of("sit_vanhove")
    assert stub.names() == ["sit_vanhove"]                        # no deferred pass is collected
    assert (ctx._deferred, ctx.labels_version, ctx.labels_digest) == (1, 5, (5, "digest"))
    assert args[1] is None and (args[2], args[3]) == (F, A)       # the resident frames
    assert list(args[4]._arr) == MOBILE and args[5] == 2 and list(args[6]._arr) == [0, 1, 2] and args[7] == 3 and args[8] == 0
    assert list(args[9]._arr) == [0, 1, 4] and args[10:16] == (3, 2, 2.5, 8, 1, 4096)
    assert args[16]._arr is sc and args[17]._arr is dc and sc.shape == dc.shape == (3, 9) and sc.dtype == dc.dtype == np.uint64
    assert res == 0.125
    # a host array, one selection, a part left out
    pos = f(F, 3, 3)
    sc, dc, _ = _lib_vanhove.vanhove(ctx, [0, 1, 2], [0, 1, 2], [0], 1.0, 4, positions=pos, same=True, unwrap=False, self_part=False)
    args = stub.of("sit_vanhove")[-1]
    assert args[1]._arr.shape == (F, 3, 3) and (args[2], args[3], args[8], args[14]) == (F, 3, 1, 0)
    assert sc is None and args[16] is None and args[17]._arr is dc
    sc, dc, _ = _lib_vanhove.vanhove(ctx, [0], [1], [0], 1.0, 4, distinct_part=False)
    assert dc is None and stub.of("sit_vanhove")[-1][17] is None and sc.shape == (1, 5)


def test_a_wrong_dtype_fails_in_from_param(stub, ctx):
    argtypes = SIGNATURES["sit_vanhove"][1]
    good = np.zeros(3, dtype=np.int64)
    argtypes[4].from_param(_lib._ptr(good))
    for k, bad in ((4, np.zeros(3)), (1, np.zeros(3, dtype=np.int64)), (16, np.zeros(3, dtype=np.int64)), (18, np.zeros(3, dtype=np.float32).view(np.int32))):
        with pytest.raises((TypeError, C.ArgumentError)):
            argtypes[k].from_param(_lib._ptr(bad))
    with pytest.raises(AssertionError, match="argument 4"):       # and the stub says which argument
        stub.sit_vanhove(*([ctx._h, None, F, A, _lib._ptr(np.zeros(2)), 2, _lib._ptr(good), 3, 0, _lib._ptr(good), 3, 1, 1.0, 4, 1, 0,
                            None, None, None]))
    with pytest.raises(AssertionError, match="arguments"):
        stub.sit_vanhove(ctx._h)
    assert stub.calls == []


def test_status_codes_become_exceptions(stub, ctx):
    stub.message = b"sit_vanhove: r_max is outside"
    stub.rc["sit_vanhove"] = _lib.E_INVALID
    with pytest.raises(ValueError, match="r_max is outside"):
        _lib_vanhove.vanhove(ctx, MOBILE, MOBILE, [0], 1.0, 4, same=True)
    stub.rc["sit_vanhove"] = _lib.E_HIP
    with pytest.raises(RuntimeError, match="libsitator_hip"):
        _lib_vanhove.vanhove(ctx, MOBILE, MOBILE, [0], 1.0, 4, same=True)


def test_plan_function(stub, monkeypatch):
    monkeypatch.setattr(_lib, "_lib", stub)

    def effect(args):
        p = C.cast(args[10], C.POINTER(C.c_int64))
        for k in range(12):
            p[k] = 100 + k
    stub.effects["sit_vanhove_plan"] = effect
    plan = _lib_vanhove.vanhove_plan(100, 3, 4, 2, 16, origin_stride=3, unwrap=False, workspace_bytes=1 << 20)
    assert list(plan) == _lib_vanhove.PLAN_KEYS and list(plan.values()) == list(range(100, 112))
    assert stub.of("sit_vanhove_plan")[0][:10] == (100, 3, 4, 2, 16, 3, 1, 1, 0, 1 << 20)
    stub.rc["sit_vanhove_plan"] = _lib.E_INVALID
    with pytest.raises(ValueError, match="vanhove_plan"):
        _lib_vanhove.vanhove_plan(100, 3, 4, 2, 5000)


def test_plan_of_the_library():
    """No GPU is needed for the plan: the library's answer is the restatement's."""
    from tests import vanhove_ref as V
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    plan = _lib_vanhove.vanhove_plan(100000, 64, 512, 64, 300)
    run, span, tiles, pairs = V.split(64, 512)
    assert (plan["threads"], plan["max_bins"], plan["max_atoms"]) == (V.THREADS, V.MAX_BINS, V.MAX_ATOMS)
    assert (plan["origins_per_workgroup"], plan["b_span"], plan["b_tiles"], plan["pairs_per_workgroup"]) == (run, span, tiles, pairs)
    assert plan["window"] == V.window(100000, 64, 512, 1 << 30) < 100000 and plan["lds_bytes"] == V.lds_bytes(300, 1) < 65536
    assert plan["self_batch"] == 64 and plan["self_origins_per_workgroup"] == V.SELF_RUN
    with pytest.raises(ValueError):
        _lib_vanhove.vanhove_plan(100000, 64, 512, 64, 4096)
    with pytest.raises(ValueError):
        _lib_vanhove.vanhove_plan(100, 3, 4, 1, 16, workspace_bytes=100)
