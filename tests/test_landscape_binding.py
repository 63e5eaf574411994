"""CPU-only: what tests/test_percolation_binding.py does for the fifth header, for the sixth one, include/sitator_hip_landscape.h, and
the table of ``sitator_amd/_lib_landscape.py``: the library exports the two symbols, table and header agree in names and arity, the
six tables are disjoint and the first five headers do not name the new symbols, and the module's calls go through a stub that
converts every argument with ``argtypes[i].from_param`` - the context is the stub context of tests/test_binding_calls.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sitator_amd import _lib, _lib_density, _lib_landscape, _lib_percolation, _lib_scattering, _lib_vanhove
from sitator_amd._lib import HipContext
from sitator_amd._lib_landscape import SIGNATURES
from tests import barrier_ref as BR
from tests import landscape_ref as LR
from tests.test_binding_calls import Stub, make_ctx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sit_landscape_energies", "sit_landscape_plan"]
EARLIER = ("sitator_hip.h", "sitator_hip_vanhove.h", "sitator_hip_scattering.h", "sitator_hip_density.h", "sitator_hip_percolation.h")
FURTHER_TABLES = (_lib_vanhove.SIGNATURES, _lib_scattering.SIGNATURES, _lib_density.SIGNATURES, _lib_percolation.SIGNATURES, SIGNATURES)


def header_text(name):
    return open(os.path.join(ROOT, "include", name)).read()


def header_declarations(name="sitator_hip_landscape.h"):
    """``{symbol: number of parameters}`` of a header."""
    text = re.sub(r"/\*.*?\*/", "", header_text(name), flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\b(sit_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


class LandscapeStub(Stub):
    """The stub of test_binding_calls.py with the symbols of the five further tables beside those of the first."""

    def __getattr__(self, name):
        table = next((t for t in FURTHER_TABLES if name in t), None)
        if table is None:
            return Stub.__getattr__(self, name)
        res, argtypes = table[name]

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
    return LandscapeStub()


@pytest.fixture
def ctx(stub):
    c = make_ctx(stub)
    yield c
    c._h = None


def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib_landscape.bind(_lib.load())


def test_library_exports_the_symbols_and_the_table_is_the_header():
    lib = built()
    decl = header_declarations()
    assert sorted(decl) == sorted(SIGNATURES) == NAMES
    for name, nparams in decl.items():
        fn = getattr(lib, name)
        assert len(SIGNATURES[name][1]) == nparams == len(fn.argtypes) and fn.restype is C.c_int, name
    assert (decl["sit_landscape_energies"], decl["sit_landscape_plan"]) == (10, 5)
    with open(_lib.LIB_PATH, "rb") as fh:                        # every name of the kind the library holds: exactly the two
        assert sorted(set(re.findall(rb"sit_landscape[a-z0-9_]*", fh.read()))) == [n.encode() for n in NAMES]


def test_the_six_tables_are_disjoint_and_the_first_five_headers_stay_as_they_are():
    tables = [set(_lib.SIGNATURES)] + [set(t) for t in FURTHER_TABLES]
    assert len(tables) == 6
    for i in range(6):
        for j in range(i):
            assert not tables[i] & tables[j]
    for name in ("landscape_energies", "landscape_plan", "energy_landscape"):
        assert not hasattr(HipContext, name)
    for earlier in EARLIER:
        assert "sit_landscape" not in header_text(earlier) and "sitator_hip_landscape" not in header_text(earlier)
    assert sorted(header_declarations("sitator_hip_percolation.h")) == ["sit_percolation_components", "sit_percolation_levels", "sit_percolation_plan"]
    sixth = header_text("sitator_hip_landscape.h")
    assert '#include "sitator_hip.h"' in sixth and "SIT_ABI_VERSION" not in sixth
    assert "#define SIT_ABI_VERSION %d" % _lib.ABI_VERSION in header_text("sitator_hip.h")


def test_energies_marshals_every_argument(stub, ctx):
    def effect(args):
        args[8]._arr[...] = 2.5
        args[9]._arr[:] = [2, 12, 3, 4000]
    stub.effects["sit_landscape_energies"] = effect
    pos = np.arange(15, dtype=np.float32).reshape(5, 3)            # converted, not handed on
    energies, info = _lib_landscape.landscape_energies(ctx, pos, np.full(5, 0.5), [1, 1, 1, 2, 2], 3.25, (4, 5, 6), form=2)
    (args,) = stub.of("sit_landscape_energies")
    assert stub.names() == ["sit_landscape_energies"]
    assert args[1]._arr.shape == (5, 3) and args[1]._arr.dtype == np.float64 and np.array_equal(args[1]._arr, pos)
    assert args[2]._arr.tolist() == [0.5] * 5 and args[3]._arr.tolist() == [1.0, 1.0, 1.0, 2.0, 2.0] and args[3]._arr.dtype == np.float64
    assert args[4:6] == (5, 3.25) and list(args[6]._arr) == [4, 5, 6] and args[6]._arr.dtype == np.int64 and args[7] == 2
    assert args[8]._arr is energies and energies.shape == (4, 5, 6) and energies.dtype == np.float64 and np.all(energies == 2.5)
    assert info == (2, 12, 3, 4000)
    _lib_landscape.landscape_energies(ctx, pos, np.full(5, 0.5), np.ones(5), 3.0, (1, 1, 1))
    assert stub.of("sit_landscape_energies")[-1][7] == 0
    n_calls = len(stub.calls)
    for bad in ((4, 5), (0, 5, 6), (4, 1025, 6), (1024, 1024, 129)):
        with pytest.raises(ValueError):
            _lib_landscape.landscape_energies(ctx, pos, np.full(5, 0.5), np.ones(5), 3.0, bad)
    with pytest.raises(ValueError, match="one epsilon"):
        _lib_landscape.landscape_energies(ctx, pos, np.full(4, 0.5), np.ones(5), 3.0, (4, 5, 6))
    assert len(stub.calls) == n_calls


def test_a_wrong_dtype_fails_in_from_param(stub, ctx):
    argtypes = SIGNATURES["sit_landscape_energies"][1]
    good_i, good_d = np.zeros(4, dtype=np.int64), np.zeros(4)
    argtypes[6].from_param(_lib._ptr(good_i))
    for k, bad in ((1, good_i), (2, np.zeros(3, dtype=np.int32)), (3, good_i), (6, good_d), (8, good_i), (9, good_d)):
        with pytest.raises((TypeError, C.ArgumentError)):
            argtypes[k].from_param(_lib._ptr(bad))
    with pytest.raises(AssertionError, match="argument 8"):
        stub.sit_landscape_energies(ctx._h, _lib._ptr(good_d), _lib._ptr(good_d), _lib._ptr(good_d), 1, 3.0, _lib._ptr(good_i), 0,
                                    _lib._ptr(good_i), _lib._ptr(good_i))
    with pytest.raises(AssertionError, match="arguments"):
        stub.sit_landscape_plan(_lib._ptr(good_d))
    assert stub.calls == []


def test_status_codes_become_exceptions(stub, ctx):
    call = lambda: _lib_landscape.landscape_energies(ctx, np.zeros((1, 3)), [1.0], [1.0], 3.0, (2, 2, 2))      # noqa: E731
    stub.message = b"sit_landscape_energies: form is 0, 1 or 2"
    stub.rc["sit_landscape_energies"] = _lib.E_INVALID
    with pytest.raises(ValueError, match="0, 1 or 2"):
        call()
    stub.rc["sit_landscape_energies"] = _lib.E_HIP
    with pytest.raises(RuntimeError, match="libsitator_hip"):
        call()
    stub.rc["sit_landscape_energies"] = _lib.E_CAPACITY
    with pytest.raises(RuntimeError):
        call()


def test_plan_function(stub, monkeypatch):
    monkeypatch.setattr(_lib, "_lib", stub)

    def effect(args):
        p = C.cast(args[4], C.POINTER(C.c_int64))
        for k in range(16):
            p[k] = 100 + k
    stub.effects["sit_landscape_plan"] = effect
    plan = _lib_landscape.landscape_plan(BR.TRICLINIC, 3.5, (5, 6, 7), form=2)
    assert len(_lib_landscape.PLAN_KEYS) == 16
    assert plan["translations"] == (108, 109, 110) and plan["list_translations"] == (111, 112, 113)
    assert [plan[k] for k in ("tile0", "tile1", "tile2", "threads", "lds_bytes", "list_capacity", "tiles", "form", "voxels", "atom_tile")] \
        == [100, 101, 102, 103, 104, 105, 106, 107, 114, 115]
    args = stub.of("sit_landscape_plan")[0]
    assert args[0]._arr.shape == (3, 3) and np.array_equal(args[0]._arr, BR.TRICLINIC) and args[1] == 3.5
    assert list(args[2]._arr) == [5, 6, 7] and args[3] == 2
    stub.rc["sit_landscape_plan"] = _lib.E_INVALID
    with pytest.raises(ValueError, match="landscape_plan"):
        _lib_landscape.landscape_plan(BR.TRICLINIC, 3.5, (0, 6, 7))
    with pytest.raises(ValueError, match="per axis"):
        _lib_landscape.landscape_plan(BR.TRICLINIC, 3.5, (5, 6))


def test_plan_of_the_library_is_the_restatement():
    """No GPU is needed for the plan: the library's answer is the restatement's."""
    built()
    assert _lib_landscape.landscape_plan(BR.CUBIC, 3.0, (4, 4, 4))["form"] == 2 and _lib_landscape.landscape_plan(BR.CUBIC, 13.0, (4, 4, 4))["form"] == 1
    for cell in (BR.CUBIC, BR.TRICLINIC, BR.SMALL_TRICLINIC):
        for n in ((1, 1, 1), (2, 3, 5), (17, 16, 33), (8, 16, 16), (1024, 1024, 128)):
            for rcf in (0.4, 2.2):
                for form in (0, 1, 2):
                    rc = rcf * BR.heights(cell).min()
                    exp = LR.plan(cell, rc, n, form)
                    plan = _lib_landscape.landscape_plan(cell, rc, n, form)
                    assert (plan["tile0"], plan["tile1"], plan["tile2"]) == exp["tile"] and plan["threads"] == exp["threads"]
                    assert {k: plan[k] for k in ("list_capacity", "tiles", "form", "translations", "list_translations", "voxels")} \
                        == {k: exp[k] for k in ("list_capacity", "tiles", "form", "translations", "list_translations", "voxels")}
                    assert plan["lds_bytes"] == (32288 if plan["form"] == 2 else 36864) and 4 * plan["lds_bytes"] <= 160 * 1024
                    assert plan["atom_tile"] == 512
    for bad in (dict(grid=(1025, 1, 1)), dict(grid=(0, 1, 1)), dict(grid=(1024, 1024, 129)), dict(grid=(4, 4, 4), form=3),
                dict(grid=(4, 4, 4), rc=0.0), dict(grid=(4, 4, 4), rc=256 * 12.0), dict(grid=(4, 4, 4), cell=np.ones((3, 3)))):
        kw = dict(cell=BR.CUBIC, rc=3.0, form=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            _lib_landscape.landscape_plan(**kw)
        assert LR.plan(kw["cell"], kw["rc"], kw["grid"], kw["form"]) is None
