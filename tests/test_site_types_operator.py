"""CPU-only: what ``SiteTypeAnalysis`` decides before it touches the GPU - its constructor's signature, the inputs it refuses -
and the surface of the binding (the run itself is tests/test_gpu_site_types.py)."""
import inspect

import numpy as np
import pytest


def network(K):
    from sitator_amd import SiteNetwork, Structure
    rng = np.random.default_rng(0)
    mobile = np.zeros(K + 4, dtype=bool)
    mobile[:2] = True
    sn = SiteNetwork(Structure(rng.uniform(0.0, 7.0, size=(K + 4, 3)), np.eye(3) * 7.0, np.where(mobile, 3, 8)), ~mobile, mobile)
    sn.centers = rng.uniform(0.0, 7.0, size=(K, 3))
    return sn


class Never(object):
    def get_descriptors(self, stn, **kwargs):
        raise AssertionError("the descriptor must not be asked")


def test_constructor_has_the_reference_signature():
    from sitator_amd import SiteTypeAnalysis
    sig = inspect.signature(SiteTypeAnalysis.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[2:]] == [
        ("min_pca_variance", 0.9), ("min_pca_dimensions", 2), ("n_site_types_max", 20)]
    op = SiteTypeAnalysis(Never())
    assert op._n_dvecs is None and op.n_site_types_max == 20


def test_refused_inputs():
    from sitator_amd import SiteTrajectory, SiteTypeAnalysis

    class Comm(object):
        size, rank = 2, 0

    st = SiteTrajectory(network(3), np.zeros((3, 2), dtype=np.int64))
    st._comm = Comm()
    with pytest.raises(NotImplementedError, match="frame shard"):
        SiteTypeAnalysis(Never()).run(st)
    with pytest.raises(RuntimeError, match="Input"):
        SiteTypeAnalysis(Never()).run("neither a network nor a trajectory")


def test_plan_needs_no_gpu():
    from sitator_amd import _lib
    pl = _lib.dpc_plan(2)
    assert pl["threads"] == pl["tile"] and pl["digit_bits"] * pl["passes"] == 64 and pl["max_d"] == 32
    assert pl["lds_bytes"] == pl["tile"] * 2 * 8 + 2048 and _lib.dpc_plan(3)["lds_bytes"] == pl["tile"] * 4 * 8 + 2048
    with pytest.raises(RuntimeError):
        _lib.dpc_plan(33)
    with pytest.raises(ValueError):
        _lib.dpc_plan(0)
