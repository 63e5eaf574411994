"""CPU-only: what the SOAP operators (sitator_amd/site_descriptors.py) decide before anything reaches the GPU - the reference's
constructor checks and ``_make_structure`` (SOAP.py:45-142, :215-245), the backend rule, the tables handed to the device."""
import math

import numpy as np
import pytest

from tests import soap_ref as SR


def network(numbers=(3, 3, 8, 8, 15, 8)):
    from sitator_amd import SiteNetwork, Structure
    numbers = np.array(numbers)
    mobile = numbers == 3
    pos = np.random.default_rng(1).uniform(0.0, 6.0, (len(numbers), 3))
    sn = SiteNetwork(Structure(pos, np.eye(3) * 6.0, numbers), ~mobile, mobile)
    sn.centers = pos[mobile] + 0.1
    return sn


def test_names_are_exported():
    import sitator_amd
    for name in ("SOAP", "SOAPCenters", "SOAPSampledCenters", "SOAPDescriptorAverages", "device_soap_backend", "GenerateAroundSites"):
        assert hasattr(sitator_amd, name)
    from sitator_amd.misc import GenerateAroundSites  # noqa: F401


def test_a_foreign_backend_is_a_type_error():
    from sitator_amd import SOAPCenters, SOAPDescriptorAverages, device_soap_backend
    for backend in (lambda sn, mask, tracer, env: None, "dscribe", object()):
        with pytest.raises(TypeError, match="QUIP and DScribe"):
            SOAPCenters(3, backend=backend)
    with pytest.raises(TypeError, match="QUIP and DScribe"):
        SOAPDescriptorAverages(3, averaging=2, backend=print)
    SOAPCenters(3, backend=device_soap_backend({"l_max": 2}))
    with pytest.raises(ValueError, match="Unknown SOAP parameters"):
        device_soap_backend({"rbf": "gto"})


def test_make_structure_checks():
    from sitator_amd import SOAPCenters
    sn = network()
    structure, tracer, mask = SOAPCenters(None)._make_structure(sn)
    assert tracer == 3 and np.array_equal(mask, sn.static_mask) and len(structure) == 4
    with pytest.raises(ValueError, match="same species"):
        SOAPCenters(8)._make_structure(sn)                                   # the tracer among the statics
    with pytest.raises(ValueError, match="same species"):
        SOAPCenters(None)._make_structure(network_with_static_tracer())
    with pytest.raises(AssertionError, match="excluded all host atoms"):
        SOAPCenters(3, soap_mask=np.zeros(6, dtype=bool))._make_structure(sn)
    with pytest.raises(AssertionError, match="both static and mobile"):
        SOAPCenters(3, soap_mask=np.ones(6, dtype=bool))._make_structure(sn)
    with pytest.raises(AssertionError, match="excludes all host atoms"):
        SOAPCenters(3, environment=["Si"])._make_structure(sn)
    structure, _, mask = SOAPCenters(3, soap_mask=("P", "O"))._make_structure(sn)
    assert np.array_equal(mask, sn.static_mask)
    structure, _, mask = SOAPCenters(3, soap_mask=("P",))._make_structure(sn)
    assert mask.sum() == 1 and structure.get_atomic_numbers().tolist() == [15]


def network_with_static_tracer():
    """A static atom of the mobile species: the default tracer (the first mobile atom's number) is among the statics."""
    from sitator_amd import SiteNetwork, Structure
    numbers = np.array([3, 3, 8, 8])
    mobile = np.array([True, False, False, False])
    return SiteNetwork(Structure(np.zeros((4, 3)), np.eye(3) * 6.0, numbers), ~mobile, mobile)


def test_environment_as_numbers_or_symbols():
    from sitator_amd import SOAPCenters
    from sitator_amd.site_descriptors import CHEMICAL_SYMBOLS, atomic_numbers
    assert len(CHEMICAL_SYMBOLS) == 118 and atomic_numbers["H"] == 1 and atomic_numbers["Li"] == 3 and atomic_numbers["Og"] == 118
    assert atomic_numbers["O"] == 8 and atomic_numbers["P"] == 15 and atomic_numbers["Fe"] == 26 and atomic_numbers["U"] == 92
    assert SOAPCenters(3, environment=["C", 8, "O"])._environment == [6, 8, 8]
    assert SOAPCenters(3, environment=(15,))._environment == [15]
    with pytest.raises(KeyError):
        SOAPCenters(3, environment=["Xx"])
    with pytest.raises(TypeError):
        SOAPCenters(3, environment="O")
    with pytest.raises(TypeError):
        SOAPCenters(3, environment=[8.0])
    with pytest.raises(AssertionError):
        SOAPCenters(3, environment=[119])


def test_descriptor_averages_constructor():
    from sitator_amd import SOAPDescriptorAverages
    with pytest.raises(RuntimeError):
        SOAPDescriptorAverages(3)
    with pytest.raises(AssertionError):
        SOAPDescriptorAverages(3, averaging=2, avg_descriptors_per_site=2)
    with pytest.raises(TypeError):
        SOAPDescriptorAverages(3, averaging=2.0)
    with pytest.raises(ValueError):
        SOAPDescriptorAverages(3, averaging=2, stepsize=0)
    op = SOAPDescriptorAverages(3, avg_descriptors_per_site=4, stepsize=3)
    assert op._averaging is None and op._avg_desc_per_site == 4 and op._stepsize == 3


def test_the_tables_handed_to_the_device():
    from sitator_amd.site_descriptors import soap_tables
    for Z, kw in ((1, {}), (3, {"crossover": True}), (2, {"l_max": 0, "n_max": 1}), (4, {"l_max": 8, "n_max": 8, "cutoff": 4.5})):
        soap = soap_tables(Z, kw)
        alpha, beta = SR.radial_tables(soap["cutoff"], soap["n_max"], soap["l_max"])
        assert np.allclose(soap["alpha"], alpha, rtol=1e-14, atol=0) and np.allclose(soap["beta"], beta, rtol=1e-9, atol=1e-9 * np.abs(beta).max())
        assert soap["n_dim"] == len(SR.feature_table(Z, soap["n_max"], soap["l_max"], soap["crossover"]))
        for l in range(soap["l_max"] + 1):                           # beta is the inverse root of the overlap: beta S beta = 1
            S = 0.5 * math.gamma(l + 1.5) * (alpha[l][:, None] + alpha[l][None, :]) ** -(l + 1.5)
            assert np.allclose(soap["beta"][l] @ S @ soap["beta"][l], np.eye(soap["n_max"]), atol=1e-6)
    assert soap_tables(1)["n_dim"] == 147 and soap_tables(1)["cutoff_transition_width"] == 0.0
