"""GPU: the tables of tests/probe_cases.py through the probe library with where = 1: the device compile of the csrc inline
functions (the inline-asm v_mad_u64_u32 products and the asm doubling of at2v_fu_gen.h, the reciprocal estimate of
lehmer_round32), one lane per case in 256-thread blocks, every batch ending in a partial wave. The expected values are
Python integers (tests/probe_ref.py); tests/test_probe_host.py runs the same tables through the host compile. One test
per probe group, parametrised by function: a failure names the function, the class or site, and the first failing
case's limbs. The probe is a separate compilation of the same inline functions; the verdict tests remain the check of
the kernels as compiled."""
import pytest

import probe_cases as pc
import probe_lib

pytestmark = pytest.mark.gpu
DEVICE = probe_lib.DEVICE


@pytest.mark.parametrize("name", pc.PRODUCTS)
def test_field_products(name):
    assert pc.check_product(DEVICE, name) > 2048


@pytest.mark.parametrize("name", pc.UTILS)
def test_field_utilities(name):
    assert pc.check_util(DEVICE, name) > 2048


@pytest.mark.parametrize("name", pc.POWERS)
def test_field_powers(name):
    assert pc.check_power(DEVICE, name) >= 2 * 517


@pytest.mark.parametrize("name", pc.GROUP)
def test_group_law(name):
    assert pc.check_group(DEVICE, name) >= 2 * 274


@pytest.mark.parametrize("name", pc.DECODES)
def test_decode(name):
    assert pc.check_decode(DEVICE, name) >= 14 + 38 + 1024


@pytest.mark.parametrize("name", pc.SCALARS)
def test_scalars(name):
    """the lattice case also asserts the device's record equals the host compile's, word for word"""
    assert pc.check_scalar(DEVICE, name) > 2048
