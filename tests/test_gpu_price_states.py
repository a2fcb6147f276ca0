"""Pricing with nonbasic states and reference weights on the MI355X (slip_hip_factor_price_states, slip_hip_price_select),
against Python fractions on the true values: the launch geometry, every degenerate outcome, a handle with a negative
determinant, the existing calls it must agree with, every width class of the squares (de080285 is the natural wide case),
the grouping of both staging slabs, the lifecycle of a handle, every rejected input and the ABI."""
import pytest

from price_states_helpers import (check_abi, check_against_price, check_degenerate, check_geometry, check_groups, check_lifecycle,
                                  check_natural_wide, check_negative_det, check_rejections, check_width_classes)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ncols", [1, 63, 64, 65, 130])
def test_gpu_price_states_geometry(ncols):
    check_geometry(None, (ncols,))


def test_gpu_price_states_degenerate_outcomes():
    check_degenerate(None)


def test_gpu_price_states_negative_determinant():
    assert check_negative_det(None) < 0


def test_gpu_price_states_against_price():
    check_against_price(None)


def test_gpu_price_states_width_classes():
    check_width_classes(None)


def test_gpu_price_states_natural_wide_case():
    check_natural_wide(None)


def test_gpu_price_states_groups(monkeypatch):
    check_groups(None, monkeypatch)


def test_gpu_price_states_lifecycle():
    check_lifecycle(None)


def test_gpu_price_states_rejects_bad_input():
    check_rejections(None)


def test_gpu_price_states_abi():
    from slip_lu_amd import _lib
    lib = _lib.load()
    for name in check_abi():
        getattr(lib, name)
