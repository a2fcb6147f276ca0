"""Exact pricing on the MI355X (slip_hip_factor_price), against Python fractions and against the three-call route
(solve_transpose + multiply + ratio_test) on the same operands: the launch geometry, the shapes of M, every width class of the
product (de080285 is the natural wide case), handles on complete goldens under every combination of nside, sense and key, a
handle with a negative determinant, the grouping of the staging slab, the lifecycle of a handle and every rejected input."""
import pytest

from price_helpers import (check_geometry, check_golden, check_groups, check_lifecycle, check_natural_wide, check_rejections,
                           check_shapes, check_width_classes)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ncols", [1, 63, 64, 65, 130])
def test_gpu_price_geometry(ncols):
    check_geometry(None, (ncols,))


def test_gpu_price_shapes_of_m():
    check_shapes(None)


def test_gpu_price_width_classes():
    check_width_classes(None, 50)


def test_gpu_price_natural_wide_case():
    check_natural_wide(None)


@pytest.mark.parametrize("name", ["test_mat", "gen_n40", "10teams", "prob159"])
def test_gpu_price_on_handles(name):
    check_golden(None, name)


def test_gpu_price_negative_determinant():
    assert check_golden(None, "gen_n40", negative=True) < 0


def test_gpu_price_groups(monkeypatch):
    check_groups(None, monkeypatch)


def test_gpu_price_lifecycle():
    check_lifecycle(None)


def test_gpu_price_rejects_bad_input():
    check_rejections(None)
