"""The exact sparse products on the MI355X (slip_hip_factor_multiply, slip_hip_matrix_*), against Python integers: the
synthetic corpus on both sides of every width class with the memory path in every vector, handles on complete goldens
(de080285 reaches the memory path on real data), the lifecycle of a handle and every rejected input."""
import pytest

from product_helpers import check_corpus, check_golden, check_groups, check_lifecycle, check_rejections, check_thin

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wide_everywhere", [False, True])
def test_gpu_product_corpus(wide_everywhere):
    check_corpus(None, wide_everywhere)


def test_gpu_product_in_groups(monkeypatch):
    check_groups(None, monkeypatch)


def test_gpu_product_thin_matrices():
    check_thin(None)


@pytest.mark.parametrize("name", ["test_mat", "gen_n40", "10teams", "prob159", "de080285"])
def test_gpu_product_on_handles(name):
    check_golden(None, name, memory_path=name == "de080285")


def test_gpu_product_lifecycle():
    check_lifecycle(None)


def test_gpu_product_rejects_bad_input():
    check_rejections(None)
