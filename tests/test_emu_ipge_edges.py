"""The column update at every edge of its width classes, with built operands (tests/ipge_edge_helpers.py), on the CPU emulation
of the kernel source: every case against oracle_lib.factorize bit for bit and against a dense fraction-free elimination in
Python integers, and every case's intent -- the class its update lands in -- against the plan restated in Python.

Cost on the emulator (one run, 8 CPUs): the 75 cases on libslip_emu.so 219 s, Families A and C through the helpers 143 s,
Family A in weak-store mode 129 s, the solves 5 s; 19 s the slowest case (register class 4).  tests/test_emu_raw_fill.py:
17 tests, 144 s, 24 s the slowest."""
import pytest

import ipge_edge_helpers as H
from test_emu_raw_fill import emu_farm_lib, emu_lib      # noqa: F401  (fixtures)

ALL = H.cases_of("ABCD")


@pytest.mark.parametrize("case", ALL)
def test_ipge_edge_intent(case):
    """the labelled updates and history items land in the classes the case names (no kernel runs here)"""
    H.check_intent(case)


def test_ipge_edge_case_list_covers_every_class():
    """every family reaches the lane, the four register classes and the memory path where the issue asks for them"""
    every = {"lane", "reg1", "reg2", "reg3", "reg4", "mem"}
    assert set(H.family_a()) == every and set(H.family_b()) == every
    assert set(H.family_c()) == {"lane", "reg2", "reg3", "reg4", "mem"}      # W2 one past each edge
    for cls in ("reg1", "reg2", "reg3", "reg4", "mem"):                      # both branches of wr_shr / wb_copy_shr
        z = [H.ctz(c.cols[0][0]) for c in H.family_b()[cls]]
        assert any(0 < v < 32 for v in z) and any(v >= 32 for v in z), (cls, z)


@pytest.mark.parametrize("case", ALL)
def test_ipge_edges(emu_lib, case):
    H.check_case(emu_lib, case, 2, 5 if case.n > 9 else 4, 1 + case.n % 3)


@pytest.mark.parametrize("case", H.cases_of("AC"))
def test_ipge_edges_through_helpers(emu_farm_lib, case):
    """the build that opens every queue of two or more items: helpers execute the wave items"""
    info = H.check_case(emu_farm_lib, case, 2, 6, 1)["info"]
    assert case.one_limb or info["farm_jobs"] > 0


@pytest.mark.parametrize("case", H.cases_of("A"))
def test_ipge_edges_in_weak_store_mode(emu_farm_lib, case):
    """the same hand-off under delayed, reordered write-through stores"""
    H.check_case(emu_farm_lib, case, 2, 6, 11, weak=1)


@pytest.mark.parametrize("name", H.E_CASES[:2])
def test_ipge_edges_in_the_solve(emu_lib, name):
    """Family E: the forward substitution is the same sweep; numerators against Fraction arithmetic"""
    case = H.case_named("B", name)
    H.solve_check(emu_lib, case, H.edge_rhs(case, 2), 2, 3, 2)
