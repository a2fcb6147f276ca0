"""slip_lu_amd -- MI355X-native REF sparse LU hot path behind the SLIP_LU C API.

The product is the HIP library (csrc/libslip_hip.so, C ABI in include/slip_hip.h)
and the GMP-typed drop-in shim (csrc/libslip_lu_hip.so); this package is the thin
ctypes layer the tests and bench.py use.
"""
from . import api  # noqa: F401
from .api import (BoundedStepResult, Bounds, Entering, Factorization, SlipError, SparseMatrix, bound_paths, bound_test,  # noqa: F401
                  check_solution, factorize, step_bounded, step_bounded_ms, step_bounded_paths,
                  ints_to_slab, matgen, multiply_passes, pivot_update, pivot_update_paths, price_select, price_select_paths,
                  ratio_test, ratio_test_bounded, ratio_test_paths, read_triplet, solution_to_double, solution_to_mpfr, solution_to_mpfr_paths,
                  solution_to_rational, solution_to_rational_paths, write_triplet)
