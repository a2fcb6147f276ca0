"""ctypes loader for libslip_hip.so (the HIP product library).

The product path has no CPU fallback: if the in-tree HIP library is missing or
cannot be loaded this module raises.  The environment variable
SLIP_HIP_LIBRARY may point to another build of the SAME C ABI (the test-suite
uses it to load the CPU emulation build of the kernel source, tests/emu).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_SO = os.path.join(_HERE, "csrc", "libslip_hip.so")


class Options(C.Structure):
    _fields_ = [("pivot", C.c_int32), ("tol", C.c_double), ("limb_cap", C.c_int32),
                ("waves", C.c_int32), ("lnz_hint", C.c_int64), ("unz_hint", C.c_int64),
                ("workers", C.c_int32), ("reserved", C.c_int32)]


class BoundsRec(C.Structure):
    """slip_hip_bounds"""
    _fields_ = [("kind", C.c_void_p), ("lolen", C.c_void_p), ("lolimbs", C.c_void_p), ("lo_limbs", C.c_int64),
                ("hilen", C.c_void_p), ("hilimbs", C.c_void_p), ("hi_limbs", C.c_int64),
                ("bdlen", C.c_int32), ("bdlimbs", C.c_void_p)]


class EnteringRec(C.Structure):
    """slip_hip_entering"""
    _fields_ = [("finite", C.c_void_p), ("erlen", C.c_void_p), ("erlimbs", C.c_void_p), ("er_limbs", C.c_int64),
                ("evlen", C.c_void_p), ("evlimbs", C.c_void_p), ("ev_limbs", C.c_int64)]


class Info(C.Structure):
    _fields_ = [("n", C.c_int32), ("K", C.c_int32), ("status", C.c_int32), ("window_end", C.c_int32),
                ("lnz", C.c_int64), ("unz", C.c_int64), ("l_limbs", C.c_int64), ("u_limbs", C.c_int64),
                ("n_upd", C.c_int64), ("b_read", C.c_int64), ("b_write", C.c_int64), ("n_src", C.c_int64),
                ("l_streamed", C.c_int64), ("max_limbs", C.c_int64),
                ("kernel_ms", C.c_double), ("launches", C.c_int32), ("xcap_digits", C.c_int32),
                ("limb_macs", C.c_int64), ("workers", C.c_int32), ("waves", C.c_int32),
                ("lds_bytes", C.c_int32), ("short_commits", C.c_int32), ("committer_commits", C.c_int32), ("farm_jobs", C.c_int32), ("farm_items", C.c_int32), ("batch_commits", C.c_int32),
                ("engine_commits", C.c_int32), ("engine_sources", C.c_int32), ("retractions", C.c_int32), ("reexports", C.c_int32),
                ("raw_fills", C.c_int64)]


EXPORTS = ("slip_hip_default_options", "slip_hip_device_count", "slip_hip_factor_create",
           "slip_hip_factor_reset", "slip_hip_factor_run", "slip_hip_factor_info",
           "slip_hip_factor_download", "slip_hip_factor_destroy", "slip_hip_matgen",
           "slip_hip_free", "slip_hip_wave_op_test", "slip_hip_version",
           "slip_hip_factor_phase_cycles", "slip_hip_factor_solve", "slip_hip_factor_solve_ms",
           "slip_hip_factor_from_factors", "slip_hip_factor_rescale", "slip_hip_factor_set_prefix", "slip_hip_pool_release", "slip_hip_read_triplet", "slip_hip_write_triplet",
           "slip_hip_factor_check", "slip_hip_check_solution", "slip_hip_factor_check_ms",
           "slip_hip_factor_solve_transpose", "slip_hip_factor_check_transpose", "slip_hip_factor_solve_transpose_ms",
           "slip_hip_factor_solve_double", "slip_hip_solution_to_double", "slip_hip_factor_to_double_ms",
           "slip_hip_factor_to_double_slow",
           "slip_hip_factor_solve_rational", "slip_hip_solution_to_rational", "slip_hip_factor_to_rational_ms",
           "slip_hip_factor_to_rational_paths", "slip_hip_solution_to_rational_paths",
           "slip_hip_factor_solve_mpfr", "slip_hip_solution_to_mpfr", "slip_hip_factor_to_mpfr_ms",
           "slip_hip_factor_to_mpfr_paths", "slip_hip_solution_to_mpfr_paths",
           "slip_hip_factor_rewind", "slip_hip_factor_replace_column", "slip_hip_factor_a_storage",
           "slip_hip_factor_multiply", "slip_hip_factor_multiply_ms", "slip_hip_matrix_create", "slip_hip_matrix_multiply",
           "slip_hip_matrix_multiply_ms", "slip_hip_matrix_destroy", "slip_hip_multiply_passes",
           "slip_hip_ratio_test", "slip_hip_ratio_test_paths", "slip_hip_factor_ratio_test", "slip_hip_factor_ratio_test_ms",
           "slip_hip_factor_ratio_test_paths",
           "slip_hip_factor_price", "slip_hip_factor_price_ms", "slip_hip_factor_price_paths",
           "slip_hip_factor_ratio_test_bounded", "slip_hip_factor_bound_test", "slip_hip_ratio_test_bounded", "slip_hip_bound_test",
           "slip_hip_factor_bound_ms", "slip_hip_factor_bound_paths", "slip_hip_bound_paths",
           "slip_hip_factor_price_states", "slip_hip_price_select", "slip_hip_factor_price_states_ms",
           "slip_hip_factor_price_states_paths", "slip_hip_price_select_paths",
           "slip_hip_pivot_update", "slip_hip_factor_solve_update", "slip_hip_factor_step", "slip_hip_factor_update_ms",
           "slip_hip_factor_update_paths", "slip_hip_pivot_update_paths",
           "slip_hip_factor_step_bounded", "slip_hip_step_bounded", "slip_hip_factor_step_bounded_ms",
           "slip_hip_factor_step_bounded_paths", "slip_hip_step_bounded_ms", "slip_hip_step_bounded_paths")

_libs = {}


def library_path():
    return os.environ.get("SLIP_HIP_LIBRARY", DEFAULT_SO)


def load(path=None):
    """Load (once) and return the C library; raises OSError if it is missing."""
    path = path or library_path()
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise OSError(f"{path} not found: build the HIP extension first "
                      "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.slip_hip_default_options.argtypes = [C.POINTER(Options)]
    lib.slip_hip_default_options.restype = None
    lib.slip_hip_device_count.restype = C.c_int
    lib.slip_hip_factor_create.argtypes = [C.POINTER(vp), C.c_int32, vp, vp, vp, vp, vp, C.POINTER(Options)]
    lib.slip_hip_factor_create.restype = C.c_int
    lib.slip_hip_factor_reset.argtypes = [vp]
    lib.slip_hip_factor_run.argtypes = [vp, C.c_int32, vp]
    lib.slip_hip_factor_info.argtypes = [vp, C.POINTER(Info)]
    lib.slip_hip_factor_download.argtypes = ([vp] + [vp] * 4 + [C.POINTER(C.c_int64)] + [vp] * 4 + [C.POINTER(C.c_int64)]
                                             + [vp] * 2 + [C.POINTER(C.c_int64), vp])
    lib.slip_hip_factor_destroy.argtypes = [vp]
    lib.slip_hip_factor_destroy.restype = None
    lib.slip_hip_matgen.argtypes = [C.c_int32, C.c_double, C.c_int32, C.c_uint64,
                                    C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.slip_hip_read_triplet.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)]
    lib.slip_hip_write_triplet.argtypes = [C.c_char_p, C.c_int32, vp, vp, vp, vp]
    lib.slip_hip_free.argtypes = [vp]
    lib.slip_hip_free.restype = None
    lib.slip_hip_wave_op_test.argtypes = [C.c_int32] * 5 + [vp, vp, vp]
    lib.slip_hip_version.restype = C.c_char_p
    lib.slip_hip_factor_solve.argtypes = [vp, C.c_int32, vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64), vp]
    lib.slip_hip_factor_solve.restype = C.c_int
    lib.slip_hip_factor_from_factors.argtypes = [C.POINTER(vp), C.c_int32] + [vp] * 9 + [C.POINTER(Options)]
    lib.slip_hip_factor_from_factors.restype = C.c_int
    lib.slip_hip_factor_rescale.argtypes = [vp, C.c_int32, vp, vp, vp]
    lib.slip_hip_factor_rescale.restype = C.c_int
    lib.slip_hip_factor_set_prefix.argtypes = [vp, C.c_int32] + [vp] * 9
    lib.slip_hip_factor_set_prefix.restype = C.c_int
    lib.slip_hip_factor_solve_ms.argtypes = [vp]
    lib.slip_hip_factor_solve_ms.restype = C.c_double
    i64 = C.c_int64
    lib.slip_hip_factor_check.argtypes = [vp, C.c_int32, vp, vp, i64, vp, vp, i64, vp, vp, vp]
    lib.slip_hip_factor_check.restype = C.c_int
    lib.slip_hip_check_solution.argtypes = [C.c_int32, vp, vp, vp, vp, C.c_int32, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp]
    lib.slip_hip_check_solution.restype = C.c_int
    lib.slip_hip_factor_check_ms.argtypes = [vp]
    lib.slip_hip_factor_check_ms.restype = C.c_double
    lib.slip_hip_factor_solve_transpose.argtypes = lib.slip_hip_factor_solve.argtypes
    lib.slip_hip_factor_solve_transpose.restype = C.c_int
    lib.slip_hip_factor_check_transpose.argtypes = lib.slip_hip_factor_check.argtypes
    lib.slip_hip_factor_check_transpose.restype = C.c_int
    lib.slip_hip_factor_solve_transpose_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.slip_hip_factor_solve_transpose_ms.restype = C.c_double
    lib.slip_hip_factor_solve_double.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, vp, vp, vp]
    lib.slip_hip_factor_solve_double.restype = C.c_int
    lib.slip_hip_solution_to_double.argtypes = [C.c_int32, C.c_int32, vp, vp, i64, vp, vp, i64, vp, vp]
    lib.slip_hip_solution_to_double.restype = C.c_int
    lib.slip_hip_factor_to_double_ms.argtypes = [vp]
    lib.slip_hip_factor_to_double_ms.restype = C.c_double
    lib.slip_hip_factor_to_double_slow.argtypes = [vp]
    lib.slip_hip_factor_to_double_slow.restype = C.c_int64
    slabs = [C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)] * 2
    lib.slip_hip_factor_solve_rational.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, vp] + slabs + [vp]
    lib.slip_hip_factor_solve_rational.restype = C.c_int
    lib.slip_hip_solution_to_rational.argtypes = [C.c_int32, C.c_int32, vp, vp, i64, vp, vp, i64] + slabs + [vp]
    lib.slip_hip_solution_to_rational.restype = C.c_int
    lib.slip_hip_factor_to_rational_ms.argtypes = [vp]
    lib.slip_hip_factor_to_rational_ms.restype = C.c_double
    lib.slip_hip_factor_to_rational_paths.argtypes = [vp, vp]
    lib.slip_hip_factor_to_rational_paths.restype = C.c_int
    lib.slip_hip_solution_to_rational_paths.argtypes = [vp]
    lib.slip_hip_solution_to_rational_paths.restype = C.c_int
    lib.slip_hip_factor_solve_mpfr.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, vp,
                                               C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
    lib.slip_hip_factor_solve_mpfr.restype = C.c_int
    lib.slip_hip_solution_to_mpfr.argtypes = [C.c_int32, C.c_int32, vp, vp, i64, vp, vp, i64, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
    lib.slip_hip_solution_to_mpfr.restype = C.c_int
    lib.slip_hip_factor_to_mpfr_ms.argtypes = [vp]
    lib.slip_hip_factor_to_mpfr_ms.restype = C.c_double
    lib.slip_hip_factor_to_mpfr_paths.argtypes = [vp, vp]
    lib.slip_hip_factor_to_mpfr_paths.restype = C.c_int
    lib.slip_hip_solution_to_mpfr_paths.argtypes = [vp]
    lib.slip_hip_solution_to_mpfr_paths.restype = C.c_int
    lib.slip_hip_factor_rewind.argtypes = [vp, C.c_int32, vp, vp]
    lib.slip_hip_factor_rewind.restype = C.c_int
    lib.slip_hip_factor_replace_column.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, i64, vp]
    lib.slip_hip_factor_replace_column.restype = C.c_int
    lib.slip_hip_factor_a_storage.argtypes = [vp, vp]
    lib.slip_hip_factor_a_storage.restype = C.c_int
    lib.slip_hip_factor_multiply.argtypes = ([vp, C.c_int32, C.c_int32] + [vp, vp, i64] * 3
                                             + [C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), vp])
    lib.slip_hip_factor_multiply.restype = C.c_int
    lib.slip_hip_factor_multiply_ms.argtypes = [vp]
    lib.slip_hip_factor_multiply_ms.restype = C.c_double
    lib.slip_hip_matrix_create.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32, vp, vp, vp, vp]
    lib.slip_hip_matrix_create.restype = C.c_int
    lib.slip_hip_matrix_multiply.argtypes = lib.slip_hip_factor_multiply.argtypes
    lib.slip_hip_matrix_multiply.restype = C.c_int
    lib.slip_hip_matrix_multiply_ms.argtypes = [vp]
    lib.slip_hip_matrix_multiply_ms.restype = C.c_double
    lib.slip_hip_matrix_destroy.argtypes = [vp]
    lib.slip_hip_matrix_destroy.restype = None
    lib.slip_hip_multiply_passes.argtypes = [vp]
    lib.slip_hip_multiply_passes.restype = C.c_int
    lib.slip_hip_ratio_test.argtypes = [C.c_int32, C.c_int32, vp, vp, i64, vp, vp, i64, C.c_int32, vp, vp, vp, vp, vp]
    lib.slip_hip_ratio_test.restype = C.c_int
    lib.slip_hip_ratio_test_paths.argtypes = [vp]
    lib.slip_hip_ratio_test_paths.restype = C.c_int
    lib.slip_hip_factor_ratio_test.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, vp,
                                               C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), vp]
    lib.slip_hip_factor_ratio_test.restype = C.c_int
    lib.slip_hip_factor_ratio_test_ms.argtypes = [vp]
    lib.slip_hip_factor_ratio_test_ms.restype = C.c_double
    lib.slip_hip_factor_ratio_test_paths.argtypes = [vp, vp]
    lib.slip_hip_factor_ratio_test_paths.restype = C.c_int
    lib.slip_hip_factor_price.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, i64, C.c_int32, vp, vp, vp, vp, vp,
                                          C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), vp]
    lib.slip_hip_factor_price.restype = C.c_int
    lib.slip_hip_factor_price_ms.argtypes = [vp, vp]
    lib.slip_hip_factor_price_ms.restype = C.c_int
    lib.slip_hip_factor_price_paths.argtypes = [vp, vp]
    lib.slip_hip_factor_price_paths.restype = C.c_int
    res4, win = [vp] * 4, [C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]
    bp = C.POINTER(BoundsRec)
    lib.slip_hip_factor_ratio_test_bounded.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, bp, C.c_int32, vp] + res4 + win + [vp]
    lib.slip_hip_factor_ratio_test_bounded.restype = C.c_int
    lib.slip_hip_factor_bound_test.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, bp, vp] + res4 + win + [vp]
    lib.slip_hip_factor_bound_test.restype = C.c_int
    lib.slip_hip_ratio_test_bounded.argtypes = [C.c_int32, C.c_int32] + [vp, vp, i64] * 3 + [bp, C.c_int32, vp] + res4 + win + [vp]
    lib.slip_hip_ratio_test_bounded.restype = C.c_int
    lib.slip_hip_bound_test.argtypes = [C.c_int32, C.c_int32] + [vp, vp, i64] * 2 + [bp, vp] + res4 + win + [vp]
    lib.slip_hip_bound_test.restype = C.c_int
    lib.slip_hip_factor_bound_ms.argtypes = [vp, vp]
    lib.slip_hip_factor_bound_ms.restype = C.c_int
    lib.slip_hip_factor_bound_paths.argtypes = [vp, vp]
    lib.slip_hip_factor_bound_paths.restype = C.c_int
    lib.slip_hip_bound_paths.argtypes = [vp]
    lib.slip_hip_bound_paths.restype = C.c_int
    states = [vp, vp, vp, i64, C.c_int32, vp] + res4 + win + [vp]        # state, the weights, sense, key, the results, stream
    lib.slip_hip_factor_price_states.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, i64] + states
    lib.slip_hip_factor_price_states.restype = C.c_int
    lib.slip_hip_price_select.argtypes = [C.c_int32] * 3 + [vp, vp, i64] * 3 + states
    lib.slip_hip_price_select.restype = C.c_int
    lib.slip_hip_factor_price_states_ms.argtypes = [vp, vp]
    lib.slip_hip_factor_price_states_ms.restype = C.c_int
    lib.slip_hip_factor_price_states_paths.argtypes = [vp, vp]
    lib.slip_hip_factor_price_states_paths.restype = C.c_int
    lib.slip_hip_price_select_paths.argtypes = [vp]
    lib.slip_hip_price_select_paths.restype = C.c_int
    lib.slip_hip_pivot_update.argtypes = [C.c_int32, C.c_int32] + [vp, vp, i64] * 5 + [vp, vp] + win + [vp]
    lib.slip_hip_pivot_update.restype = C.c_int
    lib.slip_hip_factor_solve_update.argtypes = [vp, C.c_int32, C.c_int32, vp, vp] + [vp, vp, i64] * 2 + [vp, vp] + win + [vp]
    lib.slip_hip_factor_solve_update.restype = C.c_int
    lib.slip_hip_factor_step.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp] + res4 + win + win + [vp]
    lib.slip_hip_factor_step.restype = C.c_int
    lib.slip_hip_factor_update_ms.argtypes = [vp, vp]
    lib.slip_hip_factor_update_ms.restype = C.c_int
    lib.slip_hip_factor_update_paths.argtypes = [vp, vp]
    lib.slip_hip_factor_update_paths.restype = C.c_int
    lib.slip_hip_pivot_update_paths.argtypes = [vp]
    lib.slip_hip_pivot_update_paths.restype = C.c_int
    ep = C.POINTER(EnteringRec)
    stepb = [bp, ep, C.c_int32, vp] + [vp] * 6 + win * 3 + [vp]     # bounds, entering, sense, key, six results, R, Dn, E, stream
    lib.slip_hip_factor_step_bounded.argtypes = [vp, C.c_int32, C.c_int32, vp, vp] + stepb
    lib.slip_hip_factor_step_bounded.restype = C.c_int
    lib.slip_hip_step_bounded.argtypes = [C.c_int32, C.c_int32] + [vp, vp, i64] * 3 + stepb
    lib.slip_hip_step_bounded.restype = C.c_int
    lib.slip_hip_factor_step_bounded_ms.argtypes = [vp, vp]
    lib.slip_hip_factor_step_bounded_ms.restype = C.c_int
    lib.slip_hip_factor_step_bounded_paths.argtypes = [vp, vp]
    lib.slip_hip_factor_step_bounded_paths.restype = C.c_int
    lib.slip_hip_step_bounded_ms.argtypes = [vp]
    lib.slip_hip_step_bounded_ms.restype = C.c_int
    lib.slip_hip_step_bounded_paths.argtypes = [vp]
    lib.slip_hip_step_bounded_paths.restype = C.c_int
    _libs[path] = lib
    return lib
