/* slip_hip.h -- C ABI of the MI355X-native REF sparse LU hot path (libslip_hip.so).
 *
 * Plain pointers and sizes only: no GMP, no torch, no C++ types.  Big integers
 * cross this boundary as "limb slabs": per entry a signed limb count
 * (sign * number of 64-bit limbs, 0 = zero) and the limbs little-endian, back
 * to back -- the same words GMP keeps behind an mpz_t (_mp_size, _mp_d).
 *
 * What each entry point replaces in cjh10644/SLIP_LU (reference file:line):
 *
 *   slip_hip_factor_create/run/download  <->  SLIP_LU_factorize
 *        SLIP_LU/Include/SLIP_LU.h:854-863, SLIP_LU/Source/SLIP_LU_factorize.c:36-314
 *        (with slip_REF_triangular_solve.c:65-265, slip_reach.c, slip_dfs.c,
 *         slip_sort_xi.c and slip_get_pivot.c:30-183 inside the column loop)
 *   slip_hip_options                     <->  SLIP_options.pivot / .tol
 *        SLIP_LU/Include/SLIP_LU.h:212-223; defaults SLIP_LU_internal.h:136-149
 *   slip_hip_factor_solve                <->  the integer core of SLIP_LU_solve
 *        SLIP_LU/Source/SLIP_LU_solve.c:41-86 (slip_forward_sub.c, slip_array_mul.c, slip_back_sub.c)
 *   slip_hip_factor_check,               <->  SLIP_check_solution (integer form)
 *   slip_hip_check_solution                   SLIP_LU/Source/SLIP_check_solution.c:31-113, SLIP_LU.h:988-993
 *   slip_hip_factor_solve_double,        <->  the rest of SLIP_solve_double: SLIP_permute_x, SLIP_scale_x, SLIP_get_double_soln
 *   slip_hip_solution_to_double               SLIP_LU/Source/SLIP_solve_double.c:84-100, SLIP_gmp.c:1063 (mpq_get_d)
 *   slip_hip_factor_solve_rational,      <->  the rest of SLIP_solve_mpq: the mpq_div of SLIP_LU_solve, SLIP_permute_x, SLIP_scale_x
 *   slip_hip_solution_to_rational             SLIP_LU/Source/SLIP_solve_mpq.c:74-93, slip_array_div.c:36-49 (mpq_canonicalize per entry)
 *   slip_hip_factor_solve_transpose,     <->  no counterpart: the reference solves A x = b only (KLU's klu_tsolve,
 *   slip_hip_factor_check_transpose           UMFPACK's A' system are the transposed solves of other sparse LUs)
 *   slip_hip_factor_rewind,              <->  no counterpart: the reference factorises from column 0 (KLU's klu_refactor,
 *   slip_hip_factor_replace_column            a simplex code's basis change are what other codes offer between two solves)
 *   slip_hip_factor_multiply,            <->  no counterpart (SLIP_check_solution forms A x - b and keeps only the verdict):
 *   slip_hip_matrix_*                         the exact sparse products of a simplex code's pricing and of a residual
 *   slip_hip_ratio_test,                 <->  no counterpart: the exact ratio test of a simplex step (the leaving row, the
 *   slip_hip_factor_ratio_test                most negative reduced cost, the dual ratio test); only the choice comes back
 *   slip_hip_*ratio_test_bounded,        <->  no counterpart: the ratio test of a basis with boxed variables l <= x <= u, and
 *   slip_hip_*bound_test                      the most violated bound (primal feasibility, the dual simplex's leaving row)
 *   status codes                         <->  SLIP_info, SLIP_LU.h:160-168
 *
 * The GMP-typed drop-in  SLIP_LU_factorize(L,U,A,S,rhos,pinv,option)  built on
 * top of this ABI is declared in include/SLIP_LU_hip.h (libslip_lu_hip.so).
 *
 * Threading: like the reference, one factorisation per handle at a time; the
 * calls block until the device work is complete.
 */
#ifndef SLIP_HIP_H
#define SLIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* SLIP_info values (SLIP_LU.h:160-168), plus one code kept outside them */
#define SLIP_HIP_OK               0
#define SLIP_HIP_OUT_OF_MEMORY   (-1)
#define SLIP_HIP_SINGULAR        (-2)
#define SLIP_HIP_INCORRECT_INPUT (-3)
#define SLIP_HIP_INCORRECT       (-4)     /* SLIP_INCORRECT: a checked solution is not exact */
#define SLIP_HIP_DEVICE_ERROR    (-100)   /* HIP runtime failure (no GPU, launch error) */

typedef struct slip_hip_options {
    int32_t pivot;        /* SLIP_pivot 0..5; default 3 = SLIP_TOL_SMALLEST            */
    double  tol;          /* SLIP_options.tol; default 1.0                             */
    int32_t limb_cap;     /* > 0: column-window mode -- stop BEFORE the first column   */
                          /*      that holds a value of more than limb_cap limbs       */
    int32_t waves;        /* waves per workgroup (0 = default 8)                        */
    int64_t lnz_hint;     /* initial capacity of L / U in entries (0 = 4*nnz(A)+n),    */
    int64_t unz_hint;     /*   cf. SLIP_LU_analysis.lnz/.unz; both grow on demand      */
    int32_t workers;      /* column workers (workgroups of a launch; each owns a private */
                          /*   dense vector): 0 = as many as can be resident            */
    int32_t reserved;     /* diagnostics: bit 0 = no early commit, bit 1 = no committer workgroup, bit 2 = no helping with long update queues, bit 3 = no full packages (chain engine off); bits 4-5 = experiment: workers on CUs within this distance of the committer's stand aside (measured: no effect) */
} slip_hip_options;

typedef struct slip_hip_info {
    int32_t n;
    int32_t K;            /* columns committed so far                                  */
    int32_t status;       /* SLIP_HIP_* of the last run                                */
    int32_t window_end;   /* 1: run stopped at the limb cap (column K not committed)   */
    int64_t lnz, unz;     /* entries of L(:,0:K), U(:,0:K) (pivots in both)            */
    int64_t l_limbs, u_limbs;
    /* algorithmic counters of SURVEY.md 8(d), counted by the device */
    int64_t n_upd, b_read, b_write, n_src, l_streamed, max_limbs;
    double  kernel_ms;    /* device time of the factorisation kernels of the last run  */
    int32_t launches;     /* kernel launches of the last run (regrows relaunch)        */
    int32_t xcap_digits;  /* current stride of the dense scatter vectors, 32-bit digits */
    int64_t limb_macs;    /* sum over the IPGE updates of l(L_m)*l(x_j) + l(x_i)*l(rho_jn), 64-bit limbs */
    int32_t workers, waves;   /* launch shape: column workers x wavefronts each          */
    int32_t lds_bytes;        /* dynamic LDS per worker                                   */
    int32_t short_commits;    /* columns whose pivot was published by the short commit chain (diagnostic) */
    int32_t committer_commits;         /* ... of those, by the committer workgroup */
    int32_t farm_jobs, farm_items, batch_commits;   /* update queues opened to helpers; items helpers ran (diagnostic); columns the committer committed side by side */
    int32_t engine_commits, engine_sources; /* columns committed by the committer's chain engine from FULL packages; late sources it applied */
    int32_t retractions, reexports;        /* packages a worker took back because a source arrived; packages exported again */
    int64_t raw_fills;                     /* rows filled in as -a_j * L(i,j) from a source entry no earlier source had touched: no division (diagnostic; factorisation and the solves' forward sweeps) */
} slip_hip_info;

typedef struct slip_hip_factor slip_hip_factor;

void slip_hip_default_options(slip_hip_options *opt);

/* number of HIP devices visible (0 if none / runtime missing) */
int slip_hip_device_count(void);

/* Upload A (CSC: Ap[n+1], Ai, per-entry signed limb counts Alen, limbs back to
 * back in Alimbs, entry order as in the reference's SLIP_sparse: unsorted rows
 * allowed, a duplicated row keeps the LAST value as slip_get_column.c:22 does)
 * and the column order q[n] (SLIP_LU_analysis.q).  All inputs are host
 * pointers; they are copied. */
int slip_hip_factor_create(slip_hip_factor **out, int32_t n,
                           const int64_t *Ap, const int32_t *Ai,
                           const int32_t *Alen, const uint64_t *Alimbs,
                           const int32_t *q, const slip_hip_options *opt);

/* Forget all columns: back to k = 0 with A and q still resident. */
int slip_hip_factor_reset(slip_hip_factor *f);

/* Factorise columns [K, kmax) (kmax <= 0 or > n: n).  stream: a hipStream_t
 * passed as void* (NULL = default stream).  Returns SLIP_HIP_OK when kmax (or
 * the limb cap) was reached, SLIP_HIP_SINGULAR, SLIP_HIP_OUT_OF_MEMORY, ... */
int slip_hip_factor_run(slip_hip_factor *f, int32_t kmax, void *stream);

int slip_hip_factor_info(const slip_hip_factor *f, slip_hip_info *info);

/* Copy the factors to host arrays sized from slip_hip_factor_info:
 *   Lp[K+1], Li[lnz], Llen[lnz], Llimbs[l_limbs]   (same for U)
 *   rholen[K], rholimbs[sum |rholen|], pinv[n]
 * Row indices are ORIGINAL row ids in the reference's entry order
 * (SLIP_LU_factorize.c:226-263); apply pinv for the final relabel (:293-301).
 * Any pointer may be NULL to skip that array.  Every limb array travels with its
 * capacity: *_limbs_inout: in = capacity of the array in limbs, out = limbs written
 * (required whenever the array is given).  The entry records on the device are checked
 * against the device's own limb counters and against the slab before anything is
 * copied: an inconsistency is SLIP_HIP_DEVICE_ERROR, a short array SLIP_HIP_INCORRECT_INPUT;
 * in neither case is a limb array written. */
int slip_hip_factor_download(const slip_hip_factor *f,
                             int64_t *Lp, int32_t *Li, int32_t *Llen, uint64_t *Llimbs, int64_t *L_limbs_inout,
                             int64_t *Up, int32_t *Ui, int32_t *Ulen, uint64_t *Ulimbs, int64_t *U_limbs_inout,
                             int32_t *rholen, uint64_t *rholimbs, int64_t *rho_limbs_inout,
                             int32_t *pinv);

/* REF forward/back substitution on the factors still resident in HBM -- the arithmetic of
 * SLIP_LU_solve (SLIP_LU/Source/SLIP_LU_solve.c:41-86: b2 = P b, slip_forward_sub.c:61-158,
 * slip_array_mul.c:19 by det = rhos[n-1], slip_back_sub.c:36-52).  Needs the complete
 * factorisation (K == n).  b is dense, nrhs columns of n entries in ORIGINAL row order:
 * blen[c*n+i] = signed limb count, limbs back to back in blimbs in that order.  The result is
 * what SLIP_LU_solve leaves in x before SLIP_permute_x / the division by det*scale
 * (slip_hip_factor_solve_double below does those on the device too): integer numerators over det, entry c*n+p for
 * pivot POSITION p (x_final[q[p]] = xnum[p] / det), same signed-limb-slab form.  *xlen_out and
 * *xlimbs_out are malloc'ed; release with slip_hip_free. */
int slip_hip_factor_solve(slip_hip_factor *f, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                          int32_t **xlen_out, uint64_t **xlimbs_out, int64_t *xnl_out, void *stream);
/* A handle around factors the CALLER already holds (what SLIP_LU_solve is given, SLIP_LU.h:941-949), for
 * slip_hip_factor_solve only (run/reset refuse it).  L, U in the form slip_hip_factor_download produces:
 * column pointers, ORIGINAL row ids in the reference's entry order (the pivot LAST in every U column,
 * slip_back_sub.c:43), signed limb counts, limbs back to back; pinv[n].  The pivots rho_k are read from L
 * (the entry of L(:,k) in the row with pinv == k).  Host pointers, copied. */
int slip_hip_factor_from_factors(slip_hip_factor **out, int32_t n,
                                 const int64_t *Lp, const int32_t *Li, const int32_t *Llen, const uint64_t *Llimbs,
                                 const int64_t *Up, const int32_t *Ui, const int32_t *Ulen, const uint64_t *Ulimbs,
                                 const int32_t *pinv, const slip_hip_options *opt);
/* device time of the solve kernels of the last slip_hip_factor_solve, milliseconds */
double slip_hip_factor_solve_ms(const slip_hip_factor *f);

/* Exact solution check (SLIP_check_solution, SLIP_LU/Source/SLIP_check_solution.c:31-113, as one integer test on the
 * device): with x_c = xnum_c / d_c over one common denominator, A * xnum_c == d_c * b_c row by row, exactly.
 *
 * slip_hip_factor_check: on a handle made by slip_hip_factor_create with the factorisation complete (K == n).  b as
 * slip_hip_factor_solve takes it (nrhs columns of n entries, ORIGINAL row order); x in exactly the form slip_hip_factor_solve
 * returns it: numerators by pivot POSITION p (x_final[q[p]] = xnum[p] / det) over det = rho[n-1] of the handle's own,
 * unrescaled factors.  Checks A(:,q) * xnum_c == det * b_c for every right-hand side c.
 *
 * slip_hip_check_solution: no handle.  A as slip_hip_factor_create takes it; x in ORIGINAL column order (x[c*n + j]
 * multiplies A(:,j)); one nonzero integer denominator d_c per right-hand side (dlen[nrhs], limbs back to back).  Checks
 * A * x_c == d_c * b_c.
 *
 * Return: SLIP_HIP_OK when every right-hand side is exact, SLIP_HIP_INCORRECT when at least one is not.  In both cases
 * first_bad_row[c] = the smallest original row id i with r_i != 0 (-1: none) and bad_rows[c] = the number of such rows;
 * either pointer may be NULL.  Every limb array travels with its capacity in limbs (b_limbs, x_limbs, d_limbs).
 * SLIP_HIP_INCORRECT_INPUT, before any array is read past its end: nrhs < 1; a limb array whose sum |len| exceeds its
 * capacity; d_c == 0; a handle from slip_hip_factor_from_factors (it holds no A); an incomplete factorisation.  High zero
 * limbs in the inputs are allowed.  No CPU fallback: without a device the result is SLIP_HIP_DEVICE_ERROR.
 *
 * Duplicates: a row repeated in a column of A keeps its LAST value, as slip_hip_factor_create does (slip_get_column.c:22),
 * so the check tests the matrix that was factorised.  Here it differs from SLIP_check_solution, which sums duplicates. */
int slip_hip_factor_check(slip_hip_factor *f, int32_t nrhs,
                          const int32_t *blen, const uint64_t *blimbs, int64_t b_limbs,
                          const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                          int32_t *first_bad_row, int64_t *bad_rows, void *stream);
int slip_hip_check_solution(int32_t n, const int64_t *Ap, const int32_t *Ai, const int32_t *Alen, const uint64_t *Alimbs,
                            int32_t nrhs, const int32_t *blen, const uint64_t *blimbs, int64_t b_limbs,
                            const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                            const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                            int32_t *first_bad_row, int64_t *bad_rows, void *stream);
/* device time of the check kernel of the last slip_hip_factor_check, milliseconds */
double slip_hip_factor_check_ms(const slip_hip_factor *f);

/* Exact transposed solve on the same resident factors: A(:,q)^T x = b, the system slip_hip_factor_solve solves, transposed
 * (the dual of an LP basis, a simplex code's BTRAN).  No second factorisation: the REF factorisation of the transpose of
 * the factorised matrix, in the identity pivot order, is (U^T, L^T) with the same pivots, and the same substitution kernels
 * run on that view of the factors (built on the device on the first call, kept until reset; no limb is copied).  Needs the
 * complete factorisation (K == n); a handle from slip_hip_factor_from_factors works too.
 *   b: dense, nrhs columns of n entries by pivot POSITION -- b[c*n + k] pairs with column q[k] of A;
 *   x: numerators over det = rho[n-1] (the denominator of slip_hip_factor_solve) by ORIGINAL row id: x[c*n + i] is for row i
 *      of A, i.e. for column i of A^T.  To solve A^T x = b_orig, pass b[k] = b_orig[q[k]] (the input-side counterpart of
 *      SLIP_permute_x).
 * Slabs, ownership and statuses as slip_hip_factor_solve. */
int slip_hip_factor_solve_transpose(slip_hip_factor *f, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                                    int32_t **xlen_out, uint64_t **xlimbs_out, int64_t *xnl_out, void *stream);
/* Exact check of a transposed solve: for every position k, sum_i A(i, q[k]) * xnum_c[i] == det * b_c[k], with b and x exactly
 * as slip_hip_factor_solve_transpose takes and returns them (a row repeated in a column of A keeps its LAST value, as in
 * slip_hip_factor_check).  first_bad_pos[c] = the smallest position k with a nonzero residual (-1: none), bad_pos[c] = how
 * many; statuses and rejected inputs as slip_hip_factor_check (nrhs < 1, a limb array longer than its capacity, a handle from
 * slip_hip_factor_from_factors, an incomplete factorisation: SLIP_HIP_INCORRECT_INPUT). */
int slip_hip_factor_check_transpose(slip_hip_factor *f, int32_t nrhs,
                                    const int32_t *blen, const uint64_t *blimbs, int64_t b_limbs,
                                    const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                    int32_t *first_bad_pos, int64_t *bad_pos, void *stream);
/* device ms of the last transposed solve's substitution kernels; *view_ms (may be NULL): the view build of that call, 0 if reused */
double slip_hip_factor_solve_transpose_ms(const slip_hip_factor *f, double *view_ms);

/* Solve straight to doubles: the tail of SLIP_solve_double (SLIP_LU/Source/SLIP_solve_double.c:84-100: SLIP_permute_x,
 * SLIP_scale_x, SLIP_get_double_soln -> mpq_get_d per entry, SLIP_gmp.c:1063) on the device, after the substitution of
 * slip_hip_factor_solve (transpose = 0) or slip_hip_factor_solve_transpose (transpose != 0), whose numerators never leave it.
 *
 * Every result is the EXACT rational truncated toward zero onto the double grid, bit for bit what mpq_get_d returns: 53
 * significant bits in the normal range, never rounded up ((2^1024 - 1) / 1 -> 0x1.fffffffffffffp+1023); below 2^-1022 a
 * multiple of 2^-1074 with the sign kept (-3 / 2^1075 -> -0x0.0000000000001p-1022); +0.0 when |q| < 2^-1074 or the numerator is
 * zero (the sign is dropped); +-inf from 2^1024 on.  A quotient that lies exactly on the grid (integer and dyadic solutions)
 * comes back exactly: the kernel settles what the leading bits leave open with one exact big-integer comparison.
 *
 * slip_hip_factor_solve_double: b as slip_hip_factor_solve (transpose = 0) or slip_hip_factor_solve_transpose (transpose != 0)
 * takes it.  scale = snum / sden is applied before the ONE truncation: x = trunc(xnum * snum / (det * sden)); each part as a
 * signed limb count and its limbs, a NULL limb pointer meaning 1 (then the count is ignored); a negative part carries its
 * sign.  x_out[nrhs * n], allocated by the caller, is all that comes back: for the plain solve in ORIGINAL column order,
 * x_out[c*n + q[p]] for pivot position p (SLIP_permute_x applied), for the transposed solve by original row id, as
 * slip_hip_factor_solve_transpose returns its numerators.  Statuses as slip_hip_factor_solve; SLIP_HIP_INCORRECT_INPUT also for
 * a scale part that is zero and for a plain (transpose = 0) call on a handle from slip_hip_factor_from_factors, which holds
 * no q (the transposed call works there).  slip_hip_factor_solve / _solve_transpose afterwards return what they always did.
 *
 * slip_hip_solution_to_double: no handle; numerators x (n per right-hand side) and one nonzero denominator d_c per right-hand
 * side, in the (x, d) form of slip_hip_check_solution; out[nrhs * n] in the order of the input.  Limb arrays travel with
 * their capacities (x_limbs, d_limbs), high zero limbs are allowed.  For solutions the caller holds: a handle around given
 * factors, rescaled output.  SLIP_HIP_INCORRECT_INPUT: nrhs < 1, a limb array longer than its capacity, d_c == 0.
 *
 * No CPU fallback: without a device the result is SLIP_HIP_DEVICE_ERROR. */
int slip_hip_factor_solve_double(slip_hip_factor *f, int32_t transpose, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                                 int32_t snlen, const uint64_t *snlimbs, int32_t sdlen, const uint64_t *sdlimbs,
                                 double *x_out, void *stream);
int slip_hip_solution_to_double(int32_t n, int32_t nrhs, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs, double *out, void *stream);
/* device ms of the conversion kernel of the last slip_hip_factor_solve_double; how many of its entries the kernel's lane pass
 * (leading bits only) left to the exact wave pass */
double slip_hip_factor_to_double_ms(const slip_hip_factor *f);
int64_t slip_hip_factor_to_double_slow(const slip_hip_factor *f);

/* Solve to reduced fractions: the tail of SLIP_solve_mpq (SLIP_LU/Source/SLIP_solve_mpq.c:74-93: the mpq_div of SLIP_LU_solve,
 * slip_array_div.c:36-49, then SLIP_permute_x and SLIP_scale_x, every mpq_* call canonicalising) on the device, after the
 * substitution of slip_hip_factor_solve (transpose = 0) or slip_hip_factor_solve_transpose (transpose != 0).
 *
 * Every result is GMP's canonical form of the exact rational: with g = gcd(|N|, |D|), num = sgn(N * D) * |N| / g and
 * den = |D| / g -- den > 0, the sign on the numerator, 0 as 0 / 1.
 *
 * slip_hip_factor_solve_rational: b, transpose, the scale parts and the statuses exactly as slip_hip_factor_solve_double takes
 * and returns them (NULL limbs = 1, a zero part is SLIP_HIP_INCORRECT_INPUT, a negative part carries its sign; a plain call
 * on a handle from slip_hip_factor_from_factors is SLIP_HIP_INCORRECT_INPUT, the transposed call works there).  Entry c*n + j
 * of the result is the canonical form of xnum * snum / (det * sden) -- SLIP_scale_x applied once, exactly -- with j the
 * ORIGINAL column for the plain solve (SLIP_permute_x applied: j = q[p] for pivot position p) and the original row id for
 * the transposed one.  The result is two compact slabs allocated by the library (release each of the four arrays with
 * slip_hip_free): numlen / denlen hold nrhs * n signed limb counts (numlen 0 for a zero, denlen always >= 1), the limbs lie
 * back to back in entry order without high zero limbs, *num_limbs_out / *den_limbs_out say how many there are.  Nothing but
 * these slabs comes back from the device: neither the unreduced numerators nor the factors are downloaded.
 * slip_hip_factor_solve / _solve_transpose / _solve_double afterwards return what they always did.
 *
 * slip_hip_solution_to_rational: no handle; the (x, d) form of slip_hip_check_solution and slip_hip_solution_to_double, one
 * nonzero denominator per right-hand side, the result in the order of the input.  Limb arrays travel with their capacities,
 * high zero limbs are allowed.  SLIP_HIP_INCORRECT_INPUT: nrhs < 1, a limb array longer than its capacity, d_c == 0.
 *
 * No CPU fallback: without a device the result is SLIP_HIP_DEVICE_ERROR. */
int slip_hip_factor_solve_rational(slip_hip_factor *f, int32_t transpose, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                                   int32_t snlen, const uint64_t *snlimbs, int32_t sdlen, const uint64_t *sdlimbs,
                                   int32_t **numlen_out, uint64_t **numlimbs_out, int64_t *num_limbs_out,
                                   int32_t **denlen_out, uint64_t **denlimbs_out, int64_t *den_limbs_out, void *stream);
int slip_hip_solution_to_rational(int32_t n, int32_t nrhs, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                  const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                                  int32_t **numlen_out, uint64_t **numlimbs_out, int64_t *num_limbs_out,
                                  int32_t **denlen_out, uint64_t **denlimbs_out, int64_t *den_limbs_out, void *stream);
/* device ms of the reduction kernel of the last slip_hip_factor_solve_rational; out[4]: the entries of that call settled by
 * the kernel's lane pass (a zero numerator, or both parts within 64 bits), by the wave pass in registers (operands of at most
 * 256 digits of 32 bits) with g = 1 and with g > 1, and by the wave pass through memory (wider operands) */
double slip_hip_factor_to_rational_ms(const slip_hip_factor *f);
int    slip_hip_factor_to_rational_paths(const slip_hip_factor *f, int64_t out[4]);
/* the same four counts for the calling thread's last slip_hip_solution_to_rational */
int    slip_hip_solution_to_rational_paths(int64_t out[4]);

/* Solve to multi-precision floats: the tail of SLIP_solve_mpfr (SLIP_LU/Source/SLIP_solve_mpfr.c:82-104: SLIP_permute_x,
 * SLIP_scale_x, SLIP_get_mpfr_soln, i.e. mpfr_set_q per entry) on the device, after the substitution of slip_hip_factor_solve
 * (transpose = 0) or slip_hip_factor_solve_transpose (transpose != 0).
 *
 * Every result is what mpfr_set_q(x, N / D, rnd) leaves in an mpfr_t of `prec` bits, 2 <= prec <= 65536, with rnd one of
 * MPFR_RNDN = 0 (nearest, ties to the even mantissa), MPFR_RNDZ = 1, MPFR_RNDU = 2, MPFR_RNDD = 3, MPFR_RNDA = 4: the ONE
 * correct rounding of the exact rational (no gcd is taken; the scale goes in before it).  Per entry:
 *   sign     int8:  0 for a zero (always +0: the sign is dropped, also under a negative scale and under RNDD), else +1 / -1;
 *   exp      int64: MPFR's exponent e, |x| = 0.1... * 2^e, i.e. |x| = m * 2^(e - prec) with 2^(prec-1) <= m < 2^prec; 0 for a zero;
 *   mant     ceil(prec / 64) limbs, least significant first, the mantissa left-aligned as in MPFR's own limb array: the top
 *            bit of the top limb set, the bits below the prec-th zero; all zero for a zero;
 *   ternary  int8: the sign of (rounded - exact): 0 when the result is exact.
 * There is no overflow or underflow: MPFR's default exponent range cannot be reached by operands that fit in memory.
 *
 * slip_hip_factor_solve_mpfr: b, transpose, the scale parts and the statuses exactly as slip_hip_factor_solve_double takes and
 * returns them (also the refusal of a plain call on a handle from slip_hip_factor_from_factors); entry c*n + j in its order.
 * The caller allocates sign_out[nrhs*n], exp_out[nrhs*n], mant_out[nrhs*n*ceil(prec/64)] and ternary_out[nrhs*n] (or NULL);
 * nothing else crosses back.  SLIP_HIP_INCORRECT_INPUT also for prec outside 2..65536 and for any other rnd (MPFR_RNDF = 5
 * and MPFR_RNDNA = -1 among them).  slip_hip_factor_solve / _solve_transpose / _solve_double / _solve_rational afterwards
 * return what they always did.
 *
 * slip_hip_solution_to_mpfr: no handle; the (x, d) form of slip_hip_solution_to_double with its capacities and refusals, the
 * result in the order of the input.  It is the slab form of SLIP_get_mpfr_soln.
 *
 * No CPU fallback: without a device the result is SLIP_HIP_DEVICE_ERROR. */
int slip_hip_factor_solve_mpfr(slip_hip_factor *f, int32_t transpose, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                               int32_t snlen, const uint64_t *snlimbs, int32_t sdlen, const uint64_t *sdlimbs,
                               int32_t prec, int32_t rnd, int8_t *sign_out, int64_t *exp_out, uint64_t *mant_out,
                               int8_t *ternary_out, void *stream);
int slip_hip_solution_to_mpfr(int32_t n, int32_t nrhs, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                              const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs, int32_t prec, int32_t rnd,
                              int8_t *sign_out, int64_t *exp_out, uint64_t *mant_out, int8_t *ternary_out, void *stream);
/* device ms of the conversion kernel of the last slip_hip_factor_solve_mpfr; out[4]: the entries of that call settled by the
 * kernel's lane pass with both parts within 64 bits (prec <= 64 only), by the wave pass (a long division) with a denominator
 * of at most 256 digits of 32 bits, by the wave pass with a wider one, and -- out[3] -- as zero */
double slip_hip_factor_to_mpfr_ms(const slip_hip_factor *f);
int    slip_hip_factor_to_mpfr_paths(const slip_hip_factor *f, int64_t out[4]);
/* the same four counts for the calling thread's last slip_hip_solution_to_mpfr */
int    slip_hip_solution_to_mpfr_paths(int64_t out[4]);

/* Subtree farm (no counterpart in the reference, which has no parallelism): multiply the K committed
 * columns by per-column scales on the device -- L(:,k) and rho[k] by scale[k], an entry of U in the row whose pivot sits
 * at position p by scale[p] -- where scale[k] is the product of the pivots the OTHER independent blocks had produced when
 * global column k was eliminated (slip_lu_amd/parallel.py: subtree_scales).  scale[k]: signed limb counts slen[nscales], limbs back
 * to back; nscales must equal the K committed columns (SLIP_HIP_INCORRECT_INPUT otherwise).  The rescaled copy is what slip_hip_factor_download / _info then serve, until the next reset (or rescale);
 * the handle's own factors are untouched, so run / solve keep working on the local values. */
int slip_hip_factor_rescale(slip_hip_factor *f, int32_t nscales, const int32_t *slen, const uint64_t *slimbs, void *stream);

/* Subtree farm, last step ("completed L columns gathered", then the separator columns): the first K columns
 * of THIS matrix's factorisation are given -- the blocks' columns, factorised on other handles / ranks and rescaled -- and
 * slip_hip_factor_run continues with column K exactly as SLIP_LU_factorize.c:190-264 does from k = K.  L, U: the K columns in
 * the form slip_hip_factor_download produces (column pointers Lp[K+1] / Up[K+1], ORIGINAL row ids in the reference's entry
 * order, the pivot LAST in every U column, signed limb counts, limbs back to back); piv_row[K]: the pivot row of every
 * column, from which the row permutation is replayed (slip_get_pivot.c:164-176).  The handle is reset first; K = 0 is a
 * reset.  Host pointers, copied.  Inconsistent input (a pivot row that is already pivotal or missing from its column, an
 * empty U column) is SLIP_HIP_INCORRECT_INPUT. */
int slip_hip_factor_set_prefix(slip_hip_factor *f, int32_t K,
                               const int64_t *Lp, const int32_t *Li, const int32_t *Llen, const uint64_t *Llimbs,
                               const int64_t *Up, const int32_t *Ui, const int32_t *Ulen, const uint64_t *Ulimbs,
                               const int32_t *piv_row);

/* Back to column K, and a column of A replaced in place: what a code that solves a sequence of nearly equal systems does
 * between two solves (an exact simplex code's basis change; cf. klu_refactor).  No counterpart in the reference, which offers
 * SLIP_LU_factorize from column 0 only.  REF LU is left-looking: columns 0..p-1 of L and U, their pivots and their row swaps
 * depend on A(:, q[0..p-1]) alone, so after a change to the column at position p they still are the exact factorisation.
 * All of it is device work on the resident data; only a new column crosses to the device.
 *
 * slip_hip_factor_rewind: a handle made by slip_hip_factor_create is put back into the state slip_hip_factor_run(f, K) from a
 * reset would have left: columns K.. forgotten, their row swaps undone from the swap log, slip_hip_factor_run continues with
 * column K.  0 <= K <= info.K.  K == info.K with q_tail == NULL changes nothing; K == 0 is slip_hip_factor_reset.  What
 * _info / _download then serve (K, lnz, unz, l_limbs, u_limbs, the columns, the pivots, pinv) is that of a run to K.  The
 * algorithmic counters (n_upd .. limb_macs, raw_fills and the commit diagnostics) restart at zero and then count the work
 * SINCE the rewind; max_limbs keeps its value, an upper bound from then on.  The transposed view and a rescaled copy are
 * dropped, as by reset.  q_tail: NULL, or n - K original column ids, the new order of positions K..n-1 (the columns there
 * are factorised again anyway) -- this is how a replaced column moves to the last position, Forrest-Tomlin style.  It must
 * be a permutation of the ids that stand there now.
 *
 * slip_hip_factor_replace_column: column j of A (ORIGINAL column id) gets new content, nz >= 1 entries in the per-column form
 * of slip_hip_factor_create: row ids, signed limb counts, limbs back to back, limbs_cap = the limbs the array holds.  The
 * rules of slip_hip_factor_create hold: unsorted rows are allowed, a repeated row keeps its LAST value, high zero limbs are
 * trimmed.  The handle is rewound to min(info.K, p) with q[p] = j (not at all when column j has not been reached yet), and
 * slip_hip_factor_run continues from there.  Everything the handle serves afterwards -- factors, pivots, pinv, the solves,
 * the checks -- is bit for bit what a fresh handle on the new matrix (same q, same options) serves.  The resident CSC is
 * edited on the device: the new limbs are appended to the limb slab, the entry arrays are spliced; limbs of replaced columns
 * are compacted away once they outnumber the live ones, so the storage of A stays within twice its live content plus the
 * initial allocation (slip_hip_factor_a_storage).
 *
 * Statuses: SLIP_HIP_INCORRECT_INPUT, with the handle untouched, for a handle from slip_hip_factor_from_factors, K outside
 * [0, info.K], a q_tail that is no permutation of the tail, j outside [0, n), nz < 1, a row id outside [0, n), sum |len| >
 * limbs_cap.  A device step that fails after the resident arrays began to change leaves a handle that refuses every further
 * call but slip_hip_factor_destroy with SLIP_HIP_DEVICE_ERROR: it never serves a mixed matrix. */
int slip_hip_factor_rewind(slip_hip_factor *f, int32_t K, const int32_t *q_tail, void *stream);
int slip_hip_factor_replace_column(slip_hip_factor *f, int32_t j, int32_t nz, const int32_t *rows, const int32_t *len,
                                   const uint64_t *limbs, int64_t limbs_cap, void *stream);
/* the storage of the resident A: out[0] live entries, out[1] entries the entry arrays can hold, out[2] live limbs, out[3]
 * limbs the slab can hold.  After any sequence of replacements out[1] <= 2 * out[0] + (entries at creation) and
 * out[3] <= 2 * out[2] + (limbs at creation). */
int slip_hip_factor_a_storage(const slip_hip_factor *f, int64_t out[4]);

/* Exact sparse products on the device, returned:  r_c = op(A) x_c - d_c b_c  for nvec vectors, every r an exact signed big
 * integer (the residual slip_hip_factor_check only tests for zero; with blen == NULL the product op(A) x_c alone).  x, b and d
 * are limb slabs as everywhere (signed limb counts, limbs back to back, x_limbs / b_limbs / d_limbs the limbs each array
 * holds); the result is one such slab, normalised: the top limb of an entry is nonzero, a zero has count 0 and no limbs.
 * *rlen_out (entries of one vector times nvec counts) and *rlimbs_out (*rnl_out limbs) are malloc'ed: slip_hip_free.
 *
 * slip_hip_factor_multiply works on the resident A of a handle made by slip_hip_factor_create, in the conventions of the
 * solves and checks, so what a solve returns goes straight in:
 *   transpose 0:  r = A(:,q) x - d b:    x[c*n + p] by pivot POSITION (as slip_hip_factor_solve returns it), r and b by
 *                 original row;
 *   transpose 1:  r = A(:,q)^T x - d b:  x[c*n + i] by original ROW id (as slip_hip_factor_solve_transpose returns it), r and b
 *                 by position k (column q[k]).
 * b given and dlen == NULL: every d_c is det = rho[n-1], which needs the complete factorisation (then a solve's output
 * gives r = 0).  Without b, or with d given (one nonzero d_c per vector), only the resident A is used: any state of the
 * factorisation will do, also after slip_hip_factor_rewind or slip_hip_factor_replace_column (the new matrix).  A row
 * repeated in a column keeps its LAST value, as everywhere on a handle.
 *
 * slip_hip_matrix_*: an m x ncols CSC integer matrix kept resident without a factorisation (the non-basic columns a simplex
 * code prices every iteration), prepared as slip_hip_factor_create prepares A (bounds, a repeated row keeps its LAST value,
 * high zero limbs trimmed; m and ncols below 2^24 - 1).  transpose 0: r = M x (x: ncols entries per vector, r and b: m);
 * transpose 1: r = M^T x (x: m, r and b: ncols).  With b, d is required.
 *
 * SLIP_HIP_INCORRECT_INPUT: a NULL required argument, nvec < 1, a limb array shorter than its counts say, d without b, a
 * zero d_c, b without d on a matrix or on an incomplete factorisation, a handle from slip_hip_factor_from_factors; a broken
 * handle answers SLIP_HIP_DEVICE_ERROR. */
int slip_hip_factor_multiply(slip_hip_factor *f, int32_t transpose, int32_t nvec,
                             const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                             const int32_t *blen, const uint64_t *blimbs, int64_t b_limbs,      /* optional */
                             const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,      /* optional: one per vector */
                             int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out, void *stream);
/* device time of the kernels of the last product of the handle / the matrix, milliseconds */
double slip_hip_factor_multiply_ms(const slip_hip_factor *f);

typedef struct slip_hip_matrix slip_hip_matrix;
int slip_hip_matrix_create(slip_hip_matrix **out, int32_t m, int32_t ncols,
                           const int64_t *Ap, const int32_t *Ai, const int32_t *Alen, const uint64_t *Alimbs);
int slip_hip_matrix_multiply(slip_hip_matrix *M, int32_t transpose, int32_t nvec,
                             const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                             const int32_t *blen, const uint64_t *blimbs, int64_t b_limbs,
                             const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                             int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out, void *stream);
double slip_hip_matrix_multiply_ms(const slip_hip_matrix *M);
void slip_hip_matrix_destroy(slip_hip_matrix *M);
/* that time of this thread's last product by pass: out[0] the widths, out[1] the offset scans, out[2] the products, out[3] the
 * packing (the staging slab of a product is bounded: SLIP_HIP_PRODUCT_STAGE_KB kilobytes, environment, default 262144; vectors
 * beyond it are taken in further groups) */
int slip_hip_multiply_passes(double out[4]);

/* Exact ratio test on the device: per problem c, over n pairs of signed big integers (x_i, a_i), the entry with the smallest
 * ratio, compared exactly.  Entry i is ELIGIBLE iff sense * a_i > 0 (a zero a_i never is); its ratio is r_i = x_i / (sense *
 * a_i), a positive denominator under a numerator of any sign.  best[c] is the eligible i with the smallest r_i, among exact ties
 * the smallest (key[i], i) (key == NULL: the smallest i), or -1 when nothing is eligible (the unbounded ray); nties[c] counts the
 * eligible entries whose ratio equals the minimum exactly, the winner included (0 with best = -1); neligible[c] the eligible
 * entries.  sense is +1 or -1; key (n values, optional) is shared by all problems.  Only these 3 * nprob integers come back.
 *
 * slip_hip_ratio_test: x and a are limb slabs of nprob * n entries each (entry c*n + i), with the limbs each array holds as
 * slip_hip_solution_to_double takes its x; high zero limbs are allowed.  alen == alimbs == NULL: no denominators -- every
 * entry is eligible and r_i = sense * x_i, the argmin (sense +1) or argmax (-1) of a signed integer vector (Dantzig pricing on
 * the result of slip_hip_factor_multiply).
 *
 * slip_hip_factor_ratio_test: the fused form.  b holds 2 * nprob right-hand sides as slip_hip_factor_solve (transpose 0) or
 * slip_hip_factor_solve_transpose (1) takes them: column 2c is the x side of problem c, column 2c + 1 its a side.  The
 * substitution runs, its numerators stay on the device and the selection runs on them.  Both sides are numerators over the
 * same det = rho[n-1]: det cancels in the ratio but not in the eligibility -- entry i is eligible iff sense * sign(det) *
 * anum_i > 0 (the true alpha_i = anum_i / det), and r_i = xnum_i / (sense * anum_i).  The indices reported, and the indices
 * into key, are those of the matching solve's output: pivot POSITION p for transpose 0 (what slip_hip_factor_replace_column
 * and _rewind work with through q[p]), original ROW id for transpose 1.  wlen_out / wlimbs_out / wnl_out (all three or
 * none): the winners' two numerators, xnum_best and anum_best of problem c as entries 2c and 2c + 1 of one malloc'ed slab
 * (slip_hip_free), both of length 0 when best = -1 -- the step theta = xnum_best / anum_best without a second solve.  Needs the
 * complete factorisation; transpose 0 is refused on a handle from slip_hip_factor_from_factors (it holds no q), transpose 1
 * works there.
 *
 * SLIP_HIP_INCORRECT_INPUT: n <= 0, nprob < 1, sense not +1 or -1, exactly one of alen / alimbs NULL, a limb array shorter than
 * its counts say, a NULL result array, an incomplete factorisation; a broken handle answers SLIP_HIP_DEVICE_ERROR.  Nothing is
 * written to the results then.
 *
 * _ms: device time of the selection kernels of the handle's last call (the substitution before them is in
 * slip_hip_factor_solve_ms / _solve_transpose_ms).  _paths (of the handle's last call; of this thread's last handle-less
 * call): out[0] eligible entries, out[1] entries the bound pass left to the exact pass, out[2] exact comparisons that formed
 * products, out[3] of those, the comparisons on the memory path (products above 256 digits). */
int slip_hip_ratio_test(int32_t n, int32_t nprob, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                        const int32_t *alen, const uint64_t *alimbs, int64_t a_limbs,             /* optional */
                        int32_t sense, const int32_t *key,
                        int32_t *best, int32_t *nties, int32_t *neligible, void *stream);
int slip_hip_ratio_test_paths(int64_t out[4]);
int slip_hip_factor_ratio_test(slip_hip_factor *f, int32_t transpose, int32_t nprob, const int32_t *blen, const uint64_t *blimbs,
                               int32_t sense, const int32_t *key, int32_t *best, int32_t *nties, int32_t *neligible,
                               int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream);
double slip_hip_factor_ratio_test_ms(const slip_hip_factor *f);
int slip_hip_factor_ratio_test_paths(const slip_hip_factor *f, int64_t out[4]);

/* Exact pricing on the device: the transposed substitution, the products with a resident matrix and the selection in one
 * call -- the entering column of a simplex step (Dantzig pricing) or the dual ratio test, with no numerator downloaded.
 *
 * Operands.  M is a slip_hip_matrix with m == f->n: its rows are original row ids of A, its ncols columns the candidates.
 * b holds nside * nprob right-hand sides exactly as slip_hip_factor_solve_transpose takes them (by pivot position, column
 * q[k] of A); nside is 1 or 2.  y_v is the numerator vector of right-hand side v, by original row id, over det = rho[n-1].
 * Problem c has the x side v = nside * c and, with nside = 2, the a side v = 2c + 1.  g is optional: glen and glimbs both
 * non-NULL hold nprob * ncols entries, g_c[j] at c * ncols + j, g_limbs being the capacity of glimbs in limbs.
 *
 * Values formed for column j of M:
 *   X_j = sum_i M(i,j) * y_x[i] - det * g_c[j]     (without g: the sum alone); its true value is X_j / det
 *   A_j = sum_i M(i,j) * y_a[i]                    (nside = 2; never a g term); its true value is alpha_j = A_j / det
 * With B y = c_B (b = c_B by position) and g = c_N the reduced cost of column j is d_j = c_j - a_j^T y = -X_j / det: the most
 * negative reduced cost is sense = -1 (the largest X_j / det).
 *
 * Selection.  nside = 1, Dantzig pricing: every column is eligible and best[c] is the j with the smallest sense * X_j / det.
 * nside = 2, the dual ratio test: slip_hip_factor_ratio_test's definition on (X, A) -- column j is eligible iff sense *
 * sign(det) * A_j > 0 and its ratio is X_j / (sense * A_j).  Exact ties go to the smallest (key[j], j); key holds ncols entries
 * or is NULL.  nties[c] counts the eligible columns whose ratio equals the minimum exactly, the winner included; neligible[c]
 * the eligible columns; best[c] = -1 (nties 0) when nothing is eligible.
 *
 * vsign[c] is the sign (-1, 0, +1) of the winner's true x-side value X_best / det, 0 when best[c] = -1: optimality ("no
 * negative reduced cost") is tested without any numerator.  wlen_out / wlimbs_out / wnl_out (all three or none): the winners'
 * numerators as one malloc'ed slab (slip_hip_free), entries 2c and 2c + 1 of problem c: X_best and A_best (nside 2), X_best
 * and an entry of length 0 (nside 1), both of length 0 when best = -1.
 *
 * Only the 4 * nprob result integers and, on request, the winners' slab come back from the device: no numerator of y, X or A
 * is downloaded otherwise.  The products are staged in groups of whole problems under SLIP_HIP_PRODUCT_STAGE_KB (at least one
 * problem a group; the bound never refuses).
 *
 * Needs the complete factorisation; a handle from slip_hip_factor_from_factors is accepted (the transposed solve works
 * there and nothing of A or q is needed).  SLIP_HIP_INCORRECT_INPUT, with nothing written: a NULL f, M, b or result array,
 * M->m != f->n, nside not 1 or 2, nprob < 1, sense not +1 or -1, exactly one of glen / glimbs NULL, a g slab longer than
 * g_limbs, a partial winners' triple, an incomplete factorisation.  A broken handle answers SLIP_HIP_DEVICE_ERROR.  The
 * handle's solve, solve_transpose, multiply and ratio_test return afterwards what they always did.
 *
 * _ms: device ms of the last call by pass: out[0] the record gather and the width pass, out[1] the offset scans, out[2] the
 * products, out[3] the selection (the substitution: slip_hip_factor_solve_transpose_ms).  _paths: the four counts of
 * slip_hip_factor_ratio_test_paths for the last price call, summed over its groups. */
int slip_hip_factor_price(slip_hip_factor *f, slip_hip_matrix *M, int32_t nside, int32_t nprob,
                          const int32_t *blen, const uint64_t *blimbs,                 /* nside*nprob right-hand sides */
                          const int32_t *glen, const uint64_t *glimbs, int64_t g_limbs, /* optional: nprob cost vectors of ncols */
                          int32_t sense, const int32_t *key,
                          int32_t *best, int32_t *nties, int32_t *neligible, int32_t *vsign,
                          int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream);
int slip_hip_factor_price_ms(const slip_hip_factor *f, double out[4]);
int slip_hip_factor_price_paths(const slip_hip_factor *f, int64_t out[4]);

/* Bounds in the exact selections: the ratio test of a basis whose variables are boxed, l_i <= x_i <= u_i with either side
 * possibly infinite, and the exact feasibility test (the most violated bound: the dual simplex's leaving row).
 *
 * A set of bounds: kind[i] bit 0 = a finite lower bound, bit 1 = a finite upper bound (any other bit is refused); integer
 * numerators lonum_i, hinum_i as two limb slabs of n entries (the entry of a side kind switches off is ignored and may have
 * length 0; a side no entry switches on may be NULL, NULL, 0); one common denominator bd > 0 as a signed limb count and limbs,
 * NULL limbs meaning 1.  l_i = lonum_i / bd, u_i = hinum_i / bd; nothing requires l_i <= u_i.  One set is shared by all
 * problems of a call, as key is; entry i, key[i] and every reported index are in the index of the matching solve's output
 * (pivot position for transpose 0, original row id for transpose 1). */
typedef struct slip_hip_bounds {
    const int32_t *kind;                                   /* n entries: bit 0 lower, bit 1 upper */
    const int32_t *lolen; const uint64_t *lolimbs; int64_t lo_limbs;   /* n entries; NULL,NULL,0 iff no entry has bit 0 */
    const int32_t *hilen; const uint64_t *hilimbs; int64_t hi_limbs;   /* likewise for bit 1 */
    int32_t bdlen; const uint64_t *bdlimbs;                /* common denominator > 0; NULL limbs = 1 */
} slip_hip_bounds;

/* Bounded ratio test.  Problem c: numerators xnum, anum over one nonzero signed d (on a handle d = det = rho[n-1]).  With
 * s = sign(d) and t_i = sense * s * anum_i:
 *   t_i > 0: eligible iff bit 0 of kind[i];  N_i = bd * xnum_i - d * lonum_i,  a'_i =  anum_i,  side -1
 *   t_i < 0: eligible iff bit 1 of kind[i];  N_i = d * hinum_i - bd * xnum_i,  a'_i = -anum_i,  side +1
 *   t_i = 0: never eligible.
 * The ratio of an eligible entry is r_i = N_i / (sense * a'_i) (the true step to the bound is r_i / bd); best[c] is the
 * eligible i with the smallest r_i compared exactly, among exact ties the smallest (key[i], i), -1 when nothing is eligible;
 * nties[c] the eligible entries whose ratio equals the minimum, the winner included; neligible[c] the eligible entries;
 * side[c] the winner's side, 0 with best = -1.  A numerator of any sign is allowed (an x_i outside its bounds gives a
 * negative ratio).  The winners' slab (all three pointers or none; malloc'ed, slip_hip_free): entries 2c and 2c + 1 are
 * N_best and a'_best, theta = N_best / (bd * sense * a'_best); both empty with best = -1.  With kind = 1, lonum = 0, bd = 1
 * this is slip_hip_factor_ratio_test's definition with side -1.
 *
 * Bound test.  Problem c: one numerator vector xnum over d.  Vlo_i = s * (d * lonum_i - bd * xnum_i) with bit 0 of kind[i],
 * else 0; Vhi_i = s * (bd * xnum_i - d * hinum_i) with bit 1, else 0 -- the violations over the common positive denominator
 * |d| * bd.  v_i = max(Vlo_i, Vhi_i), of side -1 when Vlo_i >= Vhi_i, else +1; entry i is violated iff v_i > 0 (an entry
 * exactly on its bound is not).  nviolated[c] counts the violated entries; worst[c] is the violated i with the largest v_i,
 * ties to the smallest (key[i], i), -1 when the vector is feasible; nties[c] the violated entries that share that maximum (0
 * when feasible); side[c] the side of worst[c] (0 when feasible).  The winners' slab holds nprob entries, v_worst of problem
 * c as entry c, empty when feasible.
 *
 * slip_hip_factor_ratio_test_bounded: right-hand sides, conventions, statuses and refusals are those of
 * slip_hip_factor_ratio_test (column 2c the x side, 2c + 1 the a side).  slip_hip_factor_bound_test: nprob right-hand sides
 * as the matching solve takes them.  slip_hip_ratio_test_bounded, slip_hip_bound_test: the handle-less forms on caller slabs
 * of nprob * n entries, with one nonzero signed d_c per problem as slip_hip_check_solution takes its denominators.  High zero
 * limbs are allowed in every operand.  The numerators are staged in groups of whole problems under
 * SLIP_HIP_PRODUCT_STAGE_KB (at least one problem a group; the bound never refuses).
 *
 * SLIP_HIP_INCORRECT_INPUT, with nothing written and before any array is read past its end: a NULL bounds, kind or result
 * array; a kind outside 0..3; a side some kind switches on whose slab is NULL; a slab whose sum |len| exceeds its capacity;
 * bd <= 0; a zero d_c; a partial winners' triple; everything the unbounded counterpart refuses.  No device:
 * SLIP_HIP_DEVICE_ERROR.  The handle's solve, solve_transpose, multiply, ratio_test and price return afterwards what they
 * always did.
 *
 * slip_hip_factor_bound_ms: device ms of the handle's last bounded call, out[0] the classify, offset and form passes, out[1]
 * the selection.  _paths (of the handle's last call; of this thread's last handle-less call): out[0..3] the entries the form
 * pass settled [0] without a product, [1] in a lane, [2] by a wavefront in registers, [3] by a wavefront through memory;
 * out[4..7] the four counts of slip_hip_factor_ratio_test_paths for the selection. */
int slip_hip_factor_ratio_test_bounded(slip_hip_factor *f, int32_t transpose, int32_t nprob, const int32_t *blen, const uint64_t *blimbs,
                                       const slip_hip_bounds *bounds, int32_t sense, const int32_t *key,
                                       int32_t *best, int32_t *nties, int32_t *neligible, int32_t *side,
                                       int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream);
int slip_hip_factor_bound_test(slip_hip_factor *f, int32_t transpose, int32_t nprob, const int32_t *blen, const uint64_t *blimbs,
                               const slip_hip_bounds *bounds, const int32_t *key,
                               int32_t *worst, int32_t *nties, int32_t *nviolated, int32_t *side,
                               int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream);
int slip_hip_ratio_test_bounded(int32_t n, int32_t nprob, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                const int32_t *alen, const uint64_t *alimbs, int64_t a_limbs,
                                const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                                const slip_hip_bounds *bounds, int32_t sense, const int32_t *key,
                                int32_t *best, int32_t *nties, int32_t *neligible, int32_t *side,
                                int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream);
int slip_hip_bound_test(int32_t n, int32_t nprob, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                        const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                        const slip_hip_bounds *bounds, const int32_t *key,
                        int32_t *worst, int32_t *nties, int32_t *nviolated, int32_t *side,
                        int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream);
int slip_hip_factor_bound_ms(const slip_hip_factor *f, double out[2]);
int slip_hip_factor_bound_paths(const slip_hip_factor *f, int64_t out[8]);
int slip_hip_bound_paths(int64_t out[8]);

/* Nonbasic states and reference weights in exact pricing: the entering side of a simplex step on a boxed LP, the
 * counterpart of the bounded ratio test above.  Operands as slip_hip_factor_price takes them (M with m == n, nside * nprob
 * right-hand sides, optional g, sense, optional key[ncols]); X_j and A_j are formed exactly as there.  With s = sign(det),
 * v_j = X_j / det and alpha_j = A_j / det, and two more operands shared by all problems of a call, as key is:
 *   state[ncols]: 0 never eligible, 1 at its lower bound, 2 at its upper bound, 3 free (any other value is refused);
 *   weights: an optional limb slab of ncols integers w_j > 0 (reference weights: Devex, steepest edge), nside 1 only.
 *
 * nside 1, primal pricing: column j is eligible iff sense * v_j < 0 (state 1), sense * v_j > 0 (state 2), v_j != 0 (state
 * 3).  Its score is |v_j| without weights and v_j^2 / w_j with them; best[c] is the eligible j with the largest score
 * compared exactly, among exact ties the smallest (key[j], j), -1 when nothing is eligible (optimality).  With sense = -1
 * and the reduced cost d_j = -v_j, state 1 is "d_j < 0" (slip_hip_factor_price's correspondence).
 * nside 2, dual ratio test: with t_j = sense * s * A_j column j is eligible iff t_j > 0 (state 1), t_j < 0 (state 2),
 * t_j != 0 (state 3); best[c] is the eligible j with the smallest r_j = X_j / (sense * A_j), an exact rational of any sign,
 * ties by (key[j], j).  With state = 1 everywhere this is slip_hip_factor_price's nside = 2 definition.
 * nties[c] counts the eligible columns whose score (ratio) equals the winner's, the winner included; neligible[c] the
 * eligible columns; vsign[c] is the sign of v_best, 0 with best = -1 (a free column needs it: which way to move).  The
 * winners' slab (all three pointers or none; malloc'ed, slip_hip_free): entries 2c and 2c + 1 are X_best and A_best with
 * their own signs, the second empty with nside 1, both empty with best = -1.  Squares never leave the device.
 *
 * slip_hip_factor_price_states is fused as slip_hip_factor_price is: nothing of y, X, A or X^2 is downloaded.
 * slip_hip_price_select is the handle-less form on caller slabs of nprob * ncols entries over one nonzero signed d_c per
 * problem (as slip_hip_ratio_test_bounded takes its d; d_c stands for det); a is required iff nside = 2.  High zero limbs
 * are allowed in every operand.  The squares are staged in groups of whole problems under SLIP_HIP_PRODUCT_STAGE_KB (at
 * least one problem a group; the bound never refuses).
 *
 * SLIP_HIP_INCORRECT_INPUT, with nothing written and before any array is read past its end: a NULL state; a state outside
 * 0..3; exactly one of wlen / wlimbs NULL; a weights slab whose sum |len| exceeds w_limbs; any w_j <= 0 (all-zero limbs
 * included, also for a column of state 0); weights with nside = 2; a zero d_c; a missing with nside = 2 or given with nside
 * = 1 (handle-less form); a partial winners' triple; everything slip_hip_factor_price refuses.  A broken handle, or no
 * device: SLIP_HIP_DEVICE_ERROR.  The handle's solve, solve_transpose, multiply, ratio_test, price and bounded calls return
 * afterwards what they always did.
 *
 * slip_hip_factor_price_states_ms: device ms of the handle's last call, out[0] the classify, offset and square passes,
 * out[1] the selection.  _paths (of the handle's last call; of this thread's last slip_hip_price_select): out[0..3] the
 * eligible entries [0] settled without a product (no weights, or nside 2), [1] squared in a lane, [2] squared by a
 * wavefront in registers, [3] squared by a wavefront through memory; out[4..7] the four counts of
 * slip_hip_factor_ratio_test_paths for the selection. */
int slip_hip_factor_price_states(slip_hip_factor *f, slip_hip_matrix *M, int32_t nside, int32_t nprob,
                                 const int32_t *blen, const uint64_t *blimbs,                 /* nside*nprob right-hand sides */
                                 const int32_t *glen, const uint64_t *glimbs, int64_t g_limbs, /* optional: nprob cost vectors of ncols */
                                 const int32_t *state,                                        /* ncols entries, 0..3 */
                                 const int32_t *wlen, const uint64_t *wlimbs, int64_t w_limbs, /* optional: ncols weights > 0 */
                                 int32_t sense, const int32_t *key,
                                 int32_t *best, int32_t *nties, int32_t *neligible, int32_t *vsign,
                                 int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream);
int slip_hip_price_select(int32_t ncols, int32_t nprob, int32_t nside,
                          const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                          const int32_t *alen, const uint64_t *alimbs, int64_t a_limbs,
                          const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                          const int32_t *state, const int32_t *wlen, const uint64_t *wlimbs, int64_t w_limbs,
                          int32_t sense, const int32_t *key,
                          int32_t *best, int32_t *nties, int32_t *neligible, int32_t *vsign,
                          int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream);
int slip_hip_factor_price_states_ms(const slip_hip_factor *f, double out[2]);
int slip_hip_factor_price_states_paths(const slip_hip_factor *f, int64_t out[8]);
int slip_hip_price_select_paths(int64_t out[8]);

/* Exact pivot update: the numerators of the next iterate from those the ratio test already holds, without a second
 * substitution (no counterpart in the reference).  With x = X / d the basic solution, alpha = A / d = B^-1 a_q
 * the entering column and r the leaving position, the basis B' (a_q at position r) has det B' = +-A_r and
 *     X'_i = (A_r X_i - X_r A_i) / d  (i != r),   X'_r = X_r           over the denominator A_r;
 * the division is exact (Cramer's rule on B' x' = b).  The duals update alike: Y' = (A_r Y + D_q R) / d over A_r with R = d
 * B^-T e_r and D_q = d c_q - a_q^T Y.  The kernel computes, per problem c and entry i,
 *     R_i = (P_c V_i - T_c A_i) / D_c
 * in signed big integers, and tests every division: an entry D_c does not divide comes back with length 0 and is counted in
 * ninexact[c].  Slabs, status and stream as slip_hip_ratio_test_bounded; high zero limbs are allowed in every operand; the
 * result is a normalised slab (the top limb of an entry is nonzero, a zero has count 0), malloc'ed, release with slip_hip_free.
 *
 * slip_hip_pivot_update, on caller slabs: v, a of nprob * n entries; p, t one scalar per problem; d optional (dlen == dlimbs
 *   == NULL: no division), else one nonzero D_c per problem; place optional, nprob indices in [-1, n): entry place[c] of
 *   problem c (when >= 0) is T_c itself.  r: nprob * n entries.
 * slip_hip_factor_solve_update, fused: b holds 2 * nprob right-hand sides as slip_hip_factor_ratio_test takes them (2c the V
 *   side, 2c + 1 the A side); the substitution runs, D = det = rho[n-1], P and T from the caller; the numerators of V and A
 *   never leave the device.  Indices (place, the order of r) are those of the matching solve's output: pivot position for
 *   transpose 0, original row id for transpose 1.
 * slip_hip_factor_step, the step: slip_hip_factor_ratio_test's selection (sense, key, best, nties, neligible as there), then
 *   P = anum_best, T = xnum_best, D = det, place = best.  r: nprob * n entries, the new numerators over dnew[c] = anum_best
 *   (nprob entries); best[c] = -1 leaves the n entries of problem c and dnew[c] with length 0.  The ratio counts of a step
 *   stay readable through slip_hip_factor_ratio_test_paths.
 * The fused forms need a complete factorisation; transpose 0 is refused on a handle from slip_hip_factor_from_factors.
 * SLIP_HIP_INCORRECT_INPUT, with nothing written and before any array is read past its end: a NULL required argument (every
 * pointer but d, place, key and stream), n <= 0 or nprob < 1, exactly one of dlen / dlimbs NULL, a zero D_c, a slab whose sum
 * of |len| exceeds its capacity, a place[c] outside [-1, n), everything slip_hip_factor_ratio_test refuses.  A broken handle
 * or no device: SLIP_HIP_DEVICE_ERROR.
 *
 * slip_hip_factor_update_ms: device ms of the handle's last fused call, out[0] the classify, offset and form passes, out[1]
 * the selection of a step (the substitution: slip_hip_factor_solve_ms).  _paths: out[0 .. 3] the entries [0] that needed no
 * arithmetic (both terms zero, placed, or of a problem without a winner), formed [1] in a lane, [2] by a wavefront in
 * registers, [3] by a wavefront through memory; out[4] the inexact entries; out[5 .. 7] are reserved and hold 0.
 * slip_hip_pivot_update_paths: the same of this thread's last slip_hip_pivot_update. */
int slip_hip_pivot_update(int32_t n, int32_t nprob,
                          const int32_t *vlen, const uint64_t *vlimbs, int64_t v_limbs,
                          const int32_t *alen, const uint64_t *alimbs, int64_t a_limbs,
                          const int32_t *plen, const uint64_t *plimbs, int64_t p_limbs,
                          const int32_t *tlen, const uint64_t *tlimbs, int64_t t_limbs,
                          const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                          const int32_t *place, int32_t *ninexact,
                          int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out, void *stream);
int slip_hip_factor_solve_update(slip_hip_factor *f, int32_t transpose, int32_t nprob,
                                 const int32_t *blen, const uint64_t *blimbs,
                                 const int32_t *plen, const uint64_t *plimbs, int64_t p_limbs,
                                 const int32_t *tlen, const uint64_t *tlimbs, int64_t t_limbs,
                                 const int32_t *place, int32_t *ninexact,
                                 int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out, void *stream);
int slip_hip_factor_step(slip_hip_factor *f, int32_t transpose, int32_t nprob,
                         const int32_t *blen, const uint64_t *blimbs, int32_t sense, const int32_t *key,
                         int32_t *best, int32_t *nties, int32_t *neligible, int32_t *ninexact,
                         int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out,
                         int32_t **dlen_out, uint64_t **dlimbs_out, int64_t *dnl_out, void *stream);
int slip_hip_factor_update_ms(const slip_hip_factor *f, double out[2]);
int slip_hip_factor_update_paths(const slip_hip_factor *f, int64_t out[8]);
int slip_hip_pivot_update_paths(int64_t out[8]);

/* Bounded exact simplex step: the bounded ratio test above, the comparison of the winning step with the entering variable's
 * own range, and the update of all n numerators -- a pivot or a bound flip -- in one call; between the selection and the
 * update no numerator leaves the device.
 *
 * The entering variable of problem c over the bounds' denominator bd: its current value ev_c / bd (evlen NULL: 0) and, with
 * finite[c] = 1, a range er_c / bd >= 0, the distance to its opposite bound (finite NULL: no range is finite).  er and ev
 * are limb slabs of nprob entries; er is required iff some finite[c] is set, and the entry of a problem whose flag is 0 is
 * never read.  A NULL slip_hip_entering: no range is finite and every value is 0. */
typedef struct slip_hip_entering {
    const int32_t *finite;                                 /* nprob flags 0 / 1, or NULL */
    const int32_t *erlen; const uint64_t *erlimbs; int64_t er_limbs;   /* nprob entries >= 0 */
    const int32_t *evlen; const uint64_t *evlimbs; int64_t ev_limbs;   /* nprob entries, optional */
} slip_hip_entering;

/* Problem c: xnum, anum over one nonzero signed d (on a handle d = det), s = sign(d).  The selection is
 * slip_hip_factor_ratio_test_bounded's: best, nties, neligible, side; r = best[c], N_r and a'_r as defined there, the step
 * theta = N_r / (bd * sense * a'_r).  Then move[c]:
 *   2, a flip, iff finite[c] and (best = -1 or er_c * |a'_r| <= s * N_r) -- an exact tie flips, it needs no basis change:
 *        R_i = bd * xnum_i - sense * er_c * anum_i for all n entries, Dn = bd * d, E = (ev_c + sense * er_c) * d;
 *   1, a pivot, iff best >= 0 and no flip:
 *        R_i = (bd * a'_r * xnum_i - N_r * anum_i) / d for i != r, R_r = E = ev_c * a'_r + N_r, Dn = bd * a'_r;
 *   0, unbounded, otherwise: the n entries of R, Dn and E of that problem have length 0.
 * The new basic values are R_i / Dn, the entering variable's new value E / Dn; after a pivot the leaving variable sits on
 * the bound side[c] names.  On a handle every division is exact; on caller slabs an entry d does not divide comes back with
 * length 0 and is counted in ninexact[c].  With kind = 1, lonum = 0, bd = 1 and no entering data R, Dn, best, nties and
 * neligible are slip_hip_factor_step's.
 *
 * slip_hip_factor_step_bounded: b holds 2 * nprob right-hand sides as slip_hip_factor_ratio_test takes them; indices are
 * those of the matching solve (pivot position for transpose 0, original row id for transpose 1).  slip_hip_step_bounded: the
 * same on caller slabs of nprob * n entries and one d_c per problem.  r (nprob * n entries), dn and e (nprob entries each)
 * are normalised malloc'ed slabs (slip_hip_free).  Results are written only when every staging group has succeeded.
 *
 * SLIP_HIP_INCORRECT_INPUT, with nothing written and before any array is read past its end: everything
 * slip_hip_factor_ratio_test_bounded and slip_hip_factor_step refuse; a finite[c] outside {0, 1}; a finite range with a NULL
 * er slab; exactly one of evlen / evlimbs NULL; a negative er_c with finite[c] set; a slab whose sum |len| exceeds its
 * capacity; any NULL output.  A broken handle or no device: SLIP_HIP_DEVICE_ERROR.
 *
 * _ms (of the handle's last call; of this thread's last handle-less call): device ms of out[0] the selection's classify,
 * offset and form passes, out[1] the selection, out[2] slip_bstep_kernel (capture, classify, form), out[3] the update.
 * _paths: out[0..7] slip_hip_factor_bound_paths' counts, out[8..12] the first five of slip_hip_factor_update_paths (the slot
 * of a pivot's leaving entry is computed like any other before E replaces it), out[13..15] the problems that were
 * unbounded, pivoted, flipped, out[16..19] the scalars slip_bstep_kernel formed [16] without arithmetic (both terms zero),
 * [17] in a lane, [18] in registers, [19] through memory: per problem the comparison (finite[c] and best >= 0), then the
 * two of its move (P and E of a pivot, Dn and E of a flip). */
int slip_hip_factor_step_bounded(slip_hip_factor *f, int32_t transpose, int32_t nprob, const int32_t *blen, const uint64_t *blimbs,
                                 const slip_hip_bounds *bounds, const slip_hip_entering *entering, int32_t sense, const int32_t *key,
                                 int32_t *best, int32_t *nties, int32_t *neligible, int32_t *side, int32_t *move, int32_t *ninexact,
                                 int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out,
                                 int32_t **dnlen_out, uint64_t **dnlimbs_out, int64_t *dnnl_out,
                                 int32_t **elen_out, uint64_t **elimbs_out, int64_t *enl_out, void *stream);
int slip_hip_step_bounded(int32_t n, int32_t nprob, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                          const int32_t *alen, const uint64_t *alimbs, int64_t a_limbs,
                          const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                          const slip_hip_bounds *bounds, const slip_hip_entering *entering, int32_t sense, const int32_t *key,
                          int32_t *best, int32_t *nties, int32_t *neligible, int32_t *side, int32_t *move, int32_t *ninexact,
                          int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out,
                          int32_t **dnlen_out, uint64_t **dnlimbs_out, int64_t *dnnl_out,
                          int32_t **elen_out, uint64_t **elimbs_out, int64_t *enl_out, void *stream);
int slip_hip_factor_step_bounded_ms(const slip_hip_factor *f, double out[4]);
int slip_hip_factor_step_bounded_paths(const slip_hip_factor *f, int64_t out[20]);
int slip_hip_step_bounded_ms(double out[4]);
int slip_hip_step_bounded_paths(int64_t out[20]);

void slip_hip_factor_destroy(slip_hip_factor *f);
/* Device buffers of destroyed handles are kept in a process-level pool for the next handle (the drop-in SLIP_LU_factorize
 * creates and destroys one per call): at most SLIP_HIP_POOL_MB megabytes (environment, default 32768; 0 = no pool).  This
 * gives them all back to the runtime. */
void slip_hip_pool_release(void);

/* Triplet files <-> limb slabs, host only.  read: what SLIP_tripread + SLIP_build_sparse_trip_mpz
 * produce (SLIP_LU/Demo/demos.c:245-331, SLIP_LU/Source/slip_trip_to_mat.c:23-69: "m n nz" then nz lines "i j value",
 * indices 1-based unless the first entry holds a 0, columns by counting sort in file order, duplicates kept), as the
 * arrays slip_hip_factor_create takes; they are malloc'ed, release with slip_hip_free.  Malformed input is
 * SLIP_HIP_INCORRECT_INPUT as in the reference.  write: the inverse (1-based, decimal), readable by either. */
int slip_hip_read_triplet(const char *path, int32_t *n_out, int64_t **Ap, int32_t **Ai, int32_t **Alen, uint64_t **Alimbs,
                          int64_t *nlimbs_out);
int slip_hip_write_triplet(const char *path, int32_t n, const int64_t *Ap, const int32_t *Ai, const int32_t *Alen,
                           const uint64_t *Alimbs);

/* Deterministic synthetic CSC generator of the benchmark configs
 * (slip_matgen.h): arrays are malloc'ed, release with slip_hip_free. */
int slip_hip_matgen(int32_t n, double density, int32_t bits, uint64_t seed,
                    int64_t **Ap, int32_t **Ai, int64_t **Ax);
void slip_hip_free(void *p);

/* Wave-level limb kernels (wave_bigint.h) run in isolation on the device, one
 * wavefront per operation, for the parity unit tests.  Operands are arrays of
 * 32-bit digits.  op: 0 = low product a*b mod B^W, 1 = a+b mod B^W,
 * 2 = a-b mod B^W, 3 = inverse of odd a modulo B^W (b unused); 10..13 = the same four
 * on the register-resident primitives (wave_bigint_reg.h, W <= 256), 14 = a >> lb bits.
 * out receives nops*W digits. */
int slip_hip_wave_op_test(int32_t op, int32_t nops, int32_t la, int32_t lb, int32_t W,
                          const uint32_t *a, const uint32_t *b, uint32_t *out);

/* Diagnostics builds (slip_lu_amd/csrc/Makefile: `make prof`, `make cprof`) only: shader cycles thread 0 of every worker
 * spent per phase of its columns during the last run (summed over the workers; `cprof`: the committer's phase times);
 * all zero in the product build. */
int slip_hip_factor_phase_cycles(const slip_hip_factor *f, unsigned long long *out24);   /* 24 slots */

const char *slip_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SLIP_HIP_H */
