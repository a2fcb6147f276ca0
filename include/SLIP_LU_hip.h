/* SLIP_LU_hip.h -- the GMP-typed drop-in of the hot path (libslip_lu_hip.so).
 *
 * Exports the reference's own entry point
 *
 *     SLIP_info SLIP_LU_factorize(SLIP_sparse *L, SLIP_sparse *U, SLIP_sparse *A,
 *                                 SLIP_LU_analysis *S, mpz_t *rhos, int32_t *pinv,
 *                                 SLIP_options *option);
 *
 * with the prototype, argument meaning, ownership and error codes of
 * cjh10644/SLIP_LU, SLIP_LU/Include/SLIP_LU.h:854-863 (implementation replaced:
 * SLIP_LU/Source/SLIP_LU_factorize.c:36-314).  A program built against the
 * reference's SLIP_LU.h needs NO source change: link libslip_lu_hip.so ahead of
 * (or instead of the SLIP_LU_factorize.o inside) the reference library; every
 * other SLIP_* symbol keeps coming from the reference.  See INTEGRATION.md.
 *
 * The same function is also exported as SLIP_hip_LU_factorize, for processes
 * that load both libraries and want to call either explicitly (the tests do).
 *
 * SLIP_LU_solve (SLIP_LU.h:941-949) is served the same way (SLIP_hip_LU_solve below), and so is SLIP_solve_double of the
 * simple interface (SLIP_hip_solve_double below), which never leaves the device between the factorisation and the doubles,
 * and SLIP_solve_mpq (SLIP_hip_solve_mpq below), which brings back nothing but the reduced fractions, and SLIP_solve_mpfr
 * (SLIP_hip_solve_mpfr below; declared once mpfr.h is in scope: define SLIP_HAVE_MPFR or include mpfr.h / SLIP_LU.h first),
 * which brings back nothing but the rounded mantissas.
 *
 * When the reference's SLIP_LU.h has been included first, this header only adds
 * the aliases; otherwise it declares layout-compatible mirrors of the four types
 * the call touches (SLIP_LU.h:160-168 SLIP_info, :212-223 SLIP_options,
 * :246-256 SLIP_sparse, :308-316 SLIP_LU_analysis).
 */
#ifndef SLIP_LU_HIP_H
#define SLIP_LU_HIP_H

#include <stdint.h>
#include <gmp.h>
#if defined(SLIP_HAVE_MPFR) && !defined(MPFR_VERSION)
#include <mpfr.h>                /* SLIP_hip_solve_mpfr below: only where mpfr.h is available (the reference's header includes it) */
#endif

#ifdef __cplusplus
extern "C" {
#endif

#ifndef SLIP_LU_VERSION          /* the reference's header is not in scope */
typedef enum {
    SLIP_OK = 0, SLIP_OUT_OF_MEMORY = -1, SLIP_SINGULAR = -2,
    SLIP_INCORRECT_INPUT = -3, SLIP_INCORRECT = -4
} SLIP_info;

typedef struct SLIP_options {
    int32_t pivot;               /* SLIP_pivot: 0 smallest .. 3 tol-smallest (default) .. 5 largest */
    int32_t order;               /* SLIP_col_order (used by SLIP_LU_analyze only) */
    double  tol;
    int32_t print_level;
    uint64_t prec;
    int32_t SLIP_MPFR_ROUND;     /* mpfr_rnd_t */
} SLIP_options;

typedef struct {
    int32_t m, n, nzmax, nz;
    int32_t *p, *i;
    mpz_t *x;
    mpq_t scale;
} SLIP_sparse;

typedef struct {
    int32_t *q;
    int32_t lnz, unz;
} SLIP_LU_analysis;

typedef struct {                 /* SLIP_LU.h:277-284 */
    int32_t m, n;
    mpz_t **x;                   /* x[i][k]: row i of right-hand side k */
    mpq_t scale;
} SLIP_dense;

SLIP_info SLIP_LU_solve(mpq_t **x, SLIP_dense *b, const mpz_t *rhos, const SLIP_sparse *L,
                        const SLIP_sparse *U, const int32_t *pinv);

SLIP_info SLIP_LU_factorize(SLIP_sparse *L, SLIP_sparse *U, SLIP_sparse *A, SLIP_LU_analysis *S,
                            mpz_t *rhos, int32_t *pinv, SLIP_options *option);

SLIP_info SLIP_solve_double(double **x_doub, SLIP_sparse *A, SLIP_LU_analysis *S, SLIP_dense *b, SLIP_options *option);

SLIP_info SLIP_solve_mpq(mpq_t **x_mpq, SLIP_sparse *A, SLIP_LU_analysis *S, SLIP_dense *b, SLIP_options *option);

#ifdef MPFR_VERSION
SLIP_info SLIP_solve_mpfr(mpfr_t **x_mpfr, SLIP_sparse *A, SLIP_LU_analysis *S, SLIP_dense *b, SLIP_options *option);
#endif
#endif

SLIP_info SLIP_hip_LU_factorize(SLIP_sparse *L, SLIP_sparse *U, SLIP_sparse *A, SLIP_LU_analysis *S,
                                mpz_t *rhos, int32_t *pinv, SLIP_options *option);

/* SLIP_LU_solve (SLIP_LU.h:941-949; SLIP_LU_solve.c:41-86) on the GPU: forward substitution, scaling by
 * det = rhos[n-1] and back substitution run in slip_hip_factor_solve on the uploaded L, U; the rational
 * x = b2/det is formed on the host exactly as slip_array_div.c does.  Same arguments, ownership and
 * error codes as the reference; also exported under the reference's own name. */
SLIP_info SLIP_hip_LU_solve(mpq_t **x, SLIP_dense *b, const mpz_t *rhos, const SLIP_sparse *L,
                            const SLIP_sparse *U, const int32_t *pinv);

/* SLIP_solve_double (SLIP_LU/Source/SLIP_solve_double.c:41-104) on the GPU, with its prototype, argument checks (:53-57) and
 * error codes: factorisation, substitution, SLIP_permute_x, SLIP_scale_x (times A->scale, over b->scale, a scale of 1 or 0
 * left out as SLIP_scale_x.c:29-31, :43-45 do) and SLIP_get_double_soln all run on the device (slip_hip_factor_solve_double):
 * x_doub[i][j], allocated by the caller (n rows of b->n doubles), receives entry i of the solution of right-hand side j, the
 * exact rational truncated toward zero as mpq_get_d returns it.  Only those doubles cross back: no L, U, rhos or numerator
 * is downloaded.  Also exported under the reference's own name. */
SLIP_info SLIP_hip_solve_double(double **x_doub, SLIP_sparse *A, SLIP_LU_analysis *S, SLIP_dense *b, SLIP_options *option);

/* SLIP_solve_mpq (SLIP_LU/Source/SLIP_solve_mpq.c:41-97) on the GPU, with its prototype, argument checks (:51-55) and error
 * codes: factorisation, substitution, the division by det (slip_array_div.c:36-49), SLIP_permute_x and SLIP_scale_x (as above)
 * all run on the device (slip_hip_factor_solve_rational).  x_mpq[i][j] (n rows of b->n mpq_t, initialised, as
 * SLIP_create_mpq_mat leaves them) receives entry i of the solution of right-hand side j in GMP's canonical form: lowest
 * terms, a positive denominator, 0 as 0/1 -- what the reference's mpq_* calls leave.  Only the reduced numerators and
 * denominators cross back and are copied into the mpq_t limb by limb; no GMP arithmetic runs per entry.  Also exported under
 * the reference's own name. */
SLIP_info SLIP_hip_solve_mpq(mpq_t **x_mpq, SLIP_sparse *A, SLIP_LU_analysis *S, SLIP_dense *b, SLIP_options *option);

#ifdef MPFR_VERSION
/* SLIP_solve_mpfr (SLIP_LU/Source/SLIP_solve_mpfr.c:40-104) on the GPU, with its prototype, argument checks (:52-56) and error
 * codes: factorisation, substitution, SLIP_permute_x, SLIP_scale_x (as above) and SLIP_get_mpfr_soln (mpfr_set_q per entry,
 * under option->SLIP_MPFR_ROUND) all run on the device (slip_hip_factor_solve_mpfr).  x_mpfr[i][j] (n rows of b->n mpfr_t,
 * initialised by the caller -- SLIP_create_mpfr_mat gives every entry option->prec bits) receives entry i of the solution of
 * right-hand side j: the exact rational rounded ONCE to the precision the entries carry, mpfr_get_prec(x_mpfr[0][0]), from 2
 * to 65536 bits.  A difference from the reference: entries of differing precisions are SLIP_INCORRECT_INPUT (the reference
 * rounds each entry to its own).  Only sign, exponent and mantissa limbs cross back; every mpfr_t is filled through MPFR's
 * public interface (mpz_roinit_n, mpfr_set_z_2exp -- exact -- and mpfr_set_zero).  Also exported under the reference's own
 * name.  Present in libslip_lu_hip.so when it was built where mpfr.h is available. */
SLIP_info SLIP_hip_solve_mpfr(mpfr_t **x_mpfr, SLIP_sparse *A, SLIP_LU_analysis *S, SLIP_dense *b, SLIP_options *option);
#endif

#ifdef __cplusplus
}
#endif
#endif /* SLIP_LU_HIP_H */
