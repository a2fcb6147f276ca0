/* slip_hip.hip -- libslip_hip.so: kernels' entry points and the host side of the
 * C ABI declared in include/slip_hip.h.
 *
 * Host responsibilities (the part of SLIP_LU/Source/SLIP_LU_factorize.c:58-211
 * that is not arithmetic): validate, upload A and q once, size the workers'
 * private scatter vectors and the shared L / U slabs in HBM, launch the grid of
 * column workers (ref_lu_pipe.h), and grow a buffer and relaunch from the first
 * uncommitted column when the kernel asks (the reference doubles L/U at
 * :200-211 and lets GMP realloc x).
 *
 * Built by hipcc for gfx950.  With -DSLIP_EMULATE (tests/emu, g++) the same
 * source runs the kernel lane-by-lane on the CPU for unit tests; that build is
 * never the product.
 */
#include "ref_lu_pipe.h"
#include "slip_matgen.h"
#include "../../include/slip_hip.h"

#ifdef SLIP_EMULATE
#include "hip_rt_emu.h"
#endif

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>
#include <functional>

#define SLIP_LDS_MAX_WORDS 40000          /* of the 40960 words (160 KiB) per CU */
#define SLIP_BITMAP_LDS_MAX_WORDS 16384   /* n <= 524288 keeps the pattern bitmap in LDS */

/* ------------------------------------------------------------------ */
/* kernels                                                             */
/* ------------------------------------------------------------------ */
/* register-resident primitives (wave_bigint_reg.h) for the unit tests: op 10 product, 11 add, 12 sub,
 * 13 inverse of odd a, 14 a >> lb (lb = shift in bits), 15 a / b for odd b (Hensel); all modulo B^W, W <= 256 */
template <int D> SLIP_DEV void slip_reg_op_test_d(int op, const uint32_t *A, int la, const uint32_t *B, int lb, int W,
                                                   uint32_t *O, uint32_t *scratch)
{
    WR<D> a = wr_load<D>(A, la < W ? la : W), r;
    if (op == 14) r = wr_shr<D>(a, lb, scratch);
    else if (op == 13) r = wr_inv_extend<D>(wr_zero<D>(), 0, W, a);
    else {
        WR<D> b = wr_load<D>(B, lb < W ? lb : W);
        const int ea = la < W ? la : W, eb = lb < W ? lb : W;
        if (op == 10) r = ea <= eb ? wr_mul<D>(a, ea, b) : wr_mul<D>(b, eb, a);
        else if (op == 15) r = wr_div_hensel<D>(a, W, b);
        else r = wr_addsub<D>(a, b, op == 12);
    }
    wr_store<D>(O, r, W);
}
SLIP_DEV void slip_reg_op_test(int op, const uint32_t *A, int la, const uint32_t *B, int lb, int W, uint32_t *O, uint32_t *scratch)
{
    if (op >= 20) {                                   /* raw cross-lane primitives: W must be 64 */
        const int lane = slip_lane();
        const uint32_t v = A[lane];
        uint32_t r = 0;
        if (op == 24) r = slip_wave_sum_u32(v);
        else if (op == 25) r = slip_wave_max_u32(v);
        else if (op == 26) r = slip_wave_min_u32(v);
        else if (op == 27) r = slip_bcast0_u32(v);
        else if (op == 20) r = slip_dpp_shr1(v, 0xAAAAu);
        else if (op == 21) r = slip_dpp_shl1(v, 0xBBBBu);
        else if (op == 22) r = slip_readlane(v, lb);
        else if (op == 23) r = slip_shfl_up_u32(v, 1);
        O[lane] = r;
        return;
    }
    const int D = (W + 63) >> 6;
    if (D <= 1) slip_reg_op_test_d<1>(op, A, la, B, lb, W, O, scratch);
    else if (D == 2) slip_reg_op_test_d<2>(op, A, la, B, lb, W, O, scratch);
    else if (D == 3) slip_reg_op_test_d<3>(op, A, la, B, lb, W, O, scratch);
    else slip_reg_op_test_d<4>(op, A, la, B, lb, W, O, scratch);
}

/* a worker's view of the parameters: the private arrays start at this workgroup's share */
SLIP_DEV void slip_worker_params(SlipParams *Pw, const SlipParams &P, int worker)
{
    *Pw = P;
    Pw->worker = worker;
    Pw->xrow = P.xrow + (int64_t) worker * P.priv_rows;
    Pw->xd = P.xd + (int64_t) worker * P.priv_rows * P.xcap;
    Pw->pat = P.pat + (int64_t) worker * P.priv_rows;
    Pw->rlist = P.rlist + (int64_t) worker * P.priv_rows;
    Pw->rpos = P.rpos + (int64_t) worker * P.priv_rows;
    Pw->srow = P.srow + (int64_t) worker * P.priv_rows;
    Pw->gbitmap = P.gbitmap + (int64_t) worker * (P.bitmap_in_lds ? 0 : P.bm_words + 64);
    Pw->gscratch = P.gscratch + (int64_t) worker * (P.scratch_in_lds ? 0 : (int64_t) SLIP_SCRATCH_WAVES * 3 * P.wcap);
}

/* the last worker to leave records where the factorisation stands (the host reads the state once) */
SLIP_DEV void slip_worker_exit(const SlipParams &P, SlipState *st)
{
    slip_block_sync();
    if (slip_tid() == 0) {
        if (slip_agent_add_i32(&st->exited, 1) == P.nworkers - 1) {
            int pr_; const int F = slip_ld_frontier(st, &pr_);
            st->k_next = F;
            st->Lnz = slip_ld_i64(&P.Lp[F]); st->Lnl = slip_ld_i64(&P.Lo[F]);
            st->Unz = slip_ld_i64(&P.Up[F]); st->Unl = slip_ld_i64(&P.Uo[F]);
        }
    }
}

/* Subtree farm: rescale a block's factors by the pivots the OTHER blocks produced meanwhile.
 * One wavefront per stored entry: out = entry * scale[s], s = the entry's column (L) or the pivot position of its
 * row (U).  Entries are written into new slabs at offsets the host laid out from the operands' lengths. */
struct SlipRescaleArgs {
    const SlipEnt *ent; const uint64_t *limbs; const int32_t *idx; int64_t nz;     /* source entries; idx: row ids */
    const int64_t *colp; int32_t ncols;                                            /* L: column pointers (scale = column); U: null */
    const int32_t *pinv;                                                           /* U: scale = pinv[row]                          */
    const int32_t *slen; const int64_t *soff; const uint64_t *slimbs;              /* scales: signed digit counts, limb offsets      */
    SlipEnt *oent; uint64_t *olimbs;                                               /* destination (oent[e].off set by the host)     */
    int64_t *pividx; const int32_t *row_perm;                                      /* L: which entry of column k is the pivot         */
};

template <int D> SLIP_DEV void slip_rescale_entry_reg(const dig_t *a, int la, const dig_t *b, int lb, dig_t *out, int W, int *len_out, uint32_t *top_out)
{
    WR<D> A = wr_load<D>(a, la), B = wr_load<D>(b, lb);
    WR<D> Y = la <= lb ? wr_mul<D>(A, la, B) : wr_mul<D>(B, lb, A);
    const int len = wr_len<D>(Y);
    wr_store<D>(out, Y, (len + 1) & ~1);
    (void) W;
    *len_out = len; *top_out = len ? wr_digit<D>(Y, len - 1) : 0u;
}

/* out = a * b, written as whole limbs (la + lb digits rounded up to even; nothing is written for la == 0): registers up to
 * 256 digits, wb_mul_lo above.  *len_out = the product's significant digits, *top_out = the highest of them. */
SLIP_DEV void slip_mul_entry(const dig_t *a, int la, const dig_t *b, int lb, dig_t *out, int *len_out, uint32_t *top_out)
{
    int len = 0; uint32_t top = 0;
    if (la != 0) {
        const int W = la + lb;
        if (W <= 64) slip_rescale_entry_reg<1>(a, la, b, lb, out, W, &len, &top);
        else if (W <= 128) slip_rescale_entry_reg<2>(a, la, b, lb, out, W, &len, &top);
        else if (W <= 192) slip_rescale_entry_reg<3>(a, la, b, lb, out, W, &len, &top);
        else if (W <= 256) slip_rescale_entry_reg<4>(a, la, b, lb, out, W, &len, &top);
        else {
            const int Wp = (W + 1) & ~1;
            wb_mul_lo(out, a, la, b, lb, Wp);
            len = wb_len(out, Wp);
            top = len ? out[len - 1] : 0u;
        }
    }
    *len_out = len; *top_out = top;
}

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_rescale_kernel(SlipRescaleArgs A)
#else
static void slip_rescale_body(SlipRescaleArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    for (int64_t e = wave0; e < A.nz; e += nwaves) {
        const SlipEnt en = A.ent[e];
        const int row = A.idx[e];
        int sidx;
        if (A.colp) {                       /* column of entry e: binary search over the column pointers */
            int lo = 0, hi = A.ncols - 1;
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (A.colp[mid] <= e) lo = mid; else hi = mid - 1; }
            sidx = lo;
        } else sidx = A.pinv[row];
        const int32_t sl = A.slen[sidx];
        const dig_t *a = (const dig_t *)(A.limbs + en.off), *b = (const dig_t *)(A.slimbs + A.soff[sidx]);
        const int la = slip_abs(en.len), lb = slip_abs(sl);
        SlipEnt o = A.oent[e];
        dig_t *out = (dig_t *)(A.olimbs + o.off);
        int len = 0; uint32_t top = 0;
        slip_mul_entry(a, la, b, lb, out, &len, &top);
        if (lane == 0) {
            o.len = (slip_sgn(en.len) * slip_sgn(sl)) < 0 ? -len : len;
            o.bits = len ? 32 * len - slip_clz32(top) : 0;
            A.oent[e] = o;
            if (A.colp && A.row_perm[sidx] == row) A.pividx[sidx] = e;
        }
    }
}

/* Exact solution check (slip_hip_factor_check, slip_hip_check_solution): the integer form of SLIP_check_solution
 * (SLIP_check_solution.c:31-113).  With x_c = xnum_c / d_c over one common denominator the test is
 *     r_i = sum_e A(i, j_e) * xnum_c[x(e)]  -  d_c * b_c[i]  == 0      for every row i and right-hand side c,
 * a sparse big-integer product over a row-ordered view of A (rp: row pointer; re: CSC entry of each term; rx: the index of
 * x it multiplies).  One wavefront per (row, right-hand side), grid-stride; everything in the loop is wave-uniform.
 *
 * Why a fixed-width sum is an exact test: the (row, rhs) picks W = max(max_e(|a_e| + |x_e|), |d| + |b_i|) + 1 digits from
 * the ACTUAL operand lengths.  Every term is below B^(W-1) in magnitude and a row has fewer than 2^24 terms (n < 2^24 - 1,
 * duplicates removed, plus the d*b term), so |r_i| < 2^24 * B^(W-1) < B^W.  The sum is formed modulo B^M for some M >= W
 * (M = 64*D on the register path, M = W on the memory path), a ring homomorphism: the accumulator holds r_i mod B^M, and
 * since |r_i| < B^M that is all zero digits exactly when r_i = 0.  No sign or overflow is ever tracked. */
struct SlipCheckArgs {
    int32_t n, nrhs;
    const int64_t *rp, *re; const int32_t *rx;                                     /* row view of A                          */
    const int32_t *alen; const int64_t *aoff; const uint64_t *alimbs;              /* A: signed digit counts, limb offsets   */
    const int32_t *xlen; const int64_t *xoff; const uint64_t *xlimbs;              /* x: entry c*n + x(e)                    */
    const int32_t *blen; const int64_t *boff; const uint64_t *blimbs;              /* b: entry c*n + i                       */
    const int32_t *dlen; const int64_t *doff; const uint64_t *dlimbs;              /* d_c: entry c                           */
    int32_t *first_bad, *nbad;                                                     /* per right-hand side                    */
    dig_t *scratch; int32_t wcap;                                                  /* memory path: 2 * wcap digits per wave  */
};

/* x * B modulo B^(64*D): every digit one lane up, lane 63 of a chunk into lane 0 of the next */
template <int D> SLIP_DEV WR<D> wr_shl_digit(const WR<D> &x)
{
    WR<D> out;
#pragma unroll
    for (int r = D - 1; r >= 0; r--) out.d[r] = slip_dpp_shr1_in(x.d[r], r > 0 ? slip_readlane(x.d[r - 1], 63) : 0u);
    return out;
}

/* acc +/- a * y modulo B^(64*D), la, ly >= 1; a of one or two digits (nearly every entry of A) takes one-digit products */
template <int D> SLIP_DEV WR<D> slip_check_mac_reg(WR<D> acc, const dig_t *a, int la, const dig_t *y, int ly, int sub)
{
    const WR<D> Y = wr_load<D>(y, ly);
    if (la == 1) return wr_addsub<D>(acc, wr_mul_digit<D>(a[0], Y), sub);
    if (la == 2) {
        WR<D> p0, p1;
        wr_mul_digit2<D>(a[0], a[1], Y, p0, p1);
        return wr_addsub<D>(wr_addsub<D>(acc, p0, sub), wr_shl_digit<D>(p1), sub);
    }
    const WR<D> Av = wr_load<D>(a, la);
    return wr_addsub<D>(acc, la <= ly ? wr_mul<D>(Av, la, Y) : wr_mul<D>(Y, ly, Av), sub);
}

/* The sums below are shared by slip_check_kernel and slip_product_kernel (Args: SlipCheckArgs or SlipProductArgs; xb: the
 * vector's first entry of x; bi: the entry of b, negative for none). */

/* the width of one (row, vector), from the operands' own lengths: W = max(max_e(|a_e| + |x_e|), |d| + |b_i|) + 1 */
template <class Args> SLIP_DEV int slip_row_width(const Args &A, int64_t xb, int64_t bi, int c, int64_t r0, int64_t r1)
{
    uint32_t w = 0;
    for (int64_t t = r0 + slip_lane(); t < r1; t += SLIP_WAVE) {
        const uint32_t s = (uint32_t)(slip_abs(A.alen[A.re[t]]) + slip_abs(A.xlen[xb + A.rx[t]]));
        if (s > w) w = s;
    }
    w = slip_wave_max_u32(w);
    const uint32_t wdb = bi >= 0 ? (uint32_t)(slip_abs(A.dlen[c]) + slip_abs(A.blen[bi])) : 0u;
    return (int)(w > wdb ? w : wdb) + 1;
}

/* r_i modulo B^(64*D): register path, W <= 64*D */
template <int D, class Args> SLIP_DEV WR<D> slip_row_sum_reg(const Args &A, int64_t xb, int64_t bi, int c, int64_t r0, int64_t r1)
{
    WR<D> acc = wr_zero<D>();
    for (int64_t t = r0; t < r1; t++) {
        const int64_t e = A.re[t], xe = xb + A.rx[t];
        const int32_t sa = A.alen[e], sx = A.xlen[xe];
        if (sa == 0 || sx == 0) continue;
        acc = slip_check_mac_reg<D>(acc, (const dig_t *)(A.alimbs + A.aoff[e]), slip_abs(sa),
                                    (const dig_t *)(A.xlimbs + A.xoff[xe]), slip_abs(sx), (sa < 0) != (sx < 0));
    }
    if (bi < 0) return acc;
    const int32_t sd = A.dlen[c], sb = A.blen[bi];
    if (sd != 0 && sb != 0) {
        const dig_t *d = (const dig_t *)(A.dlimbs + A.doff[c]), *b = (const dig_t *)(A.blimbs + A.boff[bi]);
        const int ld = slip_abs(sd), lb = slip_abs(sb), sub = (sd < 0) == (sb < 0);     /* acc -= d*b */
        acc = lb <= ld ? slip_check_mac_reg<D>(acc, b, lb, d, ld, sub) : slip_check_mac_reg<D>(acc, d, ld, b, lb, sub);
    }
    return acc;
}

/* the same modulo B^W on W-digit buffers in global memory (acc: the sum; prod: this wave's scratch) */
template <class Args> SLIP_DEV void slip_row_sum_wide(const Args &A, int64_t xb, int64_t bi, int c, int64_t r0, int64_t r1, int W,
                                                      dig_t *acc, dig_t *prod)
{
    for (int k = slip_lane(); k < W; k += SLIP_WAVE) acc[k] = 0u;
    slip_wave_sync();
    for (int64_t t = r0; t < r1; t++) {
        const int64_t e = A.re[t], xe = xb + A.rx[t];
        const int32_t sa = A.alen[e], sx = A.xlen[xe];
        if (sa == 0 || sx == 0) continue;
        wb_mul_lo(prod, (const dig_t *)(A.alimbs + A.aoff[e]), slip_abs(sa), (const dig_t *)(A.xlimbs + A.xoff[xe]), slip_abs(sx), W);
        wb_addsub(acc, acc, W, prod, W, W, (sa < 0) != (sx < 0));
    }
    if (bi < 0) return;
    const int32_t sd = A.dlen[c], sb = A.blen[bi];
    if (sd != 0 && sb != 0) {
        wb_mul_lo(prod, (const dig_t *)(A.dlimbs + A.doff[c]), slip_abs(sd), (const dig_t *)(A.blimbs + A.boff[bi]), slip_abs(sb), W);
        wb_addsub(acc, acc, W, prod, W, W, (sd < 0) == (sb < 0));
    }
}

/* nonzero when r_i != 0: register path, W <= 64*D */
template <int D> SLIP_DEV int slip_check_row_reg(const SlipCheckArgs &A, int64_t xb, int64_t bi, int c, int64_t r0, int64_t r1)
{
    return wr_len<D>(slip_row_sum_reg<D>(A, xb, bi, c, r0, r1)) != 0;
}

/* the same on the memory path (acc, prod: this wave's scratch) */
SLIP_DEV int slip_check_row_wide(const SlipCheckArgs &A, int64_t xb, int64_t bi, int c, int64_t r0, int64_t r1, int W,
                                 dig_t *acc, dig_t *prod)
{
    slip_row_sum_wide(A, xb, bi, c, r0, r1, W, acc, prod);
    return wb_len(acc, W) != 0;
}

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_check_kernel(SlipCheckArgs A)
#else
static void slip_check_body(SlipCheckArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    dig_t *acc = A.scratch ? A.scratch + wave0 * 2 * A.wcap : (dig_t *) 0, *prod = acc ? acc + A.wcap : (dig_t *) 0;
    const int64_t items = (int64_t) A.n * A.nrhs;
    for (int64_t it = wave0; it < items; it += nwaves) {
        const int c = (int)(it / A.n), i = (int)(it - (int64_t) c * A.n);
        const int64_t xb = (int64_t) c * A.n, bi = xb + i, r0 = A.rp[i], r1 = A.rp[i + 1];
        const int W = slip_row_width(A, xb, bi, c, r0, r1);
        int bad;
        if (W <= 64) bad = slip_check_row_reg<1>(A, xb, bi, c, r0, r1);
        else if (W <= 128) bad = slip_check_row_reg<2>(A, xb, bi, c, r0, r1);
        else if (W <= 192) bad = slip_check_row_reg<3>(A, xb, bi, c, r0, r1);
        else if (W <= 256) bad = slip_check_row_reg<4>(A, xb, bi, c, r0, r1);
        else bad = slip_check_row_wide(A, xb, bi, c, r0, r1, W, acc, prod);      /* W <= wcap: the host sized it */
        if (bad && lane == 0) {
            slip_atomic_min_i32(&A.first_bad[c], i);
            slip_atomic_add_i32(&A.nbad[c], 1);
        }
    }
}

/* Exact sparse product (slip_hip_factor_multiply, slip_hip_matrix_multiply): the residual of the check, kept.
 *     r_i = sum_e A(i, j_e) * x_c[x(e)]  -  d_c * b_c[i]        (blen == NULL: the product alone)
 * over the same kind of view and operand records as SlipCheckArgs, except that the output rows (nout) and the entries of one
 * vector of x (nx) need not be as many: the view may be that of a rectangular matrix.  One wavefront per (row, vector),
 * grid-stride, wave-uniform.
 *
 * The sign: |r_i| < 2^24 * B^(W-1) < B^W / 2 by the check's bound on the terms of a row, so the sum modulo B^M, M >= W, is
 * r_i in two's complement: the top bit of digit M-1 is its sign, and 0 - acc its magnitude when that bit is set.
 *
 * phase 0 writes W per item (wlen); the host lays the staging slab out from it (slip_offscan_kernel: an item owns
 * (W + 1) / 2 limbs at soff) and phase 1 leaves the magnitude there in whole limbs and the signed digit count in rlen.  On
 * the memory path (W > 256) the sum is formed in the item's own staging region, M = its (W + 1) & ~1 digits, and only the
 * product of a term lives in the wave's scratch (wcap digits, wcap even). */
struct SlipProductArgs {
    int32_t nout, nx, nvec, phase;
    const int64_t *rp, *re; const int32_t *rx;                                     /* view of A: nout rows                   */
    const int32_t *alen; const int64_t *aoff; const uint64_t *alimbs;              /* A: signed digit counts, limb offsets   */
    const int32_t *xlen; const int64_t *xoff; const uint64_t *xlimbs;              /* x: entry c*nx + x(e)                   */
    const int32_t *blen; const int64_t *boff; const uint64_t *blimbs;              /* b: entry c*nout + i, or NULL           */
    const int32_t *dlen; const int64_t *doff; const uint64_t *dlimbs;              /* d_c: entry c (with b)                  */
    int32_t *wlen;                                                                 /* W per item                             */
    const int64_t *soff; uint64_t *stage; int32_t *rlen;                           /* phase 1: staging slab, signed digits   */
    dig_t *scratch; int32_t wcap;                                                  /* memory path: wcap digits per wave      */
};

/* the sum of one item on the register path, W <= 64*D: its signed digit count; the magnitude goes to out in whole limbs */
template <int D> SLIP_DEV int slip_product_row_reg(const SlipProductArgs &A, int64_t xb, int64_t bi, int c, int64_t r0, int64_t r1, dig_t *out)
{
    WR<D> acc = slip_row_sum_reg<D>(A, xb, bi, c, r0, r1);
    const int neg = (int)(wr_digit<D>(acc, 64 * D - 1) >> 31);
    if (neg) acc = wr_addsub<D>(wr_zero<D>(), acc, 1);
    const int len = wr_len<D>(acc);
    wr_store<D>(out, acc, (len + 1) & ~1);
    return neg ? -len : len;
}

/* the same on the memory path: the sum is formed in out, Wp = (W + 1) & ~1 digits */
SLIP_DEV int slip_product_row_wide(const SlipProductArgs &A, int64_t xb, int64_t bi, int c, int64_t r0, int64_t r1, int Wp,
                                   dig_t *out, dig_t *prod)
{
    slip_row_sum_wide(A, xb, bi, c, r0, r1, Wp, out, prod);
    const int neg = (int)(out[Wp - 1] >> 31);
    if (neg) wb_addsub(out, (const dig_t *) 0, 1, out, Wp, Wp, 1, 0u);
    const int len = wb_len(out, Wp);
    return neg ? -len : len;
}

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_product_kernel(SlipProductArgs A)
#else
static void slip_product_body(SlipProductArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    dig_t *prod = A.scratch ? A.scratch + wave0 * A.wcap : (dig_t *) 0;
    const int64_t items = (int64_t) A.nout * A.nvec;
    for (int64_t it = wave0; it < items; it += nwaves) {
        const int c = (int)(it / A.nout), i = (int)(it - (int64_t) c * A.nout);
        const int64_t xb = (int64_t) c * A.nx, bi = A.blen ? it : -1, r0 = A.rp[i], r1 = A.rp[i + 1];
        if (A.phase == 0) {
            const int W = slip_row_width(A, xb, bi, c, r0, r1);
            if (lane == 0) A.wlen[it] = W;
            continue;
        }
        const int W = A.wlen[it];
        dig_t *out = (dig_t *)(A.stage + A.soff[it]);
        int len;
        if (W <= 64) len = slip_product_row_reg<1>(A, xb, bi, c, r0, r1, out);
        else if (W <= 128) len = slip_product_row_reg<2>(A, xb, bi, c, r0, r1, out);
        else if (W <= 192) len = slip_product_row_reg<3>(A, xb, bi, c, r0, r1, out);
        else if (W <= 256) len = slip_product_row_reg<4>(A, xb, bi, c, r0, r1, out);
        else len = slip_product_row_wide(A, xb, bi, c, r0, r1, (W + 1) & ~1, out, prod);     /* at most wcap: the host sized it */
        if (lane == 0) A.rlen[it] = len;
    }
}

/* A scale applied to a solution before it is converted (slip_hip_factor_solve_double): out[t] = src[t] * s for one
 * multiplier s, one wavefront per entry, through slip_mul_entry (the product path of slip_rescale_kernel).  The host laid the
 * destination offsets out from the operands' lengths; the kernel writes the product's signed digit count. */
struct SlipScaleArgs {
    int64_t count;
    const int32_t *len; const int64_t *off; const uint64_t *limbs;                 /* source: signed digit counts, limb offsets */
    int32_t slen; const uint64_t *slimbs;                                          /* the multiplier: signed digit count        */
    int32_t *olen; const int64_t *ooff; uint64_t *olimbs;                          /* destination                               */
};

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_scale_kernel(SlipScaleArgs A)
#else
static void slip_scale_body(SlipScaleArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    for (int64_t e = wave0; e < A.count; e += nwaves) {
        const int32_t sa = A.len[e];
        int len = 0; uint32_t top = 0;
        slip_mul_entry((const dig_t *)(A.limbs + A.off[e]), slip_abs(sa), (const dig_t *) A.slimbs, slip_abs(A.slen),
                       (dig_t *)(A.olimbs + A.ooff[e]), &len, &top);
        if (lane == 0) A.olen[e] = (sa < 0) != (A.slen < 0) ? -len : len;
    }
}

/* Solution to doubles (slip_hip_factor_solve_double, slip_hip_solution_to_double): out = trunc(N / D) onto the double grid,
 * toward zero, for every numerator N of a solution over its right-hand side's denominator D -- bit for bit what mpq_get_d
 * returns (SLIP_get_double_soln -> SLIP_gmp.c:1063).  Magnitudes below; the sign is that of N * D, dropped when the result is 0.
 *
 * Lane pass, one lane per entry.  n64, d64: the leading 64 bits of N and D, left-aligned (bn, bd their bit lengths), so
 *     N * 2^(64-bn) in [n64, n64 + 1),   D * 2^(64-bd) in [d64, d64 + 1),   2^63 <= n64, d64 < 2^64.
 * k = 64 when n64 < d64, else 63; X = n64 * 2^k / d64 then lies in [2^63, 2^64) and Q = floor(X) is one 128-by-64 division.
 * T = (N / D) * 2^(k - bn + bd) is the true quotient on that scale, and
 *     T > n64 * 2^k / (d64 + 1) = X - X / (d64 + 1) > X - 2^64 / 2^63 = X - 2 >= Q - 2,
 *     T < (n64 + 1) * 2^k / d64 = X + 2^k / d64 <= X + 2 < Q + 3,
 * so floor(T) is one of Q-2 .. Q+2 (and equals Q when bn, bd <= 64: both leading parts are then the whole numbers).  The
 * double keeps the top 53 bits: r = 11 bits of T are dropped, more when the grid 2^G of the result, G = r - k + bn - bd,
 * would be finer than the subnormal spacing 2^-1074 (then r grows until G = -1074).  With m_lo = (Q-2) >> r and
 * m_hi = (Q+2) >> r the answer is trunc = m * 2^G for m = floor(T) >> r in [m_lo, m_hi].  If m_lo * 2^G and m_hi * 2^G are the
 * same double (slip_double_bits: also both +0.0, both inf) the lane stores it.  (T in [2^63, 2^64) is what makes 2^G the
 * double's own grid; Q-2 < 2^63 or Q+2 >= 2^64 leave the exponent open too, and slip_double_bits names the two candidates
 * of those cases: they are neighbouring doubles again.)
 *
 * Wave pass.  THE INVARIANT: r >= 11, so the five values Q-2 .. Q+2 cross at most one multiple of 2^r and m_hi - m_lo <= 1:
 * when the lane pass does not decide, the answer is m_hi * 2^G if m_hi * 2^G <= N / D and m_lo * 2^G = (m_hi - 1) * 2^G
 * otherwise -- two candidates, never more, and one exact comparison picks:  m_hi * 2^G * D <= N.  This is the case of every
 * quotient that lies ON the grid (integer and dyadic solutions: T is a multiple of 2^r, Q-2 is below it), where leading
 * bits alone would land one step low.  Undecided lanes are ballotted and the wave takes them one at a time: with
 * G = 32 * Gd + gb, 0 <= gb < 32, the product P = (m_hi << gb) * D is a three-digit by ld-digit wb_mul_lo into this wave's
 * scratch, and P * B^Gd <= N is a comparison of digit strings at an offset: no big shift is ever formed.
 *   Gd >= 0:  P <= floor(N / B^Gd), the digits of N from Gd up (false when N has none there, since P >= 1);
 *   Gd <  0:  P <= N * B^-Gd: true when P has at most -Gd digits (P * B^Gd < 1 <= N), else compare the digits of P from -Gd up
 *             with N; if those are equal, P <= N * B^-Gd exactly when the low -Gd digits of P are all zero.
 * The kernel never aborts: zero numerators give +0.0, a zero denominator (refused by the host) gives +0.0 as well. */
struct SlipToDoubleArgs {
    int32_t n, nrhs;
    const int32_t *xlen; const int64_t *xoff; const uint64_t *xlimbs;              /* N: entry c*n + p, signed digit counts, limb offsets */
    const int32_t *dlen; const int64_t *doff; const uint64_t *dlimbs;              /* D: one per right-hand side                         */
    const int32_t *oidx;                                                           /* entry p goes to out[c*n + oidx[p]]; null: to p     */
    int32_t flip;                                                                  /* negate every result (the sign of a scale)          */
    double *out;
    dig_t *scratch; int32_t wcap;                                                  /* wave pass: 4 + wcap digits per wave                */
    unsigned long long *nslow;                                                     /* entries that took the wave pass                     */
};

/* the leading 64 bits of a normalised la-digit number (la >= 1, top digit nonzero), left-aligned */
SLIP_DEV uint64_t slip_lead64(const dig_t *x, int la)
{
    const int z = slip_clz32(x[la - 1]);
    const uint64_t v = ((uint64_t) x[la - 1] << 32) | (la >= 2 ? x[la - 2] : 0u);
    return z ? (v << z) | ((uint64_t)(la >= 3 ? x[la - 3] : 0u) >> (32 - z)) : v;
}

/* floor((u1 * 2^64 + u0) / v) for u1 < v and v >= 2^63: Knuth's algorithm D in base 2^32, two quotient digits */
SLIP_DEV uint64_t slip_div128by64(uint64_t u1, uint64_t u0, uint64_t v)
{
    const uint64_t b = 1ull << 32, v1 = v >> 32, v0 = v & 0xFFFFFFFFull, u01 = u0 >> 32, u00 = u0 & 0xFFFFFFFFull;
    uint64_t q1 = u1 / v1, rh = u1 - q1 * v1;
    while (q1 >= b || q1 * v0 > b * rh + u01) { q1--; rh += v1; if (rh >= b) break; }
    const uint64_t u21 = u1 * b + u01 - q1 * v;
    uint64_t q0 = u21 / v1;
    rh = u21 - q0 * v1;
    while (q0 >= b || q0 * v0 > b * rh + u00) { q0--; rh += v1; if (rh >= b) break; }
    return q1 * b + q0;
}

/* the bits of the candidate double of mantissa m on the grid 2^G, 0 <= m <= 2^53, G >= -1074: m * 2^G, inf from 2^1024 on.
 * On a normal grid (G > -1074, so r = 11) m >= 2^52 except for the lower candidate m_lo = 2^52 - 1 of Q < 2^63 + 2: there T may
 * lie below 2^63, the double then has the next lower exponent and keeps one more bit of T, and T > 2^63 - 2 makes that
 * floor(T / 2^10) = 2^53 - 1 on the grid 2^(G-1): the double just below the upper candidate 2^52 * 2^G. */
SLIP_DEV uint64_t slip_double_bits(uint64_t m, int64_t G)
{
    if (m == 0) return 0;
    if (m >> 53) { m >>= 1; G++; }                                   /* 2^53 = 2^52 * 2 */
    if (m < (1ull << 52) && G > -1074) { m = 2 * m + 1; G--; }       /* m = 2^52 - 1 (see above): 2^53 - 1 on the finer grid */
    if (G == -1074) return m;                                        /* subnormals, and exponent field 1 when m >= 2^52 */
    if (G + 1075 >= 2047) return 0x7FF0000000000000ull;
    return ((uint64_t)(G + 1075) << 52) | (m - (1ull << 52));
}

/* number of significant digits of x[0..la) seen by one lane (records from the solve are normalised; this keeps any input safe) */
SLIP_DEV int slip_trim_digits(const dig_t *x, int la)
{
    while (la > 0 && x[la - 1] == 0) la--;
    return la;
}

/* the wave pass for entry `it` (all arguments wave-uniform): is m * 2^G * |D| <= |N| ? */
SLIP_DEV int slip_todouble_exact(const SlipToDoubleArgs &A, int64_t it, uint64_t m, int64_t G, dig_t *scr)
{
    const int lane = slip_lane();
    const int c = (int)(it / A.n);
    const dig_t *x = (const dig_t *)(A.xlimbs + A.xoff[it]), *d = (const dig_t *)(A.dlimbs + A.doff[c]);
    const int la = slip_trim_digits(x, slip_abs(A.xlen[it])), ld = slip_trim_digits(d, slip_abs(A.dlen[c]));
    const int gb = (int)(((G % 32) + 32) % 32);
    const int64_t Gd = (G - gb) / 32;
    const uint64_t mlo = m << gb, mtop = gb ? m >> (64 - gb) : 0;    /* m << gb: at most 54 + 31 bits, three digits */
    dig_t *md = scr, *P = scr + 4;
    if (lane < 4) md[lane] = lane == 0 ? (dig_t) mlo : (lane == 1 ? (dig_t)(mlo >> 32) : (lane == 2 ? (dig_t) mtop : 0u));
    slip_wave_sync();
    const int W = ld + 3 <= A.wcap ? ld + 3 : A.wcap;                /* ld + 3 <= wcap: the host sized it */
    wb_mul_lo(P, md, 3, d, ld, W);
    const int lp = wb_len(P, W);
    int ok;
    if (Gd >= 0) ok = Gd < la && wb_cmp(P, lp, x + Gd, la - (int) Gd) <= 0;
    else if (lp <= -Gd) ok = 1;
    else {
        const int k = (int) -Gd, cm = wb_cmp(P + k, lp - k, x, la);
        ok = cm < 0;
        if (cm == 0) {
            int low = 0;
            for (int base = 0; base < k; base += SLIP_WAVE) low |= slip_ballot(base + lane < k && P[base + lane] != 0) != 0;
            ok = !low;
        }
    }
    slip_wave_sync();
    return ok;
}

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_todouble_kernel(SlipToDoubleArgs A)
#else
static void slip_todouble_body(SlipToDoubleArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    dig_t *scr = A.scratch + wave0 * (4 + (int64_t) A.wcap);
    const int64_t items = (int64_t) A.n * A.nrhs;
    unsigned long long slow_total = 0;
    for (int64_t base = wave0 * SLIP_WAVE; base < items; base += nwaves * SLIP_WAVE) {
        const int64_t it = base + lane;
        uint64_t lo = 0, hi = 0, mhi = 0;
        int64_t G = 0;
        int neg = 0;
        if (it < items) {
            const int c = (int)(it / A.n);
            const int32_t sx = A.xlen[it], sd = A.dlen[c];
            const dig_t *x = (const dig_t *)(A.xlimbs + A.xoff[it]), *d = (const dig_t *)(A.dlimbs + A.doff[c]);
            const int la = slip_trim_digits(x, slip_abs(sx)), ld = slip_trim_digits(d, slip_abs(sd));
            neg = ((sx < 0) != (sd < 0)) != (A.flip != 0);
            if (la > 0 && ld > 0) {
                const int64_t bn = 32 * (int64_t) la - slip_clz32(x[la - 1]), bd = 32 * (int64_t) ld - slip_clz32(d[ld - 1]);
                const uint64_t n64 = slip_lead64(x, la), d64 = slip_lead64(d, ld);
                const int k = n64 < d64 ? 64 : 63;
                const uint64_t Q = k == 64 ? slip_div128by64(n64, 0, d64) : slip_div128by64(n64 >> 1, n64 << 63, d64);
                int64_t r = 11;
                G = r - k + bn - bd;
                if (G < -1074) { r += -1074 - G; G = -1074; }
                if (r < 66) {                                        /* else T < 2^64 + 3 < 2^r: +0.0 */
                    const int whole = bn <= 64 && bd <= 64;          /* T = X exactly */
                    const uint64_t qlo = whole ? Q : Q - 2, qhi = whole ? Q : Q + 2, carry = qhi < Q;      /* Q + 2 may reach 2^64 */
                    mhi = r < 64 ? (qhi >> r) | (carry << (64 - r)) : (r == 64 ? carry : 0);
                    lo = slip_double_bits(r < 64 ? qlo >> r : 0, G);
                    hi = slip_double_bits(mhi, G);
                }
            }
        }
        uint64_t pend = slip_ballot(lo != hi);
        slow_total += (unsigned long long) slip_popc64(pend);
        while (pend) {
            const int src = slip_ctz64(pend);
            pend &= pend - 1;
            const uint64_t m_src = slip_shfl_u64(mhi, src);
            const int64_t G_src = (int64_t) slip_shfl_u64((uint64_t) G, src);
            const int ok = slip_todouble_exact(A, base + src, m_src, G_src, scr);
            if (lane == src) lo = ok ? hi : lo;
        }
        if (it < items) {
            const int c = (int)(it / A.n), p = (int)(it - (int64_t) c * A.n);
            union { uint64_t u; double f; } v;
            v.u = lo | (lo != 0 && neg ? 0x8000000000000000ull : 0ull);
            A.out[(int64_t) c * A.n + (A.oidx ? A.oidx[p] : p)] = v.f;
        }
    }
    if (lane == 0 && slow_total) slip_atomic_add_u64(A.nslow, slow_total);
}

/* Solution to multi-precision floats (slip_hip_factor_solve_mpfr, slip_hip_solution_to_mpfr): per entry what mpfr_set_q leaves
 * in an mpfr_t of `prec` bits under the rounding mode `rnd` (SLIP_get_mpfr_soln.c:53) -- the ONE correct rounding of the exact
 * quotient v = N / D, with its ternary value.  Magnitudes below; the sign is that of N * D (times flip), and 0 is +0.
 *
 * With bn, bd the bit lengths of N and D:  2^(bn-bd-1) < v < 2^(bn-bd+1).  The quotient is formed with one bit to spare,
 *     Q = floor(v * 2^s),  s = prec + 1 - (bn - bd),  2^prec <= Q < 2^(prec+2),
 * and its leading bit says on which side of 2^(bn-bd) v lies: hi = bit prec+1 of Q, e0 = bn - bd + hi (2^(e0-1) <= v < 2^e0:
 * MPFR's exponent before rounding; no separate comparison of N and D is made).  t = Q >> hi has prec + 1 bits,
 *     m0 = t >> 1,   rb = t & 1,   st = (the bit of Q below t, when hi) | (v * 2^s is not an integer),
 * and the mantissa is m0 + inc, inc = 0 toward zero, rb | st away from zero (RNDU / RNDD are one of the two by sign),
 * rb & (st | (m0 & 1)) to nearest-even.  m0 + inc = 2^prec becomes 2^(prec-1) with exponent e0 + 1.  The ternary value is 0
 * when rb | st = 0, else the sign of the value when inc = 1 and its opposite when inc = 0.
 *
 * Lane pass, one lane per entry: N = 0, and -- for prec <= 64, where the result is one limb -- every pair within 64 bits:
 * both parts left-aligned, two 128-by-64 divisions (slip_div128by64) give 127 or 128 quotient bits, which hold t for every
 * such prec, and their remainder gives st.  Beyond 64 bits of precision the lane would carry a multi-limb mantissa; those
 * entries go to the wave.
 *
 * Wave pass, one wavefront per remaining entry, wave-uniform throughout: Knuth's algorithm D in base B = 2^32.  D' = D << zd
 * has its top bit set (ld digits); U = floor(N * 2^(s + zd)) has exactly prec + 1 + 32*ld bits, so it fills at most
 * nq + ld digits with nq = ceil((prec + 2) / 32) quotient digits, whatever the lengths of N and D: digits of N below that
 * window never enter the division, they only make st (a trailing-zero count, wb_ctz: a ballot over "nonzero").  Per quotient
 * digit, from the top: the estimate from the three leading digits of the running remainder and the two of D'
 *     qh = floor((w[ld] * B + w[ld-1]) / v1), lowered while qh * v2 > (remainder of that) * B + w[ld-2]
 * is the true digit or one above it (Knuth 4.3.1 Theorem B needs v1 >= B/2: the normalisation; the v2 test brings the
 * error of at most 2 down to at most 1); the wave forms qh * D' (wb_mul_lo, 1 x ld), subtracts it from the ld + 1 digits
 * of the window (wb_addsub, one digit wider so that the digit above the window shows a borrow as 0xFFFFFFFF) and adds D'
 * back while that digit is nonzero (at most twice).  The running remainder lives in this wave's scratch, in place in U.
 * st = remainder != 0 or dropped digits != 0.  The mantissa is written left-aligned into ceil(prec / 64) limbs -- Q shifted
 * so that bit prec-1 of m0 is the top bit, the bits below the last place filled with ones when inc = 1 so that adding 1 at the
 * bottom (wb_addsub) carries into the last place and leaves them zero; all limbs zero afterwards is the carry to 2^prec.
 *
 * Scratch per wave (stride, sized by the host from the widest D and prec): U nq + dcap + 2, the product dcap + 2, D' dcap,
 * the quotient nq + 1 digits.  The kernel never aborts: a zero denominator (refused by the host) gives +0. */
struct SlipMpfrArgs {
    int32_t n, nrhs;
    const int32_t *xlen; const int64_t *xoff; const uint64_t *xlimbs;              /* N: entry c*n + p, signed digit counts, limb offsets */
    const int32_t *dlen; const int64_t *doff; const uint64_t *dlimbs;              /* D: one per right-hand side                         */
    const int32_t *oidx;                                                           /* entry p goes to slot c*n + oidx[p]; null: to p     */
    int32_t flip;                                                                  /* negate every result (the sign of a scale)          */
    int32_t prec, rnd;                                                             /* 2..65536; MPFR_RNDN 0, Z 1, U 2, D 3, A 4          */
    int32_t chunk;                                                                 /* entries a wave takes per round, 1..64              */
    int8_t *sign; int64_t *exp; uint64_t *mant; int8_t *ternary;                   /* per slot; mant: ceil(prec / 64) limbs              */
    dig_t *scratch; int32_t dcap; int64_t stride;                                  /* wave pass: stride digits per wave, D <= dcap digits */
    unsigned long long *paths;                                                     /* entries settled by: lane (64 bits), wave with D <= 256 digits, wave wider, zero */
};

/* what is added to the truncated mantissa m0: rnd as mpfr_rnd_t, neg the sign of the value, odd = m0 & 1 */
SLIP_DEV int slip_mpfr_inc(int rnd, int neg, int odd, int rb, int st)
{
    if (rnd == 0) return rb & (st | odd);
    const int away = rnd == 4 || (rnd == 2 && !neg) || (rnd == 3 && neg);
    return away ? (rb | st) : 0;
}

/* the ternary value: the sign of (rounded - exact) of the signed number */
SLIP_DEV int slip_mpfr_ternary(int neg, int inexact, int inc)
{
    if (!inexact) return 0;
    return (inc != 0) != (neg != 0) ? 1 : -1;
}

/* the lane pass for N, D < 2^64 (both nonzero) and prec <= 64: the one limb of the mantissa, the exponent, the ternary value */
SLIP_DEV uint64_t slip_mpfr_lane64(uint64_t N, uint64_t D, int prec, int rnd, int neg, int64_t *e_out, int *tern_out)
{
    const int zn = slip_clz64(N), zd = slip_clz64(D);
    const uint64_t nn = N << zn, dn = D << zd;
    /* X = Q1 * 2^64 + Q2 = floor(nn * 2^127 / dn) in [2^126, 2^128), r2 its remainder */
    const uint64_t Q1 = slip_div128by64(nn >> 1, nn << 63, dn), r1 = (nn << 63) - Q1 * dn;
    const uint64_t Q2 = slip_div128by64(r1, 0, dn), r2 = 0 - Q2 * dn;
    const int sig = (Q1 >> 63) ? 128 : 127, k = sig - (prec + 1), j = k + 1;      /* t = X >> k; 62 <= k <= 125 */
    const uint64_t m0 = j < 64 ? (Q1 << 1) | (Q2 >> 63) : (j == 64 ? Q1 : Q1 >> (j - 64));
    const int rb = (int)((k < 64 ? Q2 >> k : Q1 >> (k - 64)) & 1);
    const uint64_t low = k < 64 ? Q2 & ((1ull << k) - 1) : Q2 | (Q1 & ((1ull << (k - 64)) - 1));
    const int st = low != 0 || r2 != 0;
    const int inc = slip_mpfr_inc(rnd, neg, (int)(m0 & 1), rb, st);
    int64_t e = (int64_t) sig - 127 + zd - zn;                                     /* bn - bd = zd - zn */
    uint64_t m = m0 + (uint64_t) inc;
    if (prec == 64 ? (inc && m == 0) : (m >> prec) != 0) { m = 1ull << (prec - 1); e++; }
    *e_out = e; *tern_out = slip_mpfr_ternary(neg, rb | st, inc);
    return m << (64 - prec);
}

/* the wave pass for entry `it` (wave-uniform); returns the digits of its denominator (0: nothing to divide, +0 written) */
SLIP_DEV int slip_mpfr_wave(const SlipMpfrArgs &A, int64_t it, dig_t *scr)
{
    const int lane = slip_lane();
    const int c = (int)(it / A.n), p = (int)(it - (int64_t) c * A.n);
    const int64_t slot = (int64_t) c * A.n + (A.oidx ? A.oidx[p] : p);
    const int32_t sx = A.xlen[it], sd = A.dlen[c];
    const dig_t *x = (const dig_t *)(A.xlimbs + A.xoff[it]), *d = (const dig_t *)(A.dlimbs + A.doff[c]);
    const int la = slip_trim_digits(x, slip_abs(sx)), ld = slip_trim_digits(d, slip_abs(sd));
    const int neg = ((sx < 0) != (sd < 0)) != (A.flip != 0);
    const int prec = A.prec, nl = (prec + 63) >> 6, nq = (prec + 2 + 31) >> 5;
    dig_t *out = (dig_t *)(A.mant + slot * nl);
    if (la == 0 || ld == 0 || ld > A.dcap) {                                       /* ld <= dcap: the host sized it */
        for (int cc = lane; cc < 2 * nl; cc += SLIP_WAVE) out[cc] = 0u;
        if (lane == 0) { A.sign[slot] = 0; A.exp[slot] = 0; A.ternary[slot] = 0; }
        slip_wave_sync();
        return 0;
    }
    dig_t *u = scr, *P = u + nq + A.dcap + 2, *Dn = P + A.dcap + 2, *qd = Dn + A.dcap;
    const int zd = slip_clz32(d[ld - 1]), nu = nq + ld;
    const int64_t bn = 32 * (int64_t) la - slip_clz32(x[la - 1]), bd = 32 * (int64_t) ld - zd;
    const int64_t S = (int64_t) prec + 1 - bn + bd + zd;                           /* U = floor(N * 2^S) */
    const int sb = (int)(((S % 32) + 32) % 32);
    const int64_t sw = (S - sb) / 32;
    wb_copy_shl(Dn, d, ld, zd, ld);
    for (int cc = lane; cc < nu + 2; cc += SLIP_WAVE) {
        const int64_t idx = (int64_t) cc - sw;
        const uint32_t lo = idx >= 0 && idx < la ? x[idx] : 0u, below = idx >= 1 && idx <= la ? x[idx - 1] : 0u;
        u[cc] = cc < nu ? (sb ? (lo << sb) | (below >> (32 - sb)) : lo) : 0u;      /* the two digits above U: zero */
    }
    if (lane == 0) qd[nq] = 0u;
    slip_wave_sync();
    int st = S < 0 && (int64_t) wb_ctz(x, la) < -S;                                /* bits of N below the window */
    const uint64_t B = 1ull << 32;
    const uint32_t v1 = Dn[ld - 1], v2 = ld >= 2 ? Dn[ld - 2] : 0u;
    for (int j = nq - 1; j >= 0; j--) {
        dig_t *w = u + j;                                                          /* the window: ld + 1 digits, w[ld + 1] == 0 */
        const uint64_t num = ((uint64_t) w[ld] << 32) | w[ld - 1];
        const uint32_t w2 = ld >= 2 ? w[ld - 2] : 0u;
        uint64_t qh = num / v1, rh = num - qh * v1;
        while (qh >= B || qh * v2 > ((rh << 32) | w2)) { qh--; rh += v1; if (rh >= B) break; }
        if (qh >= B) qh = B - 1;                                                   /* the true digit is below B */
        if (lane == 0) qd[j] = (dig_t) qh;
        slip_wave_sync();
        if (qh) {
            wb_mul_lo(P, qd + j, 1, Dn, ld, ld + 1);
            wb_addsub(w, w, ld + 2, P, ld + 1, ld + 2, 1);
            int back = 0;
            while (w[ld + 1] != 0u && back < 2) { wb_addsub(w, w, ld + 2, Dn, ld, ld + 2, 0); back++; }
            if (back) {
                if (lane == 0) qd[j] = (dig_t)(qh - (uint64_t) back);
                slip_wave_sync();
            }
        }
    }
    st |= wb_len(u, ld) != 0;
    const int hi = (int)((qd[(prec + 1) >> 5] >> ((prec + 1) & 31)) & 1u);
    const uint32_t q0 = qd[0];
    const int rb = (int)((q0 >> hi) & 1u), odd = (int)((q0 >> (hi + 1)) & 1u);
    st |= hi & (int)(q0 & 1u);
    const int inc = slip_mpfr_inc(A.rnd, neg, odd, rb, st);
    int64_t e = bn - bd + hi;
    /* m0 = Q >> (1 + hi), left-aligned: shifted up by z = 64*nl - prec; the z bits below the last place are ones when inc */
    const int z = 64 * nl - prec, sh = z - 1 - hi;
    for (int cc = lane; cc < 2 * nl; cc += SLIP_WAVE) {
        uint32_t v;
        if (sh >= 0) {
            const int idx = cc - (sh >> 5), b = sh & 31;
            const uint32_t lo = idx >= 0 && idx <= nq ? qd[idx] : 0u, below = idx >= 1 && idx - 1 <= nq ? qd[idx - 1] : 0u;
            v = b ? (lo << b) | (below >> (32 - b)) : lo;
        } else {
            const int r = -sh;                                                     /* 1 or 2 */
            const uint32_t lo = cc <= nq ? qd[cc] : 0u, above = cc + 1 <= nq ? qd[cc + 1] : 0u;
            v = (lo >> r) | (above << (32 - r));
        }
        const int nlow = z - 32 * cc;                                              /* bits of this digit below the last place */
        const uint32_t mask = nlow >= 32 ? 0xFFFFFFFFu : (nlow > 0 ? (1u << nlow) - 1u : 0u);
        out[cc] = inc ? v | mask : v & ~mask;
    }
    slip_wave_sync();
    if (inc) {
        wb_addsub(out, (const dig_t *) 0, 1, out, 2 * nl, 2 * nl, 0, 1u);
        if (!(out[2 * nl - 1] >> 31)) {                                            /* 2^prec: every digit is zero now */
            slip_wave_sync();
            if (lane == 0) out[2 * nl - 1] = 0x80000000u;
            e++;
        }
    }
    if (lane == 0) { A.sign[slot] = neg ? -1 : 1; A.exp[slot] = e; A.ternary[slot] = (int8_t) slip_mpfr_ternary(neg, rb | st, inc); }
    slip_wave_sync();
    return ld;
}

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_mpfr_kernel(SlipMpfrArgs A)
#else
static void slip_mpfr_body(SlipMpfrArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    dig_t *scr = A.scratch + wave0 * A.stride;
    const int64_t items = (int64_t) A.n * A.nrhs;
    const int nl = (A.prec + 63) >> 6;
    unsigned long long cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0;
    for (int64_t base = wave0 * A.chunk; base < items; base += nwaves * A.chunk) {
        const int64_t it = base + lane;
        const int mine = lane < A.chunk && it < items;
        int wide = 0, zero = 0;
        if (mine) {
            const int c = (int)(it / A.n), p = (int)(it - (int64_t) c * A.n);
            const int64_t slot = (int64_t) c * A.n + (A.oidx ? A.oidx[p] : p);
            const int32_t sx = A.xlen[it], sd = A.dlen[c];
            const dig_t *x = (const dig_t *)(A.xlimbs + A.xoff[it]), *d = (const dig_t *)(A.dlimbs + A.doff[c]);
            const int la = slip_trim_digits(x, slip_abs(sx)), ld = slip_trim_digits(d, slip_abs(sd));
            if (la == 0 || ld == 0) {
                zero = 1;
                for (int k = 0; k < nl; k++) A.mant[slot * nl + k] = 0ull;
                A.sign[slot] = 0; A.exp[slot] = 0; A.ternary[slot] = 0;
            } else if (la <= 2 && ld <= 2 && A.prec <= 64) {
                const uint64_t N = x[0] | ((uint64_t)(la > 1 ? x[1] : 0u) << 32), D = d[0] | ((uint64_t)(ld > 1 ? d[1] : 0u) << 32);
                const int neg = ((sx < 0) != (sd < 0)) != (A.flip != 0);
                int64_t e; int tern;
                A.mant[slot] = slip_mpfr_lane64(N, D, A.prec, A.rnd, neg, &e, &tern);
                A.sign[slot] = neg ? -1 : 1; A.exp[slot] = e; A.ternary[slot] = (int8_t) tern;
            } else wide = 1;
        }
        uint64_t pend = slip_ballot(wide);
        const int nzero = slip_popc64(slip_ballot(zero));
        cnt3 += (unsigned long long) nzero;
        cnt0 += (unsigned long long)(slip_popc64(slip_ballot(mine)) - slip_popc64(pend) - nzero);
        while (pend) {
            const int src = slip_ctz64(pend);
            pend &= pend - 1;
            const int ld = slip_mpfr_wave(A, base + src, scr);
            if (ld == 0) cnt3++; else if (ld <= 256) cnt1++; else cnt2++;
        }
    }
    if (lane == 0) {
        if (cnt0) slip_atomic_add_u64(A.paths + 0, cnt0);
        if (cnt1) slip_atomic_add_u64(A.paths + 1, cnt1);
        if (cnt2) slip_atomic_add_u64(A.paths + 2, cnt2);
        if (cnt3) slip_atomic_add_u64(A.paths + 3, cnt3);
    }
}

/* Solution as reduced fractions (slip_hip_factor_solve_rational, slip_hip_solution_to_rational): per entry the canonical form
 * of N / D that mpq_canonicalize leaves (SLIP_solve_mpq's output: SLIP_LU_solve's mpq_div, SLIP_permute_x, SLIP_scale_x):
 *     g = gcd(|N|, |D|),   num = sgn(N * D) * |N| / g,   den = |D| / g > 0,   0 = 0 / 1.
 *
 * Lane pass, one lane per entry: N = 0, and every pair that fits 64 bits (a binary gcd and two divisions in the lane).
 * Wave pass, one wavefront per remaining entry, wave-uniform throughout.  With N = 2^zn * N', D = 2^zd * D' (N', D' odd) and
 * z = min(zn, zd):  g = 2^z * h,  h = gcd(N', D') odd,  num = (N >> z) / h,  den = (D >> z) / h: the power of two is a shift
 * and the odd part an exact 2-adic division (Hensel in registers, the Newton inverse of h through memory; nothing when h = 1).
 *
 * h = gcd(a, b) of two numbers of which at least one is odd (both, at the start), a >= b (slip_gcd_odd_reg /
 * slip_reduce_wide).  Every step replaces (a, b) by a pair with the same set of common divisors -- an EXACT invariant, no
 * factor is ever introduced -- and retires digits, not bits:
 *   (i)  bits(a) - bits(b) = G >= 8, b odd (an even b has its trailing zeros shifted out first):  t = a * b^-1 mod 2^G,
 *        a <- |a - t*b| / 2^G.  2^G divides a - t*b by the choice of t; t*b < 2^(G + bits(b)) = 2^bits(a), so the difference
 *        needs no headroom and a comes down to b's length in ONE step, however many digits apart they were; odd b shares
 *        no factor with 2^G, so gcd(a', b) = gcd(a, b).  G <= 32: t is one digit (a scalar Newton inverse).  Above,
 *        b^-1 modulo B^ceil(G/32) is a Newton iteration (wr_inv_extend / wb_inv_extend) and t, t*b are two products.
 *   (ii) G < 8, Lehmer: ah = floor(a / 2^s), bh = floor(b / 2^s) with s = bits(a) - 62.  Euclid's algorithm runs on (ah, bh)
 *        while the quotient is the same for both ends of the intervals the leading parts leave open,
 *            floor((ah + A) / (bh + C)) == floor((ah + B) / (bh + D))              (Knuth 4.5.2, Algorithm L)
 *        -- then it IS the quotient of the full numbers -- and while the cofactors stay below 2^31.  The wave applies the
 *        matrix, a' = A*a + B*b, b' = C*a + D*b (determinant +-1: the same common divisors): two consecutive remainders of
 *        Euclid's sequence for (a, b), both >= 0, so the arithmetic modulo B^W is exact.  About 30 bits go per step.  The
 *        remainders may be even; h is odd, so at most one of the two is, and (i) and (iii) shift its trailing zeros out
 *        when they need an odd number (dividing one of the two by 2 leaves an odd gcd what it was).
 *   (iii) no matrix (the first quotient is already open: a / b within 2^-54 of an integer):  a <- (a - b) >> ctz, both odd.
 *   When both fit 64 bits the binary gcd of the lane pass finishes.  a == b or b == 0 ends the loop.
 * Two width classes: max(|N|, |D|) <= 256 digits in registers (WR<1..4>), wider through this wave's scratch in global memory
 * (five buffers of wcap digits, sized by the host from the widest operand of the call).
 *
 * Output: entry (c, p) goes to slot c*n + oidx[p]; the host gave every slot room for |N| and |D| themselves (numoff, denoff:
 * limb offsets), the kernel writes whole limbs (an odd digit count is padded with a zero digit) and the signed digit counts.
 * The kernel never aborts: a zero denominator (refused by the host) gives 0 digits of num and den. */
struct SlipReduceArgs {
    int32_t n, nrhs;
    const int32_t *xlen; const int64_t *xoff; const uint64_t *xlimbs;              /* N: entry c*n + p, signed digit counts, limb offsets */
    const int32_t *dlen; const int64_t *doff; const uint64_t *dlimbs;              /* D: one per right-hand side                         */
    const int32_t *oidx;                                                           /* entry p goes to slot c*n + oidx[p]; null: to p     */
    int32_t flip;                                                                  /* negate every result (the sign of a scale)          */
    int32_t chunk;                                                                 /* entries a wave takes per round, 1..64              */
    int32_t *numlen, *denlen;                                                      /* per slot: signed digit count of num, digits of den */
    const int64_t *numoff, *denoff; uint64_t *numlimbs, *denlimbs;                 /* per slot: where its limbs go                       */
    dig_t *scratch; int32_t wcap;                                                  /* wave pass: 8 + 5 * wcap digits per wave, wcap >= 264 */
    unsigned long long *paths;                                                     /* entries settled by: lane, reg g = 1, reg g > 1, memory */
};

/* gcd of two odd 64-bit numbers (binary) */
SLIP_DEV uint64_t slip_gcd64_odd(uint64_t u, uint64_t v)
{
    while (u != v) {
        if (u < v) { const uint64_t t = u; u = v; v = t; }
        u -= v;
        u >>= slip_ctz64(u);
    }
    return u;
}

/* Lehmer's cofactors from the leading parts ah >= bh > 0 (both below 2^62, the same shift of a and b): m = |A|, |B|, |C|, |D|,
 * each below 2^31; *bneg: B < 0 (then A >= 0: a' = |A|a - |B|b, else |B|b - |A|a), *dpos: D > 0 (b' = |D|b - |C|a, else the
 * reverse).  0 when the leading parts allow no step. */
SLIP_DEV int slip_lehmer(uint64_t ah, uint64_t bh, uint32_t *m, int *bneg, int *dpos)
{
    const int64_t LIM = 0x7FFFFFFFll;
    int64_t A = 1, B = 0, C = 0, Dd = 1, a = (int64_t) ah, b = (int64_t) bh;
    for (;;) {
        if (b + C <= 0 || b + Dd <= 0) break;
        const int64_t q = (a + A) / (b + C);
        if (q != (a + B) / (b + Dd) || q > LIM) break;
        const int64_t nC = A - q * C, nD = B - q * Dd;
        if (nC > LIM || nC < -LIM || nD > LIM || nD < -LIM) break;
        const int64_t t = a - q * b;
        A = C; C = nC; B = Dd; Dd = nD; a = b; b = t;
    }
    if (B == 0) return 0;
    m[0] = (uint32_t)(A < 0 ? -A : A); m[1] = (uint32_t)(B < 0 ? -B : B);
    m[2] = (uint32_t)(C < 0 ? -C : C); m[3] = (uint32_t)(Dd < 0 ? -Dd : Dd);
    *bneg = B < 0; *dpos = Dd > 0;
    return 1;
}

/* the 2-adic multiplier of step (i): t = a0 / b0 mod 2^k for odd b0, 1 <= k <= 32 */
SLIP_DEV uint32_t slip_gcd_quot(uint32_t a0, uint32_t b0, int k)
{
    const uint32_t t = a0 * wb_inv32(b0);
    return k < 32 ? t & ((1u << k) - 1u) : t;
}

/* digits [0, 64*D) of (p >> shift), p of len digits */
template <int D> SLIP_DEV WR<D> wr_load_shr(const dig_t *p, int len, int shift)
{
    const int lane = slip_lane(), sw = shift >> 5, sb = shift & 31;
    WR<D> x;
#pragma unroll
    for (int q = 0; q < D; q++) {
        const int idx = 64 * q + lane + sw;
        const uint32_t lo = idx < len ? p[idx] : 0u, hi = idx + 1 < len ? p[idx + 1] : 0u;
        x.d[q] = sb ? ((lo >> sb) | (hi << (32 - sb))) : lo;
    }
    return x;
}

/* x modulo 2^K */
template <int D> SLIP_DEV WR<D> wr_mask_bits(const WR<D> &x, int K)
{
    const int lane = slip_lane(), w = K >> 5;
    const uint32_t top = (K & 31) ? (1u << (K & 31)) - 1u : 0u;
    WR<D> r;
#pragma unroll
    for (int q = 0; q < D; q++) { const int c = 64 * q + lane; r.d[q] = c < w ? x.d[q] : (c == w ? x.d[q] & top : 0u); }
    return r;
}

/* x with its trailing zero bits shifted out (0 stays 0); scratch: 64*D + 2 digits */
template <int D> SLIP_DEV WR<D> wr_strip(const WR<D> &x, dig_t *scratch)
{
#pragma unroll
    for (int q = 0; q < D; q++) {
        const uint64_t nz = slip_ballot(x.d[q] != 0);
        if (nz) { const int t = slip_ctz64(nz); return wr_shr<D>(x, 32 * (64 * q + t) + slip_ctz32(slip_readlane(x.d[q], t)), scratch); }
    }
    return x;
}

/* floor(x / 2^s) modulo 2^64 as a wave-uniform value */
template <int D> SLIP_DEV uint64_t wr_window(const WR<D> &x, int s)
{
    const int i = s >> 5, sb = s & 31;
    const uint64_t lo = (uint64_t) wr_digit<D>(x, i) | ((uint64_t) wr_digit<D>(x, i + 1) << 32);
    return sb ? (lo >> sb) | ((uint64_t) wr_digit<D>(x, i + 2) << (64 - sb)) : lo;
}

/* gcd of two numbers of which at least one is odd, in registers (steps (i)-(iii) above); a half that has become narrow enough
 * goes on in fewer registers */
template <int D> SLIP_DEV WR<D> slip_gcd_odd_reg(WR<D> a, WR<D> b, dig_t *scratch)
{
    int ordered = 0;                                                 /* a > b is known: two consecutive remainders */
    for (;;) {
        int la = wr_len<D>(a), lb = wr_len<D>(b);
        if (lb == 0) return a;
        if (la == 0) return b;
        if (!ordered) {
            const int c = la != lb ? (la > lb ? 1 : -1) : wr_cmp<D>(a, b);
            if (c == 0) return a;
            if (c < 0) { const WR<D> t = a; a = b; b = t; const int tl = la; la = lb; lb = tl; }
        }
        ordered = 0;
        if constexpr (D > 1) {
            if (la <= 64 * (D / 2)) {
                WR<D / 2> na, nb;
#pragma unroll
                for (int q = 0; q < D / 2; q++) { na.d[q] = a.d[q]; nb.d[q] = b.d[q]; }
                const WR<D / 2> g = slip_gcd_odd_reg<D / 2>(na, nb, scratch);
                WR<D> r = wr_zero<D>();
#pragma unroll
                for (int q = 0; q < D / 2; q++) r.d[q] = g.d[q];
                return r;
            }
        }
        if (la <= 2) {
            const uint64_t u = wr_window<D>(a, 0), v = wr_window<D>(b, 0);
            const uint64_t g = slip_gcd64_odd(u >> slip_ctz64(u), v >> slip_ctz64(v));
            WR<D> r = wr_zero<D>();
            if (slip_lane() < 2) r.d[0] = slip_lane() ? (uint32_t)(g >> 32) : (uint32_t) g;
            return r;
        }
        const int ba = 32 * la - slip_clz32(wr_digit<D>(a, la - 1)), bb = 32 * lb - slip_clz32(wr_digit<D>(b, lb - 1));
        const uint32_t a0 = slip_readlane(a.d[0], 0), b0 = slip_readlane(b.d[0], 0);
        if (ba - bb >= 8) {
            if (!(b0 & 1u)) { b = wr_strip<D>(b, scratch); continue; }           /* then a is odd: the gcd stays */
            const int K = ba - bb, md = (K + 31) >> 5;
            WR<D> p;
            if (md == 1) p = wr_mul_digit<D>(slip_gcd_quot(a0, b0, K), b);
            else p = wr_mul<D>(wr_mask_bits<D>(wr_mul<D>(wr_inv_extend<D>(wr_zero<D>(), 0, md, b), md, a), K), md, b);
            const int cp = wr_cmp<D>(a, p);
            if (cp == 0) return b;                                   /* a = t * b */
            a = wr_shr<D>(cp > 0 ? wr_addsub<D>(a, p, 1) : wr_addsub<D>(p, a, 1), K, scratch);
            continue;
        }
        const int s = ba > 62 ? ba - 62 : 0;
        uint32_t m[4]; int bneg, dpos;
        if (slip_lehmer(wr_window<D>(a, s), wr_window<D>(b, s), m, &bneg, &dpos)) {
            WR<D> pa, pb, pc, pd;
            wr_mul_digit2<D>(m[0], m[2], a, pa, pc);
            wr_mul_digit2<D>(m[1], m[3], b, pb, pd);
            a = bneg ? wr_addsub<D>(pa, pb, 1) : wr_addsub<D>(pb, pa, 1);
            b = dpos ? wr_addsub<D>(pd, pc, 1) : wr_addsub<D>(pc, pd, 1);
            ordered = 1;
        } else if (!(a0 & 1u)) a = wr_strip<D>(a, scratch);
        else if (!(b0 & 1u)) b = wr_strip<D>(b, scratch);
        else a = wr_strip<D>(wr_addsub<D>(a, b, 1), scratch);
    }
}

/* the wave pass in registers: num and den of (x >> z) / h, (d >> z) / h written as whole limbs; returns 1 when g = 2^z * h > 1 */
template <int D> SLIP_DEV int slip_reduce_reg(const dig_t *x, int la, int zn, const dig_t *d, int ld, int zd, dig_t *scratch,
                                              dig_t *onum, dig_t *oden, int *lnum, int *lden)
{
    const int z = zn < zd ? zn : zd;
    const WR<D> h = slip_gcd_odd_reg<D>(wr_load_shr<D>(x, la, zn), wr_load_shr<D>(d, ld, zd), scratch);
    const int lh = wr_len<D>(h), one = lh == 1 && slip_readlane(h.d[0], 0) == 1u;
    WR<D> T = wr_load_shr<D>(x, la, z);
    if (!one) T = wr_div_hensel<D>(T, wr_len<D>(T) - lh + 1, h);
    *lnum = wr_len<D>(T);
    wr_store<D>(onum, T, (*lnum + 1) & ~1);
    T = wr_load_shr<D>(d, ld, z);
    if (!one) T = wr_div_hensel<D>(T, wr_len<D>(T) - lh + 1, h);
    *lden = wr_len<D>(T);
    wr_store<D>(oden, T, (*lden + 1) & ~1);
    return !one || z > 0;
}

/* floor(x / 2^s) modulo 2^64 of a number in memory */
SLIP_DEV uint64_t wb_window(const dig_t *x, int lx, int s)
{
    const int i = s >> 5, sb = s & 31;
    const uint64_t lo = (uint64_t)(i < lx ? x[i] : 0u) | ((uint64_t)(i + 1 < lx ? x[i + 1] : 0u) << 32);
    return sb ? (lo >> sb) | ((uint64_t)(i + 2 < lx ? x[i + 2] : 0u) << (64 - sb)) : lo;
}

/* dst = src with its trailing zero bits shifted out; returns its digits (src: ls >= 0 significant digits; no overlap) */
SLIP_DEV int wb_strip(dig_t *dst, const dig_t *src, int ls)
{
    if (ls == 0) return 0;
    wb_copy_shr(dst, src, ls, wb_ctz(src, ls), ls);
    return wb_len(dst, ls);
}

/* the wave pass through memory (operands above 256 digits): the same steps on five buffers of wcap digits; sm: 8 digits */
SLIP_DEV void slip_reduce_wide(const dig_t *x, int la, int zn, const dig_t *d, int ld, int zd, dig_t *sm, dig_t *buf, int wcap,
                               dig_t *onum, dig_t *oden, int *lnum, int *lden)
{
    const int lane = slip_lane(), z = zn < zd ? zn : zd;
    dig_t *a = buf, *b = buf + wcap, *P = b + wcap, *Q = P + wcap, *R = Q + wcap;
    wb_copy_shr(a, x, la, zn, la);
    wb_copy_shr(b, d, ld, zd, ld);
    int na = wb_len(a, la), nb = wb_len(b, ld), ordered = 0;
    for (;;) {
        if (nb == 0) break;
        if (!ordered) {
            const int c = na == 0 ? -1 : wb_cmp(a, na, b, nb);
            if (c == 0) break;
            if (c < 0) { dig_t *t = a; a = b; b = t; const int tl = na; na = nb; nb = tl; }
            if (nb == 0) break;
        }
        ordered = 0;
        if (na <= 2) {
            const uint64_t u = wb_window(a, na, 0), v = wb_window(b, nb, 0);
            const uint64_t g = slip_gcd64_odd(u >> slip_ctz64(u), v >> slip_ctz64(v));
            slip_wave_sync();
            if (lane < 2) a[lane] = lane ? (uint32_t)(g >> 32) : (uint32_t) g;
            slip_wave_sync();
            na = (g >> 32) ? 2 : 1;
            break;
        }
        const int ba = wb_bits(a, na), bb = wb_bits(b, nb);
        if (ba - bb >= 8) {
            if (!(b[0] & 1u)) { nb = wb_strip(P, b, nb); dig_t *t = b; b = P; P = t; continue; }      /* then a is odd: the gcd stays */
            const int K = ba - bb, md = (K + 31) >> 5;
            wb_inv_extend(P, 0, md, b, nb, Q, R);                            /* 1 / b modulo B^md */
            wb_mul_lo(Q, a, na, P, md, md);
            if (lane == 0 && (K & 31)) Q[md - 1] &= (1u << (K & 31)) - 1u;    /* t = a / b modulo 2^K */
            slip_wave_sync();
            wb_mul_lo(R, Q, wb_len(Q, md), b, nb, na);
            const int np = wb_len(R, na), cp = wb_cmp(a, na, R, np);
            if (cp == 0) { dig_t *u = a; a = b; b = u; na = nb; break; }        /* a = t * b */
            if (cp > 0) wb_addsub(R, a, na, R, np, na, 1); else wb_addsub(R, R, np, a, na, na, 1);
            const int nr = wb_len(R, na);
            wb_copy_shr(a, R, nr, K, nr);
            na = wb_len(a, nr);
            continue;
        }
        const int s = ba > 62 ? ba - 62 : 0;
        uint32_t m[4]; int bneg, dpos;
        if (slip_lehmer(wb_window(a, na, s), wb_window(b, nb, s), m, &bneg, &dpos)) {
            if (lane < 4) sm[lane] = lane == 0 ? m[0] : (lane == 1 ? m[1] : (lane == 2 ? m[2] : m[3]));
            slip_wave_sync();
            const int W = na;
            wb_mul_lo(P, sm, 1, a, na, W);
            wb_mul_lo(Q, sm + 1, 1, b, nb, W);
            if (bneg) wb_addsub(P, P, W, Q, W, W, 1); else wb_addsub(P, Q, W, P, W, W, 1);
            wb_mul_lo(Q, sm + 2, 1, a, na, W);
            wb_mul_lo(R, sm + 3, 1, b, nb, W);
            if (dpos) wb_addsub(Q, R, W, Q, W, W, 1); else wb_addsub(Q, Q, W, R, W, W, 1);
            dig_t *t = a; a = P; P = t; t = b; b = Q; Q = t;
            na = wb_len(a, W); nb = wb_len(b, W);
            ordered = 1;
        } else if (!(a[0] & 1u)) { na = wb_strip(P, a, na); dig_t *t = a; a = P; P = t; }
        else if (!(b[0] & 1u)) { nb = wb_strip(P, b, nb); dig_t *t = b; b = P; P = t; }
        else {
            wb_addsub(P, a, na, b, nb, na, 1);
            na = wb_strip(a, P, wb_len(P, na));
        }
    }
    /* h = a[0..na); b, P, Q and R are free */
    dig_t *T = b;
    const int one = na == 1 && a[0] == 1u;
    const int lt = (wb_bits(x, la) - z + 31) >> 5, ltd = (wb_bits(d, ld) - z + 31) >> 5;
    if (one) {
        wb_copy_shr(onum, x, la, z, (lt + 1) & ~1);
        wb_copy_shr(oden, d, ld, z, (ltd + 1) & ~1);
        *lnum = lt; *lden = ltd;
        return;
    }
    const int qn = lt - na + 1, qd = ltd - na + 1;
    wb_inv_extend(P, 0, qn > qd ? qn : qd, a, na, Q, R);             /* 1 / h modulo B^max(qn, qd) */
    wb_copy_shr(T, x, la, z, lt);
    wb_mul_lo(onum, T, lt, P, qn, qn);                               /* the quotient is below B^qn: exact modulo B^qn */
    *lnum = wb_len(onum, qn);
    wb_copy_shr(T, d, ld, z, ltd);
    wb_mul_lo(oden, T, ltd, P, qd, qd);
    *lden = wb_len(oden, qd);
    if (lane == 0) { if (qn & 1) onum[qn] = 0u; if (qd & 1) oden[qd] = 0u; }      /* whole limbs */
}

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_reduce_kernel(SlipReduceArgs A)
#else
static void slip_reduce_body(SlipReduceArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    dig_t *sm = A.scratch + wave0 * (8 + 5 * (int64_t) A.wcap), *buf = sm + 8;
    const int64_t items = (int64_t) A.n * A.nrhs;
    unsigned long long cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0;
    for (int64_t base = wave0 * A.chunk; base < items; base += nwaves * A.chunk) {
        const int64_t it = base + lane;
        const int mine = lane < A.chunk && it < items;
        int wide = 0;
        if (mine) {
            const int c = (int)(it / A.n), p = (int)(it - (int64_t) c * A.n);
            const int64_t slot = (int64_t) c * A.n + (A.oidx ? A.oidx[p] : p);
            const int32_t sx = A.xlen[it], sd = A.dlen[c];
            const dig_t *x = (const dig_t *)(A.xlimbs + A.xoff[it]), *d = (const dig_t *)(A.dlimbs + A.doff[c]);
            const int la = slip_trim_digits(x, slip_abs(sx)), ld = slip_trim_digits(d, slip_abs(sd));
            const int neg = ((sx < 0) != (sd < 0)) != (A.flip != 0);
            if (ld == 0) { A.numlen[slot] = 0; A.denlen[slot] = 0; }
            else if (la == 0) {
                A.numlen[slot] = 0; A.denlen[slot] = 1;
                A.denlimbs[A.denoff[slot]] = 1ull;
            } else if (la <= 2 && ld <= 2) {
                uint64_t u = x[0] | ((uint64_t)(la > 1 ? x[1] : 0u) << 32), v = d[0] | ((uint64_t)(ld > 1 ? d[1] : 0u) << 32);
                const int zu = slip_ctz64(u), zv = slip_ctz64(v);
                const uint64_t g = slip_gcd64_odd(u >> zu, v >> zv) << (zu < zv ? zu : zv);
                u /= g; v /= g;
                const int lu = (u >> 32) ? 2 : 1;
                A.numlen[slot] = neg ? -lu : lu; A.denlen[slot] = (v >> 32) ? 2 : 1;
                A.numlimbs[A.numoff[slot]] = u; A.denlimbs[A.denoff[slot]] = v;
            } else wide = 1;
        }
        uint64_t pend = slip_ballot(wide);
        cnt0 += (unsigned long long)(slip_popc64(slip_ballot(mine)) - slip_popc64(pend));
        while (pend) {
            const int src = slip_ctz64(pend);
            pend &= pend - 1;
            const int64_t e = base + src;
            const int c = (int)(e / A.n), p = (int)(e - (int64_t) c * A.n);
            const int64_t slot = (int64_t) c * A.n + (A.oidx ? A.oidx[p] : p);
            const int32_t sx = A.xlen[e], sd = A.dlen[c];
            const dig_t *x = (const dig_t *)(A.xlimbs + A.xoff[e]), *d = (const dig_t *)(A.dlimbs + A.doff[c]);
            const int la = slip_trim_digits(x, slip_abs(sx)), ld = slip_trim_digits(d, slip_abs(sd));
            const int zn = wb_ctz(x, la), zd = wb_ctz(d, ld), need = la > ld ? la : ld;
            dig_t *onum = (dig_t *)(A.numlimbs + A.numoff[slot]), *oden = (dig_t *)(A.denlimbs + A.denoff[slot]);
            int lnum = 0, lden = 0, g1 = 0;
            if (need <= 64) g1 = slip_reduce_reg<1>(x, la, zn, d, ld, zd, buf, onum, oden, &lnum, &lden);
            else if (need <= 128) g1 = slip_reduce_reg<2>(x, la, zn, d, ld, zd, buf, onum, oden, &lnum, &lden);
            else if (need <= 192) g1 = slip_reduce_reg<3>(x, la, zn, d, ld, zd, buf, onum, oden, &lnum, &lden);
            else if (need <= 256) g1 = slip_reduce_reg<4>(x, la, zn, d, ld, zd, buf, onum, oden, &lnum, &lden);
            else slip_reduce_wide(x, la, zn, d, ld, zd, sm, buf, A.wcap, onum, oden, &lnum, &lden);      /* need + 2 <= wcap: the host sized it */
            if (need > 256) cnt3++; else if (g1) cnt2++; else cnt1++;
            if (lane == 0) {
                A.numlen[slot] = (((sx < 0) != (sd < 0)) != (A.flip != 0)) ? -lnum : lnum;
                A.denlen[slot] = lden;
            }
            slip_wave_sync();
        }
    }
    if (lane == 0) {
        if (cnt0) slip_atomic_add_u64(A.paths + 0, cnt0);
        if (cnt1) slip_atomic_add_u64(A.paths + 1, cnt1);
        if (cnt2) slip_atomic_add_u64(A.paths + 2, cnt2);
        if (cnt3) slip_atomic_add_u64(A.paths + 3, cnt3);
    }
}

/* The reduced fractions packed: slot t's limbs move from where slip_reduce_kernel left them (soff) to their place in the compact
 * slab the ABI returns (doff), one wavefront per slot.  len: signed digit counts. */
struct SlipPackArgs {
    int64_t count;
    const int32_t *len; const int64_t *soff, *doff; const uint64_t *src; uint64_t *dst;
};

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_pack_kernel(SlipPackArgs A)
#else
static void slip_pack_body(SlipPackArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    for (int64_t t = wave0; t < A.count; t += nwaves) {
        const int l = (slip_abs(A.len[t]) + 1) >> 1;
        const uint64_t *s = A.src + A.soff[t];
        uint64_t *o = A.dst + A.doff[t];
        for (int k = lane; k < l; k += SLIP_WAVE) o[k] = s[k];
    }
}

/* Exact ratio test (slip_hip_ratio_test, slip_hip_factor_ratio_test): per problem c the eligible entry i with the
 * smallest ratio  r_i = x_i / |a_i|  (negated when xflip is set), ties broken by the smallest (key[idx], idx), idx = oidx[i]
 * being the index that is reported; the number of eligible entries that tie with it; the number of eligible entries.  Entry
 * i of problem c is entry c * pstride + i of the x records and of the a records.  An entry is eligible when sign(a_i) ==
 * asense; with alen == NULL every entry is eligible and a_i = 1.  The host turns sense and the sign of det into asense and
 * xflip.  Nothing depends on the launch geometry: (r_i, key, idx) is a total order and the tie count is a count.
 *
 * phase 0, the bound pass, one lane per entry (a wave's 64 entries are of one problem): from the signs, the bit lengths and
 *   the leading 64 bits of both parts (the lane pass of slip_todouble_kernel: T = |r| * 2^(k - bn + bd), floor(T) is one of
 *   Q-2 .. Q+2) an enclosure (Qs - 1) * 2^e < |r| < (Qs + 2) * 2^e, Qs = Q >> 2, e = bn - bd - k + 2, is packed into two
 *   monotone 64-bit keys (slip_ratio_key: a biased exponent above 22 bits of mantissa, truncated for the lower end, truncated
 *   plus one for the upper end; negated and swapped for a negative ratio; x_i = 0 is the point 0).  The lower key is kept per
 *   entry (INT64_MAX: not eligible); the minimum of the upper keys goes to minhi[c], one atomic per wave.
 * phase 1, the filter: an eligible entry whose lower key is at most minhi[c] is appended to the problem's candidates (an
 *   atomic cursor; their order does not matter).  The winner and all that tie with it pass: no enclosure of theirs lies above
 *   another entry's.
 * phase 2, the exact fold, one wave per chunk of SLIP_RATIO_CHUNK candidates: a running best by slip_ratio_cmp.
 * phase 3, one wave per problem: the chunk winners folded by the same comparison, the tie counts of equal winners added.
 *
 * slip_ratio_cmp settles sign(r_i - r_j) = sign(x_i |a_j| - x_j |a_i|) without a product when the numerators differ in sign,
 * both are zero, or bits(x_i) + bits(a_j) and bits(x_j) + bits(a_i) differ by two or more (a product of p-bit and q-bit factors
 * has p + q - 1 or p + q bits); without denominators it compares the numerators themselves.  Otherwise both products are
 * formed, in registers up to 256 digits, above that with wb_mul_lo into this wave's scratch (2 * wcap digits).
 * paths: [0] eligible entries, [1] candidates, [2] comparisons that formed products, [3] of those on the memory path. */
#define SLIP_RATIO_CHUNK 64
struct SlipRatioArgs {
    int32_t n, nprob, phase, asense, xflip;
    int64_t pstride;
    const int32_t *xlen; const int64_t *xoff; const uint64_t *xlimbs;              /* x: signed digit counts, limb offsets   */
    const int32_t *alen; const int64_t *aoff; const uint64_t *alimbs;              /* a likewise, or alen NULL               */
    const int32_t *oidx, *key;                                                     /* reported index of entry i; key by it   */
    int64_t *lokey, *minhi;                                                        /* per entry c*n + i; per problem         */
    int32_t *ncand, *cand;                                                         /* per problem; candidates at c*n + t     */
    int32_t nchunk; int32_t *cwpos, *cwties;                                       /* chunk winners at c*nchunk + k          */
    int32_t *best, *nties, *nelig;                                                 /* the result, per problem                */
    int32_t *wlen; int64_t *woff;                                                  /* the winner's records at 2c, 2c+1, or NULL */
    int32_t *maxdig;                                                               /* [0], [1]: widest eligible x, a         */
    dig_t *scratch; int32_t wcap; int32_t *err;                                    /* memory path; a product wider than wcap */
    unsigned long long *paths;
};

/* the monotone key of q * 2^e, 0 < q < 2^63: the exponent of its leading bit, biased, above the 22 bits that follow that bit */
SLIP_DEV int64_t slip_ratio_key(uint64_t q, int64_t e)
{
    const int z = slip_clz64(q);
    const uint64_t norm = q << z;
    return ((e + 63 - z + ((int64_t) 1 << 40)) << 22) | (int64_t)((norm >> 41) & 0x3FFFFFu);
}

/* one side of a comparison: the trimmed numerator and denominator of entry i of problem c */
struct SlipRatioEnt { const dig_t *x, *a; int lx, la, sx; };
SLIP_DEV SlipRatioEnt slip_ratio_ent(const SlipRatioArgs &A, int c, int i)
{
    SlipRatioEnt E;
    const int64_t e = (int64_t) c * A.pstride + i;
    const int32_t sx = A.xlen[e];
    E.x = (const dig_t *)(A.xlimbs + A.xoff[e]);
    E.lx = slip_trim_digits(E.x, slip_abs(sx));
    E.sx = E.lx == 0 ? 0 : (((sx < 0) != (A.xflip != 0)) ? -1 : 1);
    E.a = (const dig_t *) 0; E.la = 0;
    if (A.alen) { E.a = (const dig_t *)(A.alimbs + A.aoff[e]); E.la = slip_trim_digits(E.a, slip_abs(A.alen[e])); }
    return E;
}

/* sign(P - Q) of the two products in registers, all of them at most 64*D digits */
template <int D> SLIP_DEV int slip_ratio_cmp_reg(const dig_t *x1, int lx1, const dig_t *a2, int la2, const dig_t *x2, int lx2, const dig_t *a1, int la1)
{
    const WR<D> X1 = wr_load<D>(x1, lx1), A2 = wr_load<D>(a2, la2), X2 = wr_load<D>(x2, lx2), A1 = wr_load<D>(a1, la1);
    const WR<D> P = lx1 <= la2 ? wr_mul<D>(X1, lx1, A2) : wr_mul<D>(A2, la2, X1);
    const WR<D> Q = lx2 <= la1 ? wr_mul<D>(X2, lx2, A1) : wr_mul<D>(A1, la1, X2);
    return wr_cmp<D>(P, Q);
}

/* sign(r_i - r_j) for two eligible entries of problem c (all arguments wave-uniform); cnt[0], cnt[1]: paths 2 and 3 */
SLIP_DEV int slip_ratio_cmp(const SlipRatioArgs &A, int c, int i, int j, dig_t *scr, unsigned long long *cnt)
{
    const SlipRatioEnt I = slip_ratio_ent(A, c, i), J = slip_ratio_ent(A, c, j);
    if (I.sx != J.sx) return I.sx < J.sx ? -1 : 1;
    if (I.sx == 0) return 0;
    if (!A.alen) return I.sx * wb_cmp(I.x, I.lx, J.x, J.lx);
    const int64_t s1 = (int64_t) wb_bits(I.x, I.lx) + wb_bits(J.a, J.la), s2 = (int64_t) wb_bits(J.x, J.lx) + wb_bits(I.a, I.la);
    if (s1 >= s2 + 2) return I.sx;
    if (s2 >= s1 + 2) return -I.sx;
    const int w1 = I.lx + J.la, w2 = J.lx + I.la, W = w1 > w2 ? w1 : w2;
    int cm;
    cnt[0]++;
    if (W <= 64) cm = slip_ratio_cmp_reg<1>(I.x, I.lx, J.a, J.la, J.x, J.lx, I.a, I.la);
    else if (W <= 128) cm = slip_ratio_cmp_reg<2>(I.x, I.lx, J.a, J.la, J.x, J.lx, I.a, I.la);
    else if (W <= 192) cm = slip_ratio_cmp_reg<3>(I.x, I.lx, J.a, J.la, J.x, J.lx, I.a, I.la);
    else if (W <= 256) cm = slip_ratio_cmp_reg<4>(I.x, I.lx, J.a, J.la, J.x, J.lx, I.a, I.la);
    else {
        cnt[1]++;
        if (!scr || W > A.wcap) {                                    /* (W <= wcap: the host sized it from maxdig) */
            if (slip_lane() == 0) *A.err = 1;
            return 0;
        }
        dig_t *P = scr, *Q = scr + A.wcap;
        wb_mul_lo(P, I.x, I.lx, J.a, J.la, W);
        wb_mul_lo(Q, J.x, J.lx, I.a, I.la, W);
        const int lp = wb_len(P, W), lq = wb_len(Q, W);
        cm = wb_cmp(P, lp, Q, lq);
        slip_wave_sync();
    }
    return I.sx * cm;
}

/* does entry i come before entry j among equal ratios: the smaller (key[idx], idx) */
SLIP_DEV int slip_ratio_before(const SlipRatioArgs &A, int i, int j)
{
    const int32_t ii = A.oidx ? A.oidx[i] : i, ij = A.oidx ? A.oidx[j] : j;
    const int32_t ki = A.key ? A.key[ii] : 0, kj = A.key ? A.key[ij] : 0;
    return ki != kj ? ki < kj : ii < ij;
}

/* the best of count >= 1 entries pos[0..count) of problem c and the ties it stands for; wt[t]: the entries that pos[t]
 * already stands for (NULL: one each) */
SLIP_DEV void slip_ratio_fold(const SlipRatioArgs &A, int c, const int32_t *pos, const int32_t *wt, int count, dig_t *scr,
                              unsigned long long *cnt, int *best_out, int *ties_out)
{
    int best = pos[0], ties = wt ? wt[0] : 1;
    for (int t = 1; t < count; t++) {
        const int p = pos[t], w = wt ? wt[t] : 1;
        const int cm = slip_ratio_cmp(A, c, p, best, scr, cnt);
        if (cm < 0) { best = p; ties = w; }
        else if (cm == 0) { ties += w; if (slip_ratio_before(A, p, best)) best = p; }
    }
    *best_out = best; *ties_out = ties;
}

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_ratio_kernel(SlipRatioArgs A)
#else
static void slip_ratio_body(SlipRatioArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    unsigned long long cnt[2] = {0, 0};
    if (A.phase <= 1) {
        const int64_t rpp = ((int64_t) A.n + SLIP_WAVE - 1) / SLIP_WAVE, rounds = rpp * A.nprob;
        unsigned long long total = 0;
        for (int64_t r = wave0; r < rounds; r += nwaves) {
            const int c = (int)(r / rpp);
            const int64_t i = (r - (int64_t) c * rpp) * SLIP_WAVE + lane, it = (int64_t) c * A.n + i;
            if (A.phase == 1) {
                const int take = i < A.n && A.lokey[it] != INT64_MAX && A.lokey[it] <= A.minhi[c];
                if (take) A.cand[(int64_t) c * A.n + slip_atomic_add_i32(A.ncand + c, 1)] = (int32_t) i;
                total += (unsigned long long) slip_popc64(slip_ballot(take));
                continue;
            }
            int64_t lo = INT64_MAX, hi = INT64_MAX;
            int el = 0;
            uint32_t dx = 0, da = 0;
            if (i < A.n) {
                const SlipRatioEnt E = slip_ratio_ent(A, c, (int) i);
                el = !A.alen || (E.la > 0 && (A.alen[(int64_t) c * A.pstride + i] < 0 ? -1 : 1) == A.asense);
                if (el && E.sx == 0) lo = hi = 0;
                else if (el) {
                    const int64_t bn = 32 * (int64_t) E.lx - slip_clz32(E.x[E.lx - 1]), bd = E.a ? 32 * (int64_t) E.la - slip_clz32(E.a[E.la - 1]) : 1;
                    const uint64_t n64 = slip_lead64(E.x, E.lx), d64 = E.a ? slip_lead64(E.a, E.la) : 1ull << 63;
                    const int k = n64 < d64 ? 64 : 63;
                    const uint64_t Qs = (k == 64 ? slip_div128by64(n64, 0, d64) : slip_div128by64(n64 >> 1, n64 << 63, d64)) >> 2;
                    const int64_t e = bn - bd - k + 2, kd = slip_ratio_key(Qs - 1, e), ku = slip_ratio_key(Qs + 2, e) + 1;
                    lo = E.sx < 0 ? -ku : kd; hi = E.sx < 0 ? -kd : ku;
                }
                if (el) { dx = (uint32_t) E.lx; da = (uint32_t) E.la; }
                A.lokey[it] = lo;
            }
            const int nel = slip_popc64(slip_ballot(el));
            const int64_t mh = slip_wave_min_i64(hi);
            dx = slip_wave_max_u32(dx); da = slip_wave_max_u32(da);
            if (lane == 0 && nel) {
                slip_agent_min_i64(A.minhi + c, mh);
                slip_atomic_add_i32(A.nelig + c, nel);
                slip_atomic_max_i32(A.maxdig + 0, (int32_t) dx); slip_atomic_max_i32(A.maxdig + 1, (int32_t) da);
            }
            total += (unsigned long long) nel;
        }
        if (lane == 0 && total) slip_atomic_add_u64(A.paths + A.phase, total);
        return;
    }
    dig_t *scr = A.scratch ? A.scratch + wave0 * 2 * (int64_t) A.wcap : (dig_t *) 0;
    if (A.phase == 2) {
        const int64_t items = (int64_t) A.nprob * A.nchunk;
        for (int64_t it = wave0; it < items; it += nwaves) {
            const int c = (int)(it / A.nchunk), k = (int)(it - (int64_t) c * A.nchunk);
            const int nc = A.ncand[c], t0 = k * SLIP_RATIO_CHUNK;
            if (t0 >= nc) continue;
            int best, ties;
            slip_ratio_fold(A, c, A.cand + (int64_t) c * A.n + t0, (const int32_t *) 0, nc - t0 < SLIP_RATIO_CHUNK ? nc - t0 : SLIP_RATIO_CHUNK,
                            scr, cnt, &best, &ties);
            if (lane == 0) { A.cwpos[it] = best; A.cwties[it] = ties; }
        }
    } else {
        for (int64_t c = wave0; c < A.nprob; c += nwaves) {
            const int nc = A.ncand[c];
            int best = -1, ties = 0;
            if (nc > 0) slip_ratio_fold(A, (int) c, A.cwpos + c * A.nchunk, A.cwties + c * A.nchunk, (nc + SLIP_RATIO_CHUNK - 1) / SLIP_RATIO_CHUNK,
                                        scr, cnt, &best, &ties);
            if (lane == 0) {
                A.best[c] = best < 0 ? -1 : (A.oidx ? A.oidx[best] : best);
                A.nties[c] = ties;
                if (A.wlen) {
                    const int64_t e = c * A.pstride + (best < 0 ? 0 : best);
                    A.wlen[2 * c] = best < 0 ? 0 : A.xlen[e]; A.woff[2 * c] = best < 0 ? 0 : A.xoff[e];
                    A.wlen[2 * c + 1] = best < 0 ? 0 : A.alen[e]; A.woff[2 * c + 1] = best < 0 ? 0 : A.aoff[e];
                }
            }
        }
    }
    if (lane == 0) {
        if (cnt[0]) slip_atomic_add_u64(A.paths + 2, cnt[0]);
        if (cnt[1]) slip_atomic_add_u64(A.paths + 3, cnt[1]);
    }
}

/* Exact pricing (slip_hip_factor_price): the record work between the transposed substitution, slip_product_kernel
 * and slip_ratio_kernel.  Every phase takes `count` entries one to a lane, a wave's 64 entries a round (the loops are
 * wave-uniform); no limb moves.
 * phase 0, the record gather: the substitution leaves its output by pivot position p, the column view of a matrix indexes x
 *   by row id i, pinv[i] = p: xlen[v*n + i] = olen[v*n + pinv[i]] and the offsets likewise, count = n * the vectors.
 * phase 1, the widest item: the maximum of w[0..count) into wmax[0], one atomic per wave (the widths of slip_product_kernel's
 *   phase 0: the host sizes the memory path's scratch from it).
 * phase 2, one lane per problem, count = nprob: vsign[c] = the sign of the winner's x-side value over det (dneg: det < 0)
 *   from its signed digit count, 0 when best[c] = -1; with wlen, the records of the winners' slab of a selection without
 *   denominators (entry 2c: the winner's x record, 2c + 1: empty). */
struct SlipPriceArgs {
    int32_t phase, n, dneg; int64_t count, pstride;
    const int32_t *pinv, *olen; const int64_t *ooff; int32_t *xlen; int64_t *xoff;        /* phase 0                          */
    const int32_t *w; int32_t *wmax;                                                       /* phase 1                          */
    const int32_t *best, *rlen; const int64_t *soff;                                       /* phase 2: x of problem c at c * pstride */
    int32_t *vsign, *wlen; int64_t *woff;
};

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_price_kernel(SlipPriceArgs A)
#else
static void slip_price_body(SlipPriceArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    const int64_t rounds = (A.count + SLIP_WAVE - 1) / SLIP_WAVE;
    uint32_t wm = 0;
    for (int64_t r = wave0; r < rounds; r += nwaves) {
        const int64_t t = r * SLIP_WAVE + lane;
        if (A.phase == 0) {
            if (t < A.count) {
                const int64_t v = t / A.n, s = v * A.n + A.pinv[t - v * A.n];
                A.xlen[t] = A.olen[s]; A.xoff[t] = A.ooff[s];
            }
        } else if (A.phase == 1) {
            const uint32_t w = slip_wave_max_u32(t < A.count ? (uint32_t) A.w[t] : 0u);
            if (w > wm) wm = w;
        } else if (t < A.count) {
            const int32_t b = A.best[t];
            const int64_t e = t * A.pstride + (b < 0 ? 0 : b);
            const int32_t sx = b < 0 ? 0 : A.rlen[e];
            A.vsign[t] = sx == 0 ? 0 : (((sx < 0) != (A.dneg != 0)) ? -1 : 1);
            if (A.wlen) {
                A.wlen[2 * t] = sx; A.woff[2 * t] = b < 0 ? 0 : A.soff[e];
                A.wlen[2 * t + 1] = 0; A.woff[2 * t + 1] = 0;
            }
        }
    }
    if (A.phase == 1 && lane == 0 && wm) slip_atomic_max_i32(A.wmax, (int32_t) wm);
}

/* Bounds in the exact selections (slip_hip_factor_ratio_test_bounded, slip_hip_factor_bound_test and their handle-less
 * forms): the numerators slip_ratio_kernel selects on, formed from a solve's output and a set of bounds
 * l_i = lonum_i / bd, u_i = hinum_i / bd.  With s = sign(d_c) and
 *     G(b) = s * bd * x_i - |d_c| * b
 * mode 0 (ratio test) stages s * N_i: G(lonum_i) for an entry heading for its lower bound (sense * s * a_i > 0, bit 0 of
 * kind), -G(hinum_i) for one heading for its upper bound (sense * s * a_i < 0, bit 1), and the a record sense * |a_i| on
 * a_i's own limbs, so that the selection runs with asense = sense and no flip whatever the sign of d_c (one d per problem
 * in the handle-less form); mode 1 (bound test) stages v_i = max(Vlo_i, Vhi_i), Vlo_i = -G(lonum_i), Vhi_i = G(hinum_i)
 * (the lower side on equality), over the denominator record 1 when v_i > 0 and 0 otherwise.  Entry i of problem c is
 * entry c * xstride + i of x (c * astride + i of a) and entry c * n + i of every array written here; its bounds and kind are
 * those of idx = oidx[i].
 *
 * phase 0, classify and size, one lane per entry (a wave's 64 entries are of one problem): cls = the sides to form (bit 0
 *   lower, bit 1 upper; 0: not eligible) | the path << 2, w = the digits the entry owns in the staging slab (W =
 *   max(dig(bd) + dig(x), dig(d) + dig(bound)) + 1 with an absent factor's term 0; dig(x) on path 0), the a record in mode
 *   0; the widest w and the widest w of the wave paths go to wmax[0], wmax[1], one atomic each per wave.
 * phase 1, the lane pass, one lane per entry: path 1, both products of at most four digits, finished in 128-bit pieces.
 * phase 2, the wave pass, one wave per entry, wave-uniform: path 0 (bd = 1 and every bound that counts is zero) copies |x|;
 *   path 2, both products of at most 256 digits by their operands' bit lengths (the class D = 1 .. 4 is kept in cls >> 4),
 *   forms them in registers (slip_check_mac_reg) and G in sign and magnitude: a comparison and a subtraction, or a sum
 *   whose carry is digit 64 D; path 3 forms G modulo B^Wp, Wp = (W + 1) & ~1, in the entry's own staging region with
 *   the products in this wave's scratch (2 * wcap digits: a product, and the second side of a bound test), the top bit
 *   being the sign as in slip_product_kernel.
 *   Every path leaves the magnitude in whole limbs and the trimmed signed digit count in rlen.
 * phase 3, one lane per problem: side[c] from cls at the winner (pos: the entry of a reported index), and the records of the
 *   winners' numerators with the sign of d_c taken out again.
 * paths: entries by the path that formed them. */
struct SlipBoundArgs {
    int32_t n, nprob, phase, mode, sense, bdunit;
    int64_t xstride, astride;
    const int32_t *xlen; const int64_t *xoff; const uint64_t *xlimbs;              /* x: signed digit counts, limb offsets   */
    const int32_t *alen; const int64_t *aoff; const uint64_t *alimbs;              /* a likewise (mode 0)                    */
    const int32_t *dlen; const int64_t *doff; const uint64_t *dlimbs;              /* d_c: entry c                           */
    const int32_t *oidx, *pos;                                                     /* reported index of entry i; its inverse */
    const int32_t *kind;                                                           /* by reported index, as lo and hi        */
    const int32_t *lolen; const int64_t *looff; const uint64_t *lolimbs;
    const int32_t *hilen; const int64_t *hioff; const uint64_t *hilimbs;
    int32_t bddig; const uint64_t *bdlimbs;                                        /* bd > 0, trimmed                        */
    int32_t *cls, *w, *wmax;
    int32_t *alen2; int64_t *aoff2;                                                /* the a records of the selection         */
    const int64_t *soff; uint64_t *stage; int32_t *rlen;                           /* staging slab, signed digit counts      */
    dig_t *scratch; int32_t wcap;                                                  /* path 3: 2 * wcap digits per wave       */
    const int32_t *best; int32_t *side;                                            /* phase 3, per problem                   */
    int32_t *wnlen, *walen; int64_t *wnoff, *waoff;                                /* the winners' records, or NULL          */
    unsigned long long *paths;
};

/* an operand: its trimmed digits and its sign */
struct SlipBoundOp { const dig_t *p; int l, s; };
SLIP_DEV SlipBoundOp slip_bound_op(const int32_t *len, const int64_t *off, const uint64_t *limbs, int64_t e)
{
    SlipBoundOp o;
    const int32_t sl = len[e];
    o.p = (const dig_t *)(limbs + off[e]);
    o.l = slip_trim_digits(o.p, slip_abs(sl));
    o.s = o.l == 0 ? 0 : (sl < 0 ? -1 : 1);
    return o;
}

/* the operands of entry i of problem c whose sides are `sides` */
struct SlipBoundEnt { SlipBoundOp X, BD, Dn, LO, HI; int sides, mode; };
SLIP_DEV SlipBoundEnt slip_bound_ent(const SlipBoundArgs &A, int c, int i, int sides)
{
    SlipBoundEnt E;
    const int idx = A.oidx ? A.oidx[i] : i;
    E.sides = sides; E.mode = A.mode;
    E.X = slip_bound_op(A.xlen, A.xoff, A.xlimbs, (int64_t) c * A.xstride + i);
    E.Dn = slip_bound_op(A.dlen, A.doff, A.dlimbs, c);
    E.BD.p = (const dig_t *) A.bdlimbs; E.BD.l = A.bddig; E.BD.s = 1;
    E.LO.p = (const dig_t *) 0; E.LO.l = 0; E.LO.s = 0; E.HI = E.LO;
    if (sides & 1) E.LO = slip_bound_op(A.lolen, A.looff, A.lolimbs, idx);
    if (sides & 2) E.HI = slip_bound_op(A.hilen, A.hioff, A.hilimbs, idx);
    return E;
}

/* side q (1 lower, 2 upper) of an entry: the value staged is s1 * bd * |x| + s2 * |d| * |b|, b = *B */
SLIP_DEV void slip_bound_terms(const SlipBoundEnt &E, int q, const SlipBoundOp **B, int *s1, int *s2)
{
    const int f = ((q == 1) == (E.mode == 1)) ? -1 : 1;
    *B = q == 1 ? &E.LO : &E.HI;
    *s1 = f * E.Dn.s * E.X.s; *s2 = -f * (*B)->s;
}

/* is the signed number (sg2, |.| = m2) greater than (sg1, m1); cm = the comparison of the magnitudes m2 against m1 */
SLIP_DEV int slip_bound_greater(int sg2, int sg1, int cm) { return sg2 != sg1 ? sg2 > sg1 : (sg1 > 0 ? cm > 0 : sg1 < 0 ? cm < 0 : 0); }

/* lane pass: an operand of at most four digits as one 128-bit number */
SLIP_DEV slip_u128 slip_bound_load128(const SlipBoundOp &o)
{
    slip_u128 v = 0;
    for (int k = o.l - 1; k >= 0; k--) v = (v << 32) | o.p[k];
    return v;
}

/* lane pass: side q as sign, 128-bit magnitude and the carry above it */
SLIP_DEV void slip_bound_eval_lane(const SlipBoundEnt &E, int q, int *sg, slip_u128 *mag, uint32_t *top)
{
    const SlipBoundOp *Bv; int s1, s2;
    slip_bound_terms(E, q, &Bv, &s1, &s2);
    const slip_u128 P = s1 ? slip_bound_load128(E.X) * slip_bound_load128(E.BD) : 0, Q = s2 ? slip_bound_load128(E.Dn) * slip_bound_load128(*Bv) : 0;
    *top = 0;
    if (s1 == s2 || !s1 || !s2) { *mag = P + Q; *top = *mag < P ? 1u : 0u; *sg = s1 ? s1 : s2; }
    else if (P >= Q) { *mag = P - Q; *sg = P == Q ? 0 : s1; }
    else { *mag = Q - P; *sg = s2; }
}

/* the product of two operands that fits 64*D digits, the shorter one walked */
template <int D> SLIP_DEV WR<D> slip_bound_mul_reg(const SlipBoundOp &a, const SlipBoundOp &b)
{
    return a.l <= b.l ? slip_check_mac_reg<D>(wr_zero<D>(), a.p, a.l, b.p, b.l, 0) : slip_check_mac_reg<D>(wr_zero<D>(), b.p, b.l, a.p, a.l, 0);
}

/* wave pass, registers: side q, both products below B^(64*D) (the class is chosen from their bit lengths), in sign and
 * magnitude: *sg the sign, *top the digit 64*D of the magnitude (the carry of a sum: 0 or 1), the digits below it returned */
template <int D> SLIP_DEV WR<D> slip_bound_eval_reg(const SlipBoundEnt &E, int q, int *sg, uint32_t *top)
{
    const SlipBoundOp *Bv; int s1, s2;
    slip_bound_terms(E, q, &Bv, &s1, &s2);
    const WR<D> P = s1 ? slip_bound_mul_reg<D>(E.X, E.BD) : wr_zero<D>(), Q = s2 ? slip_bound_mul_reg<D>(E.Dn, *Bv) : wr_zero<D>();
    *top = 0;
    if (!s1 || !s2 || s1 == s2) {
        const WR<D> R = wr_addsub<D>(P, Q, 0);
        *top = wr_cmp<D>(R, P) < 0 ? 1u : 0u;                      /* the sum wrapped */
        *sg = s1 ? s1 : s2;
        return R;
    }
    const int cm = wr_cmp<D>(P, Q);
    *sg = cm > 0 ? s1 : cm < 0 ? s2 : 0;
    return cm >= 0 ? wr_addsub<D>(P, Q, 1) : wr_addsub<D>(Q, P, 1);
}

/* wave pass, registers: the entry's value into out in whole limbs; its signed digit count, *side the side it is of */
template <int D> SLIP_DEV int slip_bound_entry_reg(const SlipBoundEnt &E, dig_t *out, int *side)
{
    int sg, q = (E.sides & 1) ? 1 : 2;
    uint32_t top;
    WR<D> V = slip_bound_eval_reg<D>(E, q, &sg, &top);
    if (E.sides == 3) {
        int sg2; uint32_t top2;
        const WR<D> V2 = slip_bound_eval_reg<D>(E, 2, &sg2, &top2);
        const int cm = top2 != top ? (top2 > top ? 1 : -1) : wr_cmp<D>(V2, V);
        if (slip_bound_greater(sg2, sg, cm)) { V = V2; sg = sg2; top = top2; q = 2; }
    }
    /* (a carry means a product of 64*D digits: the entry owns at least 64*D + 2 digits of the staging slab) */
    const int len = top ? 64 * D + 1 : wr_len<D>(V);
    wr_store<D>(out, V, top ? 64 * D : (len + 1) & ~1);
    if (top && slip_lane() < 2) out[64 * D + slip_lane()] = slip_lane() == 0 ? 1u : 0u;
    *side = q;
    return sg < 0 ? -len : len;
}

/* wave pass, memory: side q modulo B^Wp into dst (prod: Wp digits of scratch); its signed digit count */
SLIP_DEV int slip_bound_eval_wide(const SlipBoundEnt &E, int q, int Wp, dig_t *dst, dig_t *prod)
{
    const SlipBoundOp *Bv; int s1, s2;
    slip_bound_terms(E, q, &Bv, &s1, &s2);
    for (int k = slip_lane(); k < Wp; k += SLIP_WAVE) dst[k] = 0u;
    slip_wave_sync();
    if (s1) { wb_mul_lo(prod, E.X.p, E.X.l, E.BD.p, E.BD.l, Wp); wb_addsub(dst, dst, Wp, prod, Wp, Wp, s1 < 0); }
    if (s2) { wb_mul_lo(prod, E.Dn.p, E.Dn.l, Bv->p, Bv->l, Wp); wb_addsub(dst, dst, Wp, prod, Wp, Wp, s2 < 0); }
    const int neg = (int)(dst[Wp - 1] >> 31);
    if (neg) wb_addsub(dst, (const dig_t *) 0, 1, dst, Wp, Wp, 1, 0u);
    const int len = wb_len(dst, Wp);
    return neg ? -len : len;
}

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_bound_kernel(SlipBoundArgs A)
#else
static void slip_bound_body(SlipBoundArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    if (A.phase <= 1) {
        const int64_t rpp = ((int64_t) A.n + SLIP_WAVE - 1) / SLIP_WAVE, rounds = rpp * A.nprob;
        uint32_t wall = 0, wwave = 0;
        unsigned long long total = 0;
        for (int64_t r = wave0; r < rounds; r += nwaves) {
            const int c = (int)(r / rpp);
            const int64_t i = (r - (int64_t) c * rpp) * SLIP_WAVE + lane, e = (int64_t) c * A.n + i;
            if (A.phase == 1) {
                const int code = i < A.n ? A.cls[e] : 0, take = (code & 3) != 0 && ((code >> 2) & 3) == 1;
                if (take) {
                    const SlipBoundEnt E = slip_bound_ent(A, c, (int) i, code & 3);
                    int sg, q = (code & 1) ? 1 : 2;
                    slip_u128 mag; uint32_t top;
                    slip_bound_eval_lane(E, q, &sg, &mag, &top);
                    if ((code & 3) == 3) {
                        int sg2; slip_u128 mag2; uint32_t top2;
                        slip_bound_eval_lane(E, 2, &sg2, &mag2, &top2);
                        const int cm = top2 != top ? (top2 > top ? 1 : -1) : mag2 != mag ? (mag2 > mag ? 1 : -1) : 0;
                        if (slip_bound_greater(sg2, sg, cm)) { sg = sg2; mag = mag2; top = top2; q = 2; }
                    }
                    const uint64_t l0 = (uint64_t) mag, l1 = (uint64_t)(mag >> 64);
                    const int len = top ? 9 : l1 ? (l1 >> 32 ? 8 : 7) : l0 ? (l0 >> 32 ? 6 : 5) : 4;      /* digits + 4 */
                    uint64_t *out = A.stage + A.soff[e];
                    if (len > 4) out[0] = l0;
                    if (len > 6) out[1] = l1;
                    if (len > 8) out[2] = top;
                    A.rlen[e] = sg < 0 ? -(len - 4) : len - 4;
                    if (A.mode) { A.alen2[e] = sg > 0 ? 1 : 0; A.aoff2[e] = 0; A.cls[e] = q | (1 << 2); }
                }
                total += (unsigned long long) slip_popc64(slip_ballot(take));
                continue;
            }
            uint32_t W = 0, Ww = 0;
            if (i < A.n) {
                const int idx = A.oidx ? A.oidx[i] : (int) i, k = A.kind[idx];
                const int32_t sd = A.dlen[c];
                int sides = k & 3;
                if (!A.mode) {
                    const int64_t ea = (int64_t) c * A.astride + i;
                    const SlipBoundOp Av = slip_bound_op(A.alen, A.aoff, A.alimbs, ea);
                    const int t = A.sense * (sd < 0 ? -1 : 1) * Av.s;
                    sides = t > 0 ? (k & 1) : t < 0 ? (k & 2) : 0;
                    A.alen2[e] = sides ? A.sense * Av.l : 0; A.aoff2[e] = A.aoff[ea];
                } else { A.alen2[e] = 0; A.aoff2[e] = 0; }
                int code = 0;
                if (sides) {
                    const SlipBoundEnt E = slip_bound_ent(A, c, (int) i, sides);
                    const int lb = E.LO.l > E.HI.l ? E.LO.l : E.HI.l;
                    int path = 0;
                    if (A.bdunit && lb == 0) W = (uint32_t) E.X.l;
                    else {
                        /* pd: the digits neither product exceeds, from the operands' bit lengths */
                        const int blo = wb_bits(E.LO.p, E.LO.l), bhi = wb_bits(E.HI.p, E.HI.l);
                        const int w1 = E.X.l ? E.BD.l + E.X.l : 0, w2 = lb ? E.Dn.l + lb : 0;
                        const int p1 = E.X.l ? (wb_bits(E.BD.p, E.BD.l) + wb_bits(E.X.p, E.X.l) + 31) >> 5 : 0;
                        const int p2 = lb ? (wb_bits(E.Dn.p, E.Dn.l) + (blo > bhi ? blo : bhi) + 31) >> 5 : 0, pd = p1 > p2 ? p1 : p2;
                        W = (uint32_t)((w1 > w2 ? w1 : w2) + 1);
                        path = w1 <= 4 && w2 <= 4 ? 1 : pd <= 256 ? 2 : 3;
                        if (path == 2) code = ((pd + 63) >> 6) << 4;
                    }
                    if (path == 3) Ww = W;
                    code |= sides | (path << 2);
                }
                A.cls[e] = code; A.w[e] = (int32_t) W; A.rlen[e] = 0;
            }
            W = slip_wave_max_u32(W); Ww = slip_wave_max_u32(Ww);
            if (W > wall) wall = W;
            if (Ww > wwave) wwave = Ww;
        }
        if (A.phase == 0 && lane == 0) {
            if (wall) slip_atomic_max_i32(A.wmax + 0, (int32_t) wall);
            if (wwave) slip_atomic_max_i32(A.wmax + 1, (int32_t) wwave);
        }
        if (A.phase == 1 && lane == 0 && total) slip_atomic_add_u64(A.paths + 1, total);
        return;
    }
    if (A.phase == 2) {
        dig_t *prod = A.scratch ? A.scratch + wave0 * 2 * (int64_t) A.wcap : (dig_t *) 0, *alt = prod ? prod + A.wcap : (dig_t *) 0;
        const int64_t items = (int64_t) A.n * A.nprob;
        unsigned long long cnt[4] = {0, 0, 0, 0};
        for (int64_t e = wave0; e < items; e += nwaves) {
            const int code = A.cls[e], sides = code & 3, path = (code >> 2) & 3, cls = code >> 4;
            if (!sides || path == 1) continue;
            const int c = (int)(e / A.n), i = (int)(e - (int64_t) c * A.n);
            const SlipBoundEnt E = slip_bound_ent(A, c, i, sides);
            const int W = A.w[e];
            dig_t *out = (dig_t *)(A.stage + A.soff[e]);
            int len, q = (sides & 1) ? 1 : 2;
            if (path == 0) {
                /* every bound that counts is zero and bd = 1: the value is s1 * |x| */
                const SlipBoundOp *Bv; int sg, s2;
                slip_bound_terms(E, q, &Bv, &sg, &s2);
                if (sides == 3 && -sg > sg) { sg = -sg; q = 2; }
                wb_copy_pad(out, E.X.p, E.X.l);
                len = sg < 0 ? -E.X.l : E.X.l;
            } else if (path == 2 && cls == 1) len = slip_bound_entry_reg<1>(E, out, &q);
            else if (path == 2 && cls == 2) len = slip_bound_entry_reg<2>(E, out, &q);
            else if (path == 2 && cls == 3) len = slip_bound_entry_reg<3>(E, out, &q);
            else if (path == 2) len = slip_bound_entry_reg<4>(E, out, &q);
            else {
                const int Wp = (W + 1) & ~1;                       /* at most wcap: the host sized it from wmax */
                len = slip_bound_eval_wide(E, q, Wp, out, prod);
                if (sides == 3) {
                    const int len2 = slip_bound_eval_wide(E, 2, Wp, alt, prod);
                    const int sg = len > 0 ? 1 : len < 0 ? -1 : 0, sg2 = len2 > 0 ? 1 : len2 < 0 ? -1 : 0;
                    if (slip_bound_greater(sg2, sg, wb_cmp(alt, slip_abs(len2), out, slip_abs(len)))) {
                        for (int k = lane; k < Wp; k += SLIP_WAVE) out[k] = alt[k];
                        slip_wave_sync();
                        len = len2; q = 2;
                    }
                }
            }
            if (lane == 0) {
                A.rlen[e] = len;
                if (A.mode) { A.alen2[e] = len > 0 ? 1 : 0; A.aoff2[e] = 0; A.cls[e] = q | (path << 2); }
            }
            cnt[path]++;
        }
        if (lane == 0) for (int k = 0; k < 4; k++) if (cnt[k]) slip_atomic_add_u64(A.paths + k, cnt[k]);
        return;
    }
    const int64_t rounds = ((int64_t) A.nprob + SLIP_WAVE - 1) / SLIP_WAVE;
    for (int64_t r = wave0; r < rounds; r += nwaves) {
        const int64_t c = r * SLIP_WAVE + lane;
        if (c >= A.nprob) continue;
        const int32_t b = A.best[c];
        const int64_t e = c * A.n + (b < 0 ? 0 : (A.pos ? A.pos[b] : b));
        const int s = A.mode || A.dlen[c] > 0 ? 1 : -1;
        A.side[c] = b < 0 ? 0 : ((A.cls[e] & 3) == 1 ? -1 : 1);
        if (A.wnlen) {
            A.wnlen[c] = b < 0 ? 0 : s * A.rlen[e]; A.wnoff[c] = b < 0 ? 0 : A.soff[e];
            if (A.walen) { A.walen[c] = b < 0 ? 0 : s * A.alen2[e]; A.waoff[c] = b < 0 ? 0 : A.aoff2[e]; }
        }
    }
}

/* Exact pivot update (slip_hip_pivot_update, slip_hip_factor_solve_update, slip_hip_factor_step): per problem c and
 * entry i the signed number
 *     R_i = (P_c * V_i - T_c * A_i) / D_c
 * from the numerators V and A of nprob problems and one P_c, T_c and (optionally) one nonzero D_c each: one IPGE step per entry,
 * the update of a basic solution X over d to X' over A_r when position r leaves (P = A_r, T = X_r, D = d).  Without D nothing
 * is divided.  Entry i of problem c is entry c * vstride + i of v (c * astride + i of a); what is written here is indexed by
 * the SLOT c * n + oidx[i] (oidx NULL: i), the index the result is reported under.  place[c] (NULL: none) is a reported index
 * whose slot receives T_c itself, -1 for no such slot, -2 for a problem that is skipped (all its slots come back empty).
 *
 * phase 0, classify and size, one lane per entry (a wave's 64 entries are of one problem).  With b1 = bits(P) + bits(V) and
 *   b2 = bits(T) + bits(A) (0 for a term with a zero factor) |P V - T A| < 2^nb, nb = max(b1, b2) + 1, nd = ceil(nb / 32) its
 *   digits; an exact quotient is below 2^(nb - bits(D) + 1).  w = the digits the slot owns in the staging slab: those of the
 *   quotient's bound (of nd without D, of T_c in the placed slot); the widest to wmax[0], the widest two's-complement numerator
 *   of the memory path (nd + 1) to wmax[1], one atomic each per wave.  cls = path | class << 2:
 *     path 0: both terms are zero (or the slot is placed or skipped): nothing is computed;
 *     path 1: both products of at most four digits by the factors' digit counts and D of at most two: a lane;
 *     path 2: nd <= 256: a wavefront in registers, class = ceil(nd / 64) = the D of WR<D>;
 *     path 3: above: a wavefront through its scratch in global memory.
 *   The entries by path go to paths[0 .. 3].
 * phase 1, the lane pass, one lane per entry: both products as 128-bit numbers, the signed sum as sign, 128-bit magnitude and
 *   carry; the division 2-adic (slip_inv64, one Newton step to 128 bits), exact iff the low ctz(D) bits of the numerator are
 *   zero and the 192-bit product of the quotient and D's odd part has nothing above the numerator's 128 bits but its carry.
 * phase 2, the wave pass, one wavefront per entry, wave-uniform.  Registers: the products by slip_check_mac_reg, the
 *   subtraction in sign and magnitude (no wrap: nd digits fit the class), then wr_div_hensel on the numerator shifted by
 *   ctz(D), computed to W = its digits + 1 -- in WR<D + 1> when that digit is not there.  Memory: the sum modulo B^Wp in two's
 *   complement (wb_mul_lo, wb_addsub), the inverse of D's odd part by wb_inv_extend to W digits, one wb_mul_lo.
 *   Exactness, both ways: the numerator's trailing zero bits cover those of D, and the W-digit 2-adic quotient q has no digit
 *   at or above W - len(D_odd): then q * D_odd < B^W is congruent to the numerator modulo B^W and below it, hence equal; an
 *   exact quotient of a numerator below B^(W-1) by D_odd >= B^(len - 1) passes.  An inexact entry keeps length 0 and counts in
 *   ninexact[c], one atomic per wave.
 * phase 3, one wavefront per problem: T_c copied into the slot place[c] names, its record set.
 * phase 4 (the fused step, before phase 0), one lane per problem: from best[c] of the selection the records of P_c = the a
 *   numerator and T_c = the x numerator of the winner (in place in the solve's output) and place[c] = best[c]; best[c] < 0
 *   gives empty records and place -2. */
struct SlipPivotArgs {
    int32_t n, nprob, phase;
    int64_t vstride, astride;
    const int32_t *vlen; const int64_t *voff; const uint64_t *vlimbs;              /* v: signed digit counts, limb offsets   */
    const int32_t *alen; const int64_t *aoff; const uint64_t *alimbs;              /* a likewise                             */
    const int32_t *plen; const int64_t *poff; const uint64_t *plimbs;              /* P_c: entry c                           */
    const int32_t *tlen; const int64_t *toff; const uint64_t *tlimbs;              /* T_c: entry c                           */
    const int32_t *dlen; const int64_t *doff; const uint64_t *dlimbs;              /* D_c: entry c; dlen NULL: no division   */
    const int32_t *oidx, *pos;                                                     /* reported index of entry i; its inverse */
    const int32_t *place;                                                          /* per problem, or NULL                   */
    int32_t *cls, *w, *wmax;                                                       /* by slot; wmax: two widths              */
    const int64_t *soff; uint64_t *stage; int32_t *rlen;                           /* staging slab, signed digit counts      */
    dig_t *scratch; int32_t wcap, wscr;                                            /* per wave wscr digits: 7 * wcap, >= 328 */
    int32_t *ninexact;                                                             /* per problem                            */
    const int32_t *best;                                                           /* phase 4                                */
    int32_t *wplen, *wtlen, *wplace; int64_t *wpoff, *wtoff;
    unsigned long long *paths;
};

/* the operands of entry i of problem c */
struct SlipPivotEnt { SlipBoundOp P, V, T, A, Dn; int s1, s2, hasd; };
SLIP_DEV SlipPivotEnt slip_pivot_ent(const SlipPivotArgs &A, int c, int i)
{
    SlipPivotEnt E;
    E.P = slip_bound_op(A.plen, A.poff, A.plimbs, c);
    E.T = slip_bound_op(A.tlen, A.toff, A.tlimbs, c);
    E.V = slip_bound_op(A.vlen, A.voff, A.vlimbs, (int64_t) c * A.vstride + i);
    E.A = slip_bound_op(A.alen, A.aoff, A.alimbs, (int64_t) c * A.astride + i);
    E.hasd = A.dlen != (const int32_t *) 0;
    E.Dn.p = (const dig_t *) 0; E.Dn.l = 0; E.Dn.s = 1;
    if (E.hasd) E.Dn = slip_bound_op(A.dlen, A.doff, A.dlimbs, c);
    E.s1 = E.P.s * E.V.s; E.s2 = -E.T.s * E.A.s;                   /* the value is s1 |P||V| + s2 |T||A| */
    return E;
}

/* lane pass: the entry's quotient into out (at most cap digits); its signed digit count, *bad set when it is not exact */
SLIP_DEV int slip_pivot_entry_lane(const SlipPivotEnt &E, uint64_t *out, int cap, int *bad)
{
    const slip_u128 X = E.s1 ? slip_bound_load128(E.P) * slip_bound_load128(E.V) : 0, Y = E.s2 ? slip_bound_load128(E.T) * slip_bound_load128(E.A) : 0;
    slip_u128 mag; uint32_t top = 0; int sg;
    if (E.s1 == E.s2 || !E.s1 || !E.s2) { mag = X + Y; top = mag < X ? 1u : 0u; sg = E.s1 ? E.s1 : E.s2; }
    else if (X >= Y) { mag = X - Y; sg = X == Y ? 0 : E.s1; }
    else { mag = Y - X; sg = E.s2; }
    *bad = 0;
    if (sg == 0) return 0;
    if (E.hasd) {
        const uint64_t d = slip_bound_load128(E.Dn) & 0xFFFFFFFFFFFFFFFFull;
        const int z = slip_ctz64(d);
        const uint64_t dodd = d >> z;
        if (z && ((uint64_t) mag & ((1ull << z) - 1ull))) { *bad = 1; return 0; }
        if (z) { mag = (mag >> z) | ((slip_u128) top << (128 - z)); top = 0; }
        if (dodd != 1) {                                           /* (a unit odd part: the shifted numerator, carry and all, is the quotient) */
            slip_u128 inv = (slip_u128) slip_inv64(dodd);
            inv = inv * ((slip_u128) 2 - (slip_u128) dodd * inv);
            const slip_u128 q = mag * inv;
            /* bits 128 .. 191 of q * dodd: the carry of the numerator and nothing else (dodd >= 3: q itself fits 128 bits) */
            const uint64_t hi = (uint64_t)(((slip_u128)(uint64_t)(q >> 64) * dodd + (((slip_u128)(uint64_t) q * dodd) >> 64)) >> 64);
            if (hi != top) { *bad = 1; return 0; }
            mag = q; top = 0;
        }
        sg *= E.Dn.s;
    }
    const uint64_t l0 = (uint64_t) mag, l1 = (uint64_t)(mag >> 64);
    const int len = top ? 5 : l1 ? (l1 >> 32 ? 4 : 3) : (l0 >> 32 ? 2 : 1);
    if (len > cap) { *bad = 1; return 0; }
    out[0] = l0;
    if (len > 2) out[1] = l1;
    if (len > 4) out[2] = top;
    return sg < 0 ? -len : len;
}

/* wave pass, registers: the magnitude N (ln digits, ln < 64*D) over D_c into out; the quotient's digits, -1 when not exact */
template <int D> SLIP_DEV int slip_pivot_div_reg(const WR<D> &N, const SlipBoundOp &Dv, dig_t *out, int cap, dig_t *scratch)
{
    const int z = wb_ctz(Dv.p, Dv.l), ldo = (wb_bits(Dv.p, Dv.l) - z + 31) >> 5;
    int tz = 0;
#pragma unroll
    for (int q = D - 1; q >= 0; q--) {
        const uint64_t nz = slip_ballot(N.d[q] != 0);
        if (nz) { const int t = slip_ctz64(nz); tz = 32 * (64 * q + t) + slip_ctz32(slip_readlane(N.d[q], t)); }
    }
    if (tz < z) return -1;
    const WR<D> Ns = wr_shr<D>(N, z, scratch);
    const int W = wr_len<D>(Ns) + 1;
    if (W - ldo <= 0) return -1;                                   /* D_odd exceeds the numerator */
    const WR<D> Q = wr_div_hensel<D>(Ns, W, wr_load_shr<D>(Dv.p, Dv.l, z));
    const int lq = wr_len<D>(Q);
    if (lq > W - ldo || lq > cap) return -1;
    wr_store<D>(out, Q, (lq + 1) & ~1);
    return lq;
}

/* wave pass, registers: both products below B^(64*D) and their signed sum too; the entry's signed digit count */
template <int D> SLIP_DEV int slip_pivot_entry_reg(const SlipPivotEnt &E, dig_t *out, int cap, dig_t *scratch, int *bad)
{
    const WR<D> X = E.s1 ? slip_bound_mul_reg<D>(E.P, E.V) : wr_zero<D>(), Y = E.s2 ? slip_bound_mul_reg<D>(E.T, E.A) : wr_zero<D>();
    WR<D> N; int sg;
    if (!E.s1 || !E.s2 || E.s1 == E.s2) { N = wr_addsub<D>(X, Y, 0); sg = E.s1 ? E.s1 : E.s2; }
    else {
        const int cm = wr_cmp<D>(X, Y);
        sg = cm > 0 ? E.s1 : cm < 0 ? E.s2 : 0;
        N = cm >= 0 ? wr_addsub<D>(X, Y, 1) : wr_addsub<D>(Y, X, 1);
    }
    *bad = 0;
    if (sg == 0) return 0;
    int len = wr_len<D>(N);
    if (!E.hasd) {
        if (len > cap) { *bad = 1; return 0; }
        wr_store<D>(out, N, (len + 1) & ~1);
        return sg < 0 ? -len : len;
    }
    if (len < 64 * D) len = slip_pivot_div_reg<D>(N, E.Dn, out, cap, scratch);
    else {
        WR<D + 1> Nw;
#pragma unroll
        for (int q = 0; q < D; q++) Nw.d[q] = N.d[q];
        Nw.d[D] = 0u;
        len = slip_pivot_div_reg<D + 1>(Nw, E.Dn, out, cap, scratch);
    }
    if (len < 0) { *bad = 1; return 0; }
    return sg * E.Dn.s < 0 ? -len : len;
}

/* wave pass, memory: the same modulo B^Wp, Wp even and at most wcap, on seven buffers of wcap digits */
SLIP_DEV int slip_pivot_entry_wide(const SlipPivotEnt &E, int Wp, dig_t *buf, int wcap, dig_t *out, int cap, int *bad)
{
    dig_t *num = buf, *prod = buf + wcap, *T = prod + wcap, *Dd = T + wcap, *inv = Dd + wcap, *e1 = inv + wcap, *e2 = e1 + wcap;
    for (int k = slip_lane(); k < Wp; k += SLIP_WAVE) num[k] = 0u;
    slip_wave_sync();
    if (E.s1) { wb_mul_lo(prod, E.P.p, E.P.l, E.V.p, E.V.l, Wp); wb_addsub(num, num, Wp, prod, Wp, Wp, E.s1 < 0); }
    if (E.s2) { wb_mul_lo(prod, E.T.p, E.T.l, E.A.p, E.A.l, Wp); wb_addsub(num, num, Wp, prod, Wp, Wp, E.s2 < 0); }
    const int neg = (int)(num[Wp - 1] >> 31);
    if (neg) wb_addsub(num, (const dig_t *) 0, 1, num, Wp, Wp, 1, 0u);
    const int ln = wb_len(num, Wp);
    *bad = 0;
    if (ln == 0) return 0;
    if (!E.hasd) {
        if (ln > cap) { *bad = 1; return 0; }
        wb_copy_pad(out, num, ln);
        return neg ? -ln : ln;
    }
    const int z = wb_ctz(E.Dn.p, E.Dn.l), ldo = (wb_bits(E.Dn.p, E.Dn.l) - z + 31) >> 5;
    if (wb_ctz(num, ln) < z) { *bad = 1; return 0; }
    wb_copy_shr(T, num, ln, z, ln);
    const int lt = wb_len(T, ln), W = lt + 1;                     /* W <= ln + 1 <= Wp */
    if (W - ldo <= 0) { *bad = 1; return 0; }
    wb_copy_shr(Dd, E.Dn.p, E.Dn.l, z, ldo);
    wb_inv_extend(inv, 0, W, Dd, ldo, e1, e2);
    wb_mul_lo(prod, T, lt, inv, W, W);
    const int lq = wb_len(prod, W);
    if (lq > W - ldo || lq > cap) { *bad = 1; return 0; }
    wb_copy_pad(out, prod, lq);
    return (neg ? -1 : 1) * E.Dn.s < 0 ? -lq : lq;
}

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_pivot_kernel(SlipPivotArgs A)
#else
static void slip_pivot_body(SlipPivotArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    if (A.phase == 4) {
        const int64_t rounds = ((int64_t) A.nprob + SLIP_WAVE - 1) / SLIP_WAVE;
        for (int64_t r = wave0; r < rounds; r += nwaves) {
            const int64_t c = r * SLIP_WAVE + lane;
            if (c >= A.nprob) continue;
            const int32_t b = A.best[c];
            const int64_t p = b < 0 ? 0 : (A.pos ? A.pos[b] : b), ev = c * A.vstride + p, ea = c * A.astride + p;
            A.wplen[c] = b < 0 ? 0 : A.alen[ea]; A.wpoff[c] = b < 0 ? 0 : A.aoff[ea];
            A.wtlen[c] = b < 0 ? 0 : A.vlen[ev]; A.wtoff[c] = b < 0 ? 0 : A.voff[ev];
            A.wplace[c] = b < 0 ? -2 : b;
        }
        return;
    }
    if (A.phase <= 1) {
        const int64_t rpp = ((int64_t) A.n + SLIP_WAVE - 1) / SLIP_WAVE, rounds = rpp * A.nprob;
        uint32_t wall = 0, wwave = 0;
        unsigned long long cnt[4] = {0, 0, 0, 0};
        for (int64_t r = wave0; r < rounds; r += nwaves) {
            const int c = (int)(r / rpp);
            const int64_t i = (r - (int64_t) c * rpp) * SLIP_WAVE + lane;
            const int idx = i < A.n ? (A.oidx ? A.oidx[i] : (int) i) : 0;
            const int64_t slot = (int64_t) c * A.n + idx;
            if (A.phase == 1) {
                const int take = i < A.n && (A.cls[slot] & 3) == 1;
                int bad = 0;
                if (take) {
                    const SlipPivotEnt E = slip_pivot_ent(A, c, (int) i);
                    A.rlen[slot] = slip_pivot_entry_lane(E, A.stage + A.soff[slot], A.w[slot], &bad);
                }
                const uint64_t nb = slip_ballot(bad);
                if (nb && lane == 0) slip_atomic_add_i32(A.ninexact + c, slip_popc64(nb));
                continue;
            }
            uint32_t W = 0, Ww = 0;
            int path = -1;
            if (i < A.n) {
                const int pl = A.place ? A.place[c] : -1;
                int code = 0;
                path = 0;
                if (pl == idx) W = (uint32_t) slip_bound_op(A.tlen, A.toff, A.tlimbs, c).l;
                else if (pl != -2) {
                    const SlipPivotEnt E = slip_pivot_ent(A, c, (int) i);
                    if ((E.s1 || E.s2) && (!E.hasd || E.Dn.l)) {           /* (a zero D_c, which the host refuses: nothing) */
                        const int b1 = E.s1 ? wb_bits(E.P.p, E.P.l) + wb_bits(E.V.p, E.V.l) : 0;
                        const int b2 = E.s2 ? wb_bits(E.T.p, E.T.l) + wb_bits(E.A.p, E.A.l) : 0;
                        const int w1 = E.s1 ? E.P.l + E.V.l : 0, w2 = E.s2 ? E.T.l + E.A.l : 0;
                        const int nb = (b1 > b2 ? b1 : b2) + 1, nd = (nb + 31) >> 5;
                        const int qb = E.hasd ? nb - wb_bits(E.Dn.p, E.Dn.l) + 1 : nb;
                        W = qb > 0 ? (uint32_t)((qb + 31) >> 5) : 1u;
                        path = w1 <= 4 && w2 <= 4 && E.Dn.l <= 2 ? 1 : nd <= 256 ? 2 : 3;
                        if (path == 2) code = ((nd + 63) >> 6) << 2;
                        if (path == 3) Ww = (uint32_t)(nd + 1);
                        code |= path;
                    }
                }
                A.cls[slot] = code; A.w[slot] = (int32_t) W; A.rlen[slot] = 0;
            }
            for (int k = 0; k < 4; k++) cnt[k] += (unsigned long long) slip_popc64(slip_ballot(path == k));
            W = slip_wave_max_u32(W); Ww = slip_wave_max_u32(Ww);
            if (W > wall) wall = W;
            if (Ww > wwave) wwave = Ww;
        }
        if (A.phase == 0 && lane == 0) {
            if (wall) slip_atomic_max_i32(A.wmax + 0, (int32_t) wall);
            if (wwave) slip_atomic_max_i32(A.wmax + 1, (int32_t) wwave);
            for (int k = 0; k < 4; k++) if (cnt[k]) slip_atomic_add_u64(A.paths + k, cnt[k]);
        }
        return;
    }
    if (A.phase == 2) {
        dig_t *buf = A.scratch + wave0 * (int64_t) A.wscr;
        const int64_t items = (int64_t) A.n * A.nprob;
        for (int64_t e = wave0; e < items; e += nwaves) {
            const int c = (int)(e / A.n), i = (int)(e - (int64_t) c * A.n);
            const int64_t slot = (int64_t) c * A.n + (A.oidx ? A.oidx[i] : i);
            const int code = A.cls[slot], path = code & 3, cls = code >> 2;
            if (path < 2) continue;
            const SlipPivotEnt E = slip_pivot_ent(A, c, i);
            const int cap = A.w[slot];
            dig_t *out = (dig_t *)(A.stage + A.soff[slot]);
            int len, bad = 0;
            if (path == 2 && cls == 1) len = slip_pivot_entry_reg<1>(E, out, cap, buf, &bad);
            else if (path == 2 && cls == 2) len = slip_pivot_entry_reg<2>(E, out, cap, buf, &bad);
            else if (path == 2 && cls == 3) len = slip_pivot_entry_reg<3>(E, out, cap, buf, &bad);
            else if (path == 2) len = slip_pivot_entry_reg<4>(E, out, cap, buf, &bad);
            else {
                /* nd + 1 digits in whole limbs: at most wcap, the host sized it from wmax */
                const int b1 = E.s1 ? wb_bits(E.P.p, E.P.l) + wb_bits(E.V.p, E.V.l) : 0, b2 = E.s2 ? wb_bits(E.T.p, E.T.l) + wb_bits(E.A.p, E.A.l) : 0;
                const int Wp = ((((b1 > b2 ? b1 : b2) + 1 + 31) >> 5) + 2) & ~1;
                len = slip_pivot_entry_wide(E, Wp, buf, A.wcap, out, cap, &bad);
            }
            if (lane == 0) {
                A.rlen[slot] = len;
                if (bad) slip_atomic_add_i32(A.ninexact + c, 1);
            }
            slip_wave_sync();
        }
        return;
    }
    for (int64_t c = wave0; c < A.nprob; c += nwaves) {
        const int pl = A.place ? A.place[c] : -1;
        if (pl < 0) continue;
        const int64_t slot = c * A.n + pl;
        const SlipBoundOp Tv = slip_bound_op(A.tlen, A.toff, A.tlimbs, c);
        wb_copy_pad((dig_t *)(A.stage + A.soff[slot]), Tv.p, Tv.l);
        if (lane == 0) A.rlen[slot] = Tv.s * Tv.l;
    }
}

/* The scalars of a bounded step (slip_hip_factor_step_bounded, slip_hip_step_bounded): between the bounded
 * selection (slip_bound_kernel, slip_ratio_kernel) and the update of all n numerators (slip_pivot_kernel), per problem c the
 * move and the records the update takes, formed on the device from the winner r = best[c] of the selection (N_r and a'_r as
 * DESIGN 3l defines them), d_c (s its sign), bd and the entering variable's value ev_c / bd and range er_c / bd >= 0
 * (finite[c]):
 *   flip  (2) iff finite[c] and (best < 0 or er_c |a'_r| <= s N_r):
 *               P = bd, T = sense er_c, D = 1, Dn = bd d_c, E = (ev_c + sense er_c) d_c;
 *   pivot (1) iff best >= 0 and no flip:  P = Dn = bd a'_r, T = N_r, D = d_c, E = ev_c a'_r + N_r;
 *   none  (0) otherwise: empty records, place -2 (slip_pivot_kernel skips the problem).
 * Every scalar is of the form s1 |X||Y| + s2 |Z||W| (SlipBstepJob).  One wavefront per problem in every phase, wave-uniform.
 *
 * phase 0, capture (inside the selection's sink, the group's staging slab alive): the winner's numerator, which phase 3 of
 *   slip_bound_kernel has given a record with the sign of d_c taken out again, copied into the problem's nstride limbs of a
 *   slab that outlives the group; the record of a'_r (into the a slab, which stays) copied.
 * phase 1, classify and size: from the operands' bit lengths, as phase 0 of slip_pivot_kernel, the digits nd no scalar of
 *   either move exceeds, and those of what is copied; the widest to wmax[0], the widest two's-complement sum of the memory
 *   path (nd + 1) to wmax[1].  The host reads 8 bytes back and sizes the five regions (P, T, D, E, Dn) of a problem.
 * phase 2, form: the comparison (into the E region, overwritten afterwards), the move, then the two products of the move
 *   and the copies.  A scalar whose terms are both zero takes no arithmetic (path 0); both products of at most four digits
 *   by the factors' digit counts finish in lane 0 as 128-bit numbers (path 1); nd <= 256 in registers, class ceil(nd / 64)
 *   (path 2); above through the wave's scratch, modulo B^Wp in two's complement (path 3).  Every value leaves as whole limbs
 *   with a trimmed signed digit count.  paths[0 .. 3]: the scalars formed by path; err: a value that did not fit (never, by
 *   phase 1's sizes). */
struct SlipBstepArgs {
    int32_t nprob, phase, sense;
    const int32_t *wnlen, *walen; const int64_t *wnoff, *waoff; const uint64_t *stage;    /* phase 0: the group's winners        */
    int32_t *nlen; uint64_t *nslab; int64_t nstride;                               /* N_r: nstride limbs a problem           */
    int32_t *arlen; int64_t *aroff; const uint64_t *alimbs;                        /* a'_r: records into the a slab          */
    const int32_t *dlen; const int64_t *doff; const uint64_t *dlimbs;              /* d_c: entry c                           */
    int32_t bddig; const uint64_t *bdlimbs, *one;                                  /* bd > 0, trimmed; a limb holding 1      */
    const int32_t *best, *finite;                                                  /* finite NULL: no range is finite        */
    const int32_t *erlen; const int64_t *eroff; const uint64_t *erlimbs;           /* er_c (finite set)                      */
    const int32_t *evlen; const int64_t *evoff; const uint64_t *evlimbs;           /* ev_c, or NULL: 0                       */
    int32_t *wmax;
    uint64_t *slab; int64_t stride;                                                /* region k of problem c: (5 c + k) stride */
    int32_t *rlen; int64_t *roff; int64_t rstride;                                 /* record k of problem c: k * rstride + c */
    int32_t *place, *move, *err;
    dig_t *scratch; int32_t wcap;                                                  /* path 3: 2 * wcap digits per wave       */
    unsigned long long *paths;
};

/* s1 |X||Y| + s2 |Z||W| */
struct SlipBstepJob { SlipBoundOp X, Y, Z, W; int s1, s2; };
SLIP_DEV SlipBstepJob slip_bstep_job(const SlipBoundOp &X, const SlipBoundOp &Y, int s1, const SlipBoundOp &Z, const SlipBoundOp &W, int s2)
{
    SlipBstepJob J;
    J.X = X; J.Y = Y; J.Z = Z; J.W = W; J.s1 = s1; J.s2 = s2;
    return J;
}

/* the digits the scalar does not exceed, from its factors' bit lengths; *path as slip_pivot_kernel's phase 0 chooses it */
SLIP_DEV int slip_bstep_digits(const SlipBstepJob &J, int *path)
{
    const int b1 = J.s1 ? wb_bits(J.X.p, J.X.l) + wb_bits(J.Y.p, J.Y.l) : 0, b2 = J.s2 ? wb_bits(J.Z.p, J.Z.l) + wb_bits(J.W.p, J.W.l) : 0;
    const int w1 = J.s1 ? J.X.l + J.Y.l : 0, w2 = J.s2 ? J.Z.l + J.W.l : 0;
    const int nd = ((b1 > b2 ? b1 : b2) + 1 + 31) >> 5;
    *path = !J.s1 && !J.s2 ? 0 : w1 <= 4 && w2 <= 4 ? 1 : nd <= 256 ? 2 : 3;
    return *path ? nd : 0;
}

/* lane arithmetic: both products as 128-bit numbers, the signed sum into out (at most five digits); its signed digit count */
SLIP_DEV int slip_bstep_lane(const SlipBstepJob &J, uint64_t *out)
{
    const slip_u128 P = J.s1 ? slip_bound_load128(J.X) * slip_bound_load128(J.Y) : 0, Q = J.s2 ? slip_bound_load128(J.Z) * slip_bound_load128(J.W) : 0;
    slip_u128 mag; uint32_t top = 0; int sg;
    if (J.s1 == J.s2 || !J.s1 || !J.s2) { mag = P + Q; top = mag < P ? 1u : 0u; sg = J.s1 ? J.s1 : J.s2; }
    else if (P >= Q) { mag = P - Q; sg = P == Q ? 0 : J.s1; }
    else { mag = Q - P; sg = J.s2; }
    if (sg == 0 || (!top && mag == 0)) return 0;
    const uint64_t l0 = (uint64_t) mag, l1 = (uint64_t)(mag >> 64);
    const int len = top ? 5 : l1 ? (l1 >> 32 ? 4 : 3) : (l0 >> 32 ? 2 : 1);
    out[0] = l0;
    if (len > 2) out[1] = l1;
    if (len > 4) out[2] = top;
    return sg < 0 ? -len : len;
}

/* registers: both products below B^(64*D) and their signed sum too; whole limbs into out, the signed digit count */
template <int D> SLIP_DEV int slip_bstep_reg(const SlipBstepJob &J, dig_t *out)
{
    const WR<D> P = J.s1 ? slip_bound_mul_reg<D>(J.X, J.Y) : wr_zero<D>(), Q = J.s2 ? slip_bound_mul_reg<D>(J.Z, J.W) : wr_zero<D>();
    WR<D> N; int sg;
    if (!J.s1 || !J.s2 || J.s1 == J.s2) { N = wr_addsub<D>(P, Q, 0); sg = J.s1 ? J.s1 : J.s2; }
    else {
        const int cm = wr_cmp<D>(P, Q);
        sg = cm > 0 ? J.s1 : cm < 0 ? J.s2 : 0;
        N = cm >= 0 ? wr_addsub<D>(P, Q, 1) : wr_addsub<D>(Q, P, 1);
    }
    const int len = wr_len<D>(N);
    if (sg == 0 || len == 0) return 0;
    wr_store<D>(out, N, (len + 1) & ~1);
    return sg < 0 ? -len : len;
}

/* memory: the sum modulo B^Wp, Wp even, in two's complement on two buffers of Wp digits; whole limbs into out */
SLIP_DEV int slip_bstep_wide(const SlipBstepJob &J, int Wp, dig_t *num, dig_t *prod, dig_t *out)
{
    for (int k = slip_lane(); k < Wp; k += SLIP_WAVE) num[k] = 0u;
    slip_wave_sync();
    if (J.s1) { wb_mul_lo(prod, J.X.p, J.X.l, J.Y.p, J.Y.l, Wp); wb_addsub(num, num, Wp, prod, Wp, Wp, J.s1 < 0); }
    if (J.s2) { wb_mul_lo(prod, J.Z.p, J.Z.l, J.W.p, J.W.l, Wp); wb_addsub(num, num, Wp, prod, Wp, Wp, J.s2 < 0); }
    const int neg = (int)(num[Wp - 1] >> 31);
    if (neg) wb_addsub(num, (const dig_t *) 0, 1, num, Wp, Wp, 1, 0u);
    const int ln = wb_len(num, Wp);
    wb_copy_pad(out, num, ln);
    return neg ? -ln : ln;
}

/* one scalar into its region of cap digits (buf: the wave's scratch, 2 * wcap digits, or NULL); its signed digit count,
 * *path the path that formed it, *bad set when it does not fit */
SLIP_DEV int slip_bstep_form(const SlipBstepJob &J, dig_t *out, int cap, dig_t *buf, int wcap, int *path, int *bad)
{
    const int nd = slip_bstep_digits(J, path);
    if (*path == 0) return 0;
    if (nd > cap || (*path == 3 && (!buf || ((nd + 2) & ~1) > wcap))) { *bad = 1; return 0; }
    int len = 0;
    if (*path == 1) {
        if (slip_lane() == 0) len = slip_bstep_lane(J, (uint64_t *) out);
        len = (int) slip_shfl_u32((uint32_t) len, 0);
        slip_wave_sync();
    } else if (*path == 2) {
        const int cls = (nd + 63) >> 6;
        if (cls == 1) len = slip_bstep_reg<1>(J, out);
        else if (cls == 2) len = slip_bstep_reg<2>(J, out);
        else if (cls == 3) len = slip_bstep_reg<3>(J, out);
        else len = slip_bstep_reg<4>(J, out);
        slip_wave_sync();
    } else len = slip_bstep_wide(J, (nd + 2) & ~1, buf, buf + wcap, out);
    return len;
}

/* phase 1: a scalar's digits into the widths of its problem */
SLIP_DEV void slip_bstep_size(const SlipBstepJob &J, uint32_t *W, uint32_t *Ww)
{
    int path;
    const uint32_t nd = (uint32_t) slip_bstep_digits(J, &path);
    if (nd > *W) *W = nd;
    if (path == 3 && nd + 1 > *Ww) *Ww = nd + 1;
}

/* phase 2: a scalar formed, counted by its path */
#define SLIP_BSTEP_FORM(J, out) slip_bstep_form(J, out, cap, buf, A.wcap, &path, &bad); \
    for (int k_ = 0; k_ < 4; k_++) cnt[k_] += path == k_ ? 1u : 0u

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_bstep_kernel(SlipBstepArgs A)
#else
static void slip_bstep_body(SlipBstepArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    if (A.phase == 0) {
        for (int64_t c = wave0; c < A.nprob; c += nwaves) {
            int32_t nl = A.wnlen[c];
            const int l = slip_abs(nl);
            if ((int64_t) l > 2 * A.nstride) { nl = 0; if (lane == 0) slip_atomic_add_i32(A.err, 1); }
            else wb_copy_pad((dig_t *)(A.nslab + c * A.nstride), (const dig_t *)(A.stage + A.wnoff[c]), l);
            if (lane == 0) { A.nlen[c] = nl; A.arlen[c] = A.walen[c]; A.aroff[c] = A.waoff[c]; }
        }
        return;
    }
    const int cap = (int)(2 * A.stride);
    dig_t *buf = A.scratch ? A.scratch + wave0 * 2 * (int64_t) A.wcap : (dig_t *) 0;
    unsigned long long cnt[4] = {0, 0, 0, 0};
    uint32_t wall = 0, wwave = 0;
    int nbad = 0;
    for (int64_t c = wave0; c < A.nprob; c += nwaves) {
        const int32_t b = A.best[c];
        const int fin = A.finite ? A.finite[c] != 0 : 0;
        SlipBoundOp Z, Ar, N, BD, ONE, ER, EV;
        Z.p = (const dig_t *) 0; Z.l = 0; Z.s = 0;
        Ar = Z; N = Z; ER = Z; EV = Z;
        if (b >= 0) {
            Ar = slip_bound_op(A.arlen, A.aroff, A.alimbs, c);
            const int32_t nl = A.nlen[c];
            N.p = (const dig_t *)(A.nslab + c * A.nstride);
            N.l = slip_trim_digits(N.p, slip_abs(nl));
            N.s = N.l == 0 ? 0 : (nl < 0 ? -1 : 1);
        }
        const SlipBoundOp Dd = slip_bound_op(A.dlen, A.doff, A.dlimbs, c);
        BD.p = (const dig_t *) A.bdlimbs; BD.l = A.bddig; BD.s = 1;
        ONE.p = (const dig_t *) A.one; ONE.l = 1; ONE.s = 1;
        if (fin) ER = slip_bound_op(A.erlen, A.eroff, A.erlimbs, c);
        if (A.evlen) EV = slip_bound_op(A.evlen, A.evoff, A.evlimbs, c);
        /* the comparison er |a'| - s N; the two products of a pivot; those of a flip */
        const SlipBstepJob Jc = slip_bstep_job(ER, Ar, ER.s, N, ONE, -Dd.s * N.s);
        const SlipBstepJob Jp1 = slip_bstep_job(BD, Ar, Ar.s, Z, Z, 0), Jp2 = slip_bstep_job(EV, Ar, EV.s * Ar.s, N, ONE, N.s);
        const SlipBstepJob Jf1 = slip_bstep_job(BD, Dd, Dd.s, Z, Z, 0), Jf2 = slip_bstep_job(EV, Dd, EV.s * Dd.s, ER, Dd, A.sense * ER.s * Dd.s);
        if (A.phase == 1) {
            uint32_t W = (uint32_t)(Dd.l > BD.l ? Dd.l : BD.l), Ww = 0;
            if ((uint32_t) N.l > W) W = (uint32_t) N.l;
            if ((uint32_t) ER.l > W) W = (uint32_t) ER.l;
            if (fin && b >= 0) slip_bstep_size(Jc, &W, &Ww);
            if (b >= 0) { slip_bstep_size(Jp1, &W, &Ww); slip_bstep_size(Jp2, &W, &Ww); }
            if (fin) { slip_bstep_size(Jf1, &W, &Ww); slip_bstep_size(Jf2, &W, &Ww); }
            if (W > wall) wall = W;
            if (Ww > wwave) wwave = Ww;
            continue;
        }
        dig_t *rP = (dig_t *)(A.slab + (5 * c + 0) * A.stride), *rT = (dig_t *)(A.slab + (5 * c + 1) * A.stride);
        dig_t *rD = (dig_t *)(A.slab + (5 * c + 2) * A.stride), *rE = (dig_t *)(A.slab + (5 * c + 3) * A.stride);
        dig_t *rN = (dig_t *)(A.slab + (5 * c + 4) * A.stride);
        int path, bad = 0, move;
        if (fin && b >= 0) {
            const int lc = SLIP_BSTEP_FORM(Jc, rE);
            move = lc <= 0 ? 2 : 1;                                /* (a tie: the flip) */
        } else move = fin ? 2 : b >= 0 ? 1 : 0;
        int lP = 0, lT = 0, lD = 1, lE = 0, lN = 0;
        int64_t oN = (5 * c + 4) * A.stride;
        if (move == 1) {
            lP = SLIP_BSTEP_FORM(Jp1, rP);
            lE = SLIP_BSTEP_FORM(Jp2, rE);
            wb_copy_pad(rT, N.p, N.l); lT = N.s * N.l;
            wb_copy_pad(rD, Dd.p, Dd.l); lD = Dd.s * Dd.l;
            lN = lP; oN = (5 * c + 0) * A.stride;                  /* Dn = P */
        } else {
            if (move == 2) {
                lN = SLIP_BSTEP_FORM(Jf1, rN);
                lE = SLIP_BSTEP_FORM(Jf2, rE);
                wb_copy_pad(rP, BD.p, BD.l); lP = BD.l;
                wb_copy_pad(rT, ER.p, ER.l); lT = A.sense * ER.s * ER.l;
            }
            wb_copy_pad(rD, ONE.p, 1);
        }
        if (lane == 0) {
            A.rlen[c] = lP; A.roff[c] = (5 * c + 0) * A.stride;
            A.rlen[A.rstride + c] = lT; A.roff[A.rstride + c] = (5 * c + 1) * A.stride;
            A.rlen[2 * A.rstride + c] = lD; A.roff[2 * A.rstride + c] = (5 * c + 2) * A.stride;
            A.rlen[3 * A.rstride + c] = lE; A.roff[3 * A.rstride + c] = (5 * c + 3) * A.stride;
            A.rlen[4 * A.rstride + c] = lN; A.roff[4 * A.rstride + c] = oN;
            A.place[c] = move ? -1 : -2; A.move[c] = move;
        }
        nbad += bad;
    }
    if (lane == 0) {
        if (A.phase == 1) {
            if (wall) slip_atomic_max_i32(A.wmax + 0, (int32_t) wall);
            if (wwave) slip_atomic_max_i32(A.wmax + 1, (int32_t) wwave);
        } else {
            for (int k = 0; k < 4; k++) if (cnt[k]) slip_atomic_add_u64(A.paths + k, cnt[k]);
            if (nbad) slip_atomic_add_i32(A.err, nbad);
        }
    }
}

/* Nonbasic states and reference weights in exact pricing (slip_hip_factor_price_states, slip_hip_price_select):
 * the records slip_ratio_kernel selects on, formed from the numerators X_j (and A_j, nside 2) of nprob problems over one
 * nonzero signed d_c each, the state of every column (0 never eligible, 1 at its lower bound, 2 at its upper bound, 3 free)
 * and, with nside 1, optional weights w_j > 0.  With s = sign(d_c):
 *   nside 1: t_j = sense * s * X_j; eligible iff t_j < 0 (state 1), t_j > 0 (state 2), t_j != 0 (state 3).  Without weights
 *     the x record is |X_j| on X_j's own limbs over the one-limb constant 1 (length 0 when not eligible); with weights it is
 *     X_j^2 in a staging slab of its own over w_j's record.  Either way the selection takes the largest ratio (xflip = 1,
 *     asense = 1).
 *   nside 2: t_j = sense * s * A_j; eligible iff t_j > 0 (state 1), t_j < 0 (state 2), t_j != 0 (state 3).  The a record is
 *     sense * |A_j| on A_j's limbs (length 0 when not eligible), the x record X_j with the sign of X_j / (sense * A_j): the
 *     selection runs with asense = sense and no flip whatever the signs of d_c and A_j.
 * Entry j of problem c is entry c * xstride + j of x (c * astride + j of a) and entry c * n + j of every array written here.
 *
 * phase 0, classify and size, one lane per entry (a wave's 64 entries are of one problem): the selection's records; with
 *   weights cls = the path of an eligible entry (1 the lane pass; 1 + D, D = 1 .. 4, a square of at most 64 D digits by the
 *   BIT length of X_j, a p-bit number's square having at most 2 p bits; 6 through memory; 0 not eligible) and w = 2 dig(X_j),
 *   the digits it owns in the squares' slab, the widest of them to wmax[0], one atomic per wave.  Without weights no limb
 *   moves and this phase is the whole job.
 * phase 1, the lane pass, one lane per entry: |X_j| of at most two digits, squared in the lane as one 128-bit product.
 * phase 2, the wave pass, one wavefront per entry, wave-uniform: the operand times itself in registers (slip_check_mac_reg)
 *   when the square fits 256 digits, through memory (wb_mul_lo straight into the entry's own region of the slab: no scratch)
 *   above.  Every path leaves whole limbs and the trimmed digit count in xlen2.
 * phase 3, one lane per problem: vsign[c] from the ORIGINAL record of X_best and the sign of d_c, and the records of the
 *   winners' X and A as they came in.
 * paths: eligible entries [0] settled without a product, [1] squared in a lane, [2] in registers, [3] through memory. */
struct SlipStatesArgs {
    int32_t n, nprob, phase, nside, sense, weighted;
    int64_t xstride, astride;
    const int32_t *xlen; const int64_t *xoff; const uint64_t *xlimbs;              /* X: signed digit counts, limb offsets   */
    const int32_t *alen; const int64_t *aoff; const uint64_t *alimbs;              /* A likewise (nside 2)                   */
    const int32_t *dlen;                                                           /* d_c: entry c (its sign is all it takes) */
    const int32_t *state;                                                          /* by column                              */
    const int32_t *wtlen; const int64_t *wtoff;                                    /* the weights' records, by column        */
    int32_t *cls, *w, *wmax;                                                       /* (with weights)                         */
    int32_t *xlen2, *alen2; int64_t *xoff2, *aoff2;                                /* the records of the selection           */
    const int64_t *soff; uint64_t *stage;                                          /* the squares' slab                      */
    const int32_t *best; int32_t *vsign;                                           /* phase 3, per problem                   */
    int32_t *wxlen, *walen; int64_t *wxoff, *waoff;                                /* the winners' records, or NULL          */
    unsigned long long *paths;
};

/* wave pass, registers: the square of X, at most 64*D digits, into out in whole limbs; its digit count */
template <int D> SLIP_DEV int slip_states_square_reg(const SlipBoundOp &X, dig_t *out)
{
    const WR<D> V = slip_check_mac_reg<D>(wr_zero<D>(), X.p, X.l, X.p, X.l, 0);
    const int len = wr_len<D>(V);
    wr_store<D>(out, V, (len + 1) & ~1);
    return len;
}

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_states_kernel(SlipStatesArgs A)
#else
static void slip_states_body(SlipStatesArgs A)
#endif
{
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    if (A.phase <= 1) {
        const int64_t rpp = ((int64_t) A.n + SLIP_WAVE - 1) / SLIP_WAVE, rounds = rpp * A.nprob;
        uint32_t wall = 0;
        unsigned long long total = 0;
        for (int64_t r = wave0; r < rounds; r += nwaves) {
            const int c = (int)(r / rpp);
            const int64_t i = (r - (int64_t) c * rpp) * SLIP_WAVE + lane, e = (int64_t) c * A.n + i, ex = (int64_t) c * A.xstride + i;
            if (A.phase == 1) {
                const int take = i < A.n && A.cls[e] == 1;
                if (take) {
                    const SlipBoundOp X = slip_bound_op(A.xlen, A.xoff, A.xlimbs, ex);
                    const uint64_t v = X.l > 1 ? ((uint64_t) X.p[1] << 32) | X.p[0] : X.p[0];
                    const slip_u128 sq = (slip_u128) v * v;
                    const uint64_t l0 = (uint64_t) sq, l1 = (uint64_t)(sq >> 64);
                    uint64_t *out = A.stage + A.soff[e];
                    out[0] = l0;
                    if (X.l > 1) out[1] = l1;
                    A.xlen2[e] = l1 ? (l1 >> 32 ? 4 : 3) : (l0 >> 32 ? 2 : 1);
                }
                total += (unsigned long long) slip_popc64(slip_ballot(take));
                continue;
            }
            uint32_t W = 0;
            int el = 0;
            if (i < A.n) {
                const int st = A.state[i], sd = A.dlen[c] < 0 ? -1 : 1;
                const SlipBoundOp X = slip_bound_op(A.xlen, A.xoff, A.xlimbs, ex);
                if (A.nside == 1) {
                    const int t = A.sense * sd * X.s;
                    el = st == 1 ? t < 0 : st == 2 ? t > 0 : st == 3 ? t != 0 : 0;
                    if (!A.weighted) {
                        A.xlen2[e] = X.l; A.xoff2[e] = A.xoff[ex];
                        A.alen2[e] = el; A.aoff2[e] = 0;
                    } else {
                        int code = 0;
                        if (el) {
                            const int sq = (2 * wb_bits(X.p, X.l) + 31) >> 5;      /* the digits the square cannot exceed */
                            code = X.l <= 2 ? 1 : sq <= 256 ? 1 + ((sq + 63) >> 6) : 6;
                            W = 2u * (uint32_t) X.l;
                        }
                        A.cls[e] = code; A.w[e] = (int32_t) W;
                        A.xlen2[e] = 0;
                        A.alen2[e] = el ? A.wtlen[i] : 0; A.aoff2[e] = A.wtoff[i];
                    }
                } else {
                    const int64_t ea = (int64_t) c * A.astride + i;
                    const SlipBoundOp Av = slip_bound_op(A.alen, A.aoff, A.alimbs, ea);
                    const int t = A.sense * sd * Av.s;
                    el = st == 1 ? t > 0 : st == 2 ? t < 0 : st == 3 ? t != 0 : 0;
                    A.xlen2[e] = X.s * A.sense * Av.s * X.l; A.xoff2[e] = A.xoff[ex];
                    A.alen2[e] = el ? A.sense * Av.l : 0; A.aoff2[e] = A.aoff[ea];
                }
            }
            if (A.weighted) { W = slip_wave_max_u32(W); if (W > wall) wall = W; }
            else total += (unsigned long long) slip_popc64(slip_ballot(el));
        }
        if (lane == 0 && wall) slip_atomic_max_i32(A.wmax, (int32_t) wall);
        if (lane == 0 && total) slip_atomic_add_u64(A.paths + A.phase, total);
        return;
    }
    if (A.phase == 2) {
        const int64_t items = (int64_t) A.n * A.nprob;
        unsigned long long cnt[2] = {0, 0};
        for (int64_t e = wave0; e < items; e += nwaves) {
            const int code = A.cls[e];
            if (code < 2) continue;
            const int c = (int)(e / A.n), i = (int)(e - (int64_t) c * A.n);
            const SlipBoundOp X = slip_bound_op(A.xlen, A.xoff, A.xlimbs, (int64_t) c * A.xstride + i);
            dig_t *out = (dig_t *)(A.stage + A.soff[e]);
            int len;
            if (code == 2) len = slip_states_square_reg<1>(X, out);
            else if (code == 3) len = slip_states_square_reg<2>(X, out);
            else if (code == 4) len = slip_states_square_reg<3>(X, out);
            else if (code == 5) len = slip_states_square_reg<4>(X, out);
            else {
                wb_mul_lo(out, X.p, X.l, X.p, X.l, 2 * X.l);       /* (the entry owns 2 dig(X) digits: whole limbs) */
                len = wb_len(out, 2 * X.l);
            }
            if (lane == 0) A.xlen2[e] = len;
            cnt[code == 6]++;
        }
        if (lane == 0) for (int k = 0; k < 2; k++) if (cnt[k]) slip_atomic_add_u64(A.paths + 2 + k, cnt[k]);
        return;
    }
    const int64_t rounds = ((int64_t) A.nprob + SLIP_WAVE - 1) / SLIP_WAVE;
    for (int64_t r = wave0; r < rounds; r += nwaves) {
        const int64_t c = r * SLIP_WAVE + lane;
        if (c >= A.nprob) continue;
        const int32_t b = A.best[c];
        const int64_t ex = c * A.xstride + (b < 0 ? 0 : b), ea = c * A.astride + (b < 0 ? 0 : b);
        const int32_t sx = b < 0 ? 0 : A.xlen[ex];
        A.vsign[c] = sx == 0 ? 0 : (((sx < 0) != (A.dlen[c] < 0)) ? -1 : 1);
        if (A.wxlen) {
            A.wxlen[c] = sx; A.wxoff[c] = b < 0 ? 0 : A.xoff[ex];
            A.walen[c] = b < 0 || A.nside == 1 ? 0 : A.alen[ea]; A.waoff[c] = b < 0 || A.nside == 1 ? 0 : A.aoff[ea];
        }
    }
}

/* The transposed view of complete factors (slip_hip_factor_solve_transpose).  With M = A(row_perm, q) the matrix that was
 * factorised, every entry of a REF factorisation is a minor of M (L(i,k) = det M[{0..k-1,i},{0..k}], U(k,j) =
 * det M[{0..k},{0..k-1,j}], rho_k = det M[0..k,0..k]); transposing swaps the rows and columns of every minor, so the REF
 * factorisation of M^T in the identity pivot order is L' = U^T, U' = L^T with the same rho_k.  Both are laid out by pivot
 * POSITION, from the factors in HBM: count per position, an exclusive scan, a scatter.  The entry records are copied as
 * they are and index the other slab (L' reads the U limbs, U' the L limbs); no limb moves.
 *   L'(:,p): for every U entry m of column j with pinv[Ui[m]] = p, row j and record Ue[m] (any order);
 *   U'(:,p): for every L entry m of column k with pinv[Li[m]] = p, row k and record Le[m], the pivot (k = p) LAST, in the
 *            slot kept for it (the back substitution reads Up[p+1]-1 as the pivot and skips it);
 *   piv'[k]: piv[k] reading its digits from the U pivot record, its inverse cache empty. */
struct SlipTViewArgs {
    int32_t n, phase;                                                              /* 0 count, 1 scatter, 2 pivot records    */
    const int64_t *Lp, *Up; const int32_t *Li, *Ui; const SlipEnt *Le, *Ue;       /* the complete factors                  */
    const int32_t *pinv; const SlipPiv *piv;
    int32_t *cntL, *cntU;      /* per position: entries of L'(:,p), non-pivot entries of U'(:,p); the fill counters of the scatter */
    int64_t *tLp, *tUp; int32_t *tLi, *tUi; SlipEnt *tLe, *tUe; SlipPiv *tpiv;    /* the view                              */
};

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_tview_kernel(SlipTViewArgs A)
#else
static void slip_tview_body(SlipTViewArgs A)
#endif
{
    const int n = A.n;
    if (A.phase == 2) {
        const int64_t t0 = (int64_t) slip_block() * slip_nthreads() + slip_tid(), nt = (int64_t) slip_nblocks() * slip_nthreads();
        for (int64_t k = t0; k < n; k += nt) {
            SlipPiv r = A.piv[k];
            r.off = A.Ue[A.Up[k + 1] - 1].off; r.invlen = 0; r.pad = 0;
            A.tpiv[k] = r;
        }
        return;
    }
    /* one wavefront per source column: U's n columns, then L's */
    const int lane = slip_lane();
    const int64_t wave0 = (int64_t) slip_block() * slip_nwaves() + slip_wave(), nwaves = (int64_t) slip_nblocks() * slip_nwaves();
    for (int64_t it = wave0; it < 2 * (int64_t) n; it += nwaves) {
        const int fromU = it < n, c = (int)(fromU ? it : it - n);
        const int64_t m0 = fromU ? A.Up[c] : A.Lp[c], m1 = fromU ? A.Up[c + 1] : A.Lp[c + 1];
        for (int64_t m = m0 + lane; m < m1; m += SLIP_WAVE) {
            const int p = A.pinv[fromU ? A.Ui[m] : A.Li[m]];
            if (fromU) {
                if (A.phase == 0) { slip_atomic_add_i32(&A.cntL[p], 1); continue; }
                const int64_t t = A.tLp[p] + slip_atomic_add_i32(&A.cntL[p], 1);
                A.tLi[t] = c; A.tLe[t] = A.Ue[m];
            } else {
                if (A.phase == 0) { if (p != c) slip_atomic_add_i32(&A.cntU[p], 1); continue; }
                const int64_t t = p == c ? A.tUp[p + 1] - 1 : A.tUp[p] + slip_atomic_add_i32(&A.cntU[p], 1);
                A.tUi[t] = c; A.tUe[t] = A.Le[m];
            }
        }
    }
}

/* the column pointers of the view: exclusive sums of cntL and of cntU + 1 (the pivot's slot), one workgroup, every thread a
 * contiguous share; tmp: 2 words per wave */
SLIP_DEV void slip_tview_scan_body(const SlipTViewArgs &A, uint64_t *tmp)
{
    const int tid = slip_tid(), T = slip_nthreads();
    const int64_t n = A.n, per = (n + T - 1) / T, i0 = (int64_t) tid * per < n ? (int64_t) tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    uint64_t sL = 0, sU = 0;
    for (int64_t i = i0; i < i1; i++) { sL += (uint64_t) A.cntL[i]; sU += (uint64_t) A.cntU[i] + 1u; }
    uint64_t eL, eU, tL, tU;
    slip_block_scan2(sL, sU, tmp, &eL, &eU, &tL, &tU);
    for (int64_t i = i0; i < i1; i++) {
        A.tLp[i] = (int64_t) eL; A.tUp[i] = (int64_t) eU;
        eL += (uint64_t) A.cntL[i]; eU += (uint64_t) A.cntU[i] + 1u;
    }
    if (tid == 0) { A.tLp[n] = (int64_t) tL; A.tUp[n] = (int64_t) tU; }
}
#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(1024)
slip_tview_scan_kernel(SlipTViewArgs A)
{
    __shared__ uint64_t tmp[32];
    slip_tview_scan_body(A, tmp);
}
#endif

/* Back to column K (slip_hip_factor_rewind): the swaps of columns Kold-1 ... K undone from the log, in parallel.  The serial
 * undo of column c, with r = row_perm[c], d = sw_row[c], p = sw_pos[c] (p >= c: the pivot row stood at or behind c), writes
 * row_perm[c] = d and row_perm[p] = r (the same value when p == c: then d == r), walking c downwards.  Two facts make it a
 * parallel pass: (1) the undo of a later column c' > c writes positions c' and p' >= c' only, so row_perm[c] is still what
 * the factorisation left when column c's turn comes -- every r_c can be read up front; (2) the walk goes downwards, so the
 * LAST write to a position x >= K, the one that stays, is that of the SMALLEST c >= K with c == x or sw_pos[c] == x: d_c in
 * the first case, r_c in the second.  Positions < K are never written.  pinv then follows from row_perm on [K, n): the rows
 * at those positions are the same set before and after.
 *   phase 0: rsave[c - K] = row_perm[c], win[x - K] = min over the columns c that write x (win starts at SLIP_REWIND_NONE)
 *   phase 1: row_perm[x] from the winner         phase 2: pinv[row_perm[x]] = x, Lready[x] = 0, for x in [K, n)
 *   phase 3: the limbs of the entries below Lp[K] / Up[K] summed (out[0], out[1]: SlipState.Lnl_exact / Unl_exact of the
 *            frontier K) and out[2..6] = Lp[K], Up[K], Lo[K], Uo[K], row_perm[K - 1] */
#define SLIP_REWIND_NONE 0x7f7f7f7f
struct SlipRewindArgs {
    int32_t n, K, Kold, phase;
    int32_t *row_perm, *pinv, *Lready; const int32_t *sw_row, *sw_pos;
    int32_t *win, *rsave;                                              /* n - K and Kold - K words */
    const int64_t *Lp, *Up, *Lo, *Uo; const SlipEnt *Le, *Ue;
    int64_t lnz_max, unz_max;                                          /* the entries there are: no read beyond them */
    unsigned long long *out;                                           /* 8 words, zeroed */
};

SLIP_DEV uint64_t slip_wave_sum_u64(uint64_t v)
{
    const int lane = slip_lane();
    for (int d = 32; d >= 1; d >>= 1) v += slip_shfl_u64(v, lane ^ d);
    return v;
}

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_rewind_kernel(SlipRewindArgs A)
#else
static void slip_rewind_body(SlipRewindArgs A)
#endif
{
    const int64_t t0 = (int64_t) slip_block() * slip_nthreads() + slip_tid(), nt = (int64_t) slip_nblocks() * slip_nthreads();
    const int K = A.K, n = A.n;
    if (A.phase == 0) {
        for (int64_t c = K + t0; c < A.Kold; c += nt) {
            const int p = A.sw_pos[c];
            A.rsave[c - K] = A.row_perm[c];
            slip_atomic_min_i32(&A.win[c - K], (int32_t) c);
            if (p >= K && p < n) slip_atomic_min_i32(&A.win[p - K], (int32_t) c);
        }
    } else if (A.phase == 1) {
        for (int64_t x = K + t0; x < n; x += nt) {
            const int w = A.win[x - K];
            if (w != SLIP_REWIND_NONE) A.row_perm[x] = x == w ? A.sw_row[w] : A.rsave[w - K];
        }
    } else if (A.phase == 2) {
        for (int64_t x = K + t0; x < n; x += nt) {
            const int r = A.row_perm[x];
            if (r >= 0 && r < n) A.pinv[r] = (int32_t) x;
            A.Lready[x] = 0;
        }
    } else {
        const int64_t lnz = A.Lp[K], unz = A.Up[K];
        uint64_t sl = 0, su = 0;
        for (int64_t t = t0; t < lnz && t < A.lnz_max; t += nt) sl += (uint64_t) slip_limbs(A.Le[t].len);
        for (int64_t t = t0; t < unz && t < A.unz_max; t += nt) su += (uint64_t) slip_limbs(A.Ue[t].len);
        sl = slip_wave_sum_u64(sl); su = slip_wave_sum_u64(su);
        if (slip_lane() == 0) {
            if (sl) slip_atomic_add_u64(&A.out[0], sl);
            if (su) slip_atomic_add_u64(&A.out[1], su);
        }
        if (t0 == 0) {
            A.out[2] = (unsigned long long) lnz; A.out[3] = (unsigned long long) unz;
            A.out[4] = (unsigned long long) A.Lo[K]; A.out[5] = (unsigned long long) A.Uo[K];
            A.out[6] = (unsigned long long)(K > 0 ? A.row_perm[K - 1] : 0);
        }
    }
}

/* A column of the resident A replaced (slip_hip_factor_replace_column): the entries keep their own limb offsets, so only the
 * entry arrays move.  Out of place: entry t of the old arrays goes to t (before the column, t < a0) or to t + diff (behind
 * it, t >= a1), diff = nz_new - (a1 - a0); the slots [a0, a0 + nz_new) of the new arrays are filled by the host's upload of
 * the new column.  The column pointers behind the column move by diff in place (nobody reads them here: a0, a1 are
 * arguments). */
struct SlipSpliceArgs {
    int32_t n, j; int64_t a0, a1, nz_new, nnz_old;
    const int32_t *Ai, *Alen; const int64_t *Aoff;
    int32_t *nAi, *nAlen; int64_t *nAoff; int64_t *Ap;
};

#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_splice_kernel(SlipSpliceArgs A)
#else
static void slip_splice_body(SlipSpliceArgs A)
#endif
{
    const int64_t t0 = (int64_t) slip_block() * slip_nthreads() + slip_tid(), nt = (int64_t) slip_nblocks() * slip_nthreads();
    const int64_t diff = A.nz_new - (A.a1 - A.a0);
    for (int64_t t = t0; t < A.nnz_old; t += nt) {
        if (t >= A.a0 && t < A.a1) continue;
        const int64_t d = t < A.a0 ? t : t + diff;
        A.nAi[d] = A.Ai[t]; A.nAlen[d] = A.Alen[t]; A.nAoff[d] = A.Aoff[t];
    }
    if (diff) for (int64_t c = (int64_t) A.j + 1 + t0; c <= A.n; c += nt) A.Ap[c] += diff;
}

/* The limb offsets of a compacted slab (the dead limbs of replaced columns squeezed out; slip_pack_kernel then moves the
 * limbs): off[t] = the limbs of the entries before t, len in signed digits.  Every workgroup owns a contiguous chunk of the
 * entries and every thread a contiguous share of the chunk.  phase 0: bsum[b] = the limbs of chunk b; phase 1: the offsets,
 * each workgroup starting at the sum of the chunks before its own.  tmp: 40 words per workgroup. */
struct SlipOffScanArgs { int64_t count; const int32_t *len; int64_t *off; unsigned long long *bsum; int32_t phase; };

SLIP_DEV void slip_offscan_body(const SlipOffScanArgs &A, uint64_t *tmp)
{
    const int tid = slip_tid(), T = slip_nthreads(), b = slip_block(), B = slip_nblocks();
    const int64_t chunk = (A.count + B - 1) / B, c0 = (int64_t) b * chunk < A.count ? (int64_t) b * chunk : A.count,
                  c1 = c0 + chunk < A.count ? c0 + chunk : A.count;
    const int64_t per = (c1 - c0 + T - 1) / T, i0 = c0 + (int64_t) tid * per < c1 ? c0 + (int64_t) tid * per : c1,
                  i1 = i0 + per < c1 ? i0 + per : c1;
    uint64_t s = 0;
    for (int64_t i = i0; i < i1; i++) s += (uint64_t) slip_limbs(A.len[i]);
    if (A.phase == 1 && tid == 0) { uint64_t base = 0; for (int k = 0; k < b; k++) base += A.bsum[k]; tmp[36] = base; }
    uint64_t e, e2, t, t2;
    slip_block_scan2(s, 0, tmp, &e, &e2, &t, &t2);
    if (A.phase == 0) { if (tid == 0) A.bsum[b] = t; return; }
    e += tmp[36];
    for (int64_t i = i0; i < i1; i++) { A.off[i] = (int64_t) e; e += (uint64_t) slip_limbs(A.len[i]); }
}
#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256)
slip_offscan_kernel(SlipOffScanArgs A)
{
    __shared__ uint64_t tmp[40];
    slip_offscan_body(A, tmp);
}
#endif

#ifndef SLIP_EMULATE
#define SLIP_MAX_WAVES 8                  /* at most 512 threads per worker: 256 VGPRs per lane, two waves per SIMD */
template <bool FAST>
__global__ void __launch_bounds__(64 * SLIP_MAX_WAVES)
slip_factor_kernel(SlipParams P, SlipState *st)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t slip_lds[];
    /* the parameters live in LDS for the whole launch (held in SGPRs across the column loop they made the
     * compiler spill scalars into VGPR lanes all over the lane-level phases); the private arrays are this worker's */
    __shared__ SlipParams sP;
    if (threadIdx.x == 0) slip_worker_params(&sP, P, (int) blockIdx.x);
    __syncthreads();
    /* where this workgroup runs: HW_ID (cu_id bits 11:8, sh_id 12, se_id 15:13) and the XCC id.  The instruction cache is
     * shared by neighbouring CUs: a column worker next to the committer evicts the committer's short loop all the time
     * (the worker's code is far larger than the cache), so the workers on the committer's neighbours stand aside
     * (P.quiet_neighbours; placement is read, never assumed: a worker that does not see the committer just works) */
    const uint32_t hwid = (uint32_t) __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = (uint32_t) __builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xFu;
    const uint32_t where = ((hwid >> 8) & 0xFFu) | (xcc << 8);          /* cu | sh | se | xcc */
    if (threadIdx.x == 0 && blockIdx.x < 2048) P.dbg[slip_dbg_place(P.n) + blockIdx.x] = (int32_t)(where | 0x10000u);
    if (sP.committer && blockIdx.x == 0) {
        if (threadIdx.x == 0) slip_st_i32(&st->committer_where, (int32_t)(where | 0x10000u));
        slip_committer<FAST>(sP, st, slip_lds);
    } else {
        int stand_aside = 0;
        if (sP.committer && sP.quiet_neighbours) {
            __shared__ int aside_;
            if (threadIdx.x == 0) {
                int cw = 0;
                for (int spin = 0; spin < 4000 && !(cw = slip_ld_i32(&st->committer_where)); spin++) slip_sleep();
                aside_ = 0;
                if (cw) {
                    const uint32_t c = (uint32_t) cw;
                    const int same_array = ((c >> 4) & 0xFFu) == ((where >> 4) & 0xFFu);       /* sh, se, xcc */
                    const int dcu = (int)(c & 0xFu) - (int)(where & 0xFu);
                    aside_ = same_array && dcu >= -sP.quiet_neighbours && dcu <= sP.quiet_neighbours;
                }
            }
            __syncthreads();
            stand_aside = aside_;
        }
        if (!stand_aside) slip_factor_worker<FAST>(sP, st, slip_lds);
    }
    slip_worker_exit(sP, st);
}

template <bool FAST>
__global__ void __launch_bounds__(64 * SLIP_MAX_WAVES)
slip_solve_kernel(SlipParams P, SlipState *st, SlipSolveArgs A, int32_t *rhs_done)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t slip_lds[];
    __shared__ SlipParams sP;
    if (threadIdx.x == 0) slip_worker_params(&sP, P, (int) blockIdx.x);
    __syncthreads();
    slip_solve_worker<FAST>(sP, st, A, rhs_done, slip_lds);
}

/* unit-test kernel: block b performs operation b with one wavefront */
extern "C" __global__ void __launch_bounds__(64)
slip_wave_op_kernel(int op, int la, int lb, int W, const uint32_t *a, const uint32_t *b,
                    uint32_t *out, uint32_t *scratch)
{
    const int blk = slip_block();
    const uint32_t *A = a + (int64_t) blk * la, *B = b + (int64_t) blk * (lb > 0 ? lb : 1);
    uint32_t *O = out + (int64_t) blk * W, *s0 = scratch + (int64_t) blk * 2 * (W + 1), *s1 = s0 + W + 1;
    if (op == 0) wb_mul_lo(O, A, la, B, lb, W);
    else if (op == 1) wb_addsub(O, A, la, B, lb, W, 0);
    else if (op == 2) wb_addsub(O, A, la, B, lb, W, 1);
    else if (op == 3) wb_inv_extend(O, 0, W, A, la, s0, s1);
    else slip_reg_op_test(op, A, la, B, lb, W, O, s0);
}

/* micro-benchmark kernel (development aid): cycles per wave-level primitive, nwaves waves busy */
extern "C" __global__ void __launch_bounds__(512)
slip_wave_bench_kernel(int op, int la, int lb, int W, int iters, int out_in_lds,
                       const uint32_t *a, const uint32_t *b, uint32_t *gout, unsigned long long *cycles)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t slip_lds[];
    const int wave = slip_wave();
    uint32_t *O = out_in_lds ? slip_lds + wave * 2 * (W + 2) : gout + (int64_t) wave * 2 * (W + 2);
    uint32_t *O2 = O + W + 2;
    const uint32_t *A = a + (int64_t) wave * la, *B = b + (int64_t) wave * lb;
    __syncthreads();
    unsigned long long t0 = clock64();
    for (int it = 0; it < iters; it++) {
        if (op == 0) wb_mul_lo(O, A, la, B, lb, W);
        else if (op == 1) wb_addsub(O, A, la, B, lb, W, 1);
        else if (op == 2) { int l = wb_len(B, lb); if (l == 12345) O[0] = 1; }
        else if (op == 3) wb_copy_shr(O, B, lb, 3, W);
        else if (op == 4) { wb_mul_lo(O, A, la, B, lb, W); wb_mul_lo(O2, O, W, A, la, W); }
        else if (op == 5) slip_wave_sync();
        else if (op == 6) {                    /* register product, operands already loaded */
            const int ea = la < W ? la : W;
            if (W <= 64) { WR<1> x = wr_load<1>(A, ea), y = wr_load<1>(B, lb < W ? lb : W); wr_store<1>(O, wr_mul<1>(x, ea, y), W); }
            else if (W <= 128) { WR<2> x = wr_load<2>(A, ea), y = wr_load<2>(B, lb < W ? lb : W); wr_store<2>(O, wr_mul<2>(x, ea, y), W); }
            else if (W <= 192) { WR<3> x = wr_load<3>(A, ea), y = wr_load<3>(B, lb < W ? lb : W); wr_store<3>(O, wr_mul<3>(x, ea, y), W); }
            else { WR<4> x = wr_load<4>(A, ea), y = wr_load<4>(B, lb < W ? lb : W); wr_store<4>(O, wr_mul<4>(x, ea, y), W); }
        }
        else if (op == 7 || op == 8) {         /* exact division of a W-digit number: 7 Hensel, 8 Newton inverse to W digits + product */
            const int ea = la < W ? la : W, eb = lb < W ? lb : W;
#define SLIP_BENCH_DIV(DD) do { WR<DD> x = wr_load<DD>(A, ea), y = wr_load<DD>(B, eb); if (slip_lane() == 0) y.d[0] |= 1u; \
                if (op == 7) wr_store<DD>(O, wr_div_hensel<DD>(x, W, y), W); \
                else { WR<DD> v = wr_inv_extend<DD>(wr_zero<DD>(), 0, W, y); wr_store<DD>(O, wr_mask<DD>(wr_mul<DD>(v, W, x), W), W); } } while (0)
            if (W <= 64) SLIP_BENCH_DIV(1); else if (W <= 128) SLIP_BENCH_DIV(2); else if (W <= 192) SLIP_BENCH_DIV(3); else SLIP_BENCH_DIV(4);
#undef SLIP_BENCH_DIV
        }
    }
    unsigned long long t1 = clock64();
    if (slip_lane() == 0) cycles[wave] = (t1 - t0) / (unsigned long long) iters;
}
#else
#define SLIP_MAX_WAVES 16                  /* emulation build */
#endif

/* ------------------------------------------------------------------ */
/* host state                                                          */
/* ------------------------------------------------------------------ */
struct slip_hip_factor {
    SlipParams P;         /* kernel arguments (device pointers inside; private arrays: base of worker 0) */
    SlipState hs;         /* host mirror of the mutable device state     */
    SlipState *ds;        /* device copy the kernel works on             */
    int32_t n; int64_t annz, alimbs;
    int32_t waves, lds_words, bitmap_in_lds, scratch_in_lds;
    int32_t nworkers;      /* column workers = workgroups of a launch; private arrays are sized for this many */
    int32_t workers_asked; /* slip_hip_options.workers (0: as many as can be resident) */
    int32_t no_committer;  /* diagnostics: every column is committed by its own worker */
    int32_t no_farm;       /* diagnostics: long update queues are not opened to other workers */
    int32_t no_engine;     /* diagnostics: no full packages (the committer's chain engine stays off) */
    int32_t engine_ok;     /* the committer's LDS layout with the pinv mirror fits */
    int32_t last_status, window_end, launches;
    int32_t factors_only;  /* built from given factors (slip_hip_factor_from_factors): solve only, no A */
    double kernel_ms, solve_ms;
    hipEvent_t ev0, ev1;
    int32_t *ident;        /* device: 0..n-1 (reset copies it into pinv / row_perm) */
    /* subtree farm: the rescaled copy of the committed factors (slip_hip_factor_rescale); download serves it while it exists */
    SlipEnt *rsLe, *rsUe; uint64_t *rsLl, *rsUl; int64_t rsLnl, rsUnl, rsLexact, rsUexact; int64_t *rspiv; int32_t rescaled;
    /* owned device arrays that are only reachable through const pointers in P */
    int64_t *dAp; int32_t *dAi, *dAlen; int64_t *dAoff; uint64_t *dAlimbs; int32_t *dq;
    int32_t amaxdig;       /* digits of the widest entry of A */
    /* slip_hip_factor_check: the row-ordered view of A, built on the first check (x index = pivot position) */
    int64_t *chk_rp, *chk_re; int32_t *chk_rx;
    double check_ms;
    /* slip_hip_factor_multiply: device time of the last product's kernels (slip_hip_multiply_passes splits it) */
    double multiply_ms;
    /* slip_hip_factor_solve_transpose: the transposed view of the complete factors (slip_tview_kernel), built on the first
     * transposed solve, dropped at reset; its own pivot records and inverse cache (stride tinvcap), the handle's limbs */
    int64_t *tLp, *tUp; int32_t *tLi, *tUi; SlipEnt *tLe, *tUe; SlipPiv *tpiv; uint32_t *tinvd; int32_t tinvcap;
    int32_t *tpinv;        /* host copy of pinv: the output gather x[i] = y[pinv[i]] */
    double tsolve_ms, tview_ms;
    /* slip_hip_factor_check_transpose: the column view of A in q order (row k of the check = column q[k]), built on the first
     * transposed check */
    int64_t *chkt_rp, *chkt_re; int32_t *chkt_rx;
    /* slip_hip_factor_solve_double: device time of the last conversion kernel, entries of it that took the wave pass */
    double todouble_ms; int64_t todouble_slow;
    /* slip_hip_factor_solve_rational: device time of the last reduction kernel, entries of it by the path that settled them */
    double torational_ms; int64_t torational_paths[4];
    /* slip_hip_factor_solve_mpfr: device time of the last conversion kernel, entries of it by the path that settled them */
    double tompfr_ms; int64_t tompfr_paths[4];
    /* slip_hip_factor_ratio_test: device time of the last selection's kernels, its path counts */
    double ratio_ms; int64_t ratio_paths[4];
    /* slip_hip_factor_price: device time of the last call by pass, the path counts of its selections */
    double price_ms[4]; int64_t price_paths[4];
    /* slip_hip_factor_ratio_test_bounded / _bound_test: device time of the last call (the form passes, the selection), the
     * entries by the path that formed them and the path counts of the selection */
    double bound_ms[2]; int64_t bound_paths[8];
    /* slip_hip_factor_price_states: device time of the last call (the classify, offset and square passes, the selection), the
     * eligible entries by the path that settled them and the path counts of the selection */
    double states_ms[2]; int64_t states_paths[8];
    /* slip_hip_factor_solve_update / _step: device time of the last call (the classify, offset and form passes, the selection
     * of a step), the entries by the path that formed them and the inexact ones */
    double update_ms[2]; int64_t update_paths[8];
    double bstep_ms[4]; int64_t bstep_paths[20];          /* the last bounded step */
    /* slip_hip_factor_rewind / _replace_column: the host copy of q; the storage of the resident A -- annz / alimbs are its
     * LIVE entries and limbs, Acap_nz / Acap_nl what dAi, dAlen, dAoff / dAlimbs can hold, Anl_used the limbs of the slab
     * handed out (live ones and the dead ones of replaced columns: new limbs are appended there), A0_nz / A0_nl the initial
     * allocation; broken: a device step of a replacement or rewind failed half way, every further use is refused */
    int32_t *hq;
    int64_t Acap_nz, Acap_nl, Anl_used, A0_nz, A0_nl;
    int32_t broken;
};

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
        fprintf(stderr, "slip_hip: %s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
        return SLIP_HIP_DEVICE_ERROR; } } while (0)
/* the error-accumulating steps of a host sequence: each runs only while the caller's `rc` is still 0 */
#define A_(call) do { if (!rc) rc = (call); } while (0)
#define HIP_(call) do { if (!rc && (call) != hipSuccess) rc = SLIP_HIP_DEVICE_ERROR; } while (0)
#define UP_(dst, src, bytes) do { if ((bytes) > 0) HIP_(hipMemcpy((void *)(dst), (src), (size_t)(bytes), hipMemcpyHostToDevice)); } while (0)
#define DOWN_(dst, src, bytes) do { if ((bytes) > 0) HIP_(hipMemcpy((dst), (const void *)(src), (size_t)(bytes), hipMemcpyDeviceToHost)); } while (0)
/* a step whose error ends the caller at once */
#define TRY_(call) do { const int e_ = (call); if (e_) return e_; } while (0)

static void rescale_drop(slip_hip_factor *f);
static void tview_drop(slip_hip_factor *f);

/* Device buffers go through a process-level pool: the drop-in SLIP_LU_factorize creates and destroys a
 * handle per call, and a handle's private row arrays are gigabytes -- hipMalloc / hipFree of those cost milliseconds each.
 * A freed buffer of at least 1 MiB is kept (up to SLIP_HIP_POOL_MB megabytes in all, default 32 768; 0 switches the pool off)
 * and handed to the next request it fits within a quarter of its size.  Nothing relies on fresh memory being zero: every
 * array that must start cleared is cleared where it is allocated or at reset.  Handles are destroyed after their streams
 * have been synchronised (run / solve return synchronised), so a pooled buffer is never still in use. */
#include <mutex>
#include <unordered_map>
struct SlipPoolEnt { void *p; size_t bytes; };
static std::mutex slip_pool_mu;
static std::vector<SlipPoolEnt> slip_pool;
static std::unordered_map<void *, size_t> slip_pool_live;
static size_t slip_pool_bytes = 0;
static size_t slip_pool_limit(void)
{
    static long long mb = -1;
    if (mb < 0) { const char *e = getenv("SLIP_HIP_POOL_MB"); mb = e ? atoll(e) : 32768; if (mb < 0) mb = 0; }
    return (size_t) mb << 20;
}
static int dev_malloc_bytes(void **q, size_t bytes)
{
    {
        std::lock_guard<std::mutex> g(slip_pool_mu);
        size_t best = (size_t) -1, at = 0;
        for (size_t t = 0; t < slip_pool.size(); t++)
            if (slip_pool[t].bytes >= bytes && slip_pool[t].bytes - bytes <= bytes / 4 && slip_pool[t].bytes < best) { best = slip_pool[t].bytes; at = t; }
        if (best != (size_t) -1) {
            *q = slip_pool[at].p; slip_pool_live[*q] = best; slip_pool_bytes -= best;
            slip_pool[at] = slip_pool.back(); slip_pool.pop_back();
            return 0;
        }
    }
    if (hipMalloc(q, bytes) != hipSuccess) {
        /* the pool may be what is in the way: give it back and try once more */
        std::vector<SlipPoolEnt> drop;
        { std::lock_guard<std::mutex> g(slip_pool_mu); drop.swap(slip_pool); slip_pool_bytes = 0; }
        for (const SlipPoolEnt &e : drop) hipFree(e.p);
        if (drop.empty() || hipMalloc(q, bytes) != hipSuccess) return SLIP_HIP_OUT_OF_MEMORY;
    }
    std::lock_guard<std::mutex> g(slip_pool_mu);
    slip_pool_live[*q] = bytes;
    return 0;
}
static void dev_free(void *p)
{
    if (!p) return;
    size_t bytes = 0;
    {
        std::lock_guard<std::mutex> g(slip_pool_mu);
        auto it = slip_pool_live.find(p);
        if (it != slip_pool_live.end()) { bytes = it->second; slip_pool_live.erase(it); }
        if (bytes >= ((size_t) 1 << 20) && slip_pool_bytes + bytes <= slip_pool_limit()) {
            slip_pool.push_back(SlipPoolEnt{p, bytes}); slip_pool_bytes += bytes;
            return;
        }
    }
    hipFree(p);
}
/* give every pooled buffer back to the runtime (tests; a host that wants the memory) */
extern "C" void slip_hip_pool_release(void)
{
    std::vector<SlipPoolEnt> drop;
    { std::lock_guard<std::mutex> g(slip_pool_mu); drop.swap(slip_pool); slip_pool_bytes = 0; }
    for (const SlipPoolEnt &e : drop) hipFree(e.p);
}

template <class T> static int dev_alloc(T **p, int64_t count)
{
    void *q = NULL;
    if (dev_malloc_bytes(&q, (size_t)(count > 0 ? count : 1) * sizeof(T))) return SLIP_HIP_OUT_OF_MEMORY;
    *p = (T *) q;
    return 0;
}
/* the debug buffer P.dbg (its regions: slip_dbg_* in ref_lu_pipe.h), zeroed */
static int dbg_alloc(int32_t **dbg, int n)
{
    if (dev_alloc(dbg, slip_dbg_words(n))) return SLIP_HIP_OUT_OF_MEMORY;
    return hipMemset(*dbg, 0, (size_t) slip_dbg_words(n) * sizeof(int32_t)) == hipSuccess ? 0 : SLIP_HIP_DEVICE_ERROR;
}
template <class T> static int dev_grow(T **p, int64_t old_count, int64_t new_count)
{
    T *q = NULL;
    if (dev_alloc(&q, new_count)) return SLIP_HIP_OUT_OF_MEMORY;
    if (old_count > 0 && hipMemcpy(q, *p, (size_t) old_count * sizeof(T), hipMemcpyDeviceToDevice) != hipSuccess) { dev_free(q); return SLIP_HIP_DEVICE_ERROR; }
    dev_free(*p);
    *p = q;
    return 0;
}

extern "C" const char *slip_hip_version(void) { return "slip_hip 0.2 (gfx950, column-worker pipeline)"; }

extern "C" void slip_hip_default_options(slip_hip_options *o)
{
    /* SLIP_LU_internal.h:136-149: pivot = SLIP_TOL_SMALLEST, tol = 1 */
    o->pivot = 3; o->tol = 1.0; o->limb_cap = 0; o->waves = 0; o->lnz_hint = 0; o->unz_hint = 0;
    o->workers = 0; o->reserved = 0;
}

extern "C" int slip_hip_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

/* entry points that need a device say so when there is none */
static int need_device(void)
{
    if (slip_hip_device_count() > 0) return SLIP_HIP_OK;
    fprintf(stderr, "slip_hip: no HIP device available -- this library has no CPU fallback\n");
    return SLIP_HIP_DEVICE_ERROR;
}

/* digits of a limb run (32-bit digits) with its high zero limbs trimmed; its nonzero limbs are (digits + 1) / 2 */
static inline int32_t limb_digits(const uint64_t *src, int64_t l)
{
    while (l > 0 && src[l - 1] == 0) l--;
    return l > 0 ? (int32_t)(2 * l - ((src[l - 1] >> 32) == 0)) : 0;
}

/* a limb slab of `count` entries -> signed digit counts and limb offsets (high zero limbs trimmed; the offsets advance by
 * the limbs given); total = limbs it spans, maxdig = digits of the widest entry (0 if none).  The capacity is checked from
 * the counts alone, before any limb is read. */
struct SlipSlab { int32_t *dig; int64_t *off; int64_t total; int32_t maxdig; };
static void slab_free(SlipSlab *s) { free(s->dig); free(s->off); s->dig = NULL; s->off = NULL; }
static int slab_prepare(int64_t count, const int32_t *len, const uint64_t *limbs, int64_t cap, SlipSlab *s)
{
    memset(s, 0, sizeof *s);
    int64_t total = 0;
    for (int64_t t = 0; t < count; t++) total += len[t] < 0 ? -(int64_t) len[t] : len[t];
    if (total > cap) return SLIP_HIP_INCORRECT_INPUT;
    s->dig = (int32_t *) malloc((size_t)(count > 0 ? count : 1) * 4);
    s->off = (int64_t *) malloc((size_t)(count > 0 ? count : 1) * 8);
    if (!s->dig || !s->off) { slab_free(s); return SLIP_HIP_OUT_OF_MEMORY; }
    for (int64_t t = 0, o = 0; t < count; t++) {
        const int64_t l = len[t] < 0 ? -(int64_t) len[t] : len[t];
        const int32_t dig = limb_digits(limbs + o, l);
        s->off[t] = o;
        s->dig[t] = len[t] < 0 ? -dig : dig;
        if (dig > s->maxdig) s->maxdig = dig;
        o += l;
    }
    s->total = total;
    return SLIP_HIP_OK;
}

/* operand records on the device: signed digit counts, limb offsets, the limbs */
struct SlipDevRecs { const int32_t *len; const int64_t *off; const uint64_t *limbs; };

/* a slab on the device: its three arrays and, where dev_slab_upload laid it out, the host's layout (s) */
struct SlipDevSlab { SlipSlab s; int32_t *len; int64_t *off; uint64_t *limbs; };
static void dev_slab_free(SlipDevSlab *d) { dev_free(d->len); dev_free(d->off); dev_free(d->limbs); slab_free(&d->s); memset(d, 0, sizeof *d); }
static SlipDevRecs dev_slab_recs(const SlipDevSlab &d) { const SlipDevRecs r = {d.len, d.off, d.limbs}; return r; }
/* a slab of `count` entries the host has laid out (s) into the three arrays of d (zeroed; s stays the caller's) */
static int dev_slab_put(int64_t count, const SlipSlab &s, const uint64_t *limbs, SlipDevSlab *d)
{
    int rc = 0;
    A_(dev_alloc(&d->len, count)); A_(dev_alloc(&d->off, count)); A_(dev_alloc(&d->limbs, s.total));
    UP_(d->len, s.dig, (size_t) count * 4); UP_(d->off, s.off, (size_t) count * 8); UP_(d->limbs, limbs, (size_t) s.total * 8);
    return rc;
}
/* a caller's slab of `count` entries checked, laid out (d->s) and brought to the device; d: zeroed */
static int dev_slab_upload(int64_t count, const int32_t *len, const uint64_t *limbs, int64_t cap, SlipDevSlab *d)
{
    int rc = slab_prepare(count, len, limbs, cap, &d->s);
    A_(dev_slab_put(count, d->s, limbs, d));
    return rc;
}

extern "C" void slip_hip_free(void *p) { free(p); }

/* ---- triplet files into limb slabs and back, host only, no GMP ----
 * The reference reads "m n nz" and nz lines "i j value" with gmp_fscanf %Zd (SLIP_LU/Demo/demos.c:245-331: indices are
 * 1-based unless the FIRST entry holds a 0) and builds the CSC by a counting sort on the columns that keeps the file
 * order inside a column and keeps duplicates (SLIP_LU/Source/slip_trip_to_mat.c:23-69).  Here the decimal strings go
 * straight into 64-bit limbs (base-10^18 chunks multiplied in), one pass over the file, one allocation per array. */
static int trip_parse_value(const char *s, const char *e, std::vector<uint64_t> &mag, int *neg)
{
    *neg = 0; mag.clear();
    if (s < e && (*s == '-' || *s == '+')) { *neg = *s == '-'; s++; }
    if (s >= e) return -1;
    for (const char *p = s; p < e; p++) if (*p < '0' || *p > '9') return -1;
    while (s < e) {
        const int take = (int)((e - s) % 18 ? (e - s) % 18 : 18);
        uint64_t chunk = 0, scale = 1;
        for (int q = 0; q < take; q++) { chunk = chunk * 10u + (uint64_t)(s[q] - '0'); scale *= 10u; }
        s += take;
        /* mag = mag * scale + chunk */
        unsigned __int128 carry = chunk;
        for (size_t l = 0; l < mag.size(); l++) { carry += (unsigned __int128) mag[l] * scale; mag[l] = (uint64_t) carry; carry >>= 64; }
        if (carry) mag.push_back((uint64_t) carry);
    }
    while (!mag.empty() && mag.back() == 0) mag.pop_back();
    if (mag.empty()) *neg = 0;
    return 0;
}

extern "C" int slip_hip_read_triplet(const char *path, int32_t *n_out, int64_t **Ap_out, int32_t **Ai_out, int32_t **Alen_out,
                                     uint64_t **Alimbs_out, int64_t *nlimbs_out)
{
    if (!path || !n_out || !Ap_out || !Ai_out || !Alen_out || !Alimbs_out) return SLIP_HIP_INCORRECT_INPUT;
    FILE *fp = fopen(path, "rb");
    if (!fp) return SLIP_HIP_INCORRECT_INPUT;
    std::vector<char> buf;
    { char tmp[1 << 16]; size_t r; while ((r = fread(tmp, 1, sizeof tmp, fp)) > 0) buf.insert(buf.end(), tmp, tmp + r); }
    fclose(fp);
    buf.push_back('\0');
    const char *p = buf.data(), *end = buf.data() + buf.size() - 1;
    auto token = [&](const char **ts, const char **te) -> int {
        while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++;
        if (p >= end) return -1;
        *ts = p;
        while (p < end && !(*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++;
        *te = p;
        return 0;
    };
    auto int_token = [&](long long *v) -> int {
        const char *ts, *te;
        if (token(&ts, &te)) return -1;
        char *ep = NULL; const long long x = strtoll(ts, &ep, 10);
        if (ep != te) return -1;
        *v = x; return 0;
    };
    long long m, n, nz;
    if (int_token(&m) || int_token(&n) || int_token(&nz)) return SLIP_HIP_INCORRECT_INPUT;
    if (n <= 0 || m != n || nz <= 0 || n > INT32_MAX || nz > INT32_MAX) return SLIP_HIP_INCORRECT_INPUT;
    std::vector<int32_t> I((size_t) nz), J((size_t) nz), L((size_t) nz);
    std::vector<int64_t> off((size_t) nz + 1);
    std::vector<uint64_t> limbs, mag;
    limbs.reserve((size_t) nz);
    long long dec = 0;
    for (long long t = 0; t < nz; t++) {
        long long i, j; const char *ts, *te; int neg;
        if (int_token(&i) || int_token(&j) || token(&ts, &te) || trip_parse_value(ts, te, mag, &neg)) return SLIP_HIP_INCORRECT_INPUT;
        if (t == 0) dec = (i < j ? i : j) == 0 ? 0 : 1;           /* demos.c:290-299 */
        i -= dec; j -= dec;
        if (i < 0 || j < 0 || i >= n || j >= n) return SLIP_HIP_INCORRECT_INPUT;
        I[(size_t) t] = (int32_t) i; J[(size_t) t] = (int32_t) j;
        off[(size_t) t] = (int64_t) limbs.size();
        L[(size_t) t] = neg ? -(int32_t) mag.size() : (int32_t) mag.size();
        limbs.insert(limbs.end(), mag.begin(), mag.end());
    }
    off[(size_t) nz] = (int64_t) limbs.size();
    /* counting sort on the columns, file order kept inside a column (slip_trip_to_mat.c:47-64) */
    int64_t *Ap = (int64_t *) calloc((size_t) n + 1, sizeof(int64_t));
    int32_t *Ai = (int32_t *) malloc((size_t) nz * sizeof(int32_t)), *Alen = (int32_t *) malloc((size_t) nz * sizeof(int32_t));
    uint64_t *Al = (uint64_t *) malloc((limbs.size() ? limbs.size() : 1) * sizeof(uint64_t));
    if (!Ap || !Ai || !Alen || !Al) { free(Ap); free(Ai); free(Alen); free(Al); return SLIP_HIP_OUT_OF_MEMORY; }
    for (long long t = 0; t < nz; t++) Ap[J[(size_t) t] + 1]++;
    for (long long c = 0; c < n; c++) Ap[c + 1] += Ap[c];
    std::vector<int64_t> w(Ap, Ap + n), src((size_t) nz);
    for (long long t = 0; t < nz; t++) { const int64_t q = w[(size_t) J[(size_t) t]]++; Ai[q] = I[(size_t) t]; Alen[q] = L[(size_t) t]; src[(size_t) q] = t; }
    int64_t o = 0;
    for (long long q = 0; q < nz; q++) {
        const int64_t t = src[(size_t) q], l = off[(size_t) t + 1] - off[(size_t) t];
        if (l) memcpy(Al + o, limbs.data() + off[(size_t) t], (size_t) l * 8);
        o += l;
    }
    *n_out = (int32_t) n; *Ap_out = Ap; *Ai_out = Ai; *Alen_out = Alen; *Alimbs_out = Al;
    if (nlimbs_out) *nlimbs_out = o;
    return SLIP_HIP_OK;
}

/* the inverse: CSC limb slabs to a triplet file the reference's SLIP_tripread accepts (1-based, decimal) */
extern "C" int slip_hip_write_triplet(const char *path, int32_t n, const int64_t *Ap, const int32_t *Ai, const int32_t *Alen, const uint64_t *Alimbs)
{
    if (!path || n <= 0 || !Ap || !Ai || !Alen || !Alimbs) return SLIP_HIP_INCORRECT_INPUT;
    FILE *fp = fopen(path, "wb");
    if (!fp) return SLIP_HIP_INCORRECT_INPUT;
    fprintf(fp, "%d %d %lld\n", n, n, (long long) Ap[n]);
    int64_t o = 0;
    std::vector<uint64_t> mag; std::vector<uint64_t> chunks;
    for (int32_t c = 0; c < n; c++)
        for (int64_t q = Ap[c]; q < Ap[c + 1]; q++) {
            const int l = Alen[q] < 0 ? -Alen[q] : Alen[q];
            mag.assign(Alimbs + o, Alimbs + o + l); o += l;
            chunks.clear();
            while (!mag.empty()) {                                   /* divide by 10^18, collect the remainders */
                unsigned __int128 rem = 0;
                for (size_t k = mag.size(); k-- > 0;) { rem = (rem << 64) | mag[k]; mag[k] = (uint64_t)(rem / 1000000000000000000ull); rem %= 1000000000000000000ull; }
                chunks.push_back((uint64_t) rem);
                while (!mag.empty() && mag.back() == 0) mag.pop_back();
            }
            fprintf(fp, "%d %d %s", Ai[q] + 1, c + 1, Alen[q] < 0 ? "-" : "");
            if (chunks.empty()) fprintf(fp, "0");
            else {
                fprintf(fp, "%llu", (unsigned long long) chunks.back());
                for (size_t k = chunks.size() - 1; k-- > 0;) fprintf(fp, "%018llu", (unsigned long long) chunks[k]);
            }
            fprintf(fp, "\n");
        }
    return fclose(fp) == 0 ? SLIP_HIP_OK : SLIP_HIP_DEVICE_ERROR;
}

extern "C" int slip_hip_matgen(int32_t n, double density, int32_t bits, uint64_t seed,
                               int64_t **Ap, int32_t **Ai, int64_t **Ax)
{
    return slip_matgen_csc(n, density, bits, seed, Ap, Ai, Ax) ? SLIP_HIP_OUT_OF_MEMORY : SLIP_HIP_OK;
}

/* choose waves / LDS split for the current xcap */
static void plan_launch(slip_hip_factor *f)
{
    SlipParams *P = &f->P;
    P->wcap = P->xcap + 8;
    P->bm_words = (P->n + 31) / 32;
    f->bitmap_in_lds = P->bm_words <= SLIP_BITMAP_LDS_MAX_WORDS;
    int fixed = SLIP_LDS_BITMAP + (f->bitmap_in_lds ? P->bm_words : 0);
    int nw = f->waves;
    /* per wave 3 scratch buffers of wcap digits, plus one workgroup-shared buffer */
    while (nw > 4 && fixed + (int64_t)(nw * 3 + 1) * P->wcap > SLIP_LDS_MAX_WORDS) nw /= 2;
    f->scratch_in_lds = fixed + (int64_t)(nw * 3 + 1) * P->wcap <= SLIP_LDS_MAX_WORDS;
    f->waves = nw;
    f->lds_words = fixed + (f->scratch_in_lds ? (nw * 3 + 1) * P->wcap : 0);
    P->bitmap_in_lds = f->bitmap_in_lds; P->scratch_in_lds = f->scratch_in_lds;
    /* block 0 of a factorisation launch may be the committer (ref_lu_pipe_commit.h): its rings, package copies and -- for
     * matrices up to SLIP_MIRROR_MAX rows -- the chain engine's mirror of pinv live in the same dynamic LDS */
    f->engine_ok = P->n <= SLIP_MIRROR_MAX && !f->no_engine;
    { const int cw = slip_commit_lds_words(P->n, f->engine_ok); if (!f->factors_only && cw <= SLIP_LDS_MAX_WORDS && cw > f->lds_words) f->lds_words = cw; }
}

#ifdef SLIP_EMULATE
/* test hooks of the CPU emulation build (never in the product library) */
static int64_t slip_emu_budget = 96ll << 30;
extern "C" void slip_emu_set_budget(long long bytes) { slip_emu_budget = bytes > 0 ? bytes : (96ll << 30); }
#endif
/* how many column workers: as many as can be resident (LDS-limited workgroups per CU times the CUs), capped by the
 * columns there are and by what their private vectors may take of the HBM */
static int32_t default_workers(const slip_hip_factor *f, int32_t xcap, int32_t asked)
{
    int cus = 256;
#ifndef SLIP_EMULATE
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        cus = prop.multiProcessorCount;
#else
    cus = 3;
#endif
    const int64_t lds_bytes = (int64_t) f->lds_words * 4;
    int per_cu = (int)((160 * 1024) / (lds_bytes > 0 ? lds_bytes : 1));
    const int by_waves = 8 / (f->waves > 0 ? f->waves : 1);           /* 232 VGPRs: two waves per SIMD, eight per CU */
    if (per_cu > by_waves) per_cu = by_waves;
#ifndef SLIP_EMULATE
    /* ... and never more than the runtime says can be resident with this launch shape (the default grid is what fits the
     * chip at once; larger grids asked for explicitly still work -- a workgroup that is not resident holds no ticket) */
    {
        int api = 0;
        const int fast = f->bitmap_in_lds && f->scratch_in_lds;
        const void *fn = fast ? (const void *) slip_factor_kernel<true> : (const void *) slip_factor_kernel<false>;
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds_bytes) == hipSuccess &&
            (fast ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&api, slip_factor_kernel<true>, 64 * f->waves, (size_t) lds_bytes)
                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&api, slip_factor_kernel<false>, 64 * f->waves, (size_t) lds_bytes)) == hipSuccess &&
            api >= 1 && api < per_cu) per_cu = api;
    }
#endif
    if (per_cu < 1) per_cu = 1;
    int64_t w = asked > 0 ? asked : (int64_t) cus * per_cu;
    const int64_t per_worker = (int64_t) f->n * (16 + 4 * (int64_t) xcap + 16) + 4096;
#ifdef SLIP_EMULATE
    const int64_t budget = slip_emu_budget;                             /* tests shrink it to force the re-application at a wider stride */
#else
    const int64_t budget = 96ll << 30;                                  /* of the 288 GB */
#endif
    if (w * per_worker > budget) w = budget / per_worker;
    if (w > f->n) w = f->n;
    if (w < 1) w = 1;
    return (int32_t) w;
}

/* the workers' private arrays (x rows and their digits, pattern overflow, row lists, HBM bitmap / scratch) and the
 * shared inverse cache for stride xcap */
static int alloc_x(slip_hip_factor *f, int32_t xcap, int keep_rows)
{
    SlipParams *P = &f->P;
    xcap = (xcap + 3) & ~3;
    /* plan for the new stride on a copy: the handle keeps its working buffers until every new one exists */
    const int32_t old_xcap = P->xcap, old_invcap = P->invcap, old_waves = f->waves;
    P->xcap = xcap; P->invcap = xcap + 8;
    plan_launch(f);
    /* how many workers: what was asked for (or what can be resident), never more than the HBM budget allows at THIS stride,
     * and never more than the private row arrays were sized for */
    int32_t W32 = default_workers(f, xcap, f->workers_asked);
    if (keep_rows && f->nworkers > 0 && W32 > f->nworkers) W32 = f->nworkers;
    const int64_t W = W32, n = P->n;
    uint32_t *nxd = NULL, *ninvd = NULL, *ngs = NULL, *ngb = NULL;
    int rc = 0;
    if (dev_alloc(&nxd, W * n * xcap) || dev_alloc(&ninvd, n * (int64_t) P->invcap) ||
        dev_alloc(&ngs, f->scratch_in_lds ? 1 : W * SLIP_SCRATCH_WAVES * 3 * (int64_t) P->wcap) ||
        dev_alloc(&ngb, f->bitmap_in_lds ? 1 : W * ((int64_t) P->bm_words + 64))) rc = SLIP_HIP_OUT_OF_MEMORY;
    SlipRow *nxrow = NULL; int32_t *npat = NULL, *nrlist = NULL, *nrpos = NULL, *nsrow = NULL; uint32_t *npkg = NULL, *njobs = NULL;
    if (!rc && !keep_rows) {
        if (dev_alloc(&nxrow, W * n) || dev_alloc(&npat, W * n) || dev_alloc(&nrlist, W * n) ||
            dev_alloc(&nrpos, W * n) || dev_alloc(&nsrow, W * n)) rc = SLIP_HIP_OUT_OF_MEMORY;
        /* tags start at 0 = "belongs to no column"; tickets count from 1 */
        else if (hipMemset(nxrow, 0, (size_t)(W * n) * sizeof(SlipRow)) != hipSuccess) rc = SLIP_HIP_DEVICE_ERROR;
    }
    if (!rc && (!keep_rows || !P->pkg.p_)) {
        if (dev_alloc(&npkg, W * (int64_t)(SLIP_PKG_WORDS + SLIP_MBOX_WORDS)) || dev_alloc(&njobs, W * (int64_t) SLIP_JOB_WORDS)) rc = SLIP_HIP_OUT_OF_MEMORY;
        else if (hipMemset(njobs, 0, (size_t) W * SLIP_JOB_WORDS * 4) != hipSuccess) rc = SLIP_HIP_DEVICE_ERROR;
    }
    if (rc) {
        /* nothing of the handle has been touched: it stays usable at the old stride */
        dev_free(nxd); dev_free(ninvd); dev_free(ngs); dev_free(ngb); dev_free(nxrow); dev_free(npat); dev_free(nrlist); dev_free(nrpos); dev_free(nsrow); dev_free(npkg); dev_free(njobs);
        if (old_xcap > 0) { P->xcap = old_xcap; P->invcap = old_invcap; f->waves = old_waves; plan_launch(f); }
        return rc;
    }
    dev_free(P->xd); dev_free(P->invd.p_); dev_free(P->gscratch); dev_free(P->gbitmap);
    P->xd = nxd; P->invd.p_ = ninvd; P->gscratch = ngs; P->gbitmap = ngb;
    if (!keep_rows) {
        dev_free(P->xrow); dev_free(P->pat); dev_free(P->rlist); dev_free(P->rpos); dev_free(P->srow);
        P->xrow = nxrow; P->pat = npat; P->rlist = nrlist; P->rpos = nrpos; P->srow = nsrow;
    }
    if (npkg) { dev_free(P->pkg.p_); dev_free(P->jobs.p_); P->pkg.p_ = npkg; P->jobs.p_ = njobs; }
    f->nworkers = W32; P->nworkers = W32; P->priv_rows = n;
    return 0;
}

static int upload_state(slip_hip_factor *f, hipStream_t stream)
{
    CK(hipMemcpyAsync(f->ds, &f->hs, sizeof(SlipState), hipMemcpyHostToDevice, stream));
    return 0;
}

extern "C" int slip_hip_factor_reset(slip_hip_factor *f)
{
    if (!f || f->factors_only) return SLIP_HIP_INCORRECT_INPUT;
    if (f->broken) return SLIP_HIP_DEVICE_ERROR;
    SlipParams *P = &f->P;
    const int32_t n = f->n;
    if (!P->xd || !P->xrow) return SLIP_HIP_OUT_OF_MEMORY;
    if (f->rescaled) rescale_drop(f);
    tview_drop(f);
    /* tickets double as row tags and are never reused -- until they would wrap: then every private row is untagged and
     * the count starts over (a launch draws at most one ticket per column plus one per worker) */
    if (f->hs.ticket > (1 << 30)) {
        CK(hipMemsetAsync(P->xrow, 0, (size_t)((int64_t) f->nworkers * n) * sizeof(SlipRow), 0));
        f->hs.ticket = 0;
    }
    CK(hipMemcpyAsync(P->pinv.p_, f->ident, (size_t) n * 4, hipMemcpyDeviceToDevice, 0));
    CK(hipMemcpyAsync(P->row_perm.p_, f->ident, (size_t) n * 4, hipMemcpyDeviceToDevice, 0));
    CK(hipMemsetAsync(P->Lready.p_, 0, (size_t) n * 4, 0));
    CK(hipMemsetAsync(P->Lp, 0, 8, 0)); CK(hipMemsetAsync(P->Up, 0, 8, 0));
    CK(hipMemsetAsync(P->Lo, 0, 8, 0)); CK(hipMemsetAsync(P->Uo, 0, 8, 0));
    {
        const int32_t ticket = f->hs.ticket;           /* the tickets (= row tags) never go back */
        memset(&f->hs, 0, sizeof f->hs);
        f->hs.ticket = ticket;
        f->hs.stop = INT64_MAX;
    }
    { const int e = upload_state(f, 0); if (e) return e; }
    CK(hipStreamSynchronize(0));
    f->last_status = 0; f->window_end = 0; f->kernel_ms = 0; f->launches = 0;
    return SLIP_HIP_OK;
}

extern "C" void slip_hip_factor_destroy(slip_hip_factor *f)
{
    if (!f) return;
    SlipParams *P = &f->P;
    dev_free(f->dAp); dev_free(f->dAi); dev_free(f->dAlen); dev_free(f->dAoff); dev_free(f->dAlimbs); dev_free(f->dq);
    dev_free(P->pinv.p_); dev_free(P->row_perm.p_); dev_free(P->xrow); dev_free(P->xd);
    dev_free(P->piv.p_); dev_free(P->invd.p_);
    dev_free(P->Lp); dev_free(P->Lo); dev_free(P->Li); dev_free(P->Le); dev_free(P->Llimbs);
    dev_free(P->Up); dev_free(P->Uo); dev_free(P->Ui); dev_free(P->Ue); dev_free(P->Ulimbs);
    dev_free(P->Lready.p_); dev_free(P->pat); dev_free(P->rlist); dev_free(P->rpos); dev_free(P->srow); dev_free(P->gscratch); dev_free(P->gbitmap); dev_free(P->dbg); dev_free(P->pkg.p_); dev_free(P->jobs.p_); dev_free(P->sw_row.p_); dev_free(P->sw_pos.p_);
    dev_free(f->ds); dev_free(f->ident);
    dev_free(f->chk_rp); dev_free(f->chk_re); dev_free(f->chk_rx);
    dev_free(f->chkt_rp); dev_free(f->chkt_re); dev_free(f->chkt_rx);
    rescale_drop(f);
    tview_drop(f);
    free(f->hq);
    if (f->ev0) hipEventDestroy(f->ev0);
    if (f->ev1) hipEventDestroy(f->ev1);
    free(f);
}

/* options -> the handle's launch shape */
static void apply_options(slip_hip_factor *f, const slip_hip_options &opt)
{
    f->waves = opt.waves > 0 ? opt.waves : 8;
    if (f->waves > SLIP_MAX_WAVES) f->waves = SLIP_MAX_WAVES;
    f->workers_asked = opt.workers > 0 ? (opt.workers > 4096 ? 4096 : opt.workers) : 0;
    f->nworkers = 0;       /* chosen in alloc_x once the LDS need is known */
    f->P.no_early = opt.reserved & 1;
    f->no_committer = (opt.reserved >> 1) & 1;
    f->no_farm = (opt.reserved >> 2) & 1;
    f->no_engine = (opt.reserved >> 3) & 1;
    f->P.quiet_neighbours = (opt.reserved >> 4) & 3;      /* experiment: workers within this many CUs of the committer stand aside */
}

static int make_ident(slip_hip_factor *f)
{
    const int32_t n = f->n;
    int32_t *id = (int32_t *) malloc((size_t) n * 4);
    if (!id) return SLIP_HIP_OUT_OF_MEMORY;
    for (int32_t i = 0; i < n; i++) id[i] = i;
    int rc = dev_alloc(&f->ident, n);
    UP_(f->ident, id, (size_t) n * 4);
    free(id);
    return rc;
}

/* host-side preparation of an m x n CSC (slip_hip_factor_create, slip_hip_check_solution: m = n; slip_hip_matrix_create): bounds
 * check, de-duplicate, digit counts.  out: the CSC with a repeated row of a column kept once, with its LAST value; signed
 * DIGIT counts, limb offsets, high zero limbs trimmed; maxdig = digits of the widest entry (at least 1).  Release with
 * host_a_free. */
struct SlipHostA { int64_t *Ap; int32_t *Ai, *Alen; int64_t *Aoff; uint64_t *Alimbs; int64_t nnz, nl; int32_t maxdig; };
static void host_a_free(SlipHostA *a) { free(a->Ap); free(a->Ai); free(a->Alen); free(a->Aoff); free(a->Alimbs); memset(a, 0, sizeof *a); }
static int prepare_A(int32_t m, int32_t n, const int64_t *Ap, const int32_t *Ai, const int32_t *Alen, const uint64_t *Alimbs, SlipHostA *out)
{
    memset(out, 0, sizeof *out);
    /* column and row numbers travel in 24-bit fields of the commit protocol (verdict words, package records); a row or a
     * column of fewer than 2^24 - 1 entries is also what the fixed-width sums of slip_check_kernel and slip_product_kernel need */
    if (m >= (1 << 24) - 1 || n >= (1 << 24) - 1) return SLIP_HIP_INCORRECT_INPUT;
    const int64_t annz = Ap[n];
    if (Ap[0] != 0 || annz < 1) return SLIP_HIP_INCORRECT_INPUT;

    int64_t *hAp = (int64_t *) malloc(((size_t) n + 1) * 8);
    int32_t *hAi = (int32_t *) malloc((size_t) annz * 4), *hAlen = (int32_t *) malloc((size_t) annz * 4);
    int64_t *hAoff = (int64_t *) malloc((size_t) annz * 8), *inoff = (int64_t *) malloc(((size_t) annz + 1) * 8);
    int32_t *last = (int32_t *) malloc((size_t) m * 4);
    if (!hAp || !hAi || !hAlen || !hAoff || !inoff || !last) {
        free(hAp); free(hAi); free(hAlen); free(hAoff); free(inoff); free(last);
        return SLIP_HIP_OUT_OF_MEMORY;
    }
    int bad = 0;
    inoff[0] = 0;
    for (int64_t p = 0; p < annz; p++) inoff[p + 1] = inoff[p] + (Alen[p] < 0 ? -(int64_t) Alen[p] : Alen[p]);
    for (int32_t i = 0; i < m; i++) last[i] = -1;
    uint64_t *hAlimbs = (uint64_t *) malloc((size_t)(inoff[annz] > 0 ? inoff[annz] : 1) * 8);
    if (!hAlimbs) bad = 2;
    int64_t onz = 0, ol = 0;
    int32_t maxdig = 1;
    for (int32_t j = 0; j < n && !bad; j++) {
        if (Ap[j + 1] < Ap[j]) { bad = 1; break; }
        hAp[j] = onz;
        /* a repeated row keeps its LAST value (slip_get_column.c:22 overwrites) */
        for (int64_t p = Ap[j]; p < Ap[j + 1]; p++) {
            int32_t r = Ai[p];
            if (r < 0 || r >= m) { bad = 1; break; }
            last[r] = (int32_t)(p - Ap[j]);
        }
        if (bad) break;
        for (int64_t p = Ap[j]; p < Ap[j + 1]; p++) {
            int32_t r = Ai[p];
            if (last[r] != (int32_t)(p - Ap[j])) continue;
            const uint64_t *src = Alimbs + inoff[p];
            const int32_t dig = limb_digits(src, inoff[p + 1] - inoff[p]);
            const int64_t l = (dig + 1) >> 1;
            hAi[onz] = r; hAlen[onz] = Alen[p] < 0 ? -dig : dig; hAoff[onz] = ol;
            memcpy(hAlimbs + ol, src, (size_t) l * 8);
            if (dig > maxdig) maxdig = dig;
            ol += l; onz++;
        }
        for (int64_t p = Ap[j]; p < Ap[j + 1]; p++) last[Ai[p]] = -1;
    }
    hAp[n] = onz;
    free(inoff); free(last);
    if (bad) { free(hAp); free(hAi); free(hAlen); free(hAoff); free(hAlimbs); return bad == 2 ? SLIP_HIP_OUT_OF_MEMORY : SLIP_HIP_INCORRECT_INPUT; }
    out->Ap = hAp; out->Ai = hAi; out->Alen = hAlen; out->Aoff = hAoff; out->Alimbs = hAlimbs;
    out->nnz = onz; out->nl = ol; out->maxdig = maxdig;
    return SLIP_HIP_OK;

}

extern "C" int slip_hip_factor_create(slip_hip_factor **out, int32_t n,
                                      const int64_t *Ap, const int32_t *Ai,
                                      const int32_t *Alen, const uint64_t *Alimbs,
                                      const int32_t *q, const slip_hip_options *opt_in)
{
    /* SLIP_LU_factorize.c:48-52: any missing argument is SLIP_INCORRECT_INPUT */
    if (!out || n <= 0 || !Ap || !Ai || !Alen || !Alimbs || !q) return SLIP_HIP_INCORRECT_INPUT;
    *out = NULL;
    TRY_(need_device());
    slip_hip_options opt;
    if (opt_in) opt = *opt_in; else slip_hip_default_options(&opt);
    if (opt.pivot < 0 || opt.pivot > 5) return SLIP_HIP_INCORRECT_INPUT;
    SlipHostA ha;
    TRY_(prepare_A(n, n, Ap, Ai, Alen, Alimbs, &ha));
    {
        char *seen = (char *) calloc((size_t) n, 1);
        int bad = !seen ? 2 : 0;
        for (int32_t j = 0; j < n && !bad; j++) { if (q[j] < 0 || q[j] >= n || seen[q[j]]) bad = 1; else seen[q[j]] = 1; }
        free(seen);
        if (bad) { host_a_free(&ha); return bad == 2 ? SLIP_HIP_OUT_OF_MEMORY : SLIP_HIP_INCORRECT_INPUT; }
    }
    const int64_t onz = ha.nnz, ol = ha.nl;
    const int32_t maxdig = ha.maxdig;

    slip_hip_factor *f = (slip_hip_factor *) calloc(1, sizeof(slip_hip_factor));
    if (!f) { host_a_free(&ha); return SLIP_HIP_OUT_OF_MEMORY; }
    SlipParams *P = &f->P;
    f->n = n; f->annz = onz; f->alimbs = ol; f->amaxdig = maxdig;
    f->Acap_nz = f->A0_nz = onz > 0 ? onz : 1; f->Acap_nl = f->A0_nl = ol > 0 ? ol : 1; f->Anl_used = ol;
    apply_options(f, opt);
    P->n = n; P->pivot_scheme = opt.pivot; P->limb_cap = opt.limb_cap;
    if (!(opt.tol > 0)) { P->tol_mode = 0; P->tol_m = 0; P->tol_e = 0; }
    else {
        int e; double fr = frexp(opt.tol, &e);            /* mpq_set_d takes the double exactly */
        P->tol_mode = 1; P->tol_m = (uint64_t) ldexp(fr, 53); P->tol_e = e - 53;
    }
    int rc = 0;
    A_(dev_alloc(&f->dAp, (int64_t) n + 1)); A_(dev_alloc(&f->dAi, onz)); A_(dev_alloc(&f->dAlen, onz));
    A_(dev_alloc(&f->dAoff, onz)); A_(dev_alloc(&f->dAlimbs, ol)); A_(dev_alloc(&f->dq, n));
    A_(dev_alloc(&P->pinv.p_, n)); A_(dev_alloc(&P->row_perm.p_, n));
    A_(dev_alloc(&P->piv.p_, n)); A_(dev_alloc(&P->Lready.p_, n)); A_(dbg_alloc(&P->dbg, n)); A_(dev_alloc(&P->sw_row.p_, n)); A_(dev_alloc(&P->sw_pos.p_, n));
    A_(make_ident(f));
    HIP_(hipMemset(P->piv.p_, 0, (size_t) n * sizeof(SlipPiv)));
    /* initial sizes: S->lnz/unz only size the first allocation in the reference too */
    P->Lcap_nz = opt.lnz_hint > 0 ? opt.lnz_hint : 4 * onz + n;
    P->Ucap_nz = opt.unz_hint > 0 ? opt.unz_hint : 4 * onz + n;
    if (P->Lcap_nz < n) P->Lcap_nz += n;
    if (P->Ucap_nz < n) P->Ucap_nz += n;
    /* window mode: the cap, plus room for the working width of a division item on a value at the cap (result + shifted-out zeros of rho[h] + 1) */
    const int32_t cap_digits = opt.limb_cap > 0 ? 2 * opt.limb_cap + 40 : 0;
    int32_t xcap0 = cap_digits > 0 ? cap_digits : (2 * maxdig + 8 > 16 ? 2 * maxdig + 8 : 16);
    P->Lcap_nl = P->Lcap_nz * 2;
    P->Ucap_nl = P->Ucap_nz * 2;
    A_(dev_alloc(&P->Lp, (int64_t) n + 1)); A_(dev_alloc(&P->Lo, (int64_t) n + 1)); A_(dev_alloc(&P->Li, P->Lcap_nz)); A_(dev_alloc(&P->Le, P->Lcap_nz));
    A_(dev_alloc(&P->Llimbs, P->Lcap_nl));
    A_(dev_alloc(&P->Up, (int64_t) n + 1)); A_(dev_alloc(&P->Uo, (int64_t) n + 1)); A_(dev_alloc(&P->Ui, P->Ucap_nz)); A_(dev_alloc(&P->Ue, P->Ucap_nz));
    A_(dev_alloc(&P->Ulimbs, P->Ucap_nl));
    A_(dev_alloc(&f->ds, 1));
    A_(alloc_x(f, xcap0, 0));
    UP_(f->dAp, ha.Ap, ((size_t) n + 1) * 8); UP_(f->dAi, ha.Ai, (size_t) onz * 4); UP_(f->dAlen, ha.Alen, (size_t) onz * 4);
    UP_(f->dAoff, ha.Aoff, (size_t) onz * 8); UP_(f->dAlimbs, ha.Alimbs, (size_t) ol * 8); UP_(f->dq, q, (size_t) n * 4);
    host_a_free(&ha);
    if (!rc && !(f->hq = (int32_t *) malloc((size_t) n * 4))) rc = SLIP_HIP_OUT_OF_MEMORY;
    if (!rc) memcpy(f->hq, q, (size_t) n * 4);
    P->Ap = f->dAp; P->Ai = f->dAi; P->Alen = f->dAlen; P->Aoff = f->dAoff; P->Alimbs = f->dAlimbs; P->q = f->dq;
    HIP_(hipEventCreate(&f->ev0)); HIP_(hipEventCreate(&f->ev1));
    if (!rc) { f->hs.ticket = 0; rc = slip_hip_factor_reset(f); }
    if (rc) { slip_hip_factor_destroy(f); return rc; }
    *out = f;
    return SLIP_HIP_OK;
}

/* new stride of the dense vectors; x and the inverse cache are scratch, the pivot records of the
 * K committed columns survive (their cached inverses are recomputed on demand) */
static int grow_x_keep(slip_hip_factor *f, int64_t xcap, int32_t K)
{
    SlipParams *P = &f->P;
    if (xcap > (1 << 28)) return SLIP_HIP_OUT_OF_MEMORY;
    SlipPiv *keep = NULL;
    if (K > 0) {
        keep = (SlipPiv *) malloc((size_t) K * sizeof(SlipPiv));
        if (!keep) return SLIP_HIP_OUT_OF_MEMORY;
        if (hipMemcpy(keep, P->piv.p_, (size_t) K * sizeof(SlipPiv), hipMemcpyDeviceToHost) != hipSuccess) { free(keep); return SLIP_HIP_DEVICE_ERROR; }
    }
    /* a wider stride may change how many workers fit: alloc_x re-applies the HBM budget at the new stride and never goes
     * beyond the count the private row arrays were sized for; on failure the handle keeps its old buffers */
    int e = alloc_x(f, (int32_t) xcap, 1);
    if (!e && K > 0) {
        for (int32_t k = 0; k < K; k++) keep[k].invlen = 0;
        if (hipMemcpy(P->piv.p_, keep, (size_t) K * sizeof(SlipPiv), hipMemcpyHostToDevice) != hipSuccess) e = SLIP_HIP_DEVICE_ERROR;
    }
    free(keep);
    return e;
}

#ifdef SLIP_EMULATE
static unsigned long long slip_emu_seed = 1;
extern "C" void slip_emu_set_seed(unsigned long long s) { slip_emu_seed = s; }
/* weak-store mode of the emulator (tests/emu/fiber_emu.h): sc1 stores land late and out of order */
extern "C" void slip_emu_set_weak(int on) { emu::set_weak(on); }
/* overwrite the length of entry t of L (isU 0) or U (isU 1): what a protocol error on the device would leave behind */
extern "C" int slip_emu_corrupt_entry(slip_hip_factor *f, int isU, long long t, int newlen)
{
    if (!f || t < 0 || t >= (isU ? f->hs.Unz : f->hs.Lnz)) return -1;
    SlipEnt *e = (isU ? f->P.Ue : f->P.Le) + t;
    e->len = newlen;
    return 0;
}
#endif

/* ---- the launch of a grid of column workers (slip_factor_kernel, slip_solve_kernel): each caller clears its state fields,
 * picks the workers and records ev0, then launch_device (or launch_emulated) and launch_end ---- */
#ifndef SLIP_EMULATE
/* the FAST instance (bitmap and scratch both in LDS) or the slow one of a column-worker kernel, W workgroups */
template <class... Params, class... Args>
static int launch_device(const slip_hip_factor *f, int32_t W, hipStream_t stream, void (*fast)(Params...), void (*slow)(Params...), Args... args)
{
    const size_t lds_bytes = (size_t) f->lds_words * 4;
    void (*kernel)(Params...) = f->bitmap_in_lds && f->scratch_in_lds ? fast : slow;
    CK(hipFuncSetAttribute((const void *) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds_bytes));
    hipLaunchKernelGGL(kernel, dim3(W), dim3(64 * f->waves), lds_bytes, stream, args...);
    CK(hipGetLastError());
    return 0;
}
#else
/* W emulated workgroups, each with its own LDS arena, run body(fast, Pw, lds) with the worker's share of P */
template <class Body> static int launch_emulated(const slip_hip_factor *f, const SlipParams &P, int32_t W, Body body)
{
    const int fast = f->bitmap_in_lds && f->scratch_in_lds;
    const size_t words = (((size_t) f->lds_words + 64) + 3) & ~(size_t) 3;      /* every emulated workgroup's LDS 16-byte aligned, as on the device */
    uint32_t *lds_all = (uint32_t *) calloc((size_t) W * words, 4);
    if (!lds_all) return SLIP_HIP_OUT_OF_MEMORY;
    emu::set_seed(slip_emu_seed);
    emu::launch(W, 64 * f->waves, [P, fast, body, lds_all, words]() {
        SlipParams Pw;
        slip_worker_params(&Pw, P, slip_block());
        body(fast, Pw, lds_all + (size_t) slip_block() * words);
    });
    free(lds_all);
    return 0;
}
#endif
/* the launch's end: ev1, the state read back, the stream synchronised; the launch's time is added to *ms */
static int launch_end(slip_hip_factor *f, hipStream_t stream, double *ms)
{
    CK(hipEventRecord(f->ev1, stream));
    CK(hipMemcpyAsync(&f->hs, f->ds, sizeof(SlipState), hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
    float t = 0;
    CK(hipEventElapsedTime(&t, f->ev0, f->ev1));
    *ms += t;
    return 0;
}

static int launch_columns(slip_hip_factor *f, hipStream_t stream)
{
    f->P.k0 = f->hs.F; f->P.t0 = f->hs.ticket;
    f->hs.stop = INT64_MAX; f->hs.exited = 0; for (int q_ = 0; q_ < 32; q_++) f->hs.farm_hint[q_] = 0; f->hs.dbg_who = 0; f->hs.committer_up = 0; f->hs.committer_where = 0;
    f->P.st = f->ds; f->P.in_factor = 1;
    TRY_(upload_state(f, stream));
    /* no more workers than columns left */
    int32_t W = f->nworkers;
    /* block 0 of a launch with at least two workgroups of at least two waves is the committer (ref_lu_pipe_commit.h) */
    f->P.committer = W >= 2 && f->waves >= 2 && f->bitmap_in_lds && f->scratch_in_lds && !f->P.no_early && !f->no_committer && f->P.pivot_scheme != 2 && f->P.pkg.p_ != NULL;
    if (W > f->P.k_stop - f->hs.F + f->P.committer) W = f->P.k_stop - f->hs.F + f->P.committer;
    if (W < 1) W = 1;
    if (W < 2) f->P.committer = 0;
    if (f->P.committer && slip_commit_lds_words(f->P.n, 0) > f->lds_words) f->P.committer = 0;      /* (cannot happen: plan_launch made room) */
    f->P.engine = f->P.committer && f->engine_ok && slip_commit_lds_words(f->P.n, 1) <= f->lds_words;
    f->P.nworkers = W;
    if (f->P.committer) CK(hipMemsetAsync(f->P.pkg.p_, 0, (size_t) W * (SLIP_PKG_WORDS + SLIP_MBOX_WORDS) * 4, stream));
    f->P.farm = W >= 2 && !f->no_farm && f->P.jobs.p_ != NULL;
    if (f->P.farm) CK(hipMemsetAsync(f->P.jobs.p_, 0, (size_t) W * SLIP_JOB_WORDS * 4, stream));
    CK(hipEventRecord(f->ev0, stream));
#ifndef SLIP_EMULATE
    TRY_(launch_device(f, W, stream, slip_factor_kernel<true>, slip_factor_kernel<false>, f->P, f->ds));
#else
    SlipState *ds = f->ds;
    TRY_(launch_emulated(f, f->P, W, [ds](int fast, const SlipParams &Pw, uint32_t *lds) {
        if (Pw.committer && slip_block() == 0) { if (fast) slip_committer<true>(Pw, ds, lds); else slip_committer<false>(Pw, ds, lds); }
        else if (fast) slip_factor_worker<true>(Pw, ds, lds);
        else slip_factor_worker<false>(Pw, ds, lds);
        slip_worker_exit(Pw, ds);
    }));
#endif
    TRY_(launch_end(f, stream, &f->kernel_ms));
    f->launches++;
    /* where the launch ended: the frontier; why: the stop word, if it names the frontier column */
    SlipState *h = &f->hs;
    h->k_next = h->F;
    h->status = SLIPDEV_OK; h->status_k = h->F;
    if ((int)(h->stop & 0xFF) == SLIPDEV_INTERNAL) h->status = SLIPDEV_INTERNAL;
    else if (h->stop != INT64_MAX && (h->stop >> 8) == (int64_t) h->F) h->status = (int)(h->stop & 0xFF);
    else if (h->F < f->P.k_stop) h->status = SLIPDEV_INTERNAL;       /* the workers left without a reason */
    return 0;
}

extern "C" int slip_hip_factor_run(slip_hip_factor *f, int32_t kmax, void *stream_v)
{
    if (!f || f->factors_only) return SLIP_HIP_INCORRECT_INPUT;
    if (f->broken) return SLIP_HIP_DEVICE_ERROR;
    hipStream_t stream = (hipStream_t) stream_v;
    SlipParams *P = &f->P;
    SlipState *h = &f->hs;
    if (!P->xd || !P->xrow) return SLIP_HIP_OUT_OF_MEMORY;
    if (kmax <= 0 || kmax > f->n) kmax = f->n;
    f->kernel_ms = 0; f->launches = 0; f->window_end = 0;
    P->k_stop = kmax;
    int rc = SLIP_HIP_OK;
    while (h->F < kmax) {
        int e = launch_columns(f, stream);
        if (e) { rc = e; break; }
        if (h->status == SLIPDEV_OK) continue;
        if (h->status == SLIPDEV_SINGULAR) { rc = SLIP_HIP_SINGULAR; break; }
        if (h->status == SLIPDEV_WINDOW_END) { f->window_end = 1; break; }
        if (h->status == SLIPDEV_GROW_L) {
            /* the slab that ran out is the one to double (cf. slip_sparse_realloc.c) */
            int64_t nz = P->Lcap_nz * 2, nl = P->Lcap_nl * 2;
            if ((e = dev_grow(&P->Li, h->Lnz, nz)) || (e = dev_grow(&P->Le, h->Lnz, nz)) ||
                (e = dev_grow(&P->Llimbs, h->Lnl, nl))) { rc = e; break; }
            P->Lcap_nz = nz; P->Lcap_nl = nl;
        } else if (h->status == SLIPDEV_GROW_U) {
            int64_t nz = P->Ucap_nz * 2, nl = P->Ucap_nl * 2;
            if ((e = dev_grow(&P->Ui, h->Unz, nz)) || (e = dev_grow(&P->Ue, h->Unz, nz)) ||
                (e = dev_grow(&P->Ulimbs, h->Unl, nl))) { rc = e; break; }
            P->Ucap_nz = nz; P->Ucap_nl = nl;
        } else if (h->status == SLIPDEV_GROW_X) {
            e = grow_x_keep(f, (int64_t) P->xcap * 2, h->F);
            if (e) { rc = e; break; }
        } else {
            fprintf(stderr, "slip_hip: kernel stopped with internal status %d at column %d (frontier %d, ready %d, stop %lld; wait %d of column %d: %d %d)\n",
                    h->status, h->status_k, h->F, h->F2, (long long) h->stop, h->dbg_who, h->dbg_k, h->dbg_a, h->dbg_b);
            rc = SLIP_HIP_DEVICE_ERROR; break;
        }
    }
    f->last_status = rc;
    return rc;
}

/* ---- given columns: K columns of L and U in the reference's CSC with ORIGINAL row ids and piv_row[k] the pivot row of
 * column k -- the factors of slip_hip_factor_from_factors (K = n) and the prefix of slip_hip_factor_set_prefix ---- */
struct SlipGiven {
    int32_t K, maxdig; int64_t lnz, unz, lnl, unl;
    const int64_t *Lp, *Up; const int32_t *Li, *Ui; const uint64_t *Llimbs, *Ulimbs;     /* the caller's arrays */
    SlipEnt *Le, *Ue; SlipPiv *piv; int64_t *Lo, *Uo;                                      /* the host image built from them */
};
static void given_free(SlipGiven *g) { free(g->Le); free(g->Ue); free(g->piv); free(g->Lo); free(g->Uo); memset(g, 0, sizeof *g); }

/* entry records of a limb slab (offsets advance by the limbs given); *maxdig grows to the widest entry; returns the limbs spanned */
static int64_t slab_to_entries(int64_t nz, const int32_t *len, const uint64_t *limbs, SlipEnt *ent, int32_t *maxdig)
{
    int64_t o = 0;
    for (int64_t t = 0; t < nz; t++) {
        const int64_t l = len[t] < 0 ? -(int64_t) len[t] : len[t];
        const int32_t dig = limb_digits(limbs + o, l);
        const uint64_t top = dig ? limbs[o + ((dig + 1) >> 1) - 1] : 0;
        ent[t].off = o; ent[t].len = len[t] < 0 ? -dig : dig;
        ent[t].bits = dig ? 32 * dig - __builtin_clz(dig & 1 ? (uint32_t) top : (uint32_t)(top >> 32)) : 0;
        if (dig > *maxdig) *maxdig = dig;
        o += l;
    }
    return o;
}

/* the pivot record of the L entry e (nonzero): trailing zero bits and, for one or two digits, 1/(odd part) mod 2^64 by Newton */
static SlipPiv pivot_record(const SlipEnt &e, const uint64_t *Llimbs)
{
    const uint64_t *pv = Llimbs + e.off;
    const int32_t dig = e.len < 0 ? -e.len : e.len;
    int z = 0; { int64_t w = 0; while (pv[w] == 0) { w++; z += 64; } z += __builtin_ctzll(pv[w]); }
    SlipPiv pr; memset(&pr, 0, sizeof pr);
    pr.off = e.off; pr.len = e.len; pr.bits = e.bits; pr.ctz = z; pr.invlen = 0; pr.lo = pv[0];
    if (dig <= 2) { uint64_t d = pr.lo >> z, x = d; for (int r = 0; r < 5; r++) x *= 2 - d * x; pr.inv64 = x; }
    return pr;
}

/* validate the K given columns and build their host image: the column pointers first (every later read is indexed by them),
 * then the row ids, then the entries and the pivots */
static int load_given(int32_t n, int32_t K, const int64_t *Lp, const int32_t *Li, const int32_t *Llen, const uint64_t *Llimbs,
                      const int64_t *Up, const int32_t *Ui, const int32_t *Ulen, const uint64_t *Ulimbs, const int32_t *piv_row, SlipGiven *g)
{
    memset(g, 0, sizeof *g);
    if (Lp[0] != 0 || Up[0] != 0) return SLIP_HIP_INCORRECT_INPUT;
    for (int32_t k = 0; k < K; k++) if (Lp[k + 1] < Lp[k] || Up[k + 1] <= Up[k]) return SLIP_HIP_INCORRECT_INPUT;
    const int64_t lnz = Lp[K], unz = Up[K];
    for (int64_t t = 0; t < lnz; t++) if (Li[t] < 0 || Li[t] >= n) return SLIP_HIP_INCORRECT_INPUT;
    for (int64_t t = 0; t < unz; t++) if (Ui[t] < 0 || Ui[t] >= n) return SLIP_HIP_INCORRECT_INPUT;
    g->Le = (SlipEnt *) malloc((size_t)(lnz > 0 ? lnz : 1) * sizeof(SlipEnt)); g->Ue = (SlipEnt *) malloc((size_t) unz * sizeof(SlipEnt));   /* unz >= K > 0 */
    g->piv = (SlipPiv *) calloc((size_t) K, sizeof(SlipPiv));
    g->Lo = (int64_t *) malloc(((size_t) K + 1) * 8); g->Uo = (int64_t *) malloc(((size_t) K + 1) * 8);
    if (!g->Le || !g->Ue || !g->piv || !g->Lo || !g->Uo) { given_free(g); return SLIP_HIP_OUT_OF_MEMORY; }
    g->K = K; g->lnz = lnz; g->unz = unz; g->maxdig = 1;
    g->Lp = Lp; g->Up = Up; g->Li = Li; g->Ui = Ui; g->Llimbs = Llimbs; g->Ulimbs = Ulimbs;
    g->lnl = slab_to_entries(lnz, Llen, Llimbs, g->Le, &g->maxdig);
    g->unl = slab_to_entries(unz, Ulen, Ulimbs, g->Ue, &g->maxdig);
    /* rho_k is the entry of L(:,k) in the pivot row (slip_get_pivot.c:178-182), and the last entry of U(:,k) */
    for (int32_t k = 0; k < K; k++) {
        int64_t at = -1;
        for (int64_t t = Lp[k]; t < Lp[k + 1]; t++) if (Li[t] == piv_row[k]) at = t;
        if (at < 0 || g->Le[at].len == 0 || Ui[Up[k + 1] - 1] != piv_row[k]) { given_free(g); return SLIP_HIP_INCORRECT_INPUT; }
        g->piv[k] = pivot_record(g->Le[at], Llimbs);
    }
    for (int32_t k = 0; k <= K; k++) { g->Lo[k] = k < K ? g->Le[Lp[k]].off : g->lnl; g->Uo[k] = k < K ? g->Ue[Up[k]].off : g->unl; }
    return SLIP_HIP_OK;
}

/* the given columns to the handle's slabs (which hold them), and the host state of a launch that stopped at column K */
static int given_upload(slip_hip_factor *f, const SlipGiven &g)
{
    SlipParams *P = &f->P;
    const size_t K = (size_t) g.K;
    int rc = 0;
    UP_(P->piv.p_, g.piv, K * sizeof(SlipPiv));
    UP_(P->Lp, g.Lp, (K + 1) * 8); UP_(P->Lo, g.Lo, (K + 1) * 8); UP_(P->Li, g.Li, (size_t) g.lnz * 4); UP_(P->Le, g.Le, (size_t) g.lnz * sizeof(SlipEnt)); UP_(P->Llimbs, g.Llimbs, (size_t) g.lnl * 8);
    UP_(P->Up, g.Up, (K + 1) * 8); UP_(P->Uo, g.Uo, (K + 1) * 8); UP_(P->Ui, g.Ui, (size_t) g.unz * 4); UP_(P->Ue, g.Ue, (size_t) g.unz * sizeof(SlipEnt)); UP_(P->Ulimbs, g.Ulimbs, (size_t) g.unl * 8);
    if (!rc) {
        SlipState *h = &f->hs;
        h->F = g.K; h->F2 = g.K; h->k_next = g.K;
        h->Lnz = g.lnz; h->Unz = g.unz; h->Lnl = g.lnl; h->Unl = g.unl; h->Lnl_exact = g.lnl; h->Unl_exact = g.unl;
        h->c_maxdig = (unsigned long long) g.maxdig;
    }
    return rc;
}

/* ---- a handle around GIVEN factors (the caller's L, U, pinv): what SLIP_LU_solve receives ---- */
extern "C" int slip_hip_factor_from_factors(slip_hip_factor **out, int32_t n,
                                            const int64_t *Lp, const int32_t *Li, const int32_t *Llen, const uint64_t *Llimbs,
                                            const int64_t *Up, const int32_t *Ui, const int32_t *Ulen, const uint64_t *Ulimbs,
                                            const int32_t *pinv, const slip_hip_options *opt_in)
{
    if (!out || n <= 0 || !Lp || !Li || !Llen || !Llimbs || !Up || !Ui || !Ulen || !Ulimbs || !pinv) return SLIP_HIP_INCORRECT_INPUT;
    *out = NULL;
    TRY_(need_device());
    slip_hip_options opt;
    if (opt_in) opt = *opt_in; else slip_hip_default_options(&opt);
    /* the pivot row of column k: the row i with pinv[i] = k */
    int32_t *rowperm = (int32_t *) malloc((size_t) n * 4);
    if (!rowperm) return SLIP_HIP_OUT_OF_MEMORY;
    int rc = 0;
    for (int32_t i = 0; i < n; i++) rowperm[i] = -1;
    for (int32_t i = 0; i < n && !rc; i++) { if (pinv[i] < 0 || pinv[i] >= n || rowperm[pinv[i]] >= 0) rc = SLIP_HIP_INCORRECT_INPUT; else rowperm[pinv[i]] = i; }
    SlipGiven g; memset(&g, 0, sizeof g);
    A_(load_given(n, n, Lp, Li, Llen, Llimbs, Up, Ui, Ulen, Ulimbs, rowperm, &g));
    slip_hip_factor *f = NULL;
    if (!rc && !(f = (slip_hip_factor *) calloc(1, sizeof(slip_hip_factor)))) rc = SLIP_HIP_OUT_OF_MEMORY;
    if (rc) { free(rowperm); given_free(&g); return rc; }
    SlipParams *P = &f->P;
    f->n = n; f->factors_only = 1;
    apply_options(f, opt);
    if (f->workers_asked <= 0) f->workers_asked = 64;  /* right-hand sides in flight; more are taken in turn */
    P->n = n; P->pivot_scheme = opt.pivot; P->limb_cap = 0; P->k_stop = n;
    P->Lcap_nz = g.lnz; P->Ucap_nz = g.unz; P->Lcap_nl = g.lnl > 0 ? g.lnl : 1; P->Ucap_nl = g.unl > 0 ? g.unl : 1;
    A_(dev_alloc(&P->pinv.p_, n)); A_(dev_alloc(&P->row_perm.p_, n));
    A_(dev_alloc(&P->piv.p_, n)); A_(dev_alloc(&P->Lready.p_, n)); A_(dbg_alloc(&P->dbg, n)); A_(dev_alloc(&P->sw_row.p_, n)); A_(dev_alloc(&P->sw_pos.p_, n));
    A_(dev_alloc(&P->Lp, (int64_t) n + 1)); A_(dev_alloc(&P->Lo, (int64_t) n + 1)); A_(dev_alloc(&P->Li, g.lnz)); A_(dev_alloc(&P->Le, g.lnz)); A_(dev_alloc(&P->Llimbs, P->Lcap_nl));
    A_(dev_alloc(&P->Up, (int64_t) n + 1)); A_(dev_alloc(&P->Uo, (int64_t) n + 1)); A_(dev_alloc(&P->Ui, g.unz)); A_(dev_alloc(&P->Ue, g.unz)); A_(dev_alloc(&P->Ulimbs, P->Ucap_nl));
    A_(dev_alloc(&f->ds, 1));
    A_(alloc_x(f, 2 * g.maxdig + 8, 0));
    UP_(P->pinv.p_, pinv, (size_t) n * 4); UP_(P->row_perm.p_, rowperm, (size_t) n * 4);
    f->hs.stop = INT64_MAX;
    A_(given_upload(f, g));
    HIP_(hipEventCreate(&f->ev0)); HIP_(hipEventCreate(&f->ev1));
    UP_(f->ds, &f->hs, sizeof(SlipState));
    free(rowperm); given_free(&g);
    if (rc) { slip_hip_factor_destroy(f); return rc; }
    *out = f;
    return SLIP_HIP_OK;
}

/* ---- continue from a prefix (the subtree farm's last step) ----
 * The first K columns of the factorisation are GIVEN (the blocks' columns, factorised elsewhere and rescaled to the global
 * pivot chain: slip_lu_amd/parallel.py): L(:,k), U(:,k) in the reference's CSC with ORIGINAL row ids and the pivot row of
 * every column.  The handle is put into the state a launch that stopped at column K leaves -- the permutation replayed from
 * the pivot rows (slip_get_pivot.c:164-176), the pivots' records, the column pointers, every given column ready -- and
 * slip_hip_factor_run goes on with column K (the separator columns of the farm), SLIP_LU_factorize.c:190-264 from k = K. */
extern "C" int slip_hip_factor_set_prefix(slip_hip_factor *f, int32_t K,
                                          const int64_t *Lp, const int32_t *Li, const int32_t *Llen, const uint64_t *Llimbs,
                                          const int64_t *Up, const int32_t *Ui, const int32_t *Ulen, const uint64_t *Ulimbs,
                                          const int32_t *piv_row)
{
    if (!f || f->factors_only || K < 0 || K > f->n) return SLIP_HIP_INCORRECT_INPUT;
    if (K > 0 && (!Lp || !Li || !Llen || !Llimbs || !Up || !Ui || !Ulen || !Ulimbs || !piv_row)) return SLIP_HIP_INCORRECT_INPUT;
    TRY_(slip_hip_factor_reset(f));
    if (K == 0) return SLIP_HIP_OK;
    SlipParams *P = &f->P;
    const int32_t n = f->n;
    int32_t *pinv = (int32_t *) malloc((size_t) n * 4), *rowperm = (int32_t *) malloc((size_t) n * 4);
    int32_t *swr = (int32_t *) malloc((size_t) K * 4), *swp = (int32_t *) malloc((size_t) K * 4), *ready = (int32_t *) malloc((size_t) K * 4);
    SlipGiven g; memset(&g, 0, sizeof g);
    int rc = !pinv || !rowperm || !swr || !swp || !ready ? SLIP_HIP_OUT_OF_MEMORY : 0;
    /* the permutation: column k's pivot row changes places with the row at position k (slip_get_pivot.c:164-176) */
    if (!rc) for (int32_t i = 0; i < n; i++) { pinv[i] = i; rowperm[i] = i; }
    for (int32_t k = 0; k < K && !rc; k++) {
        const int32_t r = piv_row[k];
        if (r < 0 || r >= n || pinv[r] < k) { rc = SLIP_HIP_INCORRECT_INPUT; break; }
        const int32_t p = pinv[r], d = rowperm[k];
        swr[k] = d; swp[k] = p; ready[k] = 1;
        rowperm[k] = r; rowperm[p] = d; pinv[r] = k; pinv[d] = p;
        if (p == k) { pinv[r] = k; rowperm[k] = r; }
    }
    A_(load_given(n, K, Lp, Li, Llen, Llimbs, Up, Ui, Ulen, Ulimbs, piv_row, &g));
    /* room for the prefix and as much again (the run doubles a slab that fills up) */
    if (!rc && (g.lnz + n > P->Lcap_nz || g.lnl + n > P->Lcap_nl)) {
        const int64_t nz = 2 * (g.lnz + n), nl = 2 * (g.lnl + n);
        A_(dev_grow(&P->Li, 0, nz)); A_(dev_grow(&P->Le, 0, nz)); A_(dev_grow(&P->Llimbs, 0, nl));
        if (!rc) { P->Lcap_nz = nz; P->Lcap_nl = nl; }
    }
    if (!rc && (g.unz + n > P->Ucap_nz || g.unl + n > P->Ucap_nl)) {
        const int64_t nz = 2 * (g.unz + n), nl = 2 * (g.unl + n);
        A_(dev_grow(&P->Ui, 0, nz)); A_(dev_grow(&P->Ue, 0, nz)); A_(dev_grow(&P->Ulimbs, 0, nl));
        if (!rc) { P->Ucap_nz = nz; P->Ucap_nl = nl; }
    }
    if (!rc) {
        UP_(P->pinv.p_, pinv, (size_t) n * 4); UP_(P->row_perm.p_, rowperm, (size_t) n * 4);
        UP_(P->sw_row.p_, swr, (size_t) K * 4); UP_(P->sw_pos.p_, swp, (size_t) K * 4); UP_(P->Lready.p_, ready, (size_t) K * 4);
        A_(given_upload(f, g));
        if (!rc) { f->hs.Fpiv = piv_row[K - 1]; f->hs.status_k = K; }
        A_(upload_state(f, 0));
        HIP_(hipStreamSynchronize(0));
        /* values wider than the private x rows were sized for: the stride grows now rather than in the first launch */
        if (!rc && 2 * (int64_t) g.maxdig + 8 > P->xcap) rc = grow_x_keep(f, 2 * (int64_t) g.maxdig + 8, K);
        f->last_status = rc;
    }
    free(pinv); free(rowperm); free(swr); free(swp); free(ready); given_free(&g);
    return rc;
}

/* ---- back to column K, and a column of the resident A replaced (no counterpart in the reference; cf. klu_refactor and the
 * basis change of a simplex code).  REF LU is left-looking: columns 0..p-1 of L and U, their pivots and their row swaps
 * depend on A(:, q[0..p-1]) alone, so after a change to the column at position p the first p columns still are the exact
 * factorisation and slip_hip_factor_run goes on from there.  Everything happens on data already in HBM (slip_rewind_kernel,
 * slip_splice_kernel, slip_offscan_kernel + slip_pack_kernel); only the new column crosses to the device. ---- */
static void check_views_drop(slip_hip_factor *f)
{
    dev_free(f->chk_rp); dev_free(f->chk_re); dev_free(f->chk_rx); f->chk_rp = NULL; f->chk_re = NULL; f->chk_rx = NULL;
    dev_free(f->chkt_rp); dev_free(f->chkt_re); dev_free(f->chkt_rx); f->chkt_rp = NULL; f->chkt_re = NULL; f->chkt_rx = NULL;
}

/* a device step failed after the handle's arrays had begun to change: it must not serve a mixed state */
static int handle_broken(slip_hip_factor *f)
{
    f->broken = 1; f->last_status = SLIP_HIP_DEVICE_ERROR;
    return SLIP_HIP_DEVICE_ERROR;
}

/* ---- the host side every service kernel shares (one kernel argument record, four waves a workgroup; the emulator runs
 * the same body as two workgroups of two waves, whatever the item count): the grids, the launch, the timed section ---- */
#ifndef SLIP_EMULATE
#define SERVICE_WAVES 4
#else
#define SERVICE_WAVES 2
#endif

static int64_t service_grid(int64_t items, int64_t per_block)
{
#ifndef SLIP_EMULATE
    const int64_t blocks = (items + per_block - 1) / per_block;
    return blocks > 4096 ? 4096 : blocks < 1 ? 1 : blocks;
#else
    (void) items; (void) per_block;
    return 2;
#endif
}
/* one thread per item of a service kernel's loop */
static int64_t service_blocks(int64_t items) { return service_grid(items, 64 * SERVICE_WAVES); }
/* one wave per item */
static int64_t wave_blocks(int64_t items) { return service_grid(items, SERVICE_WAVES); }

/* no more workgroups than keep the waves' scratch, per_wave digits each, within 256 MiB */
static int64_t fit_scratch(int64_t blocks, int64_t per_wave)
{
#ifndef SLIP_EMULATE
    const int64_t fit = ((int64_t) 256 << 20) / (SERVICE_WAVES * per_wave * 4);
    if (blocks > fit) blocks = fit;
    return blocks < 1 ? 1 : blocks;
#else
    (void) per_wave;
    return blocks;
#endif
}

/* the grid of a kernel whose waves take `chunk` entries per round: few entries are spread one to a wave, many fill the lanes of
 * 4096 waves; at most block_cap workgroups, and no more than fit_scratch allows */
struct SlipWaveGrid { int64_t blocks, chunk; };
static SlipWaveGrid wave_grid(int64_t ne, int64_t per_wave, int64_t block_cap)
{
    SlipWaveGrid g;
#ifndef SLIP_EMULATE
    g.chunk = (ne + 4095) / 4096;
    if (g.chunk > 64) g.chunk = 64;
    g.blocks = (ne + g.chunk * SERVICE_WAVES - 1) / (g.chunk * SERVICE_WAVES);
    if (g.blocks > block_cap) g.blocks = block_cap;
#else
    (void) ne; (void) block_cap;
    g.chunk = 5; g.blocks = 2;
#endif
    g.blocks = fit_scratch(g.blocks, per_wave);
    return g;
}

/* SERVICE_LAUNCH(X, blocks, stream, A): slip_X_kernel(A) on the stream (the emulator: slip_X_body(A), at once); the launch's
 * error is the result; nothing is synchronised.  Not for slip_offscan and slip_tview_scan, whose emulated bodies take the
 * array that is __shared__ on the device: those two sites launch by hand. */
template <class Args> static int service_launch(void (*entry)(Args), int64_t blocks, hipStream_t stream, const Args &A)
{
#ifndef SLIP_EMULATE
    hipLaunchKernelGGL(entry, dim3((unsigned) blocks), dim3(64 * SERVICE_WAVES), 0, stream, A);
    CK(hipGetLastError());
#else
    (void) stream;
    emu::launch((int) blocks, 64 * SERVICE_WAVES, [entry, A]() { entry(A); }, 256 * 1024, 1);
#endif
    return 0;
}
#ifndef SLIP_EMULATE
#define SERVICE_LAUNCH(X, blocks, stream, A) service_launch(slip_##X##_kernel, blocks, stream, A)
#else
#define SERVICE_LAUNCH(X, blocks, stream, A) service_launch(slip_##X##_body, blocks, stream, A)
#endif

/* a timed section of a stream: begin, the launches, end (which waits for them); the events go with the record */
namespace {                                               /* (its member functions are no symbols of the library) */
struct SlipTimed {
    hipEvent_t ev0 = NULL, ev1 = NULL;
    int begin(hipStream_t stream)
    {
        CK(hipEventCreate(&ev0)); CK(hipEventCreate(&ev1));
        CK(hipEventRecord(ev0, stream));
        return 0;
    }
    int end(hipStream_t stream, double *ms_out)
    {
        float ms = 0;
        CK(hipEventRecord(ev1, stream)); CK(hipStreamSynchronize(stream));
        CK(hipEventElapsedTime(&ms, ev0, ev1));
        if (ms_out) *ms_out = ms;
        return 0;
    }
    ~SlipTimed() { if (ev0) hipEventDestroy(ev0); if (ev1) hipEventDestroy(ev1); }
};
}

static int rewind_launch(SlipRewindArgs A, int phase, int64_t items, hipStream_t stream)
{
    A.phase = phase;
    return SERVICE_LAUNCH(rewind, service_blocks(items), stream, A);
}

/* the handle as slip_hip_factor_run(f, K) from a reset would have left it, 0 < K < the committed columns.  *changed: the
 * device arrays have been written (an error from then on breaks the handle). */
static int rewind_device(slip_hip_factor *f, int32_t K, hipStream_t stream, int *changed)
{
    SlipParams *P = &f->P;
    const int32_t n = f->n, Kold = f->hs.F;
    int32_t *win = NULL, *rsave = NULL; unsigned long long *dout = NULL, hout[8];
    int rc = 0;
    A_(dev_alloc(&win, (int64_t) n - K)); A_(dev_alloc(&rsave, (int64_t) Kold - K)); A_(dev_alloc(&dout, 8));
    if (!rc) {
        if (f->rescaled) rescale_drop(f);
        tview_drop(f);
        *changed = 1;
        /* tickets never go back; should they be about to wrap, every private row is untagged (as slip_hip_factor_reset) */
        if (f->hs.ticket > (1 << 30)) {
            HIP_(hipMemsetAsync(P->xrow, 0, (size_t)((int64_t) f->nworkers * n) * sizeof(SlipRow), stream));
            f->hs.ticket = 0;
        }
        HIP_(hipMemsetAsync(win, 0x7f, (size_t)(n - K) * 4, stream));
        HIP_(hipMemsetAsync(dout, 0, sizeof hout, stream));
        SlipRewindArgs A; memset(&A, 0, sizeof A);
        A.n = n; A.K = K; A.Kold = Kold;
        A.row_perm = P->row_perm.p_; A.pinv = P->pinv.p_; A.Lready = P->Lready.p_; A.sw_row = P->sw_row.p_; A.sw_pos = P->sw_pos.p_;
        A.win = win; A.rsave = rsave; A.Lp = P->Lp; A.Up = P->Up; A.Lo = P->Lo; A.Uo = P->Uo; A.Le = P->Le; A.Ue = P->Ue; A.out = dout;
        A.lnz_max = f->hs.Lnz; A.unz_max = f->hs.Unz;
        A_(rewind_launch(A, 0, Kold - K, stream));
        A_(rewind_launch(A, 1, n - K, stream));
        A_(rewind_launch(A, 2, n - K, stream));
        A_(rewind_launch(A, 3, f->hs.Lnz > f->hs.Unz ? f->hs.Lnz : f->hs.Unz, stream));
        HIP_(hipMemcpyAsync(hout, dout, sizeof hout, hipMemcpyDeviceToHost, stream));
        HIP_(hipStreamSynchronize(stream));
    }
    dev_free(win); dev_free(rsave); dev_free(dout);
    if (rc) return rc;
    SlipState *h = &f->hs;
    if ((int64_t) hout[2] > h->Lnz || (int64_t) hout[3] > h->Unz || (int64_t) hout[4] > h->Lnl || (int64_t) hout[5] > h->Unl) return SLIP_HIP_DEVICE_ERROR;
    {
        const int32_t ticket = h->ticket; const unsigned long long maxdig = h->c_maxdig;
        memset(h, 0, sizeof *h);
        h->ticket = ticket; h->c_maxdig = maxdig;         /* (an upper bound now) */
        h->stop = INT64_MAX;
    }
    h->F = K; h->F2 = K; h->k_next = K; h->status_k = K; h->Fpiv = (int32_t) hout[6];
    h->Lnl_exact = (int64_t) hout[0]; h->Unl_exact = (int64_t) hout[1];
    h->Lnz = (int64_t) hout[2]; h->Unz = (int64_t) hout[3]; h->Lnl = (int64_t) hout[4]; h->Unl = (int64_t) hout[5];
    TRY_(upload_state(f, stream));
    CK(hipStreamSynchronize(stream));
    f->last_status = 0; f->window_end = 0; f->kernel_ms = 0; f->launches = 0;
    return SLIP_HIP_OK;
}

/* rewind to K <= the committed columns (checked by the callers); K equal to them: nothing to do */
static int rewind_to(slip_hip_factor *f, int32_t K, hipStream_t stream)
{
    if (K == f->hs.F) return SLIP_HIP_OK;
    if (K == 0) return slip_hip_factor_reset(f);
    int changed = 0;
    const int rc = rewind_device(f, K, stream, &changed);
    if (rc && changed) return handle_broken(f);
    return rc;
}

extern "C" int slip_hip_factor_rewind(slip_hip_factor *f, int32_t K, const int32_t *q_tail, void *stream_v)
{
    if (!f || f->factors_only) return SLIP_HIP_INCORRECT_INPUT;
    if (f->broken || f->last_status == SLIP_HIP_DEVICE_ERROR) return SLIP_HIP_DEVICE_ERROR;
    const int32_t n = f->n;
    if (K < 0 || K > f->hs.F) return SLIP_HIP_INCORRECT_INPUT;
    if (!f->P.xd || !f->P.xrow) return SLIP_HIP_OUT_OF_MEMORY;
    if (q_tail) {
        /* a permutation of the ids at positions K..n-1 */
        char *there = (char *) calloc((size_t) n, 1);
        if (!there) return SLIP_HIP_OUT_OF_MEMORY;
        int bad = 0;
        for (int32_t p = K; p < n; p++) there[f->hq[p]] = 1;
        for (int32_t p = K; p < n && !bad; p++) { const int32_t j = q_tail[p - K]; if (j < 0 || j >= n || there[j] != 1) bad = 1; else there[j] = 2; }
        free(there);
        if (bad) return SLIP_HIP_INCORRECT_INPUT;
    }
    TRY_(rewind_to(f, K, (hipStream_t) stream_v));
    if (q_tail && K < n) {
        if (hipMemcpy(f->dq + K, q_tail, (size_t)(n - K) * 4, hipMemcpyHostToDevice) != hipSuccess) return handle_broken(f);
        memcpy(f->hq + K, q_tail, (size_t)(n - K) * 4);
        check_views_drop(f);                              /* both are laid out by position */
    }
    return SLIP_HIP_OK;
}

/* the limbs a scan counted (the sum of its workgroups' chunks) */
static int offscan_total(const unsigned long long *bsum, int64_t blocks, int64_t *total_out, hipStream_t stream)
{
    unsigned long long h[1024], total = 0;
    CK(hipMemcpyAsync(h, bsum, (size_t) blocks * 8, hipMemcpyDeviceToHost, stream));
    CK(hipStreamSynchronize(stream));
    for (int64_t b = 0; b < blocks; b++) total += h[b];
    *total_out = (int64_t) total;
    return 0;
}

/* the limbs the device counted for the live entries must be the host's figure: it sized the new slab */
static int a_compact_total(const unsigned long long *bsum, int64_t blocks, int64_t live, hipStream_t stream)
{
    int64_t total = 0;
    TRY_(offscan_total(bsum, blocks, &total, stream));
    return total == live ? 0 : SLIP_HIP_DEVICE_ERROR;
}

/* the workgroups of a scan over `count` entries (at most 1024: bsum is read back into a fixed array) */
static int64_t offscan_blocks(int64_t count)
{
#ifndef SLIP_EMULATE
    int64_t blocks = (count + 2047) / 2048; if (blocks > 1024) blocks = 1024; if (blocks < 1) blocks = 1;
    return blocks;
#else
    (void) count;
    return 2;
#endif
}

/* both phases of slip_offscan_kernel: off[t] = the limbs of the entries before t, bsum[b] = the limbs of workgroup b's chunk
 * (by hand: the emulated scan takes a block's share of tmp, which is __shared__ on the device) */
static int offscan_run(int64_t count, const int32_t *len, int64_t *off, unsigned long long *bsum, int64_t blocks, hipStream_t stream)
{
    SlipOffScanArgs S; memset(&S, 0, sizeof S);
    S.count = count; S.len = len; S.off = off; S.bsum = bsum;
    int rc = 0;
#ifndef SLIP_EMULATE
    for (int phase = 0; phase < 2 && !rc; phase++) {
        S.phase = phase;
        hipLaunchKernelGGL(slip_offscan_kernel, dim3((unsigned) blocks), dim3(256), 0, stream, S);
        HIP_(hipGetLastError());
    }
#else
    (void) stream;
    uint64_t *tmp = (uint64_t *) calloc((size_t) blocks * 40, 8);
    if (!tmp) rc = SLIP_HIP_OUT_OF_MEMORY;
    for (int phase = 0; phase < 2 && !rc; phase++) {
        S.phase = phase;
        emu::launch((int) blocks, 128, [S, tmp]() { slip_offscan_body(S, tmp + 40 * slip_block()); }, 256 * 1024, 1);
    }
    free(tmp);
#endif
    return rc;
}

/* the dead limbs squeezed out of the slab of A: new offsets by a scan over the entries, the limbs moved entry by entry */
static int a_compact(slip_hip_factor *f, hipStream_t stream)
{
    const int64_t nnz = f->annz, live = f->alimbs, newcap = live + live / 2 + 1;
    const int64_t blocks = offscan_blocks(nnz);
    uint64_t *nl = NULL; int64_t *noff = NULL; unsigned long long *bsum = NULL;
    int rc = 0;
    A_(dev_alloc(&nl, newcap)); A_(dev_alloc(&noff, f->Acap_nz)); A_(dev_alloc(&bsum, blocks));
    if (!rc) {
        SlipPackArgs A; memset(&A, 0, sizeof A);
        A.count = nnz; A.len = f->dAlen; A.soff = f->dAoff; A.doff = noff; A.src = f->dAlimbs; A.dst = nl;
        A_(offscan_run(nnz, f->dAlen, noff, bsum, blocks, stream));
        A_(a_compact_total(bsum, blocks, live, stream));
        A_(SERVICE_LAUNCH(pack, wave_blocks(nnz), stream, A));
        HIP_(hipStreamSynchronize(stream));
    }
    if (rc) { dev_free(nl); dev_free(noff); dev_free(bsum); return rc; }
    dev_free(f->dAlimbs); dev_free(f->dAoff); dev_free(bsum);
    f->dAlimbs = nl; f->dAoff = noff; f->P.Alimbs = nl; f->P.Aoff = noff;
    f->Acap_nl = newcap; f->Anl_used = live;
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_factor_replace_column(slip_hip_factor *f, int32_t j, int32_t nz, const int32_t *rows, const int32_t *len,
                                              const uint64_t *limbs, int64_t limbs_cap, void *stream_v)
{
    if (!f || f->factors_only) return SLIP_HIP_INCORRECT_INPUT;
    if (f->broken || f->last_status == SLIP_HIP_DEVICE_ERROR) return SLIP_HIP_DEVICE_ERROR;
    const int32_t n = f->n;
    if (j < 0 || j >= n || nz < 1 || !rows || !len || !limbs || limbs_cap < 0) return SLIP_HIP_INCORRECT_INPUT;
    if (!f->P.xd || !f->P.xrow) return SLIP_HIP_OUT_OF_MEMORY;
    hipStream_t stream = (hipStream_t) stream_v;
    {
        int64_t total = 0;
        for (int32_t t = 0; t < nz; t++) {
            if (rows[t] < 0 || rows[t] >= n) return SLIP_HIP_INCORRECT_INPUT;
            total += len[t] < 0 ? -(int64_t) len[t] : len[t];
            if (total > limbs_cap) return SLIP_HIP_INCORRECT_INPUT;
        }
    }
    /* the column as prepare_A would have laid it out: a repeated row once, with its LAST value; signed digit counts, high
     * zero limbs trimmed; offsets from the start of the column's limbs */
    int32_t *last = (int32_t *) malloc((size_t) n * 4), *cAi = (int32_t *) malloc((size_t) nz * 4), *cAlen = (int32_t *) malloc((size_t) nz * 4);
    int64_t *cAoff = (int64_t *) malloc((size_t) nz * 8);
    uint64_t *cl = (uint64_t *) malloc((size_t)(limbs_cap > 0 ? limbs_cap : 1) * 8);
    int32_t *oldlen = NULL;
    int64_t cnz = 0, cnl = 0; int32_t cmaxdig = 1;
    int rc = !last || !cAi || !cAlen || !cAoff || !cl ? SLIP_HIP_OUT_OF_MEMORY : 0;
    if (!rc) {
        for (int32_t t = 0; t < nz; t++) last[rows[t]] = t;
        int64_t in = 0;
        for (int32_t t = 0; t < nz; t++) {
            const int64_t l0 = len[t] < 0 ? -(int64_t) len[t] : len[t];
            if (last[rows[t]] == t) {
                const int32_t dig = limb_digits(limbs + in, l0);
                const int64_t l = (dig + 1) >> 1;
                cAi[cnz] = rows[t]; cAlen[cnz] = len[t] < 0 ? -dig : dig; cAoff[cnz] = cnl;
                memcpy(cl + cnl, limbs + in, (size_t) l * 8);
                if (dig > cmaxdig) cmaxdig = dig;
                cnl += l; cnz++;
            }
            in += l0;
        }
    }
    /* where the column stands: its position in q, its extent in the resident arrays and the limbs it holds there */
    int32_t p = 0;
    int64_t ap[2] = {0, 0}, old_l = 0;
    if (!rc) {
        while (p < n && f->hq[p] != j) p++;
        DOWN_(ap, f->dAp + j, 16);
        if (!rc && (ap[0] < 0 || ap[1] < ap[0] || ap[1] > f->annz)) rc = SLIP_HIP_DEVICE_ERROR;
    }
    const int64_t nz_old = ap[1] - ap[0], nnz_new = f->annz - nz_old + cnz;
    if (!rc && nz_old > 0) {
        if (!(oldlen = (int32_t *) malloc((size_t) nz_old * 4))) rc = SLIP_HIP_OUT_OF_MEMORY;
        DOWN_(oldlen, f->dAlen + ap[0], (size_t) nz_old * 4);
        if (!rc) for (int64_t t = 0; t < nz_old; t++) old_l += ((oldlen[t] < 0 ? -(int64_t) oldlen[t] : oldlen[t]) + 1) >> 1;
    }
    /* the new entry arrays: the old capacity, doubled when it is short, never beyond twice the live entries plus the
     * initial allocation */
    int64_t ncap = f->Acap_nz;
    if (nnz_new > ncap) ncap = 2 * ncap > nnz_new ? 2 * ncap : nnz_new;
    if (ncap > 2 * nnz_new + f->A0_nz) ncap = 2 * nnz_new + f->A0_nz;
    int32_t *nAi = NULL, *nAlen = NULL; int64_t *nAoff = NULL;
    A_(dev_alloc(&nAi, ncap)); A_(dev_alloc(&nAlen, ncap)); A_(dev_alloc(&nAoff, ncap));
    if (rc) {
        /* nothing of the handle has changed */
        dev_free(nAi); dev_free(nAlen); dev_free(nAoff);
        free(last); free(cAi); free(cAlen); free(cAoff); free(cl); free(oldlen);
        return rc;
    }
    /* from here on a failure leaves a mixed state behind: the handle then refuses further use */
    if (p < f->hs.F) rc = rewind_to(f, p, stream);
    /* the limbs: appended to the slab, which doubles when it is full */
    if (!rc && f->Anl_used + cnl > f->Acap_nl) {
        const int64_t need = f->Anl_used + cnl, cap = 2 * f->Acap_nl > need ? 2 * f->Acap_nl : need;
        rc = dev_grow(&f->dAlimbs, f->Anl_used, cap);
        if (!rc) { f->Acap_nl = cap; f->P.Alimbs = f->dAlimbs; }
    }
    if (!rc) for (int64_t t = 0; t < cnz; t++) cAoff[t] += f->Anl_used;
    UP_(f->dAlimbs + f->Anl_used, cl, (size_t) cnl * 8);
    UP_(nAi + ap[0], cAi, (size_t) cnz * 4); UP_(nAlen + ap[0], cAlen, (size_t) cnz * 4); UP_(nAoff + ap[0], cAoff, (size_t) cnz * 8);
    if (!rc) {
        SlipSpliceArgs A; memset(&A, 0, sizeof A);
        A.n = n; A.j = j; A.a0 = ap[0]; A.a1 = ap[1]; A.nz_new = cnz; A.nnz_old = f->annz;
        A.Ai = f->dAi; A.Alen = f->dAlen; A.Aoff = f->dAoff; A.nAi = nAi; A.nAlen = nAlen; A.nAoff = nAoff; A.Ap = f->dAp;
        A_(SERVICE_LAUNCH(splice, service_blocks(f->annz > n ? f->annz : n), stream, A));
        HIP_(hipStreamSynchronize(stream));
    }
    free(last); free(cAi); free(cAlen); free(cAoff); free(cl); free(oldlen);
    if (rc) { dev_free(nAi); dev_free(nAlen); dev_free(nAoff); handle_broken(f); return rc == SLIP_HIP_OUT_OF_MEMORY ? rc : SLIP_HIP_DEVICE_ERROR; }
    dev_free(f->dAi); dev_free(f->dAlen); dev_free(f->dAoff);
    f->dAi = nAi; f->dAlen = nAlen; f->dAoff = nAoff; f->P.Ai = nAi; f->P.Alen = nAlen; f->P.Aoff = nAoff;
    f->Acap_nz = ncap; f->annz = nnz_new; f->Anl_used += cnl; f->alimbs += cnl - old_l;
    if (cmaxdig > f->amaxdig) f->amaxdig = cmaxdig;       /* (an upper bound: a narrower column does not lower it) */
    check_views_drop(f);
    /* more dead limbs than live ones, or a slab larger than twice its live content plus the initial allocation: compact */
    if (f->Anl_used - f->alimbs > f->alimbs || f->Acap_nl > 2 * f->alimbs + f->A0_nl) {
        const int e = a_compact(f, stream);
        if (e) { handle_broken(f); return e; }
    }
    /* values wider than the private x rows were sized for: the stride grows now rather than in the first launch */
    if (2 * (int64_t) cmaxdig + 8 > f->P.xcap) {
        const int e = grow_x_keep(f, 2 * (int64_t) cmaxdig + 8, f->hs.F);
        if (e == SLIP_HIP_DEVICE_ERROR) return handle_broken(f);
        if (e) return e;                                  /* the handle keeps its old stride; the run would grow it */
    }
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_factor_a_storage(const slip_hip_factor *f, int64_t out[4])
{
    if (!f || !out || f->factors_only) return SLIP_HIP_INCORRECT_INPUT;
    out[0] = f->annz; out[1] = f->Acap_nz; out[2] = f->alimbs; out[3] = f->Acap_nl;
    return SLIP_HIP_OK;
}

/* ---- REF triangular solves on the resident factors (SLIP_LU_solve.c:41-86) ---- */
#ifndef SLIP_SOLVE_HELPERS
#define SLIP_SOLVE_HELPERS 16
#endif
/* one launch of slip_solve_kernel with the parameters P (the handle's, or those of its transposed view); its time is added to *ms */
static int launch_solve(slip_hip_factor *f, SlipParams &P, const SlipSolveArgs &A, int32_t *rhs_done, hipStream_t stream, double *ms)
{
    P.t0 = f->hs.ticket;
    f->hs.stop = INT64_MAX; f->hs.exited = 0;
    P.farm = 0; P.committer = 0; P.st = f->ds; P.in_factor = 0;
    for (int q_ = 0; q_ < 32; q_++) f->hs.farm_hint[q_] = 0;
    TRY_(upload_state(f, stream));
    /* one workgroup per right-hand side in flight; with fewer right-hand sides than workgroups, up to SLIP_SOLVE_HELPERS more
     * that only help with the long update queues (ref_lu_pipe_cols.h: slip_solve_worker) */
    int32_t W = f->nworkers;
    if (W > A.nrhs) {
        int32_t H = f->no_farm || !P.jobs.p_ ? 0 : SLIP_SOLVE_HELPERS;
        if (A.nrhs + H > W) H = W - A.nrhs;
        W = A.nrhs + H;
        P.farm = H > 0;
    }
    if (W < 1) W = 1;
    P.nworkers = W;
    if (P.farm) CK(hipMemsetAsync(P.jobs.p_, 0, (size_t) W * SLIP_JOB_WORDS * 4, stream));
    CK(hipEventRecord(f->ev0, stream));
#ifndef SLIP_EMULATE
    TRY_(launch_device(f, W, stream, slip_solve_kernel<true>, slip_solve_kernel<false>, P, f->ds, A, rhs_done));
#else
    SlipState *ds = f->ds;
    TRY_(launch_emulated(f, P, W, [ds, A, rhs_done](int fast, const SlipParams &Pw, uint32_t *lds) {
        if (fast) slip_solve_worker<true>(Pw, ds, A, rhs_done, lds);
        else slip_solve_worker<false>(Pw, ds, A, rhs_done, lds);
    }));
#endif
    return launch_end(f, stream, ms);
}

/* ---- the transposed view of the complete factors (slip_tview_kernel), for slip_hip_factor_solve_transpose ---- */
static void tview_drop(slip_hip_factor *f)
{
    dev_free(f->tLp); dev_free(f->tUp); dev_free(f->tLi); dev_free(f->tUi); dev_free(f->tLe); dev_free(f->tUe); dev_free(f->tpiv); dev_free(f->tinvd);
    free(f->tpinv);
    f->tLp = f->tUp = NULL; f->tLi = f->tUi = NULL; f->tLe = f->tUe = NULL; f->tpiv = NULL; f->tinvd = NULL; f->tinvcap = 0; f->tpinv = NULL;
}

static SlipTViewArgs tview_args(const slip_hip_factor *f)
{
    const SlipParams &P = f->P;
    SlipTViewArgs A; memset(&A, 0, sizeof A);
    A.n = f->n; A.Lp = P.Lp; A.Up = P.Up; A.Li = P.Li; A.Ui = P.Ui; A.Le = P.Le; A.Ue = P.Ue; A.pinv = P.pinv.p_; A.piv = P.piv.p_;
    A.tLp = f->tLp; A.tUp = f->tUp; A.tLi = f->tLi; A.tUi = f->tUi; A.tLe = f->tLe; A.tUe = f->tUe; A.tpiv = f->tpiv;
    return A;
}

static int tview_launch(SlipTViewArgs A, int phase, hipStream_t stream)
{
    A.phase = phase;
    return SERVICE_LAUNCH(tview, phase == 2 ? service_blocks(A.n) : wave_blocks(2 * (int64_t) A.n), stream, A);
}

/* the view's inverse cache follows the handle's stride (a GROW_X reallocates both): a new one starts empty, so the pivot
 * records are laid out again with invlen = 0 */
static int tview_sync(slip_hip_factor *f, hipStream_t stream)
{
    if (f->tinvcap == f->P.invcap) return 0;
    dev_free(f->tinvd); f->tinvd = NULL; f->tinvcap = 0;
    TRY_(dev_alloc(&f->tinvd, (int64_t) f->n * f->P.invcap));
    f->tinvcap = f->P.invcap;
    return tview_launch(tview_args(f), 2, stream);
}

/* count by position, exclusive scan, scatter (slip_tview_kernel), from the factors in HBM; f->tview_ms: the device time */
static int tview_build(slip_hip_factor *f, hipStream_t stream)
{
    SlipParams *P = &f->P;
    const int32_t n = f->n;
    const int64_t lnz = f->hs.Lnz, unz = f->hs.Unz;
    int32_t *cnt = NULL;
    int rc = 0;
    if (!f->ident) A_(make_ident(f));                            /* (a handle around given factors has none yet) */
    A_(dev_alloc(&f->tLp, (int64_t) n + 1)); A_(dev_alloc(&f->tUp, (int64_t) n + 1));
    A_(dev_alloc(&f->tLi, unz)); A_(dev_alloc(&f->tLe, unz)); A_(dev_alloc(&f->tUi, lnz)); A_(dev_alloc(&f->tUe, lnz));
    A_(dev_alloc(&f->tpiv, n)); A_(dev_alloc(&cnt, 2 * (int64_t) n));
    if (!rc && !(f->tpinv = (int32_t *) malloc((size_t) n * 4))) rc = SLIP_HIP_OUT_OF_MEMORY;
    DOWN_(f->tpinv, P->pinv.p_, (size_t) n * 4);
    if (!rc) {
        SlipTViewArgs A = tview_args(f);
        A.cntL = cnt; A.cntU = cnt + n;
        HIP_(hipEventRecord(f->ev0, stream));
        HIP_(hipMemsetAsync(cnt, 0, (size_t) n * 8, stream));
        A_(tview_launch(A, 0, stream));
        /* (by hand: one workgroup of 1024 threads, and the emulated scan takes the tmp that is __shared__ on the device) */
#ifndef SLIP_EMULATE
        if (!rc) { hipLaunchKernelGGL(slip_tview_scan_kernel, dim3(1), dim3(1024), 0, stream, A); HIP_(hipGetLastError()); }
#else
        if (!rc) { uint64_t tmp[32]; emu::launch(1, 256, [A, &tmp]() { slip_tview_scan_body(A, tmp); }, 256 * 1024, 1); }
#endif
        HIP_(hipMemsetAsync(cnt, 0, (size_t) n * 8, stream));
        A_(tview_launch(A, 1, stream));
        A_(tview_sync(f, stream));
        HIP_(hipEventRecord(f->ev1, stream)); HIP_(hipStreamSynchronize(stream));
        float ms = 0;
        HIP_(hipEventElapsedTime(&ms, f->ev0, f->ev1));
        f->tview_ms = ms;
    }
    dev_free(cnt);
    if (rc) tview_drop(f);
    return rc;
}

/* the parameters of a transposed solve launch: the handle's, with the view's factors, pivot records and inverse cache and the
 * identity permutation (the view's rows are positions).  Shared with the handle: x and its rows (tags from the one ticket
 * counter), the scratch and bitmap, the job slots, the state.  Lo/Uo, Lready, the swap log and the package fields stay the
 * handle's: the ungated sweep and the back substitution never read them. */
static SlipParams tview_params(const slip_hip_factor *f)
{
    SlipParams P = f->P;
    P.Lp = f->tLp; P.Li = f->tLi; P.Le = f->tLe; P.Llimbs = f->P.Ulimbs; P.Lcap_nz = f->hs.Unz; P.Lcap_nl = f->P.Ucap_nl;
    P.Up = f->tUp; P.Ui = f->tUi; P.Ue = f->tUe; P.Ulimbs = f->P.Llimbs; P.Ucap_nz = f->hs.Lnz; P.Ucap_nl = f->P.Lcap_nl;
    P.piv.p_ = f->tpiv; P.invd.p_ = f->tinvd;
    P.pinv.p_ = f->ident; P.row_perm.p_ = f->ident;
    return P;
}

/* the substitution's output while it is still on the device: per entry (rhs c, position p) at c*n + p a signed digit count
 * and a limb offset into olimbs, where every right-hand side owns `ostride` limbs */
struct SlipSolveOut { int32_t *olen; int64_t *ooff; uint64_t *olimbs; int64_t ostride; };
static void solve_out_free(SlipSolveOut *o) { dev_free(o->olen); dev_free(o->ooff); dev_free(o->olimbs); memset(o, 0, sizeof *o); }

/* slip_hip_factor_solve (transpose 0), slip_hip_factor_solve_transpose (1) and slip_hip_factor_solve_double (either): the
 * launches and the grow-and-relaunch loop are one; the transposed solve runs on the view.  The output stays on the device. */
static int solve_device(slip_hip_factor *f, int transpose, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                        hipStream_t stream, SlipSolveOut *out)
{
    memset(out, 0, sizeof *out);
    if (!f || nrhs <= 0 || !blen || !blimbs) return SLIP_HIP_INCORRECT_INPUT;
    const int32_t n = f->n;
    if (f->broken) return SLIP_HIP_DEVICE_ERROR;
    if (f->hs.F != n) return SLIP_HIP_INCORRECT_INPUT;          /* needs the complete factorisation */
    if (!f->P.xd || !f->P.xrow) return SLIP_HIP_OUT_OF_MEMORY;
    SlipParams *P = &f->P;
    double *ms = transpose ? &f->tsolve_ms : &f->solve_ms;
    if (transpose) {
        f->tview_ms = 0;
        if (!f->tLp) TRY_(tview_build(f, stream));
    }
    const int64_t ne = (int64_t) n * nrhs;
    /* b: signed limb counts -> signed digit counts + offsets (zero high limbs trimmed) */
    SlipSlab bs;
    TRY_(slab_prepare(ne, blen, blimbs, INT64_MAX, &bs));
    const int64_t bl = bs.total;
    const int32_t maxdig = bs.maxdig > 1 ? bs.maxdig : 1;
    SlipSolveArgs A; memset(&A, 0, sizeof A);
    int32_t *dblen = NULL, *dolen = NULL, *ddone = NULL; int64_t *dboff = NULL, *dooff = NULL; uint64_t *dbl = NULL, *dol = NULL;
    int32_t *hdone = NULL;
    int rc = 0;
    /* x grows to about |b| * det: make room once (the kernel still reports GROW_X if this is short) */
    {
        int64_t want = 2 * ((int64_t) f->hs.c_maxdig + 2) + maxdig + 8;
        if (want > P->xcap) rc = grow_x_keep(f, want, n);
    }
    /* every right-hand side owns `ostride` limbs of the output slab */
    int64_t ostride = (int64_t) n * (((int64_t) f->hs.c_maxdig + maxdig) / 2 + 1) + 64;
    A_(dev_alloc(&dblen, ne)); A_(dev_alloc(&dboff, ne)); A_(dev_alloc(&dbl, bl > 0 ? bl : 1));
    A_(dev_alloc(&dolen, ne)); A_(dev_alloc(&dooff, ne)); A_(dev_alloc(&dol, ostride * nrhs)); A_(dev_alloc(&ddone, nrhs));
    hdone = (int32_t *) calloc((size_t) nrhs, 4);
    if (!hdone) rc = rc ? rc : SLIP_HIP_OUT_OF_MEMORY;
    UP_(dblen, bs.dig, (size_t) ne * 4); UP_(dboff, bs.off, (size_t) ne * 8); UP_(dbl, blimbs, (size_t) bl * 8);
    HIP_(hipMemset(ddone, 0, (size_t) nrhs * 4));
    if (!rc) {
        SlipState *h = &f->hs;
        *ms = 0;
        A.nrhs = nrhs; A.blen = dblen; A.boff = dboff; A.blimbs = dbl; A.olen = dolen; A.ooff = dooff; A.olimbs = dol;
        A.ocap = ostride * nrhs; A.ostride = ostride;
        for (int guard = 0; !rc && guard < 64; guard++) {
            int e;
            if (!transpose) e = launch_solve(f, f->P, A, ddone, stream, ms);
            else if (!(e = tview_sync(f, stream))) { SlipParams Pt = tview_params(f); e = launch_solve(f, Pt, A, ddone, stream, ms); }
            if (e) { rc = e; break; }
            DOWN_(hdone, ddone, (size_t) nrhs * 4);
            if (rc) break;
            int all = 1;
            for (int32_t c = 0; c < nrhs; c++) if (!hdone[c]) all = 0;
            if (all) break;
            const int status = h->stop == INT64_MAX ? SLIPDEV_INTERNAL : (int)(h->stop & 0xFF);
            if (status == SLIPDEV_GROW_X) rc = grow_x_keep(f, (int64_t) P->xcap * 2, n);
            else if (status == SLIPDEV_GROW_U) {
                /* the output regions: twice the stride; finished right-hand sides are simply solved again */
                dev_free(dol); dol = NULL;
                ostride *= 2;
                rc = dev_alloc(&dol, ostride * nrhs);
                HIP_(hipMemset(ddone, 0, (size_t) nrhs * 4));
                A.olimbs = dol; A.ocap = ostride * nrhs; A.ostride = ostride;
            } else {
                fprintf(stderr, "slip_hip: solve kernel stopped with internal status %d (stop %lld)\n", status, (long long) h->stop);
                rc = SLIP_HIP_DEVICE_ERROR;
            }
        }
    }
    slab_free(&bs); free(hdone);
    dev_free(dblen); dev_free(dboff); dev_free(dbl); dev_free(ddone);
    if (rc) { dev_free(dolen); dev_free(dooff); dev_free(dol); return rc; }
    out->olen = dolen; out->ooff = dooff; out->olimbs = dol; out->ostride = ostride;
    return SLIP_HIP_OK;
}

/* the numerators as the ABI returns them: the per-right-hand-side regions gathered into one dense slab; the transposed solve
 * gathers its output by row id, x[i] = y[pinv[i]] */
static int solve_core(slip_hip_factor *f, int transpose, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                      int32_t **xlen_out, uint64_t **xlimbs_out, int64_t *xnl_out, void *stream_v)
{
    if (!f || nrhs <= 0 || !blen || !blimbs || !xlen_out || !xlimbs_out || !xnl_out) return SLIP_HIP_INCORRECT_INPUT;
    *xlen_out = NULL; *xlimbs_out = NULL; *xnl_out = 0;
    SlipSolveOut o;
    TRY_(solve_device(f, transpose, nrhs, blen, blimbs, (hipStream_t) stream_v, &o));
    const int32_t n = f->n;
    const int64_t ne = (int64_t) n * nrhs, ostride = o.ostride;
    int32_t *xl = NULL; uint64_t *xlimbs = NULL, *raw = NULL; int64_t *hooff = NULL;
    int rc = 0;
    {
        /* gather the per-right-hand-side regions into the dense (rhs, position) slab of the ABI */
        xl = (int32_t *) malloc((size_t) ne * 4);
        hooff = (int64_t *) malloc((size_t) ne * 8);
        raw = (uint64_t *) malloc((size_t)(ostride * nrhs) * 8);
        if (!xl || !hooff || !raw) rc = SLIP_HIP_OUT_OF_MEMORY;
        DOWN_(xl, o.olen, (size_t) ne * 4); DOWN_(hooff, o.ooff, (size_t) ne * 8); DOWN_(raw, o.olimbs, (size_t)(ostride * nrhs) * 8);
        if (!rc) {
            int64_t nl = 0;
            for (int64_t t = 0; t < ne; t++) { const int32_t d = xl[t]; nl += ((d < 0 ? -d : d) + 1) >> 1; }
            xlimbs = (uint64_t *) malloc((size_t)(nl > 0 ? nl : 1) * 8);
            int32_t *ol = transpose ? (int32_t *) malloc((size_t) ne * 4) : xl;     /* the output's counts, in its order */
            if (!xlimbs || !ol) rc = SLIP_HIP_OUT_OF_MEMORY;
            else {
                int64_t at = 0;
                for (int64_t t = 0; t < ne; t++) {
                    const int64_t s = transpose ? t - t % n + f->tpinv[t % n] : t;       /* the region entry output t comes from */
                    const int32_t d = xl[s], l = ((d < 0 ? -d : d) + 1) >> 1;
                    if (l) memcpy(xlimbs + at, raw + hooff[s], (size_t) l * 8);
                    at += l;
                    ol[t] = d < 0 ? -l : l;
                }
                *xlen_out = ol; *xlimbs_out = xlimbs; *xnl_out = nl;
                if (!transpose) xl = NULL;
                ol = NULL; xlimbs = NULL;
            }
            if (transpose) free(ol);
        }
    }
    free(xl); free(xlimbs); free(raw); free(hooff);
    solve_out_free(&o);
    return rc;
}

extern "C" int slip_hip_factor_solve(slip_hip_factor *f, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                                     int32_t **xlen_out, uint64_t **xlimbs_out, int64_t *xnl_out, void *stream_v)
{
    return solve_core(f, 0, nrhs, blen, blimbs, xlen_out, xlimbs_out, xnl_out, stream_v);
}

extern "C" int slip_hip_factor_solve_transpose(slip_hip_factor *f, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                                               int32_t **xlen_out, uint64_t **xlimbs_out, int64_t *xnl_out, void *stream_v)
{
    return solve_core(f, 1, nrhs, blen, blimbs, xlen_out, xlimbs_out, xnl_out, stream_v);
}

extern "C" double slip_hip_factor_solve_ms(const slip_hip_factor *f) { return f ? f->solve_ms : 0.0; }

extern "C" double slip_hip_factor_solve_transpose_ms(const slip_hip_factor *f, double *view_ms)
{
    if (view_ms) *view_ms = f ? f->tview_ms : 0.0;
    return f ? f->tsolve_ms : 0.0;
}

/* ---- solutions as doubles (SLIP_solve_double's tail: SLIP_permute_x, SLIP_scale_x, SLIP_get_double_soln; kernels:
 * slip_todouble_kernel, slip_scale_kernel) ---- */

/* the operands of the three conversions (to_double_core, mpfr_core, reduce_core), all device arrays of signed digit counts, limb
 * offsets and limbs: numerators (entry c*n + p) and one denominator per right-hand side; dmaxdig: digits of the widest
 * denominator; oidx: where entry p of a right-hand side goes (n entries; NULL: to p); flip: the quotients' sign changes */
struct SlipQuot {
    const int32_t *xlen; const int64_t *xoff; const uint64_t *xlimbs;
    const int32_t *dlen; const int64_t *doff; const uint64_t *dlimbs; int32_t dmaxdig;
    const int32_t *oidx; int flip;
};
/* a kernel's argument record (SlipToDoubleArgs, SlipMpfrArgs, SlipReduceArgs), zeroed but for the operands they all begin with */
template <class Args> static Args quot_args(int32_t n, int32_t nrhs, const SlipQuot &q)
{
    Args A; memset(&A, 0, sizeof A);
    A.n = n; A.nrhs = nrhs; A.xlen = q.xlen; A.xoff = q.xoff; A.xlimbs = q.xlimbs; A.dlen = q.dlen; A.doff = q.doff; A.dlimbs = q.dlimbs;
    A.oidx = q.oidx; A.flip = q.flip;
    return A;
}

/* the operands of a handle-less conversion: the caller's two slabs on the device, with the host's digit counts and offsets */
struct SlipQuotUpload { SlipQuot q; SlipSlab xs, ds; };
static void quot_upload_free(SlipQuotUpload *u)
{
    dev_free((void *) u->q.xlen); dev_free((void *) u->q.xoff); dev_free((void *) u->q.xlimbs);
    dev_free((void *) u->q.dlen); dev_free((void *) u->q.doff); dev_free((void *) u->q.dlimbs);
    slab_free(&u->xs); slab_free(&u->ds);
    memset(u, 0, sizeof *u);
}
static int quot_upload(int32_t n, int32_t nrhs, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                       const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs, SlipQuotUpload *u)
{
    memset(u, 0, sizeof *u);
    const int64_t ne = (int64_t) n * nrhs;
    SlipSlab &xs = u->xs, &ds = u->ds;
    int rc = slab_prepare(ne, xlen, xlimbs, x_limbs, &xs);
    A_(slab_prepare(nrhs, dlen, dlimbs, d_limbs, &ds));
    for (int32_t c = 0; c < nrhs && !rc; c++) if (ds.dig[c] == 0) rc = SLIP_HIP_INCORRECT_INPUT;     /* x_c / 0 is no number */
    int32_t *dxl = NULL, *ddl = NULL; int64_t *dxo = NULL, *ddo = NULL; uint64_t *dxv = NULL, *ddv = NULL;
    A_(dev_alloc(&dxl, ne)); A_(dev_alloc(&dxo, ne)); A_(dev_alloc(&dxv, xs.total));
    A_(dev_alloc(&ddl, nrhs)); A_(dev_alloc(&ddo, nrhs)); A_(dev_alloc(&ddv, ds.total));
    UP_(dxl, xs.dig, (size_t) ne * 4); UP_(dxo, xs.off, (size_t) ne * 8); UP_(dxv, xlimbs, (size_t) xs.total * 8);
    UP_(ddl, ds.dig, (size_t) nrhs * 4); UP_(ddo, ds.off, (size_t) nrhs * 8); UP_(ddv, dlimbs, (size_t) ds.total * 8);
    u->q.xlen = dxl; u->q.xoff = dxo; u->q.xlimbs = dxv; u->q.dlen = ddl; u->q.doff = ddo; u->q.dlimbs = ddv; u->q.dmaxdig = ds.maxdig;
    if (rc) quot_upload_free(u);
    return rc;
}

/* one conversion on the device.  out (host) receives n * nrhs doubles and nothing else comes back. */
static int to_double_core(int32_t n, int32_t nrhs, const SlipQuot &q, double *out, hipStream_t stream, double *ms_out, int64_t *slow_out)
{
    const int64_t ne = (int64_t) n * nrhs, wcap = (int64_t) q.dmaxdig + 4;      /* the wave pass forms a product of dmaxdig + 3 digits */
    if (wcap > (1 << 28)) return SLIP_HIP_OUT_OF_MEMORY;
    const int64_t blocks = fit_scratch(service_blocks(ne), 4 + wcap);         /* a wave takes 64 entries per round */
    double *dout = NULL; dig_t *dscr = NULL; unsigned long long *dslow = NULL, hslow = 0;
    SlipTimed timed;
    int rc = 0;
    A_(dev_alloc(&dout, ne)); A_(dev_alloc(&dscr, blocks * SERVICE_WAVES * (4 + wcap))); A_(dev_alloc(&dslow, 1));
    HIP_(hipMemsetAsync(dslow, 0, 8, stream));
    if (!rc) {
        SlipToDoubleArgs A = quot_args<SlipToDoubleArgs>(n, nrhs, q);
        A.out = dout; A.scratch = dscr; A.wcap = (int32_t) wcap; A.nslow = dslow;
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(todouble, blocks, stream, A));
        A_(timed.end(stream, ms_out));
    }
    DOWN_(out, dout, (size_t) ne * 8); DOWN_(&hslow, dslow, 8);
    if (!rc && slow_out) *slow_out = (int64_t) hslow;
    dev_free(dout); dev_free(dscr); dev_free(dslow);
    return rc;
}

/* one launch of slip_scale_kernel: count entries times the multiplier (device, signed digit count slen) */
static int scale_launch(int64_t count, const int32_t *dlen, const int64_t *doff, const uint64_t *dlimbs, int32_t slen, const uint64_t *dsl,
                        int32_t *dolen, const int64_t *dooff, uint64_t *dolimbs, hipStream_t stream)
{
    SlipScaleArgs A; memset(&A, 0, sizeof A);
    A.count = count; A.len = dlen; A.off = doff; A.limbs = dlimbs; A.slen = slen; A.slimbs = dsl; A.olen = dolen; A.ooff = dooff; A.olimbs = dolimbs;
    TRY_(SERVICE_LAUNCH(scale, wave_blocks(count), stream, A));
    CK(hipStreamSynchronize(stream));
    return 0;
}

/* one part of a scale: NULL limbs mean 1; *dig = its signed digit count (0: the part is zero, which the callers refuse) */
static void scale_part(int32_t len, const uint64_t *limbs, int32_t *dig)
{
    if (!limbs) { *dig = 1; return; }
    const int32_t d = limb_digits(limbs, len < 0 ? -(int64_t) len : len);
    *dig = len < 0 ? -d : d;
}
static int scale_is_unit(int32_t dig, const uint64_t *limbs) { return !limbs || ((dig == 1 || dig == -1) && limbs[0] == 1); }

/* a solve left on the device with the scale applied, as the conversions take it (slip_hip_factor_solve_double, _solve_rational):
 * numerators xnum * |snum| by (rhs, position), one denominator det * |sden| for every right-hand side, the sign of the scale
 * apart (flip), and where position p goes: column q[p] (SLIP_permute_x); the transposed solve's position p is row i with
 * pinv[i] = p */
struct SlipScaledSol {
    SlipQuot q;
    SlipSolveOut o;                                                                /* owned: the substitution's output ...        */
    int32_t *own_dlen, *own_oidx, *dxlen2; int64_t *own_doff, *dxoff2; uint64_t *dprod, *dxl2;      /* ... and what the scale made */
};
static void scaled_free(SlipScaledSol *s)
{
    dev_free(s->own_dlen); dev_free(s->own_doff); dev_free(s->own_oidx); dev_free(s->dxlen2); dev_free(s->dxoff2); dev_free(s->dprod); dev_free(s->dxl2);
    solve_out_free(&s->o);
    memset(s, 0, sizeof *s);
}

static int solve_scaled(slip_hip_factor *f, int32_t transpose, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                        int32_t snlen, const uint64_t *snlimbs, int32_t sdlen, const uint64_t *sdlimbs, hipStream_t stream, SlipScaledSol *s)
{
    memset(s, 0, sizeof *s);
    if (!f || nrhs < 1 || !blen || !blimbs) return SLIP_HIP_INCORRECT_INPUT;
    int32_t sndig, sddig;
    scale_part(snlen, snlimbs, &sndig); scale_part(sdlen, sdlimbs, &sddig);
    if (sndig == 0 || sddig == 0) return SLIP_HIP_INCORRECT_INPUT;                  /* a zero scale part */
    if (!transpose && f->factors_only) return SLIP_HIP_INCORRECT_INPUT;             /* no q behind such a handle */
    TRY_(solve_device(f, transpose, nrhs, blen, blimbs, stream, &s->o));
    const SlipSolveOut &o = s->o;
    const int32_t n = f->n;
    const int64_t ne = (int64_t) n * nrhs;
    SlipParams *P = &f->P;
    s->q.flip = (sndig < 0) != (sddig < 0);
    const int32_t snabs = sndig < 0 ? -sndig : sndig, sdabs = sddig < 0 ? -sddig : sddig;
    int32_t *dplen = NULL; uint64_t *dsl = NULL;
    int32_t *hl = (int32_t *) malloc((size_t)(ne > nrhs ? ne : nrhs) * 4); int64_t *ho = (int64_t *) malloc((size_t)(ne > nrhs ? ne : nrhs) * 8);
    int rc = !hl || !ho ? SLIP_HIP_OUT_OF_MEMORY : 0;
    /* D = det = rho[n-1], read in place from the L slab through its pivot record (32 bytes; no limb of it is downloaded) */
    SlipPiv pr; memset(&pr, 0, sizeof pr);
    DOWN_(&pr, P->piv.p_ + (n - 1), sizeof pr);
    int32_t ddig = pr.len < 0 ? -pr.len : pr.len;
    if (!rc && (pr.len == 0 || pr.off < 0 || pr.off + ((ddig + 1) >> 1) > P->Lcap_nl)) rc = SLIP_HIP_DEVICE_ERROR;
    s->q.dlimbs = P->Llimbs; int64_t denoff = pr.off; int32_t denlen = pr.len;
    A_(dev_alloc(&s->own_dlen, nrhs)); A_(dev_alloc(&s->own_doff, nrhs));
    /* det * |sden|, once per call, on one wave */
    if (!rc && !scale_is_unit(sddig, sdlimbs)) {
        const int64_t zero = 0;
        A_(dev_alloc(&dsl, (sdabs + 1) >> 1)); A_(dev_alloc(&s->dprod, (ddig + sdabs + 1) / 2 + 1)); A_(dev_alloc(&dplen, 1));
        UP_(dsl, sdlimbs, (size_t)((sdabs + 1) >> 1) * 8);
        UP_(s->own_dlen, &pr.len, 4); UP_(s->own_doff, &pr.off, 8);                 /* the source record; rewritten below */
        int64_t *dzero = NULL;
        A_(dev_alloc(&dzero, 1)); UP_(dzero, &zero, 8);
        A_(scale_launch(1, s->own_dlen, s->own_doff, P->Llimbs, sdabs, dsl, dplen, dzero, s->dprod, stream));
        DOWN_(&denlen, dplen, 4);
        dev_free(dzero); dev_free(dsl); dsl = NULL;
        s->q.dlimbs = s->dprod; denoff = 0; ddig = denlen < 0 ? -denlen : denlen;
    }
    s->q.dmaxdig = ddig; s->q.dlen = s->own_dlen; s->q.doff = s->own_doff;
    if (!rc) for (int32_t c = 0; c < nrhs; c++) { hl[c] = denlen; ho[c] = denoff; }
    UP_(s->own_dlen, hl, (size_t) nrhs * 4); UP_(s->own_doff, ho, (size_t) nrhs * 8);
    /* xnum * |snum| per entry, only when |snum| != 1: the counts come down (4 bytes an entry) to lay the products out */
    s->q.xlen = o.olen; s->q.xoff = o.ooff; s->q.xlimbs = o.olimbs;
    if (!rc && !scale_is_unit(sndig, snlimbs)) {
        DOWN_(hl, o.olen, (size_t) ne * 4);
        int64_t total = 0;
        if (!rc) for (int64_t t = 0; t < ne; t++) { ho[t] = total; total += ((hl[t] < 0 ? -hl[t] : hl[t]) + snabs + 1) / 2 + 1; }
        A_(dev_alloc(&dsl, (snabs + 1) >> 1)); A_(dev_alloc(&s->dxlen2, ne)); A_(dev_alloc(&s->dxoff2, ne)); A_(dev_alloc(&s->dxl2, total));
        UP_(dsl, snlimbs, (size_t)((snabs + 1) >> 1) * 8); UP_(s->dxoff2, ho, (size_t) ne * 8);
        A_(scale_launch(ne, o.olen, o.ooff, o.olimbs, snabs, dsl, s->dxlen2, s->dxoff2, s->dxl2, stream));
        s->q.xlen = s->dxlen2; s->q.xoff = s->dxoff2; s->q.xlimbs = s->dxl2;
    }
    s->q.oidx = f->dq;
    if (!rc && transpose) {
        for (int32_t i = 0; i < n; i++) hl[f->tpinv[i]] = i;
        A_(dev_alloc(&s->own_oidx, n)); UP_(s->own_oidx, hl, (size_t) n * 4);
        s->q.oidx = s->own_oidx;
    }
    free(hl); free(ho);
    dev_free(dplen); dev_free(dsl);
    if (rc) scaled_free(s);
    return rc;
}

extern "C" int slip_hip_factor_solve_double(slip_hip_factor *f, int32_t transpose, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                                            int32_t snlen, const uint64_t *snlimbs, int32_t sdlen, const uint64_t *sdlimbs,
                                            double *x_out, void *stream_v)
{
    if (!x_out) return SLIP_HIP_INCORRECT_INPUT;
    hipStream_t stream = (hipStream_t) stream_v;
    SlipScaledSol s;
    TRY_(solve_scaled(f, transpose, nrhs, blen, blimbs, snlen, snlimbs, sdlen, sdlimbs, stream, &s));
    f->todouble_ms = 0; f->todouble_slow = 0;
    const int rc = to_double_core(f->n, nrhs, s.q, x_out, stream, &f->todouble_ms, &f->todouble_slow);
    scaled_free(&s);
    return rc;
}

extern "C" double slip_hip_factor_to_double_ms(const slip_hip_factor *f) { return f ? f->todouble_ms : 0.0; }
extern "C" int64_t slip_hip_factor_to_double_slow(const slip_hip_factor *f) { return f ? f->todouble_slow : 0; }

extern "C" int slip_hip_solution_to_double(int32_t n, int32_t nrhs, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                           const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs, double *out, void *stream_v)
{
    if (n <= 0 || nrhs < 1 || !xlen || !xlimbs || !dlen || !dlimbs || !out) return SLIP_HIP_INCORRECT_INPUT;
    TRY_(need_device());
    SlipQuotUpload u;
    int rc = quot_upload(n, nrhs, xlen, xlimbs, x_limbs, dlen, dlimbs, d_limbs, &u);
    A_(to_double_core(n, nrhs, u.q, out, (hipStream_t) stream_v, NULL, NULL));
    quot_upload_free(&u);
    return rc;
}

/* ---- solutions as multi-precision floats (SLIP_solve_mpfr's tail: SLIP_permute_x, SLIP_scale_x, SLIP_get_mpfr_soln; kernels:
 * slip_mpfr_kernel, slip_scale_kernel) ---- */

/* the counts of the last slip_hip_solution_to_mpfr of this thread (the handle-less entry has nowhere else to keep them) */
static thread_local int64_t slip_mpfr_paths_last[4];

/* what both entry points refuse before anything runs: 2 <= prec <= 65536, the five rounding modes, the three arrays */
static int mpfr_args_ok(int32_t prec, int32_t rnd, const int8_t *sign_out, const int64_t *exp_out, const uint64_t *mant_out)
{
    return prec >= 2 && prec <= 65536 && rnd >= 0 && rnd <= 4 && sign_out && exp_out && mant_out;
}

/* one conversion on the device: the operands as to_double_core takes them.  The host arrays receive n * nrhs signs, exponents
 * and ternary values (ternary_out may be NULL) and n * nrhs * ceil(prec / 64) limbs; nothing else comes back. */
static int mpfr_core(int32_t n, int32_t nrhs, const SlipQuot &q, int32_t prec, int32_t rnd,
                     int8_t *sign_out, int64_t *exp_out, uint64_t *mant_out, int8_t *ternary_out,
                     hipStream_t stream, double *ms_out, int64_t *paths_out)
{
    const int64_t ne = (int64_t) n * nrhs, nl = (prec + 63) >> 6, nq = (prec + 2 + 31) >> 5;
    const int64_t dcap = q.dmaxdig > 1 ? q.dmaxdig : 1;
    if (dcap > (1 << 28)) return SLIP_HIP_OUT_OF_MEMORY;
    /* the running remainder with the quotient digits' room above it, one product, the normalised divisor, the quotient */
    const int64_t stride = ((nq + dcap + 2) + (dcap + 2) + dcap + (nq + 1) + 1) & ~(int64_t) 1;
    const SlipWaveGrid g = wave_grid(ne, stride, 1024);
    int8_t *dsign = NULL, *dtern = NULL; int64_t *dexp = NULL; uint64_t *dmant = NULL;
    dig_t *dscr = NULL; unsigned long long *dpaths = NULL, hpaths[4] = {0, 0, 0, 0};
    SlipTimed timed;
    int rc = 0;
    A_(dev_alloc(&dsign, ne)); A_(dev_alloc(&dtern, ne)); A_(dev_alloc(&dexp, ne)); A_(dev_alloc(&dmant, ne * nl));
    A_(dev_alloc(&dscr, g.blocks * SERVICE_WAVES * stride)); A_(dev_alloc(&dpaths, 4));
    HIP_(hipMemsetAsync(dpaths, 0, 32, stream));
    if (!rc) {
        SlipMpfrArgs A = quot_args<SlipMpfrArgs>(n, nrhs, q);
        A.prec = prec; A.rnd = rnd; A.chunk = (int32_t) g.chunk;
        A.sign = dsign; A.exp = dexp; A.mant = dmant; A.ternary = dtern;
        A.scratch = dscr; A.dcap = (int32_t) dcap; A.stride = stride; A.paths = dpaths;
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(mpfr, g.blocks, stream, A));
        A_(timed.end(stream, ms_out));
    }
    DOWN_(sign_out, dsign, (size_t) ne); DOWN_(exp_out, dexp, (size_t) ne * 8); DOWN_(mant_out, dmant, (size_t)(ne * nl) * 8);
    if (ternary_out) DOWN_(ternary_out, dtern, (size_t) ne);
    DOWN_(hpaths, dpaths, 32);
    if (!rc && paths_out) for (int t = 0; t < 4; t++) paths_out[t] = (int64_t) hpaths[t];
    dev_free(dsign); dev_free(dtern); dev_free(dexp); dev_free(dmant); dev_free(dscr); dev_free(dpaths);
    return rc;
}

extern "C" int slip_hip_factor_solve_mpfr(slip_hip_factor *f, int32_t transpose, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                                          int32_t snlen, const uint64_t *snlimbs, int32_t sdlen, const uint64_t *sdlimbs,
                                          int32_t prec, int32_t rnd, int8_t *sign_out, int64_t *exp_out, uint64_t *mant_out,
                                          int8_t *ternary_out, void *stream_v)
{
    if (!mpfr_args_ok(prec, rnd, sign_out, exp_out, mant_out)) return SLIP_HIP_INCORRECT_INPUT;
    hipStream_t stream = (hipStream_t) stream_v;
    SlipScaledSol s;
    TRY_(solve_scaled(f, transpose, nrhs, blen, blimbs, snlen, snlimbs, sdlen, sdlimbs, stream, &s));
    f->tompfr_ms = 0; memset(f->tompfr_paths, 0, sizeof f->tompfr_paths);
    const int rc = mpfr_core(f->n, nrhs, s.q, prec, rnd, sign_out, exp_out, mant_out, ternary_out, stream, &f->tompfr_ms, f->tompfr_paths);
    scaled_free(&s);
    return rc;
}

extern "C" double slip_hip_factor_to_mpfr_ms(const slip_hip_factor *f) { return f ? f->tompfr_ms : 0.0; }
extern "C" int slip_hip_factor_to_mpfr_paths(const slip_hip_factor *f, int64_t out[4])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->tompfr_paths, sizeof f->tompfr_paths);
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_solution_to_mpfr(int32_t n, int32_t nrhs, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                         const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs, int32_t prec, int32_t rnd,
                                         int8_t *sign_out, int64_t *exp_out, uint64_t *mant_out, int8_t *ternary_out, void *stream_v)
{
    if (n <= 0 || nrhs < 1 || !xlen || !xlimbs || !dlen || !dlimbs) return SLIP_HIP_INCORRECT_INPUT;
    if (!mpfr_args_ok(prec, rnd, sign_out, exp_out, mant_out)) return SLIP_HIP_INCORRECT_INPUT;
    TRY_(need_device());
    SlipQuotUpload u;
    int rc = quot_upload(n, nrhs, xlen, xlimbs, x_limbs, dlen, dlimbs, d_limbs, &u);
    memset(slip_mpfr_paths_last, 0, sizeof slip_mpfr_paths_last);
    A_(mpfr_core(n, nrhs, u.q, prec, rnd, sign_out, exp_out, mant_out, ternary_out, (hipStream_t) stream_v, NULL, slip_mpfr_paths_last));
    quot_upload_free(&u);
    return rc;
}

/* the path counts of this thread's last slip_hip_solution_to_mpfr, as slip_hip_factor_to_mpfr_paths lays them out */
extern "C" int slip_hip_solution_to_mpfr_paths(int64_t out[4])
{
    if (!out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, slip_mpfr_paths_last, sizeof slip_mpfr_paths_last);
    return SLIP_HIP_OK;
}

/* ---- solutions as reduced fractions (SLIP_solve_mpq's tail: mpq_div, SLIP_permute_x, SLIP_scale_x, each canonicalising;
 * kernels: slip_reduce_kernel, slip_pack_kernel, slip_scale_kernel) ---- */

/* the counts of the last slip_hip_solution_to_rational of this thread (the handle-less entry has nowhere else to keep them) */
static thread_local int64_t slip_rational_paths_last[4];

/* one slab of the result: the digit counts come down, the compact layout goes up, slip_pack_kernel moves the limbs and the
 * compact slab is all that is downloaded.  dlen: signed digit counts by slot (device); on return len_out holds signed LIMB counts. */
static int pack_download(int64_t ne, const int32_t *dlen, const int64_t *dsoff, const uint64_t *dsrc, int min_one,
                         int32_t **len_out, uint64_t **limbs_out, int64_t *nl_out, hipStream_t stream, double *pack_ms = NULL)
{
    SlipTimed timed;
    int32_t *hl = (int32_t *) malloc((size_t) ne * 4); int64_t *ho = (int64_t *) malloc((size_t) ne * 8);
    int64_t *dcoff = NULL; uint64_t *dpacked = NULL, *out = NULL;
    int rc = !hl || !ho ? SLIP_HIP_OUT_OF_MEMORY : 0;
    DOWN_(hl, dlen, (size_t) ne * 4);
    int64_t total = 0;
    if (!rc) for (int64_t t = 0; t < ne; t++) {
        const int32_t l = ((hl[t] < 0 ? -hl[t] : hl[t]) + 1) >> 1;
        if (min_one && l < 1) rc = SLIP_HIP_DEVICE_ERROR;                           /* a denominator is never empty */
        ho[t] = total; total += l;
    }
    A_(dev_alloc(&dcoff, ne)); A_(dev_alloc(&dpacked, total));
    UP_(dcoff, ho, (size_t) ne * 8);
    if (!rc) {
        SlipPackArgs A; memset(&A, 0, sizeof A);
        A.count = ne; A.len = dlen; A.soff = dsoff; A.doff = dcoff; A.src = dsrc; A.dst = dpacked;
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(pack, wave_blocks(ne), stream, A));
        A_(timed.end(stream, pack_ms));
    }
    out = (uint64_t *) malloc((size_t)(total > 0 ? total : 1) * 8);
    if (!out) rc = rc ? rc : SLIP_HIP_OUT_OF_MEMORY;
    DOWN_(out, dpacked, (size_t) total * 8);
    if (!rc) {
        for (int64_t t = 0; t < ne; t++) { const int32_t l = ((hl[t] < 0 ? -hl[t] : hl[t]) + 1) >> 1; hl[t] = hl[t] < 0 ? -l : l; }
        *len_out = hl; *limbs_out = out; *nl_out = total;
        hl = NULL; out = NULL;
    }
    free(hl); free(ho); free(out);
    dev_free(dcoff); dev_free(dpacked);
    return rc;
}

/* one reduction on the device: the operands as to_double_core takes them; hxdig, hddig: their digit counts on the host (they size
 * every slot: a fraction in lowest terms is no longer than what it came from); hoidx: the host's copy of q.oidx (both NULL: to p).
 * The six outputs are compact malloc'ed slabs in slot order. */
static int reduce_core(int32_t n, int32_t nrhs, const SlipQuot &q, const int32_t *hxdig, const int32_t *hddig, const int32_t *hoidx,
                       int32_t **numlen_out, uint64_t **numlimbs_out, int64_t *num_limbs_out,
                       int32_t **denlen_out, uint64_t **denlimbs_out, int64_t *den_limbs_out,
                       hipStream_t stream, double *ms_out, int64_t *paths_out)
{
    const int64_t ne = (int64_t) n * nrhs;
    int32_t maxdig = 0;
    int64_t ntotal = 0, dtotal = 0;
    int64_t *hno = (int64_t *) malloc((size_t) ne * 8), *hdo = (int64_t *) malloc((size_t) ne * 8);
    if (!hno || !hdo) { free(hno); free(hdo); return SLIP_HIP_OUT_OF_MEMORY; }
    for (int32_t c = 0; c < nrhs; c++) {
        const int32_t dd = hddig[c] < 0 ? -hddig[c] : hddig[c];
        if (dd > maxdig) maxdig = dd;
        for (int32_t p = 0; p < n; p++) {
            const int64_t it = (int64_t) c * n + p, slot = (int64_t) c * n + (hoidx ? hoidx[p] : p);
            const int32_t xd = hxdig[it] < 0 ? -hxdig[it] : hxdig[it];
            if (xd > maxdig) maxdig = xd;
            hno[slot] = ntotal; ntotal += (xd + 1) >> 1;
            hdo[slot] = dtotal; dtotal += (dd + 1) >> 1;
        }
    }
    /* the memory class works on five buffers of the widest operand plus two digits; the register class shifts through 258 */
    const int64_t wcap = (((int64_t) maxdig + 2 > 264 ? (int64_t) maxdig + 2 : 264) + 1) & ~(int64_t) 1, per_wave = 8 + 5 * wcap;
    if (wcap > (1 << 28)) { free(hno); free(hdo); return SLIP_HIP_OUT_OF_MEMORY; }
    const SlipWaveGrid g = wave_grid(ne, per_wave, 1024);
    int32_t *dnl = NULL, *ddl = NULL; int64_t *dno = NULL, *ddo = NULL; uint64_t *dnv = NULL, *ddv = NULL;
    dig_t *dscr = NULL; unsigned long long *dpaths = NULL, hpaths[4] = {0, 0, 0, 0};
    SlipTimed timed;
    int rc = 0;
    A_(dev_alloc(&dnl, ne)); A_(dev_alloc(&ddl, ne)); A_(dev_alloc(&dno, ne)); A_(dev_alloc(&ddo, ne));
    A_(dev_alloc(&dnv, ntotal)); A_(dev_alloc(&ddv, dtotal));
    A_(dev_alloc(&dscr, g.blocks * SERVICE_WAVES * per_wave)); A_(dev_alloc(&dpaths, 4));
    UP_(dno, hno, (size_t) ne * 8); UP_(ddo, hdo, (size_t) ne * 8);
    HIP_(hipMemsetAsync(dpaths, 0, 32, stream));
    if (!rc) {
        SlipReduceArgs A = quot_args<SlipReduceArgs>(n, nrhs, q);
        A.chunk = (int32_t) g.chunk; A.numlen = dnl; A.denlen = ddl; A.numoff = dno; A.denoff = ddo;
        A.numlimbs = dnv; A.denlimbs = ddv; A.scratch = dscr; A.wcap = (int32_t) wcap; A.paths = dpaths;
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(reduce, g.blocks, stream, A));
        A_(timed.end(stream, ms_out));
    }
    DOWN_(hpaths, dpaths, 32);
    if (!rc && paths_out) for (int t = 0; t < 4; t++) paths_out[t] = (int64_t) hpaths[t];
    int32_t *nl = NULL, *dl = NULL; uint64_t *nv = NULL, *dv = NULL; int64_t nn = 0, dn = 0;
    A_(pack_download(ne, dnl, dno, dnv, 0, &nl, &nv, &nn, stream));
    A_(pack_download(ne, ddl, ddo, ddv, 1, &dl, &dv, &dn, stream));
    if (!rc) {
        *numlen_out = nl; *numlimbs_out = nv; *num_limbs_out = nn; *denlen_out = dl; *denlimbs_out = dv; *den_limbs_out = dn;
        nl = dl = NULL; nv = dv = NULL;
    }
    free(nl); free(dl); free(nv); free(dv); free(hno); free(hdo);
    dev_free(dnl); dev_free(ddl); dev_free(dno); dev_free(ddo); dev_free(dnv); dev_free(ddv); dev_free(dscr); dev_free(dpaths);
    return rc;
}

extern "C" int slip_hip_factor_solve_rational(slip_hip_factor *f, int32_t transpose, int32_t nrhs, const int32_t *blen, const uint64_t *blimbs,
                                              int32_t snlen, const uint64_t *snlimbs, int32_t sdlen, const uint64_t *sdlimbs,
                                              int32_t **numlen_out, uint64_t **numlimbs_out, int64_t *num_limbs_out,
                                              int32_t **denlen_out, uint64_t **denlimbs_out, int64_t *den_limbs_out, void *stream_v)
{
    if (!numlen_out || !numlimbs_out || !num_limbs_out || !denlen_out || !denlimbs_out || !den_limbs_out) return SLIP_HIP_INCORRECT_INPUT;
    *numlen_out = *denlen_out = NULL; *numlimbs_out = *denlimbs_out = NULL; *num_limbs_out = *den_limbs_out = 0;
    hipStream_t stream = (hipStream_t) stream_v;
    SlipScaledSol s;
    TRY_(solve_scaled(f, transpose, nrhs, blen, blimbs, snlen, snlimbs, sdlen, sdlimbs, stream, &s));
    const int32_t n = f->n;
    const int64_t ne = (int64_t) n * nrhs;
    /* the numerators' digit counts (4 bytes an entry) and q size the slots; no limb comes down before the result is packed */
    int32_t *hx = (int32_t *) malloc((size_t) ne * 4), *hd = (int32_t *) malloc((size_t) nrhs * 4), *hoidx = (int32_t *) malloc((size_t) n * 4);
    int rc = !hx || !hd || !hoidx ? SLIP_HIP_OUT_OF_MEMORY : 0;
    DOWN_(hx, s.q.xlen, (size_t) ne * 4); DOWN_(hoidx, s.q.oidx, (size_t) n * 4);
    if (!rc) for (int32_t c = 0; c < nrhs; c++) hd[c] = s.q.dmaxdig;
    f->torational_ms = 0; memset(f->torational_paths, 0, sizeof f->torational_paths);
    A_(reduce_core(n, nrhs, s.q, hx, hd, hoidx, numlen_out, numlimbs_out, num_limbs_out, denlen_out, denlimbs_out, den_limbs_out, stream,
                   &f->torational_ms, f->torational_paths));
    free(hx); free(hd); free(hoidx);
    scaled_free(&s);
    return rc;
}

extern "C" double slip_hip_factor_to_rational_ms(const slip_hip_factor *f) { return f ? f->torational_ms : 0.0; }
extern "C" int slip_hip_factor_to_rational_paths(const slip_hip_factor *f, int64_t out[4])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->torational_paths, sizeof f->torational_paths);
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_solution_to_rational(int32_t n, int32_t nrhs, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                             const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                                             int32_t **numlen_out, uint64_t **numlimbs_out, int64_t *num_limbs_out,
                                             int32_t **denlen_out, uint64_t **denlimbs_out, int64_t *den_limbs_out, void *stream_v)
{
    if (n <= 0 || nrhs < 1 || !xlen || !xlimbs || !dlen || !dlimbs) return SLIP_HIP_INCORRECT_INPUT;
    if (!numlen_out || !numlimbs_out || !num_limbs_out || !denlen_out || !denlimbs_out || !den_limbs_out) return SLIP_HIP_INCORRECT_INPUT;
    *numlen_out = *denlen_out = NULL; *numlimbs_out = *denlimbs_out = NULL; *num_limbs_out = *den_limbs_out = 0;
    TRY_(need_device());
    SlipQuotUpload u;
    int rc = quot_upload(n, nrhs, xlen, xlimbs, x_limbs, dlen, dlimbs, d_limbs, &u);
    memset(slip_rational_paths_last, 0, sizeof slip_rational_paths_last);
    A_(reduce_core(n, nrhs, u.q, u.xs.dig, u.ds.dig, NULL, numlen_out, numlimbs_out, num_limbs_out, denlen_out, denlimbs_out, den_limbs_out,
                   (hipStream_t) stream_v, NULL, slip_rational_paths_last));
    quot_upload_free(&u);
    return rc;
}

/* the path counts of this thread's last slip_hip_solution_to_rational, as slip_hip_factor_to_rational_paths lays them out */
extern "C" int slip_hip_solution_to_rational_paths(int64_t out[4])
{
    if (!out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, slip_rational_paths_last, sizeof slip_rational_paths_last);
    return SLIP_HIP_OK;
}

/* ---- exact solution check (SLIP_check_solution.c:31-113 as one integer test; kernel: slip_check_kernel) ---- */

/* the row-ordered view of an m x n CSC pattern (counting sort on the rows): rp[m+1]; per term its CSC entry and the index of
 * x it multiplies (xidx[j] for column j, or j itself when xidx is NULL) */
static int build_row_view(int32_t m, int32_t n, const int64_t *Ap, const int32_t *Ai, const int32_t *xidx, int64_t **rp_out, int64_t **re_out, int32_t **rx_out)
{
    const int64_t nz = Ap[n];
    int64_t *rp = (int64_t *) calloc((size_t) m + 1, 8), *re = (int64_t *) malloc((size_t)(nz > 0 ? nz : 1) * 8), *w = (int64_t *) malloc((size_t) m * 8);
    int32_t *rx = (int32_t *) malloc((size_t)(nz > 0 ? nz : 1) * 4);
    if (!rp || !re || !w || !rx) { free(rp); free(re); free(w); free(rx); return SLIP_HIP_OUT_OF_MEMORY; }
    for (int64_t e = 0; e < nz; e++) rp[Ai[e] + 1]++;
    for (int32_t i = 0; i < m; i++) rp[i + 1] += rp[i];
    memcpy(w, rp, (size_t) m * 8);
    for (int32_t j = 0; j < n; j++)
        for (int64_t e = Ap[j]; e < Ap[j + 1]; e++) { const int64_t t = w[Ai[e]]++; re[t] = e; rx[t] = xidx ? xidx[j] : j; }
    free(w);
    *rp_out = rp; *re_out = re; *rx_out = rx;
    return SLIP_HIP_OK;
}

/* one check on the device: A (device, digit counts) through its row view, b and x prepared on the host, d_c on the device.
 * Writes the verdicts, returns SLIP_HIP_OK / SLIP_HIP_INCORRECT or an error. */
static int check_core(int32_t n, int32_t nrhs, const int64_t *drp, const int64_t *dre, const int32_t *drx,
                      const int32_t *dalen, const int64_t *daoff, const uint64_t *dalimbs, int32_t amaxdig,
                      const SlipSlab &bs, const uint64_t *blimbs, const SlipSlab &xs, const uint64_t *xlimbs,
                      const int32_t *ddlen, const int64_t *ddoff, const uint64_t *ddlimbs, int32_t dmaxdig,
                      int32_t *first_bad_row, int64_t *bad_rows, hipStream_t stream, double *ms_out)
{
    const int64_t ne = (int64_t) n * nrhs;
    /* every (row, rhs) width is at most this (slip_check_kernel): the memory path's scratch is sized from it */
    const int64_t wcap = (amaxdig + xs.maxdig > dmaxdig + bs.maxdig ? amaxdig + xs.maxdig : dmaxdig + bs.maxdig) + 1;
    if (wcap > (1 << 28)) return SLIP_HIP_OUT_OF_MEMORY;
    const int64_t blocks = wcap > 256 ? fit_scratch(wave_blocks(ne), 2 * wcap) : wave_blocks(ne);      /* (only the memory path has scratch) */
    int32_t *dxl = NULL, *dbl = NULL, *dfirst = NULL, *dbad = NULL; int64_t *dxo = NULL, *dbo = NULL; uint64_t *dxv = NULL, *dbv = NULL; dig_t *dscr = NULL;
    int32_t *hfirst = (int32_t *) malloc((size_t) nrhs * 4), *hbad = (int32_t *) malloc((size_t) nrhs * 4);
    SlipTimed timed;
    int rc = (!hfirst || !hbad) ? SLIP_HIP_OUT_OF_MEMORY : 0;
    A_(dev_alloc(&dxl, ne)); A_(dev_alloc(&dxo, ne)); A_(dev_alloc(&dxv, xs.total)); A_(dev_alloc(&dbl, ne)); A_(dev_alloc(&dbo, ne)); A_(dev_alloc(&dbv, bs.total));
    A_(dev_alloc(&dfirst, nrhs)); A_(dev_alloc(&dbad, nrhs));
    if (wcap > 256) A_(dev_alloc(&dscr, blocks * SERVICE_WAVES * 2 * wcap));
    if (!rc) for (int32_t c = 0; c < nrhs; c++) { hfirst[c] = n; hbad[c] = 0; }
    UP_(dxl, xs.dig, (size_t) ne * 4); UP_(dxo, xs.off, (size_t) ne * 8); UP_(dxv, xlimbs, (size_t) xs.total * 8);
    UP_(dbl, bs.dig, (size_t) ne * 4); UP_(dbo, bs.off, (size_t) ne * 8); UP_(dbv, blimbs, (size_t) bs.total * 8);
    UP_(dfirst, hfirst, (size_t) nrhs * 4); UP_(dbad, hbad, (size_t) nrhs * 4);
    if (!rc) {
        SlipCheckArgs A; memset(&A, 0, sizeof A);
        A.n = n; A.nrhs = nrhs; A.rp = drp; A.re = dre; A.rx = drx;
        A.alen = dalen; A.aoff = daoff; A.alimbs = dalimbs;
        A.xlen = dxl; A.xoff = dxo; A.xlimbs = dxv; A.blen = dbl; A.boff = dbo; A.blimbs = dbv;
        A.dlen = ddlen; A.doff = ddoff; A.dlimbs = ddlimbs;
        A.first_bad = dfirst; A.nbad = dbad; A.scratch = dscr; A.wcap = (int32_t) wcap;
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(check, blocks, stream, A));
        A_(timed.end(stream, ms_out));
    }
    DOWN_(hfirst, dfirst, (size_t) nrhs * 4); DOWN_(hbad, dbad, (size_t) nrhs * 4);
    if (!rc) {
        int exact = 1;
        for (int32_t c = 0; c < nrhs; c++) {
            if (hbad[c]) exact = 0;
            if (first_bad_row) first_bad_row[c] = hbad[c] ? hfirst[c] : -1;
            if (bad_rows) bad_rows[c] = hbad[c];
        }
        rc = exact ? SLIP_HIP_OK : SLIP_HIP_INCORRECT;
    }
    dev_free(dxl); dev_free(dxo); dev_free(dxv); dev_free(dbl); dev_free(dbo); dev_free(dbv); dev_free(dfirst); dev_free(dbad); dev_free(dscr);
    free(hfirst); free(hbad);
    return rc;
}

/* the column view of the resident A in q order, for slip_hip_factor_check_transpose: "row" k of the check is column q[k] of A,
 * its terms the column's entries, each multiplying x at the entry's row id */
static int build_col_view(slip_hip_factor *f)
{
    const int32_t n = f->n;
    int64_t *hAp = (int64_t *) malloc(((size_t) n + 1) * 8), *rp = (int64_t *) malloc(((size_t) n + 1) * 8), *re = NULL;
    int32_t *hAi = (int32_t *) malloc((size_t)(f->annz > 0 ? f->annz : 1) * 4), *hq = (int32_t *) malloc((size_t) n * 4), *rx = NULL;
    int rc = !hAp || !rp || !hAi || !hq ? SLIP_HIP_OUT_OF_MEMORY : 0;
    DOWN_(hAp, f->dAp, ((size_t) n + 1) * 8); DOWN_(hAi, f->dAi, (size_t) f->annz * 4); DOWN_(hq, f->dq, (size_t) n * 4);
    const int64_t nz = rc ? 0 : hAp[n];
    if (!rc) {
        re = (int64_t *) malloc((size_t)(nz > 0 ? nz : 1) * 8); rx = (int32_t *) malloc((size_t)(nz > 0 ? nz : 1) * 4);
        if (!re || !rx) rc = SLIP_HIP_OUT_OF_MEMORY;
    }
    if (!rc) {
        int64_t t = 0;
        rp[0] = 0;
        for (int32_t k = 0; k < n; k++) {
            for (int64_t e = hAp[hq[k]]; e < hAp[hq[k] + 1]; e++) { re[t] = e; rx[t] = hAi[e]; t++; }
            rp[k + 1] = t;
        }
        if (dev_alloc(&f->chkt_rp, (int64_t) n + 1) || dev_alloc(&f->chkt_re, nz) || dev_alloc(&f->chkt_rx, nz)) rc = SLIP_HIP_OUT_OF_MEMORY;
        UP_(f->chkt_rp, rp, ((size_t) n + 1) * 8); UP_(f->chkt_re, re, (size_t) nz * 8); UP_(f->chkt_rx, rx, (size_t) nz * 4);
        if (rc) { dev_free(f->chkt_rp); dev_free(f->chkt_re); dev_free(f->chkt_rx); f->chkt_rp = NULL; f->chkt_re = NULL; f->chkt_rx = NULL; }
    }
    free(hAp); free(rp); free(re); free(hAi); free(hq); free(rx);
    return rc;
}

/* the row view of the resident A, once per handle: x is indexed by pivot position, column q[p] -> p */
static int build_pos_row_view(slip_hip_factor *f)
{
    const int32_t n = f->n;
    int64_t *hAp = (int64_t *) malloc(((size_t) n + 1) * 8), *rp = NULL, *re = NULL;
    int32_t *hAi = (int32_t *) malloc((size_t)(f->annz > 0 ? f->annz : 1) * 4), *hq = (int32_t *) malloc((size_t) n * 4), *qinv = (int32_t *) malloc((size_t) n * 4), *rx = NULL;
    int rc = !hAp || !hAi || !hq || !qinv ? SLIP_HIP_OUT_OF_MEMORY : 0;
    DOWN_(hAp, f->dAp, ((size_t) n + 1) * 8); DOWN_(hAi, f->dAi, (size_t) f->annz * 4); DOWN_(hq, f->dq, (size_t) n * 4);
    if (!rc) { for (int32_t p = 0; p < n; p++) qinv[hq[p]] = p; rc = build_row_view(n, n, hAp, hAi, qinv, &rp, &re, &rx); }
    if (!rc) {
        const int64_t nz = hAp[n];
        if (dev_alloc(&f->chk_rp, (int64_t) n + 1) || dev_alloc(&f->chk_re, nz) || dev_alloc(&f->chk_rx, nz)) rc = SLIP_HIP_OUT_OF_MEMORY;
        UP_(f->chk_rp, rp, ((size_t) n + 1) * 8); UP_(f->chk_re, re, (size_t) nz * 8); UP_(f->chk_rx, rx, (size_t) nz * 4);
        if (rc) { dev_free(f->chk_rp); dev_free(f->chk_re); dev_free(f->chk_rx); f->chk_rp = NULL; f->chk_re = NULL; f->chk_rx = NULL; }
    }
    free(hAp); free(hAi); free(hq); free(qinv); free(rp); free(re); free(rx);
    return rc;
}

/* d = det = rho[n-1] of a complete handle, read in place from the L slab through its pivot record: the records of nrhs
 * denominators (device; limbs: P.Llimbs), dmaxdig its digits */
static int det_records(slip_hip_factor *f, int32_t nrhs, int32_t **ddlen_out, int64_t **ddoff_out, int32_t *dmaxdig_out)
{
    SlipParams *P = &f->P;
    const int32_t n = f->n;
    int32_t *ddlen = NULL; int64_t *ddoff = NULL;
    int rc = 0;
    SlipPiv pr;
    DOWN_(&pr, P->piv.p_ + (n - 1), sizeof pr);
    if (!rc && (pr.len == 0 || pr.off < 0 || pr.off + (((pr.len < 0 ? -pr.len : pr.len) + 1) >> 1) > P->Lcap_nl)) rc = SLIP_HIP_DEVICE_ERROR;
    int32_t *hl = (int32_t *) malloc((size_t) nrhs * 4); int64_t *ho = (int64_t *) malloc((size_t) nrhs * 8);
    if (!rc && (!hl || !ho)) rc = SLIP_HIP_OUT_OF_MEMORY;
    if (!rc) {
        for (int32_t c = 0; c < nrhs; c++) { hl[c] = pr.len; ho[c] = pr.off; }
        *dmaxdig_out = pr.len < 0 ? -pr.len : pr.len;
        A_(dev_alloc(&ddlen, nrhs)); A_(dev_alloc(&ddoff, nrhs));
        UP_(ddlen, hl, (size_t) nrhs * 4); UP_(ddoff, ho, (size_t) nrhs * 8);
    }
    free(hl); free(ho);
    if (rc) { dev_free(ddlen); dev_free(ddoff); return rc; }
    *ddlen_out = ddlen; *ddoff_out = ddoff;
    return SLIP_HIP_OK;
}

/* slip_hip_factor_check (transpose 0: A(:,q) xnum == det b by row) and slip_hip_factor_check_transpose (1: A(:,q)^T xnum ==
 * det b by position): the same kernel over the row view or the column view of the resident A */
static int check_on_handle(slip_hip_factor *f, int transpose, int32_t nrhs,
                           const int32_t *blen, const uint64_t *blimbs, int64_t b_limbs,
                           const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                           int32_t *first_bad, int64_t *bad, void *stream_v)
{
    if (!f || f->factors_only || nrhs < 1 || !blen || !blimbs || !xlen || !xlimbs) return SLIP_HIP_INCORRECT_INPUT;
    const int32_t n = f->n;
    if (f->broken) return SLIP_HIP_DEVICE_ERROR;
    if (f->hs.F != n || f->last_status == SLIP_HIP_DEVICE_ERROR) return SLIP_HIP_INCORRECT_INPUT;   /* needs the complete factorisation */
    const int64_t ne = (int64_t) n * nrhs;
    SlipSlab bs, xs;
    int rc = slab_prepare(ne, blen, blimbs, b_limbs, &bs);
    if (!rc) rc = slab_prepare(ne, xlen, xlimbs, x_limbs, &xs);
    else memset(&xs, 0, sizeof xs);
    SlipParams *P = &f->P;
    if (!rc && transpose && !f->chkt_rp) rc = build_col_view(f);
    if (!rc && !transpose && !f->chk_rp) rc = build_pos_row_view(f);
    int32_t *ddlen = NULL; int64_t *ddoff = NULL; int32_t dmaxdig = 0;
    A_(det_records(f, nrhs, &ddlen, &ddoff, &dmaxdig));
    if (!rc && !transpose) {
        f->check_ms = 0;
        rc = check_core(n, nrhs, f->chk_rp, f->chk_re, f->chk_rx, f->dAlen, f->dAoff, f->dAlimbs, f->amaxdig,
                        bs, blimbs, xs, xlimbs, ddlen, ddoff, P->Llimbs, dmaxdig, first_bad, bad, (hipStream_t) stream_v, &f->check_ms);
    } else if (!rc)
        rc = check_core(n, nrhs, f->chkt_rp, f->chkt_re, f->chkt_rx, f->dAlen, f->dAoff, f->dAlimbs, f->amaxdig,
                        bs, blimbs, xs, xlimbs, ddlen, ddoff, P->Llimbs, dmaxdig, first_bad, bad, (hipStream_t) stream_v, NULL);
    dev_free(ddlen); dev_free(ddoff);
    slab_free(&bs); slab_free(&xs);
    return rc;
}

extern "C" int slip_hip_factor_check(slip_hip_factor *f, int32_t nrhs,
                                     const int32_t *blen, const uint64_t *blimbs, int64_t b_limbs,
                                     const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                     int32_t *first_bad_row, int64_t *bad_rows, void *stream_v)
{
    return check_on_handle(f, 0, nrhs, blen, blimbs, b_limbs, xlen, xlimbs, x_limbs, first_bad_row, bad_rows, stream_v);
}

extern "C" int slip_hip_factor_check_transpose(slip_hip_factor *f, int32_t nrhs,
                                               const int32_t *blen, const uint64_t *blimbs, int64_t b_limbs,
                                               const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                               int32_t *first_bad_pos, int64_t *bad_pos, void *stream_v)
{
    return check_on_handle(f, 1, nrhs, blen, blimbs, b_limbs, xlen, xlimbs, x_limbs, first_bad_pos, bad_pos, stream_v);
}

extern "C" double slip_hip_factor_check_ms(const slip_hip_factor *f) { return f ? f->check_ms : 0.0; }

extern "C" int slip_hip_check_solution(int32_t n, const int64_t *Ap, const int32_t *Ai, const int32_t *Alen, const uint64_t *Alimbs,
                                       int32_t nrhs, const int32_t *blen, const uint64_t *blimbs, int64_t b_limbs,
                                       const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                       const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                                       int32_t *first_bad_row, int64_t *bad_rows, void *stream_v)
{
    if (n <= 0 || !Ap || !Ai || !Alen || !Alimbs || nrhs < 1 || !blen || !blimbs || !xlen || !xlimbs || !dlen || !dlimbs) return SLIP_HIP_INCORRECT_INPUT;
    TRY_(need_device());
    const int64_t ne = (int64_t) n * nrhs;
    SlipSlab bs, xs, ds;
    memset(&xs, 0, sizeof xs); memset(&ds, 0, sizeof ds);
    int rc = slab_prepare(ne, blen, blimbs, b_limbs, &bs);
    if (!rc) rc = slab_prepare(ne, xlen, xlimbs, x_limbs, &xs);
    if (!rc) rc = slab_prepare(nrhs, dlen, dlimbs, d_limbs, &ds);
    for (int32_t c = 0; c < nrhs && !rc; c++) if (ds.dig[c] == 0) rc = SLIP_HIP_INCORRECT_INPUT;     /* x_c / 0 is no solution */
    SlipHostA ha; memset(&ha, 0, sizeof ha);
    if (!rc) rc = prepare_A(n, n, Ap, Ai, Alen, Alimbs, &ha);
    int64_t *rp = NULL, *re = NULL; int32_t *rx = NULL;
    if (!rc) rc = build_row_view(n, n, ha.Ap, ha.Ai, NULL, &rp, &re, &rx);
    int64_t *drp = NULL, *dre = NULL, *daoff = NULL, *ddoff = NULL; int32_t *drx = NULL, *dalen = NULL, *ddlen = NULL; uint64_t *dal = NULL, *ddl = NULL;
    const int64_t nz = ha.nnz;
    A_(dev_alloc(&drp, (int64_t) n + 1)); A_(dev_alloc(&dre, nz)); A_(dev_alloc(&drx, nz));
    A_(dev_alloc(&dalen, nz)); A_(dev_alloc(&daoff, nz)); A_(dev_alloc(&dal, ha.nl));
    A_(dev_alloc(&ddlen, nrhs)); A_(dev_alloc(&ddoff, nrhs)); A_(dev_alloc(&ddl, ds.total));
    UP_(drp, rp, ((size_t) n + 1) * 8); UP_(dre, re, (size_t) nz * 8); UP_(drx, rx, (size_t) nz * 4);
    UP_(dalen, ha.Alen, (size_t) nz * 4); UP_(daoff, ha.Aoff, (size_t) nz * 8); UP_(dal, ha.Alimbs, (size_t) ha.nl * 8);
    UP_(ddlen, ds.dig, (size_t) nrhs * 4); UP_(ddoff, ds.off, (size_t) nrhs * 8); UP_(ddl, dlimbs, (size_t) ds.total * 8);
    if (!rc) rc = check_core(n, nrhs, drp, dre, drx, dalen, daoff, dal, ha.maxdig, bs, blimbs, xs, xlimbs, ddlen, ddoff, ddl, ds.maxdig,
                             first_bad_row, bad_rows, (hipStream_t) stream_v, NULL);
    dev_free(drp); dev_free(dre); dev_free(drx); dev_free(dalen); dev_free(daoff); dev_free(dal); dev_free(ddlen); dev_free(ddoff); dev_free(ddl);
    free(rp); free(re); free(rx);
    host_a_free(&ha);
    slab_free(&bs); slab_free(&xs); slab_free(&ds);
    return rc;
}

/* ---- exact sparse products r_c = op(A) x_c - d_c b_c returned (no counterpart in the reference; kernel: slip_product_kernel,
 * DESIGN 3i) ---- */

/* device ms of this thread's last product by pass: the widths, the offset scans, the products, the packing */
static thread_local double slip_product_passes_last[4];

/* a view of a resident matrix: nout output rows, nx entries in a vector of x */
struct SlipProductView {
    int32_t nout, nx; const int64_t *rp, *re; const int32_t *rx;
    const int32_t *alen; const int64_t *aoff; const uint64_t *alimbs; int32_t amaxdig;
};

/* the limbs one group of vectors may stage (fit_scratch's 256 MiB; SLIP_HIP_PRODUCT_STAGE_KB overrides it: tests of the grouping) */
static int64_t product_stage_limbs(void)
{
    const char *e = getenv("SLIP_HIP_PRODUCT_STAGE_KB");
    const long long kb = e ? atoll(e) : 0;
    return kb > 0 ? (int64_t) kb * 128 : ((int64_t) 256 << 20) / 8;
}

/* The staged form of a service: nprob problems of n items each, whose widths dw (device; digits, none above the even wcap >= 2)
 * a first pass has written, formed group by group into a staging slab no larger than product_stage_limbs() -- whole multiples
 * of `gran` problems, at least gran (the bound groups, it never refuses).  Per group of the problems c0 .. c0 + nv: the items'
 * staging offsets into dso (an offset scan), the slab, form(c0, nv, cnt, dstage) launching the passes that fill it (cnt = n * nv
 * items), sink(c0, nv, dstage) for what becomes of it; both return a status.  The device ms of the scans and of the forms are
 * added to *scan_ms and *form_ms (which may be one figure). */
template <class Form, class Sink>
static int staged_run(int64_t n, int64_t nprob, int64_t gran, int64_t wcap, const int32_t *dw, int64_t *dso, Form form, Sink sink,
                      hipStream_t stream, double *scan_ms, double *form_ms)
{
    int64_t group = product_stage_limbs() / (n * (wcap / 2)) / gran * gran;
    if (group < gran) group = gran;
    if (group > nprob) group = nprob;
    const int64_t sblocks = offscan_blocks(n * group);
    unsigned long long *bsum = NULL;
    int rc = dev_alloc(&bsum, sblocks);
    for (int64_t c0 = 0; c0 < nprob && !rc; c0 += group) {
        const int64_t nv = c0 + group <= nprob ? group : nprob - c0, cnt = n * nv;
        uint64_t *dstage = NULL; int64_t total = 0;
        double t = 0;
        {                                                  /* the staging offsets from the widths */
            SlipTimed timed;
            A_(timed.begin(stream));
            A_(offscan_run(cnt, dw + c0 * n, dso + c0 * n, bsum, sblocks, stream));
            A_(timed.end(stream, &t));
            *scan_ms += t;
        }
        A_(offscan_total(bsum, sblocks, &total, stream));
        if (!rc && total > cnt * (wcap / 2)) rc = SLIP_HIP_DEVICE_ERROR;           /* (the widths' bound: the host's own figure) */
        A_(dev_alloc(&dstage, total));
        if (!rc) {                                         /* the passes into the staging slab */
            SlipTimed timed;
            A_(timed.begin(stream));
            A_(form(c0, nv, cnt, dstage));
            A_(timed.end(stream, &t));
            *form_ms += t;
        }
        A_(sink(c0, nv, (const uint64_t *) dstage));
        dev_free(dstage);
    }
    dev_free(bsum);
    return rc;
}

/* the cnt staged records of a group packed and downloaded (pack_download) and appended to a result: their signed limb counts
 * to ol, their limbs behind the *on that *out holds (a first group's block is taken over as it stands) */
static int pack_append(int64_t cnt, const int32_t *drl, const int64_t *dso, const uint64_t *dstage, int32_t *ol, uint64_t **out, int64_t *on,
                       hipStream_t stream, double *pack_ms = NULL)
{
    int32_t *gl = NULL; uint64_t *gv = NULL; int64_t gn = 0;
    int rc = pack_download(cnt, drl, dso, dstage, 0, &gl, &gv, &gn, stream, pack_ms);
    if (!rc && !*out) { *out = gv; *on = gn; gv = NULL; }
    else if (!rc) {
        uint64_t *grown = (uint64_t *) realloc(*out, (size_t)(*on + gn > 0 ? *on + gn : 1) * 8);
        if (!grown) rc = SLIP_HIP_OUT_OF_MEMORY;
        else { *out = grown; memcpy(grown + *on, gv, (size_t) gn * 8); *on += gn; }
    }
    if (!rc) memcpy(ol, gl, (size_t) cnt * 4);
    free(gl); free(gv);
    return rc;
}

/* the winners' records of a group of nv problems appended to wl / wv (signed limb counts, limbs): record c of the first stream
 * (device: dl1, do1 into lim1), then, with lim2, record c of the second, problem by problem */
static int winners_collect(int64_t nv, const int32_t *dl1, const int64_t *do1, const uint64_t *lim1,
                           const int32_t *dl2, const int64_t *do2, const uint64_t *lim2,
                           std::vector<int32_t> *wl, std::vector<uint64_t> *wv, hipStream_t stream)
{
    int32_t *l1 = NULL, *l2 = NULL; uint64_t *v1 = NULL, *v2 = NULL; int64_t n1 = 0, n2 = 0;
    int rc = pack_download(nv, dl1, do1, lim1, 0, &l1, &v1, &n1, stream);
    if (lim2) A_(pack_download(nv, dl2, do2, lim2, 0, &l2, &v2, &n2, stream));
    if (!rc) {
        int64_t o1 = 0, o2 = 0;
        for (int64_t c = 0; c < nv; c++) {
            const int64_t a1 = l1[c] < 0 ? -l1[c] : l1[c];
            wl->push_back(l1[c]); wv->insert(wv->end(), v1 + o1, v1 + o1 + a1); o1 += a1;
            if (lim2) {
                const int64_t a2 = l2[c] < 0 ? -l2[c] : l2[c];
                wl->push_back(l2[c]); wv->insert(wv->end(), v2 + o2, v2 + o2 + a2); o2 += a2;
            }
        }
    }
    free(l1); free(l2); free(v1); free(v2);
    return rc;
}

/* the winners' records collected by winners_collect as the caller's malloc'ed slab */
static int winners_out(const std::vector<int32_t> &wl, const std::vector<uint64_t> &wv, int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out)
{
    int32_t *ol = (int32_t *) malloc((wl.size() > 0 ? wl.size() : 1) * 4); uint64_t *ov = (uint64_t *) malloc((wv.size() > 0 ? wv.size() : 1) * 8);
    if (!ol || !ov) { free(ol); free(ov); return SLIP_HIP_OUT_OF_MEMORY; }
    if (!wl.empty()) memcpy(ol, wl.data(), wl.size() * 4);
    if (!wv.empty()) memcpy(ov, wv.data(), wv.size() * 8);
    *wlen_out = ol; *wlimbs_out = ov; *wnl_out = (int64_t) wv.size();
    return SLIP_HIP_OK;
}

/* the four results of a selection, nprob each and one after the other in res, into the caller's four arrays */
static void results_out(const int32_t *res, int32_t nprob, int32_t *r0, int32_t *r1, int32_t *r2, int32_t *r3)
{
    memcpy(r0, res, (size_t) nprob * 4); memcpy(r1, res + nprob, (size_t) nprob * 4);
    memcpy(r2, res + 2 * (size_t) nprob, (size_t) nprob * 4); memcpy(r3, res + 3 * (size_t) nprob, (size_t) nprob * 4);
}

/* the winners' three outputs come all or none */
static int winners_args_bad(int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out)
{
    return (wlen_out || wlimbs_out || wnl_out) && (!wlen_out || !wlimbs_out || !wnl_out);
}

/* position p of a transposed solve is row i, pinv[i] = p: the map from a position to the index reported (*doidx) and, with
 * dpos, its inverse, on the device; both stay NULL for a plain solve */
static int transposed_maps(const slip_hip_factor *f, int transpose, int32_t **doidx, int32_t **dpos)
{
    const int32_t n = f->n;
    if (!transpose) return SLIP_HIP_OK;
    int32_t *hidx = (int32_t *) malloc((size_t) n * 4);
    int rc = !hidx ? SLIP_HIP_OUT_OF_MEMORY : 0;
    if (!rc) for (int32_t i = 0; i < n; i++) hidx[f->tpinv[i]] = i;
    A_(dev_alloc(doidx, n)); UP_(*doidx, hidx, (size_t) n * 4);
    if (dpos) { A_(dev_alloc(dpos, n)); UP_(*dpos, f->tpinv, (size_t) n * 4); }
    free(hidx);
    return rc;
}

/* the sign of det = rho[n-1] of a complete handle from its pivot record: *dneg */
static int det_negative(const slip_hip_factor *f, int *dneg)
{
    int rc = 0;
    SlipPiv pr; memset(&pr, 0, sizeof pr);
    DOWN_(&pr, f->P.piv.p_ + (f->n - 1), sizeof pr);
    if (!rc && pr.len == 0) rc = SLIP_HIP_DEVICE_ERROR;
    *dneg = pr.len < 0;
    return rc;
}

/* one product on operands that are on the device already; d_c as device records (with b).  xmaxdig: the digits of the widest
 * entry of x, or negative when only the device knows the lengths (a substitution's output): the widest item is then reduced
 * from the widths the width pass wrote (slip_price_kernel) and four bytes are read back.  The result stays on the device:
 * vectors are staged in groups of whole multiples of `gran` (at least gran: the bound groups, it never refuses) and
 * sink(c0, nv, rlen, soff, stage, &t) is handed every group -- vectors c0 .. c0 + nv, the signed digit counts and staging
 * offsets of their nout * nv items, the staging slab; its t is added to ms[3].  ms: device ms by pass (the widths, the offset
 * scans, the products, the sink's). */
template <class Sink>
static int product_device(const SlipProductView &V, int32_t nvec, const SlipDevRecs &x, int32_t xmaxdig,
                          const SlipDevRecs *b, int32_t bmaxdig, const int32_t *ddlen, const int64_t *ddoff, const uint64_t *ddlimbs, int32_t dmaxdig,
                          int64_t gran, Sink sink, hipStream_t stream, double ms[4])
{
    const int64_t nout = V.nout, ne = nout * nvec;
    /* every width is at most wtop (slip_product_kernel), wcap in whole limbs: the staging of a group and the memory path's scratch
     * are sized from it */
    int64_t wtop = (b && dmaxdig + bmaxdig > V.amaxdig + xmaxdig ? dmaxdig + bmaxdig : V.amaxdig + xmaxdig) + 1;
    if (xmaxdig >= 0 && ((wtop + 1) & ~(int64_t) 1) > (1 << 28)) return SLIP_HIP_OUT_OF_MEMORY;
    int32_t *dw = NULL, *drl = NULL, *dwmax = NULL; int64_t *dso = NULL;
    dig_t *dscr = NULL;
    int rc = 0;
    A_(dev_alloc(&dw, ne)); A_(dev_alloc(&dso, ne)); A_(dev_alloc(&drl, ne));
    if (xmaxdig < 0) A_(dev_alloc(&dwmax, 1));
    SlipProductArgs A; memset(&A, 0, sizeof A);
    A.nout = V.nout; A.nx = V.nx; A.rp = V.rp; A.re = V.re; A.rx = V.rx; A.alen = V.alen; A.aoff = V.aoff; A.alimbs = V.alimbs;
    A.xlimbs = x.limbs; A.blimbs = b ? b->limbs : NULL; A.dlimbs = ddlimbs;
    /* the vectors c0 .. c0 + nv of the operands */
    auto slice = [&](int64_t c0, int64_t nv, int phase) {
        A.nvec = (int32_t) nv; A.phase = phase;
        A.xlen = x.len + c0 * V.nx; A.xoff = x.off + c0 * V.nx;
        A.blen = b ? b->len + c0 * nout : NULL; A.boff = b ? b->off + c0 * nout : NULL;
        A.dlen = b ? ddlen + c0 : NULL; A.doff = b ? ddoff + c0 : NULL;
        A.wlen = dw + c0 * nout; A.soff = dso + c0 * nout; A.rlen = drl + c0 * nout;
    };
    if (!rc) {                                             /* pass 1: the widths of all items (and the widest of them) */
        SlipTimed timed;
        slice(0, nvec, 0);
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(product, wave_blocks(ne), stream, A));
        if (xmaxdig < 0) {
            SlipPriceArgs R; memset(&R, 0, sizeof R);
            R.phase = 1; R.count = ne; R.w = dw; R.wmax = dwmax;
            HIP_(hipMemsetAsync(dwmax, 0, 4, stream));
            A_(SERVICE_LAUNCH(price, service_blocks(ne), stream, R));
        }
        A_(timed.end(stream, &ms[0]));
    }
    if (xmaxdig < 0) {
        int32_t hwmax = 0;
        DOWN_(&hwmax, dwmax, 4);
        wtop = hwmax;
    }
    const int64_t wcap = (wtop + 1) & ~(int64_t) 1;
    if (!rc && (wcap > (1 << 28) || wcap < 2)) rc = wcap < 2 ? SLIP_HIP_DEVICE_ERROR : SLIP_HIP_OUT_OF_MEMORY;
    const int64_t blocks = wtop > 256 ? fit_scratch(wave_blocks(ne), wcap) : wave_blocks(ne);
    if (wtop > 256) A_(dev_alloc(&dscr, blocks * SERVICE_WAVES * wcap));
    A.scratch = dscr; A.wcap = (int32_t) wcap;
    /* pass 2, the staging offsets, is staged_run's; pass 3: the products of a group into the staging slab */
    auto form = [&](int64_t c0, int64_t nv, int64_t, uint64_t *dstage) {
        slice(c0, nv, 1);
        A.stage = dstage;
        return SERVICE_LAUNCH(product, blocks, stream, A);
    };
    auto staged = [&](int64_t c0, int64_t nv, const uint64_t *dstage) {
        double t = 0;
        const int rc = sink(c0, nv, (const int32_t *) drl + c0 * nout, (const int64_t *) dso + c0 * nout, dstage, &t);
        if (!rc) ms[3] += t;
        return rc;
    };
    A_(staged_run(nout, nvec, gran, wcap, dw, dso, form, staged, stream, &ms[1], &ms[2]));
    dev_free(dw); dev_free(dso); dev_free(drl); dev_free(dwmax); dev_free(dscr);
    return rc;
}

/* one product on the device: x (and b, with bs != NULL) prepared on the host; d_c as device records into ddlimbs (with b).
 * The result is one compact malloc'ed slab of V.nout * nvec entries, signed limb counts. */
static int product_core(const SlipProductView &V, int32_t nvec, const SlipSlab &xs, const uint64_t *xlimbs,
                        const SlipSlab *bs, const uint64_t *blimbs,
                        const int32_t *ddlen, const int64_t *ddoff, const uint64_t *ddlimbs, int32_t dmaxdig,
                        int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out, hipStream_t stream, double *ms_out)
{
    const int64_t nout = V.nout, ne = nout * nvec, nxe = (int64_t) V.nx * nvec;
    SlipDevSlab dx, db; memset(&dx, 0, sizeof dx); memset(&db, 0, sizeof db);
    int32_t *rl = (int32_t *) malloc((size_t) ne * 4); uint64_t *rv = NULL; int64_t rn = 0;
    double ms[4] = {0, 0, 0, 0};
    int rc = !rl ? SLIP_HIP_OUT_OF_MEMORY : 0;
    A_(dev_slab_put(nxe, xs, xlimbs, &dx));
    if (bs) A_(dev_slab_put(ne, *bs, blimbs, &db));
    const SlipDevRecs x = dev_slab_recs(dx), b = dev_slab_recs(db);
    /* a group packed, downloaded and appended to the result */
    auto sink = [&](int64_t c0, int64_t nv, const int32_t *drl, const int64_t *dso, const uint64_t *dstage, double *t) {
        return pack_append(nout * nv, drl, dso, dstage, rl + c0 * nout, &rv, &rn, stream, t);
    };
    A_(product_device(V, nvec, x, xs.maxdig, bs ? &b : NULL, bs ? bs->maxdig : 0, ddlen, ddoff, ddlimbs, dmaxdig, 1, sink, stream, ms));
    dev_slab_free(&dx); dev_slab_free(&db);
    if (rc) { free(rl); free(rv); return rc; }
    memcpy(slip_product_passes_last, ms, sizeof ms);
    if (ms_out) *ms_out = ms[0] + ms[1] + ms[2] + ms[3];
    *rlen_out = rl; *rlimbs_out = rv; *rnl_out = rn;
    return SLIP_HIP_OK;
}

/* the operands of one product checked and brought to the device, then product_core.  f != NULL: a handle whose det stands in
 * for a missing d (the caller has seen to it that the factorisation is complete). */
static int product_entry(const SlipProductView &V, slip_hip_factor *f, int32_t nvec,
                         const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                         const int32_t *blen, const uint64_t *blimbs, int64_t b_limbs,
                         const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                         int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out, hipStream_t stream, double *ms_out)
{
    SlipSlab xs, bs, ds;
    memset(&bs, 0, sizeof bs); memset(&ds, 0, sizeof ds);
    int rc = slab_prepare((int64_t) V.nx * nvec, xlen, xlimbs, x_limbs, &xs);
    if (!rc && blen) rc = slab_prepare((int64_t) V.nout * nvec, blen, blimbs, b_limbs, &bs);
    if (!rc && dlen) rc = slab_prepare(nvec, dlen, dlimbs, d_limbs, &ds);
    for (int32_t c = 0; c < nvec && !rc && dlen; c++) if (ds.dig[c] == 0) rc = SLIP_HIP_INCORRECT_INPUT;
    SlipDevSlab dd; memset(&dd, 0, sizeof dd);            /* (from det: records alone, into the L slab) */
    const uint64_t *ddlimbs = NULL; int32_t dmaxdig = 0;
    if (blen && dlen) {
        A_(dev_slab_put(nvec, ds, dlimbs, &dd));
        ddlimbs = dd.limbs; dmaxdig = ds.maxdig;
    } else if (blen) {
        A_(det_records(f, nvec, &dd.len, &dd.off, &dmaxdig));
        ddlimbs = f->P.Llimbs;
    }
    A_(product_core(V, nvec, xs, xlimbs, blen ? &bs : NULL, blimbs, dd.len, dd.off, ddlimbs, dmaxdig,
                    rlen_out, rlimbs_out, rnl_out, stream, ms_out));
    dev_slab_free(&dd);
    slab_free(&xs); slab_free(&bs); slab_free(&ds);
    return rc;
}

/* what every product entry refuses before it looks at its object */
static int product_args_bad(int32_t nvec, const int32_t *xlen, const uint64_t *xlimbs, const int32_t *blen, const uint64_t *blimbs,
                            const int32_t *dlen, const uint64_t *dlimbs, int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out)
{
    return nvec < 1 || !xlen || !xlimbs || !rlen_out || !rlimbs_out || !rnl_out || (blen && !blimbs) || (dlen && !dlimbs) || (dlen && !blen);
}

extern "C" int slip_hip_factor_multiply(slip_hip_factor *f, int32_t transpose, int32_t nvec,
                                        const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                        const int32_t *blen, const uint64_t *blimbs, int64_t b_limbs,
                                        const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                                        int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out, void *stream_v)
{
    if (!f || f->factors_only || product_args_bad(nvec, xlen, xlimbs, blen, blimbs, dlen, dlimbs, rlen_out, rlimbs_out, rnl_out))
        return SLIP_HIP_INCORRECT_INPUT;
    if (f->broken) return SLIP_HIP_DEVICE_ERROR;
    if (f->last_status == SLIP_HIP_DEVICE_ERROR) return SLIP_HIP_INCORRECT_INPUT;
    if (blen && !dlen && f->hs.F != f->n) return SLIP_HIP_INCORRECT_INPUT;         /* d = det needs the complete factorisation */
    int rc = 0;
    if (transpose && !f->chkt_rp) rc = build_col_view(f);
    if (!transpose && !f->chk_rp) rc = build_pos_row_view(f);
    SlipProductView V;
    V.nout = V.nx = f->n; V.alen = f->dAlen; V.aoff = f->dAoff; V.alimbs = f->dAlimbs; V.amaxdig = f->amaxdig;
    V.rp = transpose ? f->chkt_rp : f->chk_rp; V.re = transpose ? f->chkt_re : f->chk_re; V.rx = transpose ? f->chkt_rx : f->chk_rx;
    f->multiply_ms = 0;
    A_(product_entry(V, f, nvec, xlen, xlimbs, x_limbs, blen, blimbs, b_limbs, dlen, dlimbs, d_limbs,
                     rlen_out, rlimbs_out, rnl_out, (hipStream_t) stream_v, &f->multiply_ms));
    return rc;
}

extern "C" double slip_hip_factor_multiply_ms(const slip_hip_factor *f) { return f ? f->multiply_ms : 0.0; }

extern "C" int slip_hip_multiply_passes(double out[4])
{
    if (!out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, slip_product_passes_last, sizeof slip_product_passes_last);
    return SLIP_HIP_OK;
}

/* a resident m x ncols integer matrix with both of its views, no factorisation */
struct slip_hip_matrix {
    int32_t m, ncols, amaxdig;
    int32_t *dAlen; int64_t *dAoff; uint64_t *dAlimbs;
    int64_t *row_rp, *row_re; int32_t *row_rx;            /* M x:   row i, its terms' entries, their columns */
    int64_t *col_rp, *col_re; int32_t *col_rx;            /* M^T x: column j, its entries, their rows        */
    double multiply_ms;
};

extern "C" void slip_hip_matrix_destroy(slip_hip_matrix *M)
{
    if (!M) return;
    dev_free(M->dAlen); dev_free(M->dAoff); dev_free(M->dAlimbs);
    dev_free(M->row_rp); dev_free(M->row_re); dev_free(M->row_rx);
    dev_free(M->col_rp); dev_free(M->col_re); dev_free(M->col_rx);
    free(M);
}

extern "C" int slip_hip_matrix_create(slip_hip_matrix **out, int32_t m, int32_t ncols,
                                      const int64_t *Ap, const int32_t *Ai, const int32_t *Alen, const uint64_t *Alimbs)
{
    if (!out || m <= 0 || ncols <= 0 || !Ap || !Ai || !Alen || !Alimbs) return SLIP_HIP_INCORRECT_INPUT;
    *out = NULL;
    TRY_(need_device());
    SlipHostA ha;
    /* (its bound on m and ncols is the bound on the terms of an output row of either view: a repeated row is kept once) */
    TRY_(prepare_A(m, ncols, Ap, Ai, Alen, Alimbs, &ha));
    const int64_t nz = ha.nnz;
    int64_t *rp = NULL, *re = NULL, *ce = (int64_t *) malloc((size_t) nz * 8); int32_t *rx = NULL;
    int rc = !ce ? SLIP_HIP_OUT_OF_MEMORY : 0;
    A_(build_row_view(m, ncols, ha.Ap, ha.Ai, NULL, &rp, &re, &rx));
    if (!rc) for (int64_t e = 0; e < nz; e++) ce[e] = e;
    slip_hip_matrix *M = rc ? NULL : (slip_hip_matrix *) calloc(1, sizeof(slip_hip_matrix));
    if (!rc && !M) rc = SLIP_HIP_OUT_OF_MEMORY;
    if (!rc) {
        M->m = m; M->ncols = ncols; M->amaxdig = ha.maxdig;
        A_(dev_alloc(&M->dAlen, nz)); A_(dev_alloc(&M->dAoff, nz)); A_(dev_alloc(&M->dAlimbs, ha.nl));
        A_(dev_alloc(&M->row_rp, (int64_t) m + 1)); A_(dev_alloc(&M->row_re, nz)); A_(dev_alloc(&M->row_rx, nz));
        A_(dev_alloc(&M->col_rp, (int64_t) ncols + 1)); A_(dev_alloc(&M->col_re, nz)); A_(dev_alloc(&M->col_rx, nz));
        UP_(M->dAlen, ha.Alen, (size_t) nz * 4); UP_(M->dAoff, ha.Aoff, (size_t) nz * 8); UP_(M->dAlimbs, ha.Alimbs, (size_t) ha.nl * 8);
        UP_(M->row_rp, rp, ((size_t) m + 1) * 8); UP_(M->row_re, re, (size_t) nz * 8); UP_(M->row_rx, rx, (size_t) nz * 4);
        UP_(M->col_rp, ha.Ap, ((size_t) ncols + 1) * 8); UP_(M->col_re, ce, (size_t) nz * 8); UP_(M->col_rx, ha.Ai, (size_t) nz * 4);
    }
    free(rp); free(re); free(rx); free(ce);
    host_a_free(&ha);
    if (rc) { slip_hip_matrix_destroy(M); return rc; }
    *out = M;
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_matrix_multiply(slip_hip_matrix *M, int32_t transpose, int32_t nvec,
                                        const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                        const int32_t *blen, const uint64_t *blimbs, int64_t b_limbs,
                                        const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                                        int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out, void *stream_v)
{
    if (!M || product_args_bad(nvec, xlen, xlimbs, blen, blimbs, dlen, dlimbs, rlen_out, rlimbs_out, rnl_out) || (blen && !dlen))
        return SLIP_HIP_INCORRECT_INPUT;
    SlipProductView V;
    V.nout = transpose ? M->ncols : M->m; V.nx = transpose ? M->m : M->ncols;
    V.alen = M->dAlen; V.aoff = M->dAoff; V.alimbs = M->dAlimbs; V.amaxdig = M->amaxdig;
    V.rp = transpose ? M->col_rp : M->row_rp; V.re = transpose ? M->col_re : M->row_re; V.rx = transpose ? M->col_rx : M->row_rx;
    M->multiply_ms = 0;
    return product_entry(V, NULL, nvec, xlen, xlimbs, x_limbs, blen, blimbs, b_limbs, dlen, dlimbs, d_limbs,
                         rlen_out, rlimbs_out, rnl_out, (hipStream_t) stream_v, &M->multiply_ms);
}

extern "C" double slip_hip_matrix_multiply_ms(const slip_hip_matrix *M) { return M ? M->multiply_ms : 0.0; }

/* ---- exact ratio test: the leaving row, the most negative reduced cost, the dual ratio test of a simplex step chosen on
 * the device (no counterpart in the reference; kernel: slip_ratio_kernel) ---- */

/* the counts of the last slip_hip_ratio_test of this thread (the handle-less entry has nowhere else to keep them) */
static thread_local int64_t slip_ratio_paths_last[4];

/* one selection on the device.  A: n, nprob, asense, xflip, pstride, the x and a records and oidx are set (device arrays);
 * key: the host's n keys or NULL.  best, nties, neligible (host) receive nprob values each; with wlen_out the two numerators of
 * every winner come back as one compact malloc'ed slab (both read from A.xlimbs: the fused call, whose sides share a slab). */
static int ratio_core(SlipRatioArgs A, const int32_t *key, int32_t *best, int32_t *nties, int32_t *neligible,
                      int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, hipStream_t stream, double *ms_out, int64_t *paths_out)
{
    const int32_t n = A.n, nprob = A.nprob;
    const int64_t ne = (int64_t) n * nprob, nchunk = ((int64_t) n + SLIP_RATIO_CHUNK - 1) / SLIP_RATIO_CHUNK;
    const int64_t rounds = ((int64_t) n + SLIP_WAVE - 1) / SLIP_WAVE * nprob, nint = 4 * (int64_t) nprob + 3;
    int32_t *dkey = NULL, *dint = NULL, *dcand = NULL, *dcw = NULL, *dwlen = NULL; int64_t *dlokey = NULL, *dminhi = NULL, *dwoff = NULL;
    dig_t *dscr = NULL; unsigned long long *dpaths = NULL, hpaths[4] = {0, 0, 0, 0};
    int64_t *hminhi = (int64_t *) malloc((size_t) nprob * 8);
    int32_t *hres = (int32_t *) malloc((size_t) nint * 4);
    int32_t hmax[2] = {0, 0};
    int rc = !hminhi || !hres ? SLIP_HIP_OUT_OF_MEMORY : 0;
    /* dint: the candidate cursors, best, nties, neligible (nprob each, in this order), the two widths, the error flag */
    A_(dev_alloc(&dint, nint)); A_(dev_alloc(&dcand, ne)); A_(dev_alloc(&dcw, 2 * nprob * nchunk));
    A_(dev_alloc(&dlokey, ne)); A_(dev_alloc(&dminhi, nprob)); A_(dev_alloc(&dpaths, 4));
    if (key) { A_(dev_alloc(&dkey, n)); UP_(dkey, key, (size_t) n * 4); }
    if (wlen_out) { A_(dev_alloc(&dwlen, 2 * (int64_t) nprob)); A_(dev_alloc(&dwoff, 2 * (int64_t) nprob)); }
    if (!rc) for (int32_t c = 0; c < nprob; c++) hminhi[c] = INT64_MAX;
    UP_(dminhi, hminhi, (size_t) nprob * 8);
    HIP_(hipMemsetAsync(dint, 0, (size_t) nint * 4, stream)); HIP_(hipMemsetAsync(dpaths, 0, 32, stream));
    if (!rc) {
        SlipTimed timed;
        A.key = dkey; A.lokey = dlokey; A.minhi = dminhi; A.cand = dcand;
        A.ncand = dint; A.best = dint + nprob; A.nties = dint + 2 * (int64_t) nprob; A.nelig = dint + 3 * (int64_t) nprob;
        A.maxdig = dint + 4 * (int64_t) nprob; A.err = A.maxdig + 2;
        A.nchunk = (int32_t) nchunk; A.cwpos = dcw; A.cwties = dcw + nprob * nchunk;
        A.wlen = dwlen; A.woff = dwoff; A.paths = dpaths;
        A_(timed.begin(stream));
        A.phase = 0; A_(SERVICE_LAUNCH(ratio, wave_blocks(rounds), stream, A));
        A.phase = 1; A_(SERVICE_LAUNCH(ratio, wave_blocks(rounds), stream, A));
        /* the widest eligible operands (8 bytes) size the scratch of the memory path */
        HIP_(hipMemcpyAsync(hmax, A.maxdig, 8, hipMemcpyDeviceToHost, stream)); HIP_(hipStreamSynchronize(stream));
        const int64_t wcap = (int64_t) hmax[0] + hmax[1];
        int64_t blocks = wave_blocks(nprob * nchunk);
        if (!rc && wcap > 256) {
            if (wcap > (1 << 28)) rc = SLIP_HIP_OUT_OF_MEMORY;
            blocks = fit_scratch(blocks, 2 * wcap);
            A_(dev_alloc(&dscr, blocks * SERVICE_WAVES * 2 * wcap));
            A.scratch = dscr; A.wcap = (int32_t) wcap;
        }
        const int64_t fblocks = wave_blocks(nprob) < blocks ? wave_blocks(nprob) : blocks;
        A.phase = 2; A_(SERVICE_LAUNCH(ratio, blocks, stream, A));
        A.phase = 3; A_(SERVICE_LAUNCH(ratio, fblocks, stream, A));
        A_(timed.end(stream, ms_out));
    }
    DOWN_(hres, dint, (size_t) nint * 4); DOWN_(hpaths, dpaths, 32);
    if (!rc && hres[nint - 1]) rc = SLIP_HIP_DEVICE_ERROR;                          /* a product wider than the scratch */
    int32_t *wl = NULL; uint64_t *wv = NULL; int64_t wn = 0;
    if (wlen_out) A_(pack_download(2 * (int64_t) nprob, dwlen, dwoff, A.xlimbs, 0, &wl, &wv, &wn, stream));
    if (!rc) {
        memcpy(best, hres + nprob, (size_t) nprob * 4); memcpy(nties, hres + 2 * (size_t) nprob, (size_t) nprob * 4);
        memcpy(neligible, hres + 3 * (size_t) nprob, (size_t) nprob * 4);
        if (paths_out) for (int t = 0; t < 4; t++) paths_out[t] = (int64_t) hpaths[t];
        if (wlen_out) { *wlen_out = wl; *wlimbs_out = wv; *wnl_out = wn; wl = NULL; wv = NULL; }
    }
    free(hminhi); free(hres); free(wl); free(wv);
    dev_free(dkey); dev_free(dint); dev_free(dcand); dev_free(dcw); dev_free(dwlen); dev_free(dwoff);
    dev_free(dlokey); dev_free(dminhi); dev_free(dpaths); dev_free(dscr);
    return rc;
}

extern "C" int slip_hip_ratio_test(int32_t n, int32_t nprob, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                   const int32_t *alen, const uint64_t *alimbs, int64_t a_limbs, int32_t sense, const int32_t *key,
                                   int32_t *best, int32_t *nties, int32_t *neligible, void *stream_v)
{
    if (n <= 0 || nprob < 1 || (sense != 1 && sense != -1) || !xlen || !xlimbs || !alen != !alimbs || !best || !nties || !neligible)
        return SLIP_HIP_INCORRECT_INPUT;
    TRY_(need_device());
    const int64_t ne = (int64_t) n * nprob;
    SlipDevSlab x, a; memset(&x, 0, sizeof x); memset(&a, 0, sizeof a);
    int rc = dev_slab_upload(ne, xlen, xlimbs, x_limbs, &x);
    if (alen) A_(dev_slab_upload(ne, alen, alimbs, a_limbs, &a));
    SlipRatioArgs A; memset(&A, 0, sizeof A);
    A.n = n; A.nprob = nprob; A.pstride = n; A.xlen = x.len; A.xoff = x.off; A.xlimbs = x.limbs; A.alen = a.len; A.aoff = a.off; A.alimbs = a.limbs;
    A.asense = alen ? sense : 0; A.xflip = !alen && sense < 0;
    memset(slip_ratio_paths_last, 0, sizeof slip_ratio_paths_last);
    A_(ratio_core(A, key, best, nties, neligible, NULL, NULL, NULL, (hipStream_t) stream_v, NULL, slip_ratio_paths_last));
    dev_slab_free(&x); dev_slab_free(&a);
    return rc;
}

extern "C" int slip_hip_ratio_test_paths(int64_t out[4])
{
    if (!out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, slip_ratio_paths_last, sizeof slip_ratio_paths_last);
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_factor_ratio_test(slip_hip_factor *f, int32_t transpose, int32_t nprob, const int32_t *blen, const uint64_t *blimbs,
                                          int32_t sense, const int32_t *key, int32_t *best, int32_t *nties, int32_t *neligible,
                                          int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream_v)
{
    if (!f || nprob < 1 || nprob > (1 << 30) || (sense != 1 && sense != -1) || !blen || !blimbs || !best || !nties || !neligible)
        return SLIP_HIP_INCORRECT_INPUT;
    if ((wlen_out || wlimbs_out) && (!wlen_out || !wlimbs_out || !wnl_out)) return SLIP_HIP_INCORRECT_INPUT;
    if (!transpose && f->factors_only) return SLIP_HIP_INCORRECT_INPUT;             /* no q behind such a handle */
    if (wlen_out) { *wlen_out = NULL; *wlimbs_out = NULL; *wnl_out = 0; }
    hipStream_t stream = (hipStream_t) stream_v;
    SlipSolveOut o;
    TRY_(solve_device(f, transpose, 2 * nprob, blen, blimbs, stream, &o));
    const int32_t n = f->n;
    int32_t *doidx = NULL;
    int dneg = 0;
    int rc = det_negative(f, &dneg);                       /* the sign of det decides which sign of anum is eligible */
    A_(transposed_maps(f, transpose, &doidx, NULL));
    SlipRatioArgs A; memset(&A, 0, sizeof A);
    A.n = n; A.nprob = nprob; A.pstride = 2 * (int64_t) n; A.oidx = doidx;
    A.xlen = o.olen; A.xoff = o.ooff; A.xlimbs = o.olimbs; A.alen = o.olen + n; A.aoff = o.ooff + n; A.alimbs = o.olimbs;
    A.asense = dneg ? -sense : sense; A.xflip = dneg;
    f->ratio_ms = 0; memset(f->ratio_paths, 0, sizeof f->ratio_paths);
    A_(ratio_core(A, key, best, nties, neligible, wlen_out, wlimbs_out, wnl_out, stream, &f->ratio_ms, f->ratio_paths));
    dev_free(doidx);
    solve_out_free(&o);
    return rc;
}

extern "C" double slip_hip_factor_ratio_test_ms(const slip_hip_factor *f) { return f ? f->ratio_ms : 0.0; }
extern "C" int slip_hip_factor_ratio_test_paths(const slip_hip_factor *f, int64_t out[4])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->ratio_paths, sizeof f->ratio_paths);
    return SLIP_HIP_OK;
}

/* ---- bounds in the exact selections: the ratio test of a basis with boxed variables and the most violated bound, the
 * numerators formed on the device from a solve's output and a set of bounds, the selection slip_ratio_kernel's as it stands
 * (no counterpart in the reference; kernel: slip_bound_kernel) ---- */

/* the counts of this thread's last handle-less bounded call */
static thread_local int64_t slip_bound_paths_last[8];

/* a set of bounds checked and laid out on the host (bdl: the limbs of bd, `one` when the caller gave none) */
struct SlipHostBounds { SlipSlab lo, hi; int has_lo, has_hi; int32_t bddig; uint64_t one; };
static void host_bounds_free(SlipHostBounds *h) { slab_free(&h->lo); slab_free(&h->hi); }
static int host_bounds(int32_t n, const slip_hip_bounds *B, SlipHostBounds *h)
{
    memset(h, 0, sizeof *h);
    h->one = 1;
    if (!B || !B->kind) return SLIP_HIP_INCORRECT_INPUT;
    for (int32_t i = 0; i < n; i++) {
        const int32_t k = B->kind[i];
        if (k < 0 || k > 3) return SLIP_HIP_INCORRECT_INPUT;
        h->has_lo |= k & 1; h->has_hi |= k & 2;
    }
    if ((h->has_lo && (!B->lolen || !B->lolimbs)) || (h->has_hi && (!B->hilen || !B->hilimbs))) return SLIP_HIP_INCORRECT_INPUT;
    if (B->bdlimbs) {
        if (B->bdlen <= 0) return SLIP_HIP_INCORRECT_INPUT;
        h->bddig = limb_digits(B->bdlimbs, B->bdlen);
        if (h->bddig == 0) return SLIP_HIP_INCORRECT_INPUT;
    } else h->bddig = 1;
    int rc = h->has_lo ? slab_prepare(n, B->lolen, B->lolimbs, B->lo_limbs, &h->lo) : 0;
    if (!rc && h->has_hi) rc = slab_prepare(n, B->hilen, B->hilimbs, B->hi_limbs, &h->hi);
    if (rc) host_bounds_free(h);
    return rc;
}

/* the device operands of a bounded selection: x (and a, mode 0) of problem c from entry c * stride on, d_c, the map from an
 * entry to the index reported and its inverse (both NULL: the identity) */
struct SlipBoundIn {
    int32_t n, nprob, mode, sense;
    SlipDevRecs x, a, d; int64_t xstride, astride;
    const int32_t *oidx, *pos;
};

/* what a fused caller does with the winners of a group while its staging slab is alive: (c0, nv, wcap, the nv records of N
 * into dstage, dstage, the nv records of a' into I.a.limbs), all on the device; its status */
typedef std::function<int(int64_t, int64_t, int64_t, const int32_t *, const int64_t *, const uint64_t *, const int32_t *, const int64_t *)> SlipBoundCapture;

/* one bounded selection on the device.  res: 4 * nprob host integers (best, nties, the count, side); with wlen_out the
 * winners' slab (mode 0: N and a' of every problem, a' read from I.a.limbs; mode 1: v).  ms: the form passes, the selection.
 * capture (mode 0; NULL: none): handed the winners' records of every group after its selection. */
static int bound_core(const SlipBoundIn &I, const slip_hip_bounds *B, const SlipHostBounds &hb, const int32_t *key, int32_t *res,
                      int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, hipStream_t stream, double ms[2], int64_t paths[8],
                      const SlipBoundCapture *capture = NULL)
{
    const int32_t n = I.n, nprob = I.nprob;
    const int64_t ne = (int64_t) n * nprob, rpp = ((int64_t) n + SLIP_WAVE - 1) / SLIP_WAVE;
    int32_t *dkind = NULL, *dcls = NULL, *dw = NULL, *drl = NULL, *dal2 = NULL, *dwmax = NULL, *dsel = NULL, *dwn = NULL;
    int64_t *dso = NULL, *dao2 = NULL, *dwo = NULL;
    uint64_t *dbd = NULL;
    SlipDevSlab lo, hi; memset(&lo, 0, sizeof lo); memset(&hi, 0, sizeof hi);
    dig_t *dscr = NULL; unsigned long long *dpaths = NULL, hpaths[4] = {0, 0, 0, 0};
    int32_t *hres = (int32_t *) malloc((size_t) nprob * 16), hwmax[2] = {0, 0};
    std::vector<int32_t> wl; std::vector<uint64_t> wv;
    int rc = !hres ? SLIP_HIP_OUT_OF_MEMORY : 0;
    ms[0] = ms[1] = 0; memset(paths, 0, 8 * sizeof(int64_t));
    /* the bounds; dbd: the limbs of bd, then one limb holding 1 (the denominator record of a violated entry) */
    const int64_t bdn = ((int64_t) hb.bddig + 1) >> 1;
    A_(dev_alloc(&dkind, n)); UP_(dkind, B->kind, (size_t) n * 4);
    A_(dev_alloc(&dbd, bdn + 1)); UP_(dbd, B->bdlimbs ? B->bdlimbs : &hb.one, (size_t) bdn * 8); UP_(dbd + bdn, &hb.one, 8);
    if (hb.has_lo) A_(dev_slab_put(n, hb.lo, B->lolimbs, &lo));
    if (hb.has_hi) A_(dev_slab_put(n, hb.hi, B->hilimbs, &hi));
    A_(dev_alloc(&dcls, ne)); A_(dev_alloc(&dw, ne)); A_(dev_alloc(&drl, ne)); A_(dev_alloc(&dso, ne));
    A_(dev_alloc(&dal2, ne)); A_(dev_alloc(&dao2, ne)); A_(dev_alloc(&dwmax, 2)); A_(dev_alloc(&dpaths, 4));
    A_(dev_alloc(&dsel, 2 * (int64_t) nprob));
    if (wlen_out || capture) { A_(dev_alloc(&dwn, 2 * (int64_t) nprob)); A_(dev_alloc(&dwo, 2 * (int64_t) nprob)); }
    HIP_(hipMemsetAsync(dwmax, 0, 8, stream)); HIP_(hipMemsetAsync(dpaths, 0, 32, stream));
    SlipBoundArgs A; memset(&A, 0, sizeof A);
    A.n = n; A.mode = I.mode; A.sense = I.sense; A.xstride = I.xstride; A.astride = I.astride;
    A.xlimbs = I.x.limbs; A.alimbs = I.a.limbs; A.dlimbs = I.d.limbs; A.oidx = I.oidx; A.pos = I.pos;
    A.kind = dkind; A.lolen = lo.len; A.looff = lo.off; A.lolimbs = lo.limbs; A.hilen = hi.len; A.hioff = hi.off; A.hilimbs = hi.limbs;
    A.bddig = hb.bddig; A.bdlimbs = dbd; A.bdunit = hb.bddig == 1 && (B->bdlimbs ? B->bdlimbs[0] : 1) == 1;
    A.wmax = dwmax; A.paths = dpaths;
    /* the problems c0 .. c0 + nv of every per-problem and per-entry array */
    auto slice = [&](int64_t c0, int64_t nv, int phase) {
        A.nprob = (int32_t) nv; A.phase = phase;
        A.xlen = I.x.len + c0 * I.xstride; A.xoff = I.x.off + c0 * I.xstride;
        A.alen = I.a.len ? I.a.len + c0 * I.astride : NULL; A.aoff = I.a.off ? I.a.off + c0 * I.astride : NULL;
        A.dlen = I.d.len + c0; A.doff = I.d.off + c0;
        A.cls = dcls + c0 * n; A.w = dw + c0 * n; A.rlen = drl + c0 * n; A.soff = dso + c0 * n;
        A.alen2 = dal2 + c0 * n; A.aoff2 = dao2 + c0 * n;
    };
    if (!rc) {                                             /* the classes and widths of all entries, the widest of them */
        SlipTimed timed;
        slice(0, nprob, 0);
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(bound, wave_blocks(rpp * nprob), stream, A));
        A_(timed.end(stream, &ms[0]));
    }
    DOWN_(hwmax, dwmax, 8);
    const int64_t wcap = hwmax[0] > 1 ? ((int64_t) hwmax[0] + 1) & ~(int64_t) 1 : 2, scap = ((int64_t) hwmax[1] + 1) & ~(int64_t) 1;
    if (!rc && wcap > (1 << 28)) rc = SLIP_HIP_OUT_OF_MEMORY;
    const int64_t wblocks = hwmax[1] > 256 ? fit_scratch(wave_blocks(ne), 2 * scap) : wave_blocks(ne);
    if (hwmax[1] > 256) { A_(dev_alloc(&dscr, wblocks * SERVICE_WAVES * 2 * scap)); A.scratch = dscr; A.wcap = (int32_t) scap; }
    /* the numerators of a group of whole problems into the staging slab: the lane pass, the wave pass */
    auto form = [&](int64_t c0, int64_t nv, int64_t cnt, uint64_t *dstage) {
        int rc = 0;
        A.stage = dstage;
        slice(c0, nv, 1); A_(SERVICE_LAUNCH(bound, wave_blocks(rpp * nv), stream, A));
        slice(c0, nv, 2); A_(SERVICE_LAUNCH(bound, wave_blocks(cnt) < wblocks ? wave_blocks(cnt) : wblocks, stream, A));
        return rc;
    };
    auto select = [&](int64_t c0, int64_t nv, const uint64_t *dstage) {
        /* the selection on the group's (N, a') records */
        int64_t gp[4] = {0, 0, 0, 0};
        double t = 0;
        SlipRatioArgs R; memset(&R, 0, sizeof R);
        R.n = n; R.nprob = (int32_t) nv; R.pstride = n; R.oidx = I.oidx;
        R.xlen = drl + c0 * n; R.xoff = dso + c0 * n; R.xlimbs = dstage;
        R.alen = dal2 + c0 * n; R.aoff = dao2 + c0 * n; R.alimbs = I.mode ? dbd + bdn : I.a.limbs;
        R.asense = I.mode ? 1 : I.sense; R.xflip = I.mode;
        int rc = ratio_core(R, key, hres + c0, hres + nprob + c0, hres + 2 * (int64_t) nprob + c0, NULL, NULL, NULL, stream, &t, gp);
        if (!rc) { ms[1] += t; for (int k = 0; k < 4; k++) paths[4 + k] += gp[k]; }
        /* the winners' sides and, on request, their records */
        UP_(dsel, hres + c0, (size_t) nv * 4);
        if (!rc) {
            slice(c0, nv, 3);
            A.best = dsel; A.side = dsel + nprob;
            if (wlen_out || capture) { A.wnlen = dwn; A.wnoff = dwo; A.walen = I.mode ? NULL : dwn + nprob; A.waoff = I.mode ? NULL : dwo + nprob; }
            A_(SERVICE_LAUNCH(bound, service_blocks(nv), stream, A));
            HIP_(hipStreamSynchronize(stream));
        }
        DOWN_(hres + 3 * (int64_t) nprob + c0, dsel + nprob, (size_t) nv * 4);
        if (wlen_out) A_(winners_collect(nv, dwn, dwo, dstage, dwn + nprob, dwo + nprob, I.mode ? NULL : I.a.limbs, &wl, &wv, stream));
        if (capture) A_((*capture)(c0, nv, wcap, dwn, dwo, dstage, dwn + nprob, dwo + nprob));
        return rc;
    };
    A_(staged_run(n, nprob, 1, wcap, dw, dso, form, select, stream, &ms[0], &ms[0]));
    DOWN_(hpaths, dpaths, 32);
    if (!rc && wlen_out) rc = winners_out(wl, wv, wlen_out, wlimbs_out, wnl_out);
    if (!rc) {
        memcpy(res, hres, (size_t) nprob * 16);
        for (int k = 0; k < 4; k++) paths[k] = (int64_t) hpaths[k];
    }
    free(hres);
    dev_slab_free(&lo); dev_slab_free(&hi);
    dev_free(dkind); dev_free(dbd); dev_free(dcls); dev_free(dw); dev_free(drl); dev_free(dso); dev_free(dal2); dev_free(dao2);
    dev_free(dwmax); dev_free(dpaths); dev_free(dsel); dev_free(dwn); dev_free(dwo); dev_free(dscr);
    return rc;
}

/* both fused forms: mode 0 the bounded ratio test on 2 * nprob right-hand sides, mode 1 the bound test on nprob */
static int bound_on_handle(slip_hip_factor *f, int mode, int32_t transpose, int32_t nprob, const int32_t *blen, const uint64_t *blimbs,
                           const slip_hip_bounds *bounds, int32_t sense, const int32_t *key,
                           int32_t *r0, int32_t *r1, int32_t *r2, int32_t *r3,
                           int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream_v)
{
    if (!f || nprob < 1 || nprob > (1 << 29) || (sense != 1 && sense != -1) || !blen || !blimbs || !r0 || !r1 || !r2 || !r3 ||
        !bounds || !bounds->kind)
        return SLIP_HIP_INCORRECT_INPUT;
    if (winners_args_bad(wlen_out, wlimbs_out, wnl_out)) return SLIP_HIP_INCORRECT_INPUT;
    if (!transpose && f->factors_only) return SLIP_HIP_INCORRECT_INPUT;             /* no q behind such a handle */
    if (f->broken) return SLIP_HIP_DEVICE_ERROR;
    if (f->hs.F != f->n) return SLIP_HIP_INCORRECT_INPUT;       /* needs the complete factorisation */
    const int32_t n = f->n, per = mode ? 1 : 2;
    hipStream_t stream = (hipStream_t) stream_v;
    SlipHostBounds hb;
    TRY_(host_bounds(n, bounds, &hb));
    SlipSolveOut o;
    int rc = solve_device(f, transpose, per * nprob, blen, blimbs, stream, &o);
    if (rc) { host_bounds_free(&hb); return rc; }
    if (wlen_out) { *wlen_out = NULL; *wlimbs_out = NULL; *wnl_out = 0; }
    int32_t *ddlen = NULL, *doidx = NULL, *dpos = NULL, *res = (int32_t *) malloc((size_t) nprob * 16); int64_t *ddoff = NULL;
    int32_t dmaxdig = 0;
    if (!res) rc = SLIP_HIP_OUT_OF_MEMORY;
    A_(det_records(f, nprob, &ddlen, &ddoff, &dmaxdig));
    A_(transposed_maps(f, transpose, &doidx, &dpos));
    SlipBoundIn I; memset(&I, 0, sizeof I);
    I.n = n; I.nprob = nprob; I.mode = mode; I.sense = sense; I.oidx = doidx; I.pos = dpos;
    I.x.len = o.olen; I.x.off = o.ooff; I.x.limbs = o.olimbs; I.xstride = (int64_t) per * n;
    if (!mode) { I.a.len = o.olen + n; I.a.off = o.ooff + n; I.a.limbs = o.olimbs; I.astride = 2 * (int64_t) n; }
    I.d.len = ddlen; I.d.off = ddoff; I.d.limbs = f->P.Llimbs;
    double ms[2]; int64_t paths[8];
    A_(bound_core(I, bounds, hb, key, res, wlen_out, wlimbs_out, wnl_out, stream, ms, paths));
    if (!rc) {
        results_out(res, nprob, r0, r1, r2, r3);
        memcpy(f->bound_ms, ms, sizeof ms); memcpy(f->bound_paths, paths, sizeof paths);
    }
    free(res); dev_free(doidx); dev_free(dpos); dev_free(ddlen); dev_free(ddoff);
    solve_out_free(&o);
    host_bounds_free(&hb);
    return rc;
}

extern "C" int slip_hip_factor_ratio_test_bounded(slip_hip_factor *f, int32_t transpose, int32_t nprob, const int32_t *blen, const uint64_t *blimbs,
                                                  const slip_hip_bounds *bounds, int32_t sense, const int32_t *key,
                                                  int32_t *best, int32_t *nties, int32_t *neligible, int32_t *side,
                                                  int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream_v)
{
    return bound_on_handle(f, 0, transpose, nprob, blen, blimbs, bounds, sense, key, best, nties, neligible, side, wlen_out, wlimbs_out, wnl_out, stream_v);
}

extern "C" int slip_hip_factor_bound_test(slip_hip_factor *f, int32_t transpose, int32_t nprob, const int32_t *blen, const uint64_t *blimbs,
                                          const slip_hip_bounds *bounds, const int32_t *key,
                                          int32_t *worst, int32_t *nties, int32_t *nviolated, int32_t *side,
                                          int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream_v)
{
    return bound_on_handle(f, 1, transpose, nprob, blen, blimbs, bounds, 1, key, worst, nties, nviolated, side, wlen_out, wlimbs_out, wnl_out, stream_v);
}

/* both handle-less forms (mode 1: no a) */
static int bound_on_slabs(int mode, int32_t n, int32_t nprob, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                          const int32_t *alen, const uint64_t *alimbs, int64_t a_limbs,
                          const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                          const slip_hip_bounds *bounds, int32_t sense, const int32_t *key,
                          int32_t *r0, int32_t *r1, int32_t *r2, int32_t *r3,
                          int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream_v)
{
    if (n <= 0 || nprob < 1 || nprob > (1 << 29) || (sense != 1 && sense != -1) || !xlen || !xlimbs || (!mode && (!alen || !alimbs)) ||
        !dlen || !dlimbs || !r0 || !r1 || !r2 || !r3 || !bounds || !bounds->kind)
        return SLIP_HIP_INCORRECT_INPUT;
    if (winners_args_bad(wlen_out, wlimbs_out, wnl_out)) return SLIP_HIP_INCORRECT_INPUT;
    TRY_(need_device());
    const int64_t ne = (int64_t) n * nprob;
    SlipHostBounds hb;
    TRY_(host_bounds(n, bounds, &hb));
    SlipDevSlab x, a, d; memset(&x, 0, sizeof x); memset(&a, 0, sizeof a); memset(&d, 0, sizeof d);
    int32_t *res = NULL;
    /* (every slab is checked against its capacity before a limb of it is read) */
    int rc = dev_slab_upload(nprob, dlen, dlimbs, d_limbs, &d);
    for (int32_t c = 0; c < nprob && !rc; c++) if (d.s.dig[c] == 0) rc = SLIP_HIP_INCORRECT_INPUT;
    A_(dev_slab_upload(ne, xlen, xlimbs, x_limbs, &x));
    if (!mode) A_(dev_slab_upload(ne, alen, alimbs, a_limbs, &a));
    if (!rc && !(res = (int32_t *) malloc((size_t) nprob * 16))) rc = SLIP_HIP_OUT_OF_MEMORY;
    if (!rc && wlen_out) { *wlen_out = NULL; *wlimbs_out = NULL; *wnl_out = 0; }
    SlipBoundIn I; memset(&I, 0, sizeof I);
    I.n = n; I.nprob = nprob; I.mode = mode; I.sense = sense; I.xstride = n; I.astride = n;
    I.x = dev_slab_recs(x); I.a = dev_slab_recs(a); I.d = dev_slab_recs(d);
    double ms[2]; int64_t paths[8];
    A_(bound_core(I, bounds, hb, key, res, wlen_out, wlimbs_out, wnl_out, (hipStream_t) stream_v, ms, paths));
    if (!rc) {
        results_out(res, nprob, r0, r1, r2, r3);
        memcpy(slip_bound_paths_last, paths, sizeof paths);
    }
    free(res);
    dev_slab_free(&x); dev_slab_free(&a); dev_slab_free(&d);
    host_bounds_free(&hb);
    return rc;
}

extern "C" int slip_hip_ratio_test_bounded(int32_t n, int32_t nprob, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                           const int32_t *alen, const uint64_t *alimbs, int64_t a_limbs,
                                           const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                                           const slip_hip_bounds *bounds, int32_t sense, const int32_t *key,
                                           int32_t *best, int32_t *nties, int32_t *neligible, int32_t *side,
                                           int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream_v)
{
    return bound_on_slabs(0, n, nprob, xlen, xlimbs, x_limbs, alen, alimbs, a_limbs, dlen, dlimbs, d_limbs, bounds, sense, key,
                          best, nties, neligible, side, wlen_out, wlimbs_out, wnl_out, stream_v);
}

extern "C" int slip_hip_bound_test(int32_t n, int32_t nprob, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                   const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                                   const slip_hip_bounds *bounds, const int32_t *key,
                                   int32_t *worst, int32_t *nties, int32_t *nviolated, int32_t *side,
                                   int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream_v)
{
    return bound_on_slabs(1, n, nprob, xlen, xlimbs, x_limbs, NULL, NULL, 0, dlen, dlimbs, d_limbs, bounds, 1, key,
                          worst, nties, nviolated, side, wlen_out, wlimbs_out, wnl_out, stream_v);
}

extern "C" int slip_hip_factor_bound_ms(const slip_hip_factor *f, double out[2])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->bound_ms, sizeof f->bound_ms);
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_factor_bound_paths(const slip_hip_factor *f, int64_t out[8])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->bound_paths, sizeof f->bound_paths);
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_bound_paths(int64_t out[8])
{
    if (!out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, slip_bound_paths_last, sizeof slip_bound_paths_last);
    return SLIP_HIP_OK;
}

/* ---- exact pivot update: the numerators of the next basic solution (or of the next duals) from those the ratio test already
 * holds, R = (P V - T A) / D per entry, with no second substitution (no counterpart in the reference; kernel:
 * slip_pivot_kernel) ---- */

/* the counts of this thread's last handle-less update */
static thread_local int64_t slip_pivot_paths_last[8];

/* the device operands of an update: v and a of problem c from entry c * stride on, P_c, T_c and D_c (d.len NULL: no division),
 * the map from an entry to the index reported and its inverse (both NULL: the identity), place (NULL: none) */
struct SlipPivotIn {
    int32_t n, nprob;
    SlipDevRecs v, a, p, t, d; int64_t vstride, astride;
    const int32_t *oidx, *pos, *place;
};

/* one update on the device.  ninexact: nprob host integers; the result: one compact malloc'ed slab of n * nprob entries in
 * reported order.  ms: the classify, offset and form passes; paths: [0 .. 3] the entries by path, [4] the inexact ones. */
static int pivot_core(const SlipPivotIn &I, int32_t *ninexact, int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out,
                      hipStream_t stream, double *ms, int64_t paths[8])
{
    const int32_t n = I.n, nprob = I.nprob;
    const int64_t ne = (int64_t) n * nprob, rpp = ((int64_t) n + SLIP_WAVE - 1) / SLIP_WAVE;
    int32_t *dcls = NULL, *dw = NULL, *drl = NULL, *dwmax = NULL, *dnin = NULL; int64_t *dso = NULL;
    dig_t *dscr = NULL; unsigned long long *dpaths = NULL, hpaths[4] = {0, 0, 0, 0};
    int32_t hwmax[2] = {0, 0};
    int32_t *hnin = (int32_t *) malloc((size_t) nprob * 4), *ol = (int32_t *) malloc((size_t) ne * 4);
    uint64_t *out = NULL; int64_t on = 0;                  /* the result's limbs so far: every group's slab is appended */
    int rc = !hnin || !ol ? SLIP_HIP_OUT_OF_MEMORY : 0;
    *ms = 0; memset(paths, 0, 8 * sizeof(int64_t));
    A_(dev_alloc(&dcls, ne)); A_(dev_alloc(&dw, ne)); A_(dev_alloc(&drl, ne)); A_(dev_alloc(&dso, ne));
    A_(dev_alloc(&dwmax, 2)); A_(dev_alloc(&dpaths, 4)); A_(dev_alloc(&dnin, nprob));
    HIP_(hipMemsetAsync(dwmax, 0, 8, stream)); HIP_(hipMemsetAsync(dpaths, 0, 32, stream)); HIP_(hipMemsetAsync(dnin, 0, (size_t) nprob * 4, stream));
    SlipPivotArgs A; memset(&A, 0, sizeof A);
    A.n = n; A.vstride = I.vstride; A.astride = I.astride; A.oidx = I.oidx; A.pos = I.pos;
    A.vlimbs = I.v.limbs; A.alimbs = I.a.limbs; A.plimbs = I.p.limbs; A.tlimbs = I.t.limbs; A.dlimbs = I.d.limbs;
    A.wmax = dwmax; A.paths = dpaths;
    /* the problems c0 .. c0 + nv of every per-problem and per-entry array */
    auto slice = [&](int64_t c0, int64_t nv, int phase) {
        A.nprob = (int32_t) nv; A.phase = phase;
        A.vlen = I.v.len + c0 * I.vstride; A.voff = I.v.off + c0 * I.vstride;
        A.alen = I.a.len + c0 * I.astride; A.aoff = I.a.off + c0 * I.astride;
        A.plen = I.p.len + c0; A.poff = I.p.off + c0; A.tlen = I.t.len + c0; A.toff = I.t.off + c0;
        A.dlen = I.d.len ? I.d.len + c0 : NULL; A.doff = I.d.len ? I.d.off + c0 : NULL;
        A.place = I.place ? I.place + c0 : NULL; A.ninexact = dnin + c0;
        A.cls = dcls + c0 * n; A.w = dw + c0 * n; A.rlen = drl + c0 * n; A.soff = dso + c0 * n;
    };
    if (!rc) {                                             /* the paths and widths of all entries, the widest of them */
        SlipTimed timed;
        slice(0, nprob, 0);
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(pivot, wave_blocks(rpp * nprob), stream, A));
        A_(timed.end(stream, ms));
    }
    DOWN_(hwmax, dwmax, 8);
    const int64_t wcap = hwmax[0] > 1 ? ((int64_t) hwmax[0] + 1) & ~(int64_t) 1 : 2, scap = ((int64_t) hwmax[1] + 1) & ~(int64_t) 1;
    if (!rc && (wcap > (1 << 28) || scap > (1 << 27))) rc = SLIP_HIP_OUT_OF_MEMORY;
    /* per wave: the 64 * 5 + 2 digits a register shift goes through, or the seven buffers of the memory path */
    const int64_t wscr = 7 * scap > 328 ? 7 * scap : 328;
    const int64_t wblocks = fit_scratch(wave_blocks(ne), wscr);
    A_(dev_alloc(&dscr, wblocks * SERVICE_WAVES * wscr));
    A.scratch = dscr; A.wcap = (int32_t) scap; A.wscr = (int32_t) wscr;
    /* a group of whole problems into the staging slab: the lane pass, the wave pass, the placed entries */
    auto form = [&](int64_t c0, int64_t nv, int64_t cnt, uint64_t *dstage) {
        int rc = 0;
        A.stage = dstage;
        slice(c0, nv, 1); A_(SERVICE_LAUNCH(pivot, wave_blocks(rpp * nv), stream, A));
        slice(c0, nv, 2); A_(SERVICE_LAUNCH(pivot, wave_blocks(cnt) < wblocks ? wave_blocks(cnt) : wblocks, stream, A));
        if (I.place) { slice(c0, nv, 3); A_(SERVICE_LAUNCH(pivot, wave_blocks(nv), stream, A)); }
        return rc;
    };
    /* (the block of a call that fits one group is the result as pack_download made it) */
    auto sink = [&](int64_t c0, int64_t nv, const uint64_t *dstage) {
        return pack_append(n * nv, drl + c0 * n, dso + c0 * n, dstage, ol + c0 * n, &out, &on, stream);
    };
    A_(staged_run(n, nprob, 1, wcap, dw, dso, form, sink, stream, ms, ms));
    DOWN_(hpaths, dpaths, 32); DOWN_(hnin, dnin, (size_t) nprob * 4);
    if (!rc) {
        memcpy(ninexact, hnin, (size_t) nprob * 4);
        for (int k = 0; k < 4; k++) paths[k] = (int64_t) hpaths[k];
        for (int32_t c = 0; c < nprob; c++) paths[4] += hnin[c];
        *rlen_out = ol; *rlimbs_out = out; *rnl_out = on;
        ol = NULL; out = NULL;
    }
    free(hnin); free(ol); free(out);
    dev_free(dcls); dev_free(dw); dev_free(drl); dev_free(dso); dev_free(dwmax); dev_free(dpaths); dev_free(dnin); dev_free(dscr);
    return rc;
}

/* place: nprob indices in [-1, n), or NULL */
static int pivot_place_ok(const int32_t *place, int32_t nprob, int32_t n)
{
    if (place) for (int32_t c = 0; c < nprob; c++) if (place[c] < -1 || place[c] >= n) return 0;
    return 1;
}

extern "C" int slip_hip_pivot_update(int32_t n, int32_t nprob,
                                     const int32_t *vlen, const uint64_t *vlimbs, int64_t v_limbs,
                                     const int32_t *alen, const uint64_t *alimbs, int64_t a_limbs,
                                     const int32_t *plen, const uint64_t *plimbs, int64_t p_limbs,
                                     const int32_t *tlen, const uint64_t *tlimbs, int64_t t_limbs,
                                     const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                                     const int32_t *place, int32_t *ninexact,
                                     int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out, void *stream_v)
{
    if (n <= 0 || nprob < 1 || nprob > (1 << 29) || !vlen || !vlimbs || !alen || !alimbs || !plen || !plimbs || !tlen || !tlimbs ||
        !dlen != !dlimbs || !ninexact || !rlen_out || !rlimbs_out || !rnl_out || !pivot_place_ok(place, nprob, n))
        return SLIP_HIP_INCORRECT_INPUT;
    const int64_t ne = (int64_t) n * nprob;
    SlipDevSlab v, a, p, t, d; memset(&v, 0, sizeof v); memset(&a, 0, sizeof a); memset(&p, 0, sizeof p); memset(&t, 0, sizeof t); memset(&d, 0, sizeof d);
    int32_t *dplace = NULL;
    /* (every slab is checked against its capacity before a limb of it is read, and all of them before the device is asked for) */
    int rc = slab_prepare(ne, vlen, vlimbs, v_limbs, &v.s);
    A_(slab_prepare(ne, alen, alimbs, a_limbs, &a.s));
    A_(slab_prepare(nprob, plen, plimbs, p_limbs, &p.s));
    A_(slab_prepare(nprob, tlen, tlimbs, t_limbs, &t.s));
    if (dlen) {
        A_(slab_prepare(nprob, dlen, dlimbs, d_limbs, &d.s));
        for (int32_t c = 0; c < nprob && !rc; c++) if (d.s.dig[c] == 0) rc = SLIP_HIP_INCORRECT_INPUT;
    }
    A_(need_device());
    A_(dev_slab_put(ne, v.s, vlimbs, &v)); A_(dev_slab_put(ne, a.s, alimbs, &a));
    A_(dev_slab_put(nprob, p.s, plimbs, &p)); A_(dev_slab_put(nprob, t.s, tlimbs, &t));
    if (dlen) A_(dev_slab_put(nprob, d.s, dlimbs, &d));
    if (place) { A_(dev_alloc(&dplace, nprob)); UP_(dplace, place, (size_t) nprob * 4); }
    SlipPivotIn I; memset(&I, 0, sizeof I);
    I.n = n; I.nprob = nprob; I.vstride = n; I.astride = n; I.place = dplace;
    I.v = dev_slab_recs(v); I.a = dev_slab_recs(a); I.p = dev_slab_recs(p); I.t = dev_slab_recs(t); I.d = dev_slab_recs(d);
    double ms; int64_t paths[8];
    A_(pivot_core(I, ninexact, rlen_out, rlimbs_out, rnl_out, (hipStream_t) stream_v, &ms, paths));
    if (!rc) memcpy(slip_pivot_paths_last, paths, sizeof paths);
    dev_slab_free(&v); dev_slab_free(&a); dev_slab_free(&p); dev_slab_free(&t); dev_slab_free(&d);
    dev_free(dplace);
    return rc;
}

extern "C" int slip_hip_pivot_update_paths(int64_t out[8])
{
    if (!out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, slip_pivot_paths_last, sizeof slip_pivot_paths_last);
    return SLIP_HIP_OK;
}

/* both fused forms.  step 0 (slip_hip_factor_solve_update): P, T (host slabs ps, ts) and place from the caller.  step 1
 * (slip_hip_factor_step): the selection of slip_hip_factor_ratio_test on the solve's output, then P, T and place from its
 * winners (phase 4 of the kernel) and the slab of the new denominators P_c. */
static int update_on_handle(slip_hip_factor *f, int step, int32_t transpose, int32_t nprob, const int32_t *blen, const uint64_t *blimbs,
                            const SlipSlab *ps, const uint64_t *plimbs, const SlipSlab *ts, const uint64_t *tlimbs, const int32_t *place,
                            int32_t sense, const int32_t *key, int32_t *best, int32_t *nties, int32_t *neligible, int32_t *ninexact,
                            int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out,
                            int32_t **dlen_out, uint64_t **dlimbs_out, int64_t *dnl_out, hipStream_t stream)
{
    if (!transpose && f->factors_only) return SLIP_HIP_INCORRECT_INPUT;             /* no q behind such a handle */
    if (f->broken) return SLIP_HIP_DEVICE_ERROR;
    if (f->hs.F != f->n) return SLIP_HIP_INCORRECT_INPUT;       /* needs the complete factorisation */
    const int32_t n = f->n;
    SlipSolveOut o;
    TRY_(solve_device(f, transpose, 2 * nprob, blen, blimbs, stream, &o));
    int32_t *ddlen = NULL, *doidx = NULL, *dpos = NULL, *dplace = NULL, *dbest = NULL; int64_t *ddoff = NULL;
    SlipDevSlab dp, dt; memset(&dp, 0, sizeof dp); memset(&dt, 0, sizeof dt);      /* (step 1: records alone, into the solve's output) */
    int32_t *hbest = NULL, *hties = NULL, *helig = NULL, *rl = NULL, *nl = NULL; uint64_t *rv = NULL, *nv = NULL; int64_t rn = 0, nn = 0;
    int32_t dmaxdig = 0;
    int rc = 0;
    A_(det_records(f, nprob, &ddlen, &ddoff, &dmaxdig));
    A_(transposed_maps(f, transpose, &doidx, &dpos));
    SlipPivotIn I; memset(&I, 0, sizeof I);
    I.n = n; I.nprob = nprob; I.oidx = doidx; I.pos = dpos; I.vstride = I.astride = 2 * (int64_t) n;
    I.v.len = o.olen; I.v.off = o.ooff; I.v.limbs = o.olimbs; I.a.len = o.olen + n; I.a.off = o.ooff + n; I.a.limbs = o.olimbs;
    I.d.len = ddlen; I.d.off = ddoff; I.d.limbs = f->P.Llimbs;
    double sel_ms = 0;
    if (!step) {
        A_(dev_slab_put(nprob, *ps, plimbs, &dp)); A_(dev_slab_put(nprob, *ts, tlimbs, &dt));
        if (place) { A_(dev_alloc(&dplace, nprob)); UP_(dplace, place, (size_t) nprob * 4); }
    } else {
        A_(dev_alloc(&dp.len, nprob)); A_(dev_alloc(&dp.off, nprob)); A_(dev_alloc(&dt.len, nprob)); A_(dev_alloc(&dt.off, nprob));
        hbest = (int32_t *) malloc((size_t) nprob * 4); hties = (int32_t *) malloc((size_t) nprob * 4); helig = (int32_t *) malloc((size_t) nprob * 4);
        if (!hbest || !hties || !helig) rc = rc ? rc : SLIP_HIP_OUT_OF_MEMORY;
        /* the selection, as slip_hip_factor_ratio_test makes it: the sign of det decides which sign of anum is eligible */
        int dneg = 0;
        A_(det_negative(f, &dneg));
        SlipRatioArgs R; memset(&R, 0, sizeof R);
        R.n = n; R.nprob = nprob; R.pstride = 2 * (int64_t) n; R.oidx = doidx;
        R.xlen = o.olen; R.xoff = o.ooff; R.xlimbs = o.olimbs; R.alen = o.olen + n; R.aoff = o.ooff + n; R.alimbs = o.olimbs;
        R.asense = dneg ? -sense : sense; R.xflip = dneg;
        f->ratio_ms = 0; memset(f->ratio_paths, 0, sizeof f->ratio_paths);
        A_(ratio_core(R, key, hbest, hties, helig, NULL, NULL, NULL, stream, &f->ratio_ms, f->ratio_paths));
        sel_ms = f->ratio_ms;
        /* the winners' records and places */
        A_(dev_alloc(&dbest, nprob)); A_(dev_alloc(&dplace, nprob));
        UP_(dbest, hbest, (size_t) nprob * 4);
        if (!rc) {
            SlipPivotArgs W; memset(&W, 0, sizeof W);
            W.n = n; W.nprob = nprob; W.phase = 4; W.vstride = I.vstride; W.astride = I.astride; W.pos = dpos;
            W.vlen = I.v.len; W.voff = I.v.off; W.alen = I.a.len; W.aoff = I.a.off;
            W.best = dbest; W.wplen = dp.len; W.wpoff = dp.off; W.wtlen = dt.len; W.wtoff = dt.off; W.wplace = dplace;
            A_(SERVICE_LAUNCH(pivot, service_blocks(nprob), stream, W));
        }
    }
    I.p = dev_slab_recs(dp); I.t = dev_slab_recs(dt); I.place = dplace;
    if (step) I.p.limbs = I.t.limbs = o.olimbs;
    double ms = 0; int64_t paths[8];
    A_(pivot_core(I, ninexact, &rl, &rv, &rn, stream, &ms, paths));
    if (step) A_(pack_download(nprob, dp.len, dp.off, o.olimbs, 0, &nl, &nv, &nn, stream));
    if (!rc) {
        f->update_ms[0] = ms; f->update_ms[1] = sel_ms; memcpy(f->update_paths, paths, sizeof paths);
        *rlen_out = rl; *rlimbs_out = rv; *rnl_out = rn; rl = NULL; rv = NULL;
        if (step) {
            memcpy(best, hbest, (size_t) nprob * 4); memcpy(nties, hties, (size_t) nprob * 4); memcpy(neligible, helig, (size_t) nprob * 4);
            *dlen_out = nl; *dlimbs_out = nv; *dnl_out = nn; nl = NULL; nv = NULL;
        }
    }
    free(hbest); free(hties); free(helig); free(rl); free(rv); free(nl); free(nv);
    dev_free(ddlen); dev_free(ddoff); dev_free(doidx); dev_free(dpos); dev_free(dplace); dev_free(dbest);
    dev_slab_free(&dp); dev_slab_free(&dt);
    solve_out_free(&o);
    return rc;
}

extern "C" int slip_hip_factor_solve_update(slip_hip_factor *f, int32_t transpose, int32_t nprob,
                                            const int32_t *blen, const uint64_t *blimbs,
                                            const int32_t *plen, const uint64_t *plimbs, int64_t p_limbs,
                                            const int32_t *tlen, const uint64_t *tlimbs, int64_t t_limbs,
                                            const int32_t *place, int32_t *ninexact,
                                            int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out, void *stream_v)
{
    if (!f || nprob < 1 || nprob > (1 << 29) || !blen || !blimbs || !plen || !plimbs || !tlen || !tlimbs || !ninexact ||
        !rlen_out || !rlimbs_out || !rnl_out || !pivot_place_ok(place, nprob, f->n))
        return SLIP_HIP_INCORRECT_INPUT;
    SlipSlab ps, ts; memset(&ps, 0, sizeof ps); memset(&ts, 0, sizeof ts);
    int rc = slab_prepare(nprob, plen, plimbs, p_limbs, &ps);
    A_(slab_prepare(nprob, tlen, tlimbs, t_limbs, &ts));
    A_(update_on_handle(f, 0, transpose, nprob, blen, blimbs, &ps, plimbs, &ts, tlimbs, place, 1, NULL, NULL, NULL, NULL, ninexact,
                        rlen_out, rlimbs_out, rnl_out, NULL, NULL, NULL, (hipStream_t) stream_v));
    slab_free(&ps); slab_free(&ts);
    return rc;
}

extern "C" int slip_hip_factor_step(slip_hip_factor *f, int32_t transpose, int32_t nprob,
                                    const int32_t *blen, const uint64_t *blimbs, int32_t sense, const int32_t *key,
                                    int32_t *best, int32_t *nties, int32_t *neligible, int32_t *ninexact,
                                    int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out,
                                    int32_t **dlen_out, uint64_t **dlimbs_out, int64_t *dnl_out, void *stream_v)
{
    if (!f || nprob < 1 || nprob > (1 << 29) || (sense != 1 && sense != -1) || !blen || !blimbs || !best || !nties || !neligible ||
        !ninexact || !rlen_out || !rlimbs_out || !rnl_out || !dlen_out || !dlimbs_out || !dnl_out)
        return SLIP_HIP_INCORRECT_INPUT;
    return update_on_handle(f, 1, transpose, nprob, blen, blimbs, NULL, NULL, NULL, NULL, NULL, sense, key, best, nties, neligible, ninexact,
                            rlen_out, rlimbs_out, rnl_out, dlen_out, dlimbs_out, dnl_out, (hipStream_t) stream_v);
}

extern "C" int slip_hip_factor_update_ms(const slip_hip_factor *f, double out[2])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->update_ms, sizeof f->update_ms);
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_factor_update_paths(const slip_hip_factor *f, int64_t out[8])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->update_paths, sizeof f->update_paths);
    return SLIP_HIP_OK;
}

/* ---- the bounded step: the bounded ratio test, the comparison of the winning step with the entering variable's own range,
 * and the update of all n numerators -- a pivot or a bound flip -- with no numerator crossing the host in between (no
 * counterpart in the reference; kernels: slip_bound_kernel, slip_ratio_kernel, slip_bstep_kernel, slip_pivot_kernel;
 * DESIGN 3o) ---- */

/* the counts and passes of this thread's last handle-less bounded step */
static thread_local int64_t slip_bstep_paths_last[20];
static thread_local double slip_bstep_ms_last[4];

/* the entering variables' data checked and laid out on the host */
struct SlipHostEntering { SlipSlab er, ev; int any_finite, has_ev; };
static void host_entering_free(SlipHostEntering *h) { slab_free(&h->er); slab_free(&h->ev); }
static int host_entering(int32_t nprob, const slip_hip_entering *En, SlipHostEntering *h)
{
    memset(h, 0, sizeof *h);
    if (!En) return SLIP_HIP_OK;
    if (En->finite) for (int32_t c = 0; c < nprob; c++) {
        if (En->finite[c] != 0 && En->finite[c] != 1) return SLIP_HIP_INCORRECT_INPUT;
        h->any_finite |= En->finite[c];
    }
    if ((h->any_finite && (!En->erlen || !En->erlimbs)) || !En->evlen != !En->evlimbs) return SLIP_HIP_INCORRECT_INPUT;
    int rc = h->any_finite ? slab_prepare(nprob, En->erlen, En->erlimbs, En->er_limbs, &h->er) : 0;
    for (int32_t c = 0; c < nprob && !rc && h->any_finite; c++) if (En->finite[c] && h->er.dig[c] < 0) rc = SLIP_HIP_INCORRECT_INPUT;
    if (!rc && En->evlen) { rc = slab_prepare(nprob, En->evlen, En->evlimbs, En->ev_limbs, &h->ev); h->has_ev = !rc; }
    if (rc) host_entering_free(h);
    return rc;
}

/* E_c into the slot best[c] of every problem that pivots: the result slab (signed limb counts rl, limbs *rv of *rn) rebuilt */
static int bstep_place(int32_t n, int32_t nprob, const int32_t *best, const int32_t *move, const int32_t *el, const uint64_t *ev,
                       int32_t *rl, uint64_t **rv, int64_t *rn)
{
    auto mag = [](int32_t l) { return (int64_t)(l < 0 ? -l : l); };
    int64_t total = *rn;
    for (int32_t c = 0; c < nprob; c++) if (move[c] == 1) total += mag(el[c]) - mag(rl[(int64_t) c * n + best[c]]);
    uint64_t *out = (uint64_t *) malloc((size_t)(total > 0 ? total : 1) * 8);
    if (!out) return SLIP_HIP_OUT_OF_MEMORY;
    int64_t so = 0, dn = 0, eo = 0;
    for (int32_t c = 0; c < nprob; c++) {
        const int32_t r = move[c] == 1 ? best[c] : -1;
        for (int32_t i = 0; i < n; i++) {
            int32_t *l = rl + (int64_t) c * n + i;
            if (i == r) {
                so += mag(*l);
                memcpy(out + dn, ev + eo, (size_t) mag(el[c]) * 8); dn += mag(el[c]);
                *l = el[c];
            } else { memcpy(out + dn, *rv + so, (size_t) mag(*l) * 8); so += mag(*l); dn += mag(*l); }
        }
        eo += mag(el[c]);
    }
    free(*rv);
    *rv = out; *rn = total;
    return SLIP_HIP_OK;
}

/* one bounded step on the device: the operands as bound_core takes them (mode 0), the entering data as host_entering left
 * them.  res: 4 * nprob host integers (best, nties, neligible, side); move, ninexact: nprob each; R: n * nprob entries in
 * reported order, Dn and E: nprob entries each, compact malloc'ed slabs.  ms: the selection's form passes, the selection,
 * slip_bstep_kernel, the update; paths: bound_core's eight counts, pivot_core's five, the problems by move (0, 1, 2), the
 * scalars slip_bstep_kernel formed by path (4). */
static int bstep_core(const SlipBoundIn &I, const slip_hip_bounds *B, const SlipHostBounds &hb,
                      const slip_hip_entering *En, const SlipHostEntering &he, const int32_t *key,
                      int32_t *res, int32_t *move, int32_t *ninexact,
                      int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out,
                      int32_t **nlen_out, uint64_t **nlimbs_out, int64_t *nnl_out,
                      int32_t **elen_out, uint64_t **elimbs_out, int64_t *enl_out,
                      hipStream_t stream, double ms[4], int64_t paths[20])
{
    const int32_t n = I.n, nprob = I.nprob;
    int32_t *dnlen = NULL, *darlen = NULL, *derr = NULL, *dwmax = NULL, *dbest = NULL, *dfin = NULL, *drlen = NULL, *dplace = NULL, *dmove = NULL;
    int64_t *daroff = NULL, *droff = NULL; uint64_t *dnslab = NULL, *dbd = NULL, *dslab = NULL;
    unsigned long long *dpaths = NULL, hpaths[4] = {0, 0, 0, 0};
    dig_t *dscr = NULL;
    SlipDevSlab er, ev; memset(&er, 0, sizeof er); memset(&ev, 0, sizeof ev);
    int32_t hwmax[2] = {0, 0}, herr = 0;
    int32_t *hmove = (int32_t *) malloc((size_t) nprob * 4), *hres = (int32_t *) malloc((size_t) nprob * 16), *hnin = (int32_t *) malloc((size_t) nprob * 4);
    int32_t *rl = NULL, *nl = NULL, *el = NULL; uint64_t *rv = NULL, *nv = NULL, *evv = NULL; int64_t rn = 0, nn = 0, en = 0;
    int64_t nstride = 0;
    double bms[2] = {0, 0}, pms = 0, sms = 0; int64_t bpaths[8], ppaths[8];
    int rc = !hmove || !hres || !hnin ? SLIP_HIP_OUT_OF_MEMORY : 0;
    const int64_t bdn = ((int64_t) hb.bddig + 1) >> 1;
    A_(dev_alloc(&dnlen, nprob)); A_(dev_alloc(&darlen, nprob)); A_(dev_alloc(&daroff, nprob)); A_(dev_alloc(&derr, 1)); A_(dev_alloc(&dwmax, 2));
    A_(dev_alloc(&dpaths, 4)); A_(dev_alloc(&dbest, nprob)); A_(dev_alloc(&drlen, 5 * (int64_t) nprob)); A_(dev_alloc(&droff, 5 * (int64_t) nprob));
    A_(dev_alloc(&dplace, nprob)); A_(dev_alloc(&dmove, nprob));
    A_(dev_alloc(&dbd, bdn + 1)); UP_(dbd, B->bdlimbs ? B->bdlimbs : &hb.one, (size_t) bdn * 8); UP_(dbd + bdn, &hb.one, 8);
    if (he.any_finite) {
        A_(dev_alloc(&dfin, nprob)); UP_(dfin, En->finite, (size_t) nprob * 4);
        A_(dev_slab_put(nprob, he.er, En->erlimbs, &er));
    }
    if (he.has_ev) A_(dev_slab_put(nprob, he.ev, En->evlimbs, &ev));
    HIP_(hipMemsetAsync(derr, 0, 4, stream)); HIP_(hipMemsetAsync(dwmax, 0, 8, stream)); HIP_(hipMemsetAsync(dpaths, 0, 32, stream));
    SlipBstepArgs S; memset(&S, 0, sizeof S);
    S.sense = I.sense; S.alimbs = I.a.limbs; S.dlimbs = I.d.limbs; S.bddig = hb.bddig; S.bdlimbs = dbd; S.one = dbd + bdn;
    S.erlimbs = er.limbs; S.evlimbs = ev.limbs; S.wmax = dwmax; S.err = derr; S.paths = dpaths;
    /* the winners of a group into slabs that outlive its staging slab */
    const SlipBoundCapture capture = [&](int64_t c0, int64_t nv, int64_t wcap, const int32_t *wnl, const int64_t *wno, const uint64_t *dstage,
                                         const int32_t *wal, const int64_t *wao) {
        int rc = 0;
        double t = 0;
        if (!dnslab) { nstride = wcap / 2; A_(dev_alloc(&dnslab, nprob * nstride)); }
        SlipBstepArgs C = S;
        C.nprob = (int32_t) nv; C.phase = 0; C.wnlen = wnl; C.wnoff = wno; C.walen = wal; C.waoff = wao; C.stage = dstage;
        C.nlen = dnlen + c0; C.nslab = dnslab + c0 * nstride; C.nstride = nstride; C.arlen = darlen + c0; C.aroff = daroff + c0;
        SlipTimed timed;
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(bstep, wave_blocks(nv), stream, C));
        A_(timed.end(stream, &t));
        sms += t;
        return rc;
    };
    A_(bound_core(I, B, hb, key, hres, NULL, NULL, NULL, stream, bms, bpaths, &capture));
    UP_(dbest, hres, (size_t) nprob * 4);
    S.nprob = nprob; S.nlen = dnlen; S.nslab = dnslab; S.nstride = nstride; S.arlen = darlen; S.aroff = daroff;
    S.dlen = I.d.len; S.doff = I.d.off; S.best = dbest; S.finite = dfin;
    S.erlen = er.len; S.eroff = er.off; S.evlen = ev.len; S.evoff = ev.off;
    S.rlen = drlen; S.roff = droff; S.rstride = nprob; S.place = dplace; S.move = dmove;
    if (!rc) {                                             /* the widths of every scalar either move may need */
        SlipTimed timed;
        double t = 0;
        S.phase = 1;
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(bstep, wave_blocks(nprob), stream, S));
        A_(timed.end(stream, &t));
        sms += t;
    }
    DOWN_(hwmax, dwmax, 8);
    const int64_t stride = hwmax[0] > 1 ? ((int64_t) hwmax[0] + 1) >> 1 : 1, scap = ((int64_t) hwmax[1] + 1) & ~(int64_t) 1;
    if (!rc && (stride > (1 << 27) || scap > (1 << 27))) rc = SLIP_HIP_OUT_OF_MEMORY;
    const int64_t sblocks = hwmax[1] > 0 ? fit_scratch(wave_blocks(nprob), 2 * scap) : wave_blocks(nprob);
    if (hwmax[1] > 0) { A_(dev_alloc(&dscr, sblocks * SERVICE_WAVES * 2 * scap)); S.scratch = dscr; S.wcap = (int32_t) scap; }
    A_(dev_alloc(&dslab, 5 * (int64_t) nprob * stride));
    S.slab = dslab; S.stride = stride;
    if (!rc) {                                             /* the move and its records */
        SlipTimed timed;
        double t = 0;
        S.phase = 2;
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(bstep, sblocks, stream, S));
        A_(timed.end(stream, &t));
        sms += t;
    }
    DOWN_(&herr, derr, 4); DOWN_(hmove, dmove, (size_t) nprob * 4); DOWN_(hpaths, dpaths, 32);
    if (!rc && herr) rc = SLIP_HIP_DEVICE_ERROR;                                    /* a scalar wider than phase 1 sized it */
    SlipPivotIn U; memset(&U, 0, sizeof U);
    U.n = n; U.nprob = nprob; U.oidx = I.oidx; U.pos = I.pos; U.place = dplace;
    U.v = I.x; U.vstride = I.xstride; U.a = I.a; U.astride = I.astride;
    U.p.len = drlen; U.p.off = droff; U.t.len = drlen + nprob; U.t.off = droff + nprob; U.d.len = drlen + 2 * (int64_t) nprob; U.d.off = droff + 2 * (int64_t) nprob;
    U.p.limbs = U.t.limbs = U.d.limbs = dslab;
    A_(pivot_core(U, hnin, &rl, &rv, &rn, stream, &pms, ppaths));
    A_(pack_download(nprob, drlen + 4 * (int64_t) nprob, droff + 4 * (int64_t) nprob, dslab, 0, &nl, &nv, &nn, stream));
    A_(pack_download(nprob, drlen + 3 * (int64_t) nprob, droff + 3 * (int64_t) nprob, dslab, 0, &el, &evv, &en, stream));
    A_(bstep_place(n, nprob, hres, hmove, el, evv, rl, &rv, &rn));
    if (!rc) {
        memcpy(res, hres, (size_t) nprob * 16); memcpy(move, hmove, (size_t) nprob * 4); memcpy(ninexact, hnin, (size_t) nprob * 4);
        *rlen_out = rl; *rlimbs_out = rv; *rnl_out = rn; *nlen_out = nl; *nlimbs_out = nv; *nnl_out = nn; *elen_out = el; *elimbs_out = evv; *enl_out = en;
        rl = nl = el = NULL; rv = nv = evv = NULL;
        ms[0] = bms[0]; ms[1] = bms[1]; ms[2] = sms; ms[3] = pms;
        memset(paths, 0, 20 * sizeof(int64_t));
        memcpy(paths, bpaths, sizeof bpaths); memcpy(paths + 8, ppaths, 5 * sizeof(int64_t));
        for (int32_t c = 0; c < nprob; c++) paths[13 + hmove[c]]++;
        for (int k = 0; k < 4; k++) paths[16 + k] = (int64_t) hpaths[k];
    }
    free(hmove); free(hres); free(hnin); free(rl); free(rv); free(nl); free(nv); free(el); free(evv);
    dev_slab_free(&er); dev_slab_free(&ev);
    dev_free(dnlen); dev_free(darlen); dev_free(daroff); dev_free(derr); dev_free(dwmax); dev_free(dpaths); dev_free(dbest); dev_free(dfin);
    dev_free(drlen); dev_free(droff); dev_free(dplace); dev_free(dmove); dev_free(dnslab); dev_free(dbd); dev_free(dslab); dev_free(dscr);
    return rc;
}

/* the outputs of a bounded step: all required */
static int bstep_outputs_bad(const int32_t *best, const int32_t *nties, const int32_t *neligible, const int32_t *side, const int32_t *move,
                             const int32_t *ninexact, int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out,
                             int32_t **nlen_out, uint64_t **nlimbs_out, int64_t *nnl_out, int32_t **elen_out, uint64_t **elimbs_out, int64_t *enl_out)
{
    return !best || !nties || !neligible || !side || !move || !ninexact || !rlen_out || !rlimbs_out || !rnl_out ||
           !nlen_out || !nlimbs_out || !nnl_out || !elen_out || !elimbs_out || !enl_out;
}

extern "C" int slip_hip_factor_step_bounded(slip_hip_factor *f, int32_t transpose, int32_t nprob, const int32_t *blen, const uint64_t *blimbs,
                                            const slip_hip_bounds *bounds, const slip_hip_entering *entering, int32_t sense, const int32_t *key,
                                            int32_t *best, int32_t *nties, int32_t *neligible, int32_t *side, int32_t *move, int32_t *ninexact,
                                            int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out,
                                            int32_t **dnlen_out, uint64_t **dnlimbs_out, int64_t *dnnl_out,
                                            int32_t **elen_out, uint64_t **elimbs_out, int64_t *enl_out, void *stream_v)
{
    if (!f || nprob < 1 || nprob > (1 << 27) || (sense != 1 && sense != -1) || !blen || !blimbs || !bounds || !bounds->kind ||
        bstep_outputs_bad(best, nties, neligible, side, move, ninexact, rlen_out, rlimbs_out, rnl_out, dnlen_out, dnlimbs_out, dnnl_out,
                          elen_out, elimbs_out, enl_out))
        return SLIP_HIP_INCORRECT_INPUT;
    if (!transpose && f->factors_only) return SLIP_HIP_INCORRECT_INPUT;             /* no q behind such a handle */
    if (f->broken) return SLIP_HIP_DEVICE_ERROR;
    if (f->hs.F != f->n) return SLIP_HIP_INCORRECT_INPUT;       /* needs the complete factorisation */
    const int32_t n = f->n;
    hipStream_t stream = (hipStream_t) stream_v;
    SlipHostBounds hb; SlipHostEntering he;
    TRY_(host_bounds(n, bounds, &hb));
    int rc = host_entering(nprob, entering, &he);
    if (rc) { host_bounds_free(&hb); return rc; }
    SlipSolveOut o;
    rc = solve_device(f, transpose, 2 * nprob, blen, blimbs, stream, &o);
    if (rc) { host_bounds_free(&hb); host_entering_free(&he); return rc; }
    int32_t *ddlen = NULL, *doidx = NULL, *dpos = NULL, *res = (int32_t *) malloc((size_t) nprob * 16); int64_t *ddoff = NULL;
    int32_t dmaxdig = 0;
    if (!res) rc = SLIP_HIP_OUT_OF_MEMORY;
    A_(det_records(f, nprob, &ddlen, &ddoff, &dmaxdig));
    A_(transposed_maps(f, transpose, &doidx, &dpos));
    SlipBoundIn I; memset(&I, 0, sizeof I);
    I.n = n; I.nprob = nprob; I.mode = 0; I.sense = sense; I.oidx = doidx; I.pos = dpos;
    I.x.len = o.olen; I.x.off = o.ooff; I.x.limbs = o.olimbs; I.xstride = 2 * (int64_t) n;
    I.a.len = o.olen + n; I.a.off = o.ooff + n; I.a.limbs = o.olimbs; I.astride = 2 * (int64_t) n;
    I.d.len = ddlen; I.d.off = ddoff; I.d.limbs = f->P.Llimbs;
    double ms[4]; int64_t paths[20];
    A_(bstep_core(I, bounds, hb, entering, he, key, res, move, ninexact, rlen_out, rlimbs_out, rnl_out, dnlen_out, dnlimbs_out, dnnl_out,
                  elen_out, elimbs_out, enl_out, stream, ms, paths));
    if (!rc) {
        results_out(res, nprob, best, nties, neligible, side);
        memcpy(f->bstep_ms, ms, sizeof ms); memcpy(f->bstep_paths, paths, sizeof paths);
    }
    free(res); dev_free(doidx); dev_free(dpos); dev_free(ddlen); dev_free(ddoff);
    solve_out_free(&o);
    host_bounds_free(&hb); host_entering_free(&he);
    return rc;
}

extern "C" int slip_hip_step_bounded(int32_t n, int32_t nprob, const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                     const int32_t *alen, const uint64_t *alimbs, int64_t a_limbs,
                                     const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                                     const slip_hip_bounds *bounds, const slip_hip_entering *entering, int32_t sense, const int32_t *key,
                                     int32_t *best, int32_t *nties, int32_t *neligible, int32_t *side, int32_t *move, int32_t *ninexact,
                                     int32_t **rlen_out, uint64_t **rlimbs_out, int64_t *rnl_out,
                                     int32_t **dnlen_out, uint64_t **dnlimbs_out, int64_t *dnnl_out,
                                     int32_t **elen_out, uint64_t **elimbs_out, int64_t *enl_out, void *stream_v)
{
    if (n <= 0 || nprob < 1 || nprob > (1 << 27) || (sense != 1 && sense != -1) || !xlen || !xlimbs || !alen || !alimbs || !dlen || !dlimbs ||
        !bounds || !bounds->kind ||
        bstep_outputs_bad(best, nties, neligible, side, move, ninexact, rlen_out, rlimbs_out, rnl_out, dnlen_out, dnlimbs_out, dnnl_out,
                          elen_out, elimbs_out, enl_out))
        return SLIP_HIP_INCORRECT_INPUT;
    const int64_t ne = (int64_t) n * nprob;
    SlipHostBounds hb; SlipHostEntering he;
    TRY_(host_bounds(n, bounds, &hb));
    int rc = host_entering(nprob, entering, &he);
    if (rc) { host_bounds_free(&hb); return rc; }
    SlipDevSlab x, a, d; memset(&x, 0, sizeof x); memset(&a, 0, sizeof a); memset(&d, 0, sizeof d);
    int32_t *res = NULL;
    /* (every slab is checked against its capacity before a limb of it is read, and all of them before the device is asked for) */
    A_(slab_prepare(nprob, dlen, dlimbs, d_limbs, &d.s));
    for (int32_t c = 0; c < nprob && !rc; c++) if (d.s.dig[c] == 0) rc = SLIP_HIP_INCORRECT_INPUT;
    A_(slab_prepare(ne, xlen, xlimbs, x_limbs, &x.s));
    A_(slab_prepare(ne, alen, alimbs, a_limbs, &a.s));
    A_(need_device());
    A_(dev_slab_put(nprob, d.s, dlimbs, &d)); A_(dev_slab_put(ne, x.s, xlimbs, &x)); A_(dev_slab_put(ne, a.s, alimbs, &a));
    if (!rc && !(res = (int32_t *) malloc((size_t) nprob * 16))) rc = SLIP_HIP_OUT_OF_MEMORY;
    SlipBoundIn I; memset(&I, 0, sizeof I);
    I.n = n; I.nprob = nprob; I.mode = 0; I.sense = sense; I.xstride = n; I.astride = n;
    I.x = dev_slab_recs(x); I.a = dev_slab_recs(a); I.d = dev_slab_recs(d);
    double ms[4]; int64_t paths[20];
    A_(bstep_core(I, bounds, hb, entering, he, key, res, move, ninexact, rlen_out, rlimbs_out, rnl_out, dnlen_out, dnlimbs_out, dnnl_out,
                  elen_out, elimbs_out, enl_out, (hipStream_t) stream_v, ms, paths));
    if (!rc) {
        results_out(res, nprob, best, nties, neligible, side);
        memcpy(slip_bstep_ms_last, ms, sizeof ms); memcpy(slip_bstep_paths_last, paths, sizeof paths);
    }
    free(res);
    dev_slab_free(&x); dev_slab_free(&a); dev_slab_free(&d);
    host_bounds_free(&hb); host_entering_free(&he);
    return rc;
}

extern "C" int slip_hip_factor_step_bounded_ms(const slip_hip_factor *f, double out[4])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->bstep_ms, sizeof f->bstep_ms);
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_factor_step_bounded_paths(const slip_hip_factor *f, int64_t out[20])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->bstep_paths, sizeof f->bstep_paths);
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_step_bounded_paths(int64_t out[20])
{
    if (!out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, slip_bstep_paths_last, sizeof slip_bstep_paths_last);
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_step_bounded_ms(double out[4])
{
    if (!out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, slip_bstep_ms_last, sizeof slip_bstep_ms_last);
    return SLIP_HIP_OK;
}

/* ---- exact pricing: the entering column (Dantzig) or the dual ratio test chosen on the device, fused from the transposed
 * substitution (slip_solve_kernel on the view), the products with a resident matrix (slip_product_kernel) and the selection
 * (slip_ratio_kernel), joined by slip_price_kernel's records; no numerator leaves the device (no counterpart in the reference;
 * DESIGN 3k) ---- */

/* det * g of a pricing call: the cost vectors' records (gs: nprob * ncols, laid out by the host) on the x side of every problem,
 * empty records on its a side (nside 2), and the limbs as they came, into dg (zeroed) */
static int price_costs_put(int32_t nside, int32_t nprob, int32_t ncols, const SlipSlab &gs, const uint64_t *glimbs, SlipDevSlab *dg)
{
    const int64_t ne = (int64_t) ncols * nside * nprob;
    int32_t *hl = (int32_t *) calloc((size_t) ne, 4); int64_t *ho = (int64_t *) calloc((size_t) ne, 8);
    int rc = !hl || !ho ? SLIP_HIP_OUT_OF_MEMORY : 0;
    if (!rc) for (int32_t c = 0; c < nprob; c++) {
        memcpy(hl + (int64_t) nside * c * ncols, gs.dig + (int64_t) c * ncols, (size_t) ncols * 4);
        memcpy(ho + (int64_t) nside * c * ncols, gs.off + (int64_t) c * ncols, (size_t) ncols * 8);
    }
    A_(dev_alloc(&dg->len, ne)); A_(dev_alloc(&dg->off, ne)); A_(dev_alloc(&dg->limbs, gs.total));
    UP_(dg->len, hl, (size_t) ne * 4); UP_(dg->off, ho, (size_t) ne * 8); UP_(dg->limbs, glimbs, (size_t) gs.total * 8);
    free(hl); free(ho);
    return rc;
}

extern "C" int slip_hip_factor_price(slip_hip_factor *f, slip_hip_matrix *M, int32_t nside, int32_t nprob,
                                     const int32_t *blen, const uint64_t *blimbs,
                                     const int32_t *glen, const uint64_t *glimbs, int64_t g_limbs,
                                     int32_t sense, const int32_t *key,
                                     int32_t *best, int32_t *nties, int32_t *neligible, int32_t *vsign,
                                     int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream_v)
{
    if (!f || !M || !blen || !blimbs || !best || !nties || !neligible || !vsign || (nside != 1 && nside != 2) || nprob < 1 ||
        nprob > (1 << 29) || (sense != 1 && sense != -1) || !glen != !glimbs)
        return SLIP_HIP_INCORRECT_INPUT;
    if (winners_args_bad(wlen_out, wlimbs_out, wnl_out)) return SLIP_HIP_INCORRECT_INPUT;
    if (M->m != f->n) return SLIP_HIP_INCORRECT_INPUT;
    if (f->broken) return SLIP_HIP_DEVICE_ERROR;
    if (f->hs.F != f->n) return SLIP_HIP_INCORRECT_INPUT;       /* needs the complete factorisation */
    const int32_t n = f->n, ncols = M->ncols, nvec = nside * nprob;
    const int64_t nxe = (int64_t) n * nvec;
    hipStream_t stream = (hipStream_t) stream_v;
    SlipSlab gs; memset(&gs, 0, sizeof gs);
    if (glen) TRY_(slab_prepare((int64_t) nprob * ncols, glen, glimbs, g_limbs, &gs));
    if (wlen_out) { *wlen_out = NULL; *wlimbs_out = NULL; *wnl_out = 0; }
    SlipSolveOut o;
    int rc = solve_device(f, 1, nvec, blen, blimbs, stream, &o);
    if (rc) { slab_free(&gs); return rc; }
    int32_t *dxl = NULL, *ddlen = NULL, *dsel = NULL, *dwl = NULL; int64_t *dxo = NULL, *ddoff = NULL, *dwo = NULL;
    SlipDevSlab dg; memset(&dg, 0, sizeof dg);
    int32_t dmaxdig = 0;
    /* the result on the host until all of it stands: best, nties, neligible, vsign, nprob each */
    int32_t *hres = (int32_t *) malloc((size_t) nprob * 16), *wl = wlen_out ? (int32_t *) malloc((size_t) nprob * 8) : NULL;
    uint64_t *wv = NULL; int64_t wn = 0;
    double gather_ms = 0, ms[4] = {0, 0, 0, 0};
    int64_t paths[4] = {0, 0, 0, 0};
    if (!hres || (wlen_out && !wl)) rc = SLIP_HIP_OUT_OF_MEMORY;
    /* the sign of det: it decides the eligible sign of A, the direction of X and vsign */
    int dneg = 0;
    A_(det_negative(f, &dneg));
    /* y by row id: the records of the substitution's output gathered through pinv, its limbs where they are */
    A_(dev_alloc(&dxl, nxe)); A_(dev_alloc(&dxo, nxe));
    if (!rc) {
        SlipTimed timed;
        SlipPriceArgs G; memset(&G, 0, sizeof G);
        G.phase = 0; G.n = n; G.count = nxe; G.pinv = f->P.pinv.p_; G.olen = o.olen; G.ooff = o.ooff; G.xlen = dxl; G.xoff = dxo;
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(price, service_blocks(nxe), stream, G));
        A_(timed.end(stream, &gather_ms));
    }
    /* det * g: the cost vector's records on the x side of every problem, empty records on its a side */
    if (glen) {
        A_(price_costs_put(nside, nprob, ncols, gs, glimbs, &dg));
        A_(det_records(f, nvec, &ddlen, &ddoff, &dmaxdig));
    }
    /* per group: best (up), vsign (down), and without denominators the winners' records */
    A_(dev_alloc(&dsel, 2 * (int64_t) nprob));
    if (wlen_out && nside == 1) { A_(dev_alloc(&dwl, 2 * (int64_t) nprob)); A_(dev_alloc(&dwo, 2 * (int64_t) nprob)); }
    SlipProductView V;
    V.nout = ncols; V.nx = n; V.alen = M->dAlen; V.aoff = M->dAoff; V.alimbs = M->dAlimbs; V.amaxdig = M->amaxdig;
    V.rp = M->col_rp; V.re = M->col_re; V.rx = M->col_rx;
    const SlipDevRecs x = {dxl, dxo, o.olimbs}, g = dev_slab_recs(dg);
    /* the selection on a group of whole problems, on the staged records: X of problem c at c * pstride, A (nside 2) ncols on */
    auto select = [&](int64_t c0, int64_t nv, const int32_t *rlen, const int64_t *soff, const uint64_t *stage, double *t) {
        const int64_t p0 = c0 / nside;
        const int32_t np = (int32_t)(nv / nside);
        const int pair = wlen_out && nside == 2, single = wlen_out && nside == 1;
        int32_t *gwl = NULL; uint64_t *gwv = NULL; int64_t gwn = 0, gp[4] = {0, 0, 0, 0};
        SlipRatioArgs R; memset(&R, 0, sizeof R);
        R.n = ncols; R.nprob = np; R.pstride = (int64_t) nside * ncols;
        R.xlen = rlen; R.xoff = soff; R.xlimbs = stage;
        if (nside == 2) { R.alen = rlen + ncols; R.aoff = soff + ncols; R.alimbs = stage; R.asense = dneg ? -sense : sense; R.xflip = dneg; }
        else R.xflip = (sense < 0) != (dneg != 0);
        int rc = ratio_core(R, key, hres + p0, hres + nprob + p0, hres + 2 * (int64_t) nprob + p0,
                            pair ? &gwl : NULL, pair ? &gwv : NULL, pair ? &gwn : NULL, stream, t, gp);
        int32_t *dbest = dsel, *dvs = dsel + nprob;
        UP_(dbest, hres + p0, (size_t) np * 4);
        if (!rc) {
            SlipPriceArgs Q; memset(&Q, 0, sizeof Q);
            Q.phase = 2; Q.count = np; Q.pstride = R.pstride; Q.dneg = dneg; Q.best = dbest; Q.rlen = rlen; Q.soff = soff; Q.vsign = dvs;
            if (single) { Q.wlen = dwl; Q.woff = dwo; }
            A_(SERVICE_LAUNCH(price, service_blocks(np), stream, Q));
            HIP_(hipStreamSynchronize(stream));
        }
        DOWN_(hres + 3 * (int64_t) nprob + p0, dvs, (size_t) np * 4);
        if (single) A_(pack_download(2 * (int64_t) np, dwl, dwo, stage, 0, &gwl, &gwv, &gwn, stream));
        if (!rc && wlen_out) {
            uint64_t *grown = (uint64_t *) realloc(wv, (size_t)(wn + gwn > 0 ? wn + gwn : 1) * 8);
            if (!grown) rc = SLIP_HIP_OUT_OF_MEMORY;
            else {
                wv = grown;
                memcpy(wl + 2 * p0, gwl, (size_t) np * 8);
                if (gwn > 0) memcpy(wv + wn, gwv, (size_t) gwn * 8);
                wn += gwn;
            }
        }
        if (!rc) for (int k = 0; k < 4; k++) paths[k] += gp[k];
        free(gwl); free(gwv);
        return rc;
    };
    A_(product_device(V, nvec, x, -1, glen ? &g : NULL, gs.maxdig, ddlen, ddoff, f->P.Llimbs, dmaxdig, nside, select, stream, ms));
    dev_free(dxl); dev_free(dxo); dev_free(ddlen); dev_free(ddoff); dev_free(dsel); dev_free(dwl); dev_free(dwo);
    dev_slab_free(&dg);
    slab_free(&gs);
    solve_out_free(&o);
    if (!rc) {
        results_out(hres, nprob, best, nties, neligible, vsign);
        if (wlen_out) { *wlen_out = wl; *wlimbs_out = wv; *wnl_out = wn; wl = NULL; wv = NULL; }
        ms[0] += gather_ms;
        memcpy(f->price_ms, ms, sizeof ms); memcpy(f->price_paths, paths, sizeof paths);
    }
    free(hres); free(wl); free(wv);
    return rc;
}

extern "C" int slip_hip_factor_price_ms(const slip_hip_factor *f, double out[4])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->price_ms, sizeof f->price_ms);
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_factor_price_paths(const slip_hip_factor *f, int64_t out[4])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->price_paths, sizeof f->price_paths);
    return SLIP_HIP_OK;
}

/* ---- nonbasic states and reference weights in exact pricing: the entering column of a boxed LP (at lower, at upper, free,
 * never) under Dantzig's rule or reference weights (the largest X_j^2 / w_j), and the dual ratio test with the mirror rule
 * on the sign of A_j; the records formed on the device, the selection slip_ratio_kernel's as it stands (no counterpart in
 * the reference; kernel: slip_states_kernel) ---- */

/* the counts of this thread's last slip_hip_price_select */
static thread_local int64_t slip_states_paths_last[8];

/* the states and weights of a call checked on the host: ws receives the weights' layout (untouched without weights) */
static int states_check(int32_t ncols, int32_t nside, const int32_t *state, const int32_t *wlen, const uint64_t *wlimbs, int64_t w_limbs,
                        SlipSlab *ws)
{
    memset(ws, 0, sizeof *ws);
    if (!state || !wlen != !wlimbs || (wlen && nside != 1)) return SLIP_HIP_INCORRECT_INPUT;
    for (int32_t j = 0; j < ncols; j++) if (state[j] < 0 || state[j] > 3) return SLIP_HIP_INCORRECT_INPUT;
    if (!wlen) return SLIP_HIP_OK;
    TRY_(slab_prepare(ncols, wlen, wlimbs, w_limbs, ws));
    for (int32_t j = 0; j < ncols; j++) if (ws->dig[j] <= 0) { slab_free(ws); return SLIP_HIP_INCORRECT_INPUT; }
    return SLIP_HIP_OK;
}

/* the same on the device: the states, the weights' records and limbs (NULL without weights), one limb holding 1 */
struct SlipStatesOps { int32_t *state; SlipDevSlab wt; uint64_t *one; };
static void states_ops_free(SlipStatesOps *o)
{
    dev_free(o->state); dev_slab_free(&o->wt); dev_free(o->one);
    memset(o, 0, sizeof *o);
}
static int states_upload(int32_t ncols, const int32_t *state, const SlipSlab *ws, const uint64_t *wlimbs, SlipStatesOps *o)
{
    const uint64_t one = 1;
    int rc = 0;
    memset(o, 0, sizeof *o);
    A_(dev_alloc(&o->state, ncols)); UP_(o->state, state, (size_t) ncols * 4);
    A_(dev_alloc(&o->one, 1)); UP_(o->one, &one, 8);
    if (ws->dig) A_(dev_slab_put(ncols, *ws, wlimbs, &o->wt));
    if (rc) states_ops_free(o);
    return rc;
}

/* the device operands of one selection with states: X (and A, nside 2) of problem c from entry c * stride on, the record of
 * d_c as entry c of d (its sign is all that is read) */
struct SlipStatesIn {
    int32_t n, nprob, nside, sense;
    SlipDevRecs x, a; int64_t xstride, astride;
    const int32_t *dlen;
};

/* one selection with states on the device.  r0 .. r3 (host) receive best, nties, neligible and vsign of the nprob problems;
 * with wl the winners' records are appended to wl / wv, X_best and A_best of every problem (signed limb counts).  ms (the
 * classify, offset and square passes; the selection) and paths are added to. */
static int states_core(const SlipStatesIn &I, const SlipStatesOps &O, const int32_t *key, int32_t *r0, int32_t *r1, int32_t *r2, int32_t *r3,
                       std::vector<int32_t> *wl, std::vector<uint64_t> *wv, hipStream_t stream, double ms[2], int64_t paths[8])
{
    const int32_t n = I.n, nprob = I.nprob;
    const int weighted = O.wt.len != NULL;
    const int64_t ne = (int64_t) n * nprob, rpp = ((int64_t) n + SLIP_WAVE - 1) / SLIP_WAVE;
    int32_t *dxl2 = NULL, *dal2 = NULL, *dcls = NULL, *dw = NULL, *dwmax = NULL, *dsel = NULL, *dwn = NULL;
    int64_t *dxo2 = NULL, *dao2 = NULL, *dso = NULL, *dwo = NULL;
    unsigned long long *dpaths = NULL, hpaths[4] = {0, 0, 0, 0};
    int32_t hwmax = 0;
    int rc = 0;
    A_(dev_alloc(&dxl2, ne)); A_(dev_alloc(&dxo2, ne)); A_(dev_alloc(&dal2, ne)); A_(dev_alloc(&dao2, ne));
    A_(dev_alloc(&dpaths, 4)); A_(dev_alloc(&dsel, 2 * (int64_t) nprob));
    if (weighted) { A_(dev_alloc(&dcls, ne)); A_(dev_alloc(&dw, ne)); A_(dev_alloc(&dso, ne)); A_(dev_alloc(&dwmax, 1)); }
    if (wl) { A_(dev_alloc(&dwn, 2 * (int64_t) nprob)); A_(dev_alloc(&dwo, 2 * (int64_t) nprob)); }
    HIP_(hipMemsetAsync(dpaths, 0, 32, stream));
    if (weighted) HIP_(hipMemsetAsync(dwmax, 0, 4, stream));
    SlipStatesArgs A; memset(&A, 0, sizeof A);
    A.n = n; A.nside = I.nside; A.sense = I.sense; A.weighted = weighted; A.xstride = I.xstride; A.astride = I.astride;
    A.xlimbs = I.x.limbs; A.alimbs = I.a.limbs; A.state = O.state; A.wtlen = O.wt.len; A.wtoff = O.wt.off;
    A.wmax = dwmax; A.paths = dpaths;
    /* the problems c0 .. c0 + nv of every per-problem and per-entry array */
    auto slice = [&](int64_t c0, int64_t nv, int phase) {
        A.nprob = (int32_t) nv; A.phase = phase;
        A.xlen = I.x.len + c0 * I.xstride; A.xoff = I.x.off + c0 * I.xstride;
        A.alen = I.a.len ? I.a.len + c0 * I.astride : NULL; A.aoff = I.a.off ? I.a.off + c0 * I.astride : NULL;
        A.dlen = I.dlen + c0;
        A.xlen2 = dxl2 + c0 * n; A.xoff2 = dxo2 + c0 * n; A.alen2 = dal2 + c0 * n; A.aoff2 = dao2 + c0 * n;
        A.cls = weighted ? dcls + c0 * n : NULL; A.w = weighted ? dw + c0 * n : NULL; A.soff = weighted ? dso + c0 * n : NULL;
    };
    if (!rc) {                                             /* the records of all entries (with weights: their classes and widths) */
        SlipTimed timed;
        double t = 0;
        slice(0, nprob, 0);
        A_(timed.begin(stream));
        A_(SERVICE_LAUNCH(states, wave_blocks(rpp * nprob), stream, A));
        A_(timed.end(stream, &t));
        ms[0] += t;
    }
    /* the squares of a group of whole problems into the staging slab: the lane pass, the wave pass */
    auto form = [&](int64_t c0, int64_t nv, int64_t cnt, uint64_t *dstage) {
        int rc = 0;
        A.stage = dstage;
        slice(c0, nv, 1); A_(SERVICE_LAUNCH(states, wave_blocks(rpp * nv), stream, A));
        if (hwmax > 4) { slice(c0, nv, 2); A_(SERVICE_LAUNCH(states, wave_blocks(cnt), stream, A)); }
        return rc;
    };
    auto select = [&](int64_t c0, int64_t nv, const uint64_t *dstage) {
        /* the selection on the group's records: the largest |X_j| or X_j^2 / w_j, or the smallest X_j / (sense * A_j) */
        int64_t gp[4] = {0, 0, 0, 0};
        double t = 0;
        SlipRatioArgs R; memset(&R, 0, sizeof R);
        R.n = n; R.nprob = (int32_t) nv; R.pstride = n;
        R.xlen = dxl2 + c0 * n; R.xoff = weighted ? dso + c0 * n : dxo2 + c0 * n; R.xlimbs = weighted ? dstage : I.x.limbs;
        R.alen = dal2 + c0 * n; R.aoff = dao2 + c0 * n; R.alimbs = I.nside == 2 ? I.a.limbs : weighted ? O.wt.limbs : O.one;
        R.asense = I.nside == 2 ? I.sense : 1; R.xflip = I.nside == 1;
        int rc = ratio_core(R, key, r0 + c0, r1 + c0, r2 + c0, NULL, NULL, NULL, stream, &t, gp);
        if (!rc) { ms[1] += t; for (int k = 0; k < 4; k++) paths[4 + k] += gp[k]; }
        /* the winners' direction and, on request, their records as they came in */
        UP_(dsel, r0 + c0, (size_t) nv * 4);
        if (!rc) {
            slice(c0, nv, 3);
            A.best = dsel; A.vsign = dsel + nprob;
            if (wl) { A.wxlen = dwn; A.wxoff = dwo; A.walen = dwn + nprob; A.waoff = dwo + nprob; }
            A_(SERVICE_LAUNCH(states, service_blocks(nv), stream, A));
            HIP_(hipStreamSynchronize(stream));
        }
        DOWN_(r3 + c0, dsel + nprob, (size_t) nv * 4);
        if (wl) A_(winners_collect(nv, dwn, dwo, I.x.limbs, dwn + nprob, dwo + nprob, I.nside == 2 ? I.a.limbs : I.x.limbs, wl, wv, stream));
        return rc;
    };
    /* with weights the squares are staged in groups of whole problems; without, nothing is staged: one pass over all problems */
    if (weighted) {
        DOWN_(&hwmax, dwmax, 4);
        const int64_t wcap = hwmax > 2 ? hwmax : 2;        /* (even: twice an operand's digits) */
        if (!rc && wcap > (1 << 28)) rc = SLIP_HIP_OUT_OF_MEMORY;
        A_(staged_run(n, nprob, 1, wcap, dw, dso, form, select, stream, &ms[0], &ms[0]));
    } else A_(select(0, nprob, NULL));
    DOWN_(hpaths, dpaths, 32);
    if (!rc) for (int k = 0; k < 4; k++) paths[k] += (int64_t) hpaths[k];
    dev_free(dxl2); dev_free(dxo2); dev_free(dal2); dev_free(dao2); dev_free(dcls); dev_free(dw); dev_free(dso); dev_free(dwmax);
    dev_free(dpaths); dev_free(dsel); dev_free(dwn); dev_free(dwo);
    return rc;
}

extern "C" int slip_hip_factor_price_states(slip_hip_factor *f, slip_hip_matrix *M, int32_t nside, int32_t nprob,
                                            const int32_t *blen, const uint64_t *blimbs,
                                            const int32_t *glen, const uint64_t *glimbs, int64_t g_limbs,
                                            const int32_t *state, const int32_t *wlen, const uint64_t *wlimbs, int64_t w_limbs,
                                            int32_t sense, const int32_t *key,
                                            int32_t *best, int32_t *nties, int32_t *neligible, int32_t *vsign,
                                            int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream_v)
{
    if (!f || !M || !blen || !blimbs || !best || !nties || !neligible || !vsign || (nside != 1 && nside != 2) || nprob < 1 ||
        nprob > (1 << 29) || (sense != 1 && sense != -1) || !glen != !glimbs)
        return SLIP_HIP_INCORRECT_INPUT;
    if (winners_args_bad(wlen_out, wlimbs_out, wnl_out)) return SLIP_HIP_INCORRECT_INPUT;
    if (M->m != f->n) return SLIP_HIP_INCORRECT_INPUT;
    if (f->broken) return SLIP_HIP_DEVICE_ERROR;
    if (f->hs.F != f->n) return SLIP_HIP_INCORRECT_INPUT;       /* needs the complete factorisation */
    const int32_t n = f->n, ncols = M->ncols, nvec = nside * nprob;
    const int64_t nxe = (int64_t) n * nvec;
    hipStream_t stream = (hipStream_t) stream_v;
    SlipSlab gs, ws; memset(&gs, 0, sizeof gs);
    TRY_(states_check(ncols, nside, state, wlen, wlimbs, w_limbs, &ws));
    if (glen) { const int e_ = slab_prepare((int64_t) nprob * ncols, glen, glimbs, g_limbs, &gs); if (e_) { slab_free(&ws); return e_; } }
    SlipSolveOut o;
    int rc = solve_device(f, 1, nvec, blen, blimbs, stream, &o);
    if (rc) { slab_free(&gs); slab_free(&ws); return rc; }
    if (wlen_out) { *wlen_out = NULL; *wlimbs_out = NULL; *wnl_out = 0; }
    int32_t *dxl = NULL, *ddlen = NULL; int64_t *dxo = NULL, *ddoff = NULL;
    SlipDevSlab dg; memset(&dg, 0, sizeof dg);
    int32_t dmaxdig = 0;
    /* the result on the host until all of it stands: best, nties, neligible, vsign, nprob each */
    int32_t *hres = (int32_t *) malloc((size_t) nprob * 16);
    std::vector<int32_t> wl; std::vector<uint64_t> wv;
    double pms[4] = {0, 0, 0, 0}, ms[2] = {0, 0};
    int64_t paths[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    SlipStatesOps O; memset(&O, 0, sizeof O);
    if (!hres) rc = SLIP_HIP_OUT_OF_MEMORY;
    A_(states_upload(ncols, state, &ws, wlimbs, &O));
    /* y by row id: the records of the substitution's output gathered through pinv, its limbs where they are */
    A_(dev_alloc(&dxl, nxe)); A_(dev_alloc(&dxo, nxe));
    if (!rc) {
        SlipPriceArgs G; memset(&G, 0, sizeof G);
        G.phase = 0; G.n = n; G.count = nxe; G.pinv = f->P.pinv.p_; G.olen = o.olen; G.ooff = o.ooff; G.xlen = dxl; G.xoff = dxo;
        A_(SERVICE_LAUNCH(price, service_blocks(nxe), stream, G));
    }
    /* det * g: the cost vector's records on the x side of every problem, empty records on its a side */
    if (glen) A_(price_costs_put(nside, nprob, ncols, gs, glimbs, &dg));
    /* det's record once per vector: the products' d and, its sign alone, the d_c of every problem */
    A_(det_records(f, nvec, &ddlen, &ddoff, &dmaxdig));
    SlipProductView V;
    V.nout = ncols; V.nx = n; V.alen = M->dAlen; V.aoff = M->dAoff; V.alimbs = M->dAlimbs; V.amaxdig = M->amaxdig;
    V.rp = M->col_rp; V.re = M->col_re; V.rx = M->col_rx;
    const SlipDevRecs x = {dxl, dxo, o.olimbs}, g = dev_slab_recs(dg);
    /* the selection on a group of whole problems, on the staged records: X of problem c at c * nside * ncols, A ncols on */
    auto select = [&](int64_t c0, int64_t nv, const int32_t *rlen, const int64_t *soff, const uint64_t *stage, double *t) {
        const int64_t p0 = c0 / nside;
        SlipStatesIn I; memset(&I, 0, sizeof I);
        I.n = ncols; I.nprob = (int32_t)(nv / nside); I.nside = nside; I.sense = sense;
        I.x.len = rlen; I.x.off = soff; I.x.limbs = stage; I.xstride = (int64_t) nside * ncols;
        if (nside == 2) { I.a.len = rlen + ncols; I.a.off = soff + ncols; I.a.limbs = stage; I.astride = I.xstride; }
        I.dlen = ddlen + p0;
        const double before = ms[0] + ms[1];
        const int rc = states_core(I, O, key, hres + p0, hres + nprob + p0, hres + 2 * (int64_t) nprob + p0, hres + 3 * (int64_t) nprob + p0,
                                   wlen_out ? &wl : NULL, wlen_out ? &wv : NULL, stream, ms, paths);
        *t = ms[0] + ms[1] - before;
        return rc;
    };
    A_(product_device(V, nvec, x, -1, glen ? &g : NULL, gs.maxdig, ddlen, ddoff, f->P.Llimbs, dmaxdig, nside, select, stream, pms));
    dev_free(dxl); dev_free(dxo); dev_free(ddlen); dev_free(ddoff);
    dev_slab_free(&dg);
    states_ops_free(&O);
    slab_free(&gs); slab_free(&ws);
    solve_out_free(&o);
    if (!rc && wlen_out) rc = winners_out(wl, wv, wlen_out, wlimbs_out, wnl_out);
    if (!rc) {
        results_out(hres, nprob, best, nties, neligible, vsign);
        memcpy(f->states_ms, ms, sizeof ms); memcpy(f->states_paths, paths, sizeof paths);
    }
    free(hres);
    return rc;
}

extern "C" int slip_hip_price_select(int32_t ncols, int32_t nprob, int32_t nside,
                                     const int32_t *xlen, const uint64_t *xlimbs, int64_t x_limbs,
                                     const int32_t *alen, const uint64_t *alimbs, int64_t a_limbs,
                                     const int32_t *dlen, const uint64_t *dlimbs, int64_t d_limbs,
                                     const int32_t *state, const int32_t *wlen, const uint64_t *wlimbs, int64_t w_limbs,
                                     int32_t sense, const int32_t *key,
                                     int32_t *best, int32_t *nties, int32_t *neligible, int32_t *vsign,
                                     int32_t **wlen_out, uint64_t **wlimbs_out, int64_t *wnl_out, void *stream_v)
{
    if (ncols <= 0 || nprob < 1 || nprob > (1 << 29) || (nside != 1 && nside != 2) || (sense != 1 && sense != -1) || !xlen || !xlimbs ||
        !dlen || !dlimbs || !best || !nties || !neligible || !vsign)
        return SLIP_HIP_INCORRECT_INPUT;
    if (nside == 2 ? (!alen || !alimbs) : (alen || alimbs)) return SLIP_HIP_INCORRECT_INPUT;
    if (winners_args_bad(wlen_out, wlimbs_out, wnl_out)) return SLIP_HIP_INCORRECT_INPUT;
    TRY_(need_device());
    const int64_t ne = (int64_t) ncols * nprob;
    hipStream_t stream = (hipStream_t) stream_v;
    SlipSlab ws;
    TRY_(states_check(ncols, nside, state, wlen, wlimbs, w_limbs, &ws));
    SlipDevSlab x, a, d; memset(&x, 0, sizeof x); memset(&a, 0, sizeof a); memset(&d, 0, sizeof d);
    int32_t *res = NULL;
    std::vector<int32_t> wl; std::vector<uint64_t> wv;
    double ms[2] = {0, 0};
    int64_t paths[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    SlipStatesOps O; memset(&O, 0, sizeof O);
    /* (every slab is checked against its capacity before a limb of it is read) */
    int rc = dev_slab_upload(nprob, dlen, dlimbs, d_limbs, &d);
    for (int32_t c = 0; c < nprob && !rc; c++) if (d.s.dig[c] == 0) rc = SLIP_HIP_INCORRECT_INPUT;
    A_(dev_slab_upload(ne, xlen, xlimbs, x_limbs, &x));
    if (nside == 2) A_(dev_slab_upload(ne, alen, alimbs, a_limbs, &a));
    A_(states_upload(ncols, state, &ws, wlimbs, &O));
    if (!rc && !(res = (int32_t *) malloc((size_t) nprob * 16))) rc = SLIP_HIP_OUT_OF_MEMORY;
    if (!rc && wlen_out) { *wlen_out = NULL; *wlimbs_out = NULL; *wnl_out = 0; }
    SlipStatesIn I; memset(&I, 0, sizeof I);
    I.n = ncols; I.nprob = nprob; I.nside = nside; I.sense = sense; I.xstride = ncols; I.astride = ncols;
    I.x = dev_slab_recs(x); I.a = dev_slab_recs(a); I.dlen = d.len;
    A_(states_core(I, O, key, res, res + nprob, res + 2 * (int64_t) nprob, res + 3 * (int64_t) nprob,
                   wlen_out ? &wl : NULL, wlen_out ? &wv : NULL, stream, ms, paths));
    if (!rc && wlen_out) rc = winners_out(wl, wv, wlen_out, wlimbs_out, wnl_out);
    if (!rc) {
        results_out(res, nprob, best, nties, neligible, vsign);
        memcpy(slip_states_paths_last, paths, sizeof paths);
    }
    free(res);
    dev_slab_free(&x); dev_slab_free(&a); dev_slab_free(&d);
    states_ops_free(&O);
    slab_free(&ws);
    return rc;
}

extern "C" int slip_hip_factor_price_states_ms(const slip_hip_factor *f, double out[2])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->states_ms, sizeof f->states_ms);
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_factor_price_states_paths(const slip_hip_factor *f, int64_t out[8])
{
    if (!f || !out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, f->states_paths, sizeof f->states_paths);
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_price_select_paths(int64_t out[8])
{
    if (!out) return SLIP_HIP_INCORRECT_INPUT;
    memcpy(out, slip_states_paths_last, sizeof slip_states_paths_last);
    return SLIP_HIP_OK;
}

/* ---- subtree farm: multiply the committed factors by per-column scales ---- */
static void rescale_drop(slip_hip_factor *f)
{
    dev_free(f->rsLe); dev_free(f->rsUe); dev_free(f->rsLl); dev_free(f->rsUl); dev_free(f->rspiv);
    f->rsLe = f->rsUe = NULL; f->rsLl = f->rsUl = NULL; f->rspiv = NULL; f->rescaled = 0;
}

static int rescale_one(slip_hip_factor *f, int isL, int64_t nz, const int32_t *sdig, const int32_t *dslen, const int64_t *dsoff,
                       const uint64_t *dslimbs, hipStream_t stream)
{
    SlipParams *P = &f->P;
    const int32_t K = f->hs.F;
    if (nz <= 0) return 0;
    SlipEnt *he = (SlipEnt *) malloc((size_t) nz * sizeof(SlipEnt));
    int32_t *hidx = (int32_t *) malloc((size_t) nz * 4), *hpinv = (int32_t *) malloc((size_t) f->n * 4);
    int64_t *hp = (int64_t *) malloc(((size_t) K + 1) * 8);
    if (!he || !hidx || !hpinv || !hp) { free(he); free(hidx); free(hpinv); free(hp); return SLIP_HIP_OUT_OF_MEMORY; }
    int rc = 0;
    DOWN_(he, isL ? P->Le : P->Ue, (size_t) nz * sizeof(SlipEnt)); DOWN_(hidx, isL ? P->Li : P->Ui, (size_t) nz * 4);
    DOWN_(hpinv, P->pinv.p_, (size_t) f->n * 4); DOWN_(hp, isL ? P->Lp : P->Up, ((size_t) K + 1) * 8);
    /* lay the products out: digits(entry) + digits(scale) bound the product */
    int64_t o = 0;
    if (!rc) {
        int32_t c = 0;
        for (int64_t e = 0; e < nz; e++) {
            while (c + 1 <= K && hp[c + 1] <= e) c++;
            const int32_t sidx = isL ? c : hpinv[hidx[e]];
            if (sidx < 0 || sidx >= K) { rc = SLIP_HIP_INCORRECT_INPUT; break; }
            const int32_t la = he[e].len < 0 ? -he[e].len : he[e].len, lb = sdig[sidx] < 0 ? -sdig[sidx] : sdig[sidx];
            he[e].off = o;
            o += la ? (la + lb + 2) / 2 : 0;
        }
    }
    SlipEnt *de = NULL; uint64_t *dl = NULL;
    A_(dev_alloc(&de, nz)); A_(dev_alloc(&dl, o > 0 ? o : 1));
    UP_(de, he, (size_t) nz * sizeof(SlipEnt));
    if (!rc) {
        SlipRescaleArgs A; memset(&A, 0, sizeof A);
        A.ent = isL ? P->Le : P->Ue; A.limbs = isL ? P->Llimbs : P->Ulimbs; A.idx = isL ? P->Li : P->Ui; A.nz = nz;
        A.colp = isL ? P->Lp : NULL; A.ncols = K; A.pinv = P->pinv.p_;
        A.slen = dslen; A.soff = dsoff; A.slimbs = dslimbs; A.oent = de; A.olimbs = dl; A.pividx = f->rspiv; A.row_perm = P->row_perm.p_;
        A_(SERVICE_LAUNCH(rescale, wave_blocks(nz), stream, A));
        HIP_(hipStreamSynchronize(stream));
    }
    if (!rc) {
        if (isL) { f->rsLe = de; f->rsLl = dl; f->rsLnl = o; }
        else     { f->rsUe = de; f->rsUl = dl; f->rsUnl = o; }
        de = NULL; dl = NULL;
    }
    if (de) dev_free(de);
    if (dl) dev_free(dl);
    free(he); free(hidx); free(hpinv); free(hp);
    return rc;
}

extern "C" int slip_hip_factor_rescale(slip_hip_factor *f, int32_t nscales, const int32_t *slen, const uint64_t *slimbs, void *stream_v)
{
    if (!f || !slen || !slimbs) return SLIP_HIP_INCORRECT_INPUT;
    hipStream_t stream = (hipStream_t) stream_v;
    const int32_t K = f->hs.F;
    if (K <= 0 || nscales != K) return SLIP_HIP_INCORRECT_INPUT;      /* one scale per committed column, no more, no fewer */
    /* scales: signed limb counts -> signed digit counts + limb offsets */
    for (int32_t k = 0; k < K; k++) if (slen[k] == 0) return SLIP_HIP_INCORRECT_INPUT;     /* a scale is a product of pivots: never zero */
    SlipSlab ss;
    TRY_(slab_prepare(K, slen, slimbs, INT64_MAX, &ss));
    int32_t *dslen = NULL; int64_t *dsoff = NULL; uint64_t *dsl = NULL;
    int rc = 0;
    A_(dev_alloc(&dslen, K)); A_(dev_alloc(&dsoff, K)); A_(dev_alloc(&dsl, ss.total));
    UP_(dslen, ss.dig, (size_t) K * 4); UP_(dsoff, ss.off, (size_t) K * 8); UP_(dsl, slimbs, (size_t) ss.total * 8);
    rescale_drop(f);
    A_(dev_alloc(&f->rspiv, K));
    A_(rescale_one(f, 1, f->hs.Lnz, ss.dig, dslen, dsoff, dsl, stream));
    A_(rescale_one(f, 0, f->hs.Unz, ss.dig, dslen, dsoff, dsl, stream));
    if (!rc) {
        /* exact limb totals of the rescaled factors (download sizes its arrays from them) */
        SlipEnt *he = (SlipEnt *) malloc((size_t)(f->hs.Lnz > f->hs.Unz ? f->hs.Lnz : f->hs.Unz) * sizeof(SlipEnt));
        if (!he) rc = SLIP_HIP_OUT_OF_MEMORY;
        for (int pass = 0; pass < 2 && !rc; pass++) {
            const int64_t nz = pass == 0 ? f->hs.Lnz : f->hs.Unz;
            DOWN_(he, pass == 0 ? f->rsLe : f->rsUe, (size_t) nz * sizeof(SlipEnt));
            if (rc) break;
            int64_t tot = 0;
            for (int64_t e = 0; e < nz; e++) { const int32_t d = he[e].len < 0 ? -he[e].len : he[e].len; tot += (d + 1) >> 1; }
            if (pass == 0) f->rsLexact = tot; else f->rsUexact = tot;
        }
        free(he);
        if (!rc) f->rescaled = 1;
    }
    if (rc) rescale_drop(f);
    dev_free(dslen); dev_free(dsoff); dev_free(dsl);
    slab_free(&ss);
    return rc;
}

/* diagnostic: per-phase shader cycles of the last run (zeros unless built with -DSLIP_PROFILE: csrc/Makefile, `make prof` / `make cprof`) */
extern "C" int slip_hip_factor_phase_cycles(const slip_hip_factor *f, unsigned long long *out24)
{
    if (!f || !out24) return SLIP_HIP_INCORRECT_INPUT;
    for (int i = 0; i < 24; i++) out24[i] = f->hs.prof[i];
    return SLIP_HIP_OK;
}

/* diagnostic builds: wall-clock phase stamps of the heavy columns (more than 400 rows), 64 records of 32 words
 * (slot s = time of SLIP_STAMP(s); 29 = chain start, 30 = rows, 31 = column) */
extern "C" int slip_hip_factor_heavy_trace(const slip_hip_factor *f, int32_t *out2048)
{
    if (!f || !out2048) return SLIP_HIP_INCORRECT_INPUT;
    CK(hipMemcpy(out2048, f->P.dbg + slip_dbg_heavy(f->n), 2048 * 4, hipMemcpyDeviceToHost));
    return SLIP_HIP_OK;
}

/* diagnostic builds: the per-column trace (8 words per column: commit-chain cycles, early flag, candidates computed, rows,
 * cycles of the sweep after the last frontier wait, of the early pass, of the publish, worker) */
extern "C" int slip_hip_factor_column_trace(const slip_hip_factor *f, int32_t *out, int32_t ncols)
{
    if (!f || !out || ncols <= 0 || ncols > f->n) return SLIP_HIP_INCORRECT_INPUT;
    /* the regions of the debug buffer in their order, each cut to the first ncols columns: the trace records (8 words),
     * the 100 MHz chip clock when the column's worker saw its turn (1), the cycles of the sub-steps of the commit chain (8),
     * the path flags (1), the wall-clock time line (6) */
    const int64_t n = f->n, nc = ncols;
    const struct { int64_t at, words; } part[5] = { { slip_dbg_trace(n), 8 }, { slip_dbg_seen(n), 1 }, { slip_dbg_chain(n), 8 },
                                                   { slip_dbg_flags(n), 1 }, { slip_dbg_timeline(n), 6 } };
    for (int i = 0; i < 5; i++) {
        CK(hipMemcpy(out, f->P.dbg + part[i].at, (size_t)(nc * part[i].words) * 4, hipMemcpyDeviceToHost));
        out += nc * part[i].words;
    }

    return SLIP_HIP_OK;
}

/* diagnostic: raw words of the device debug area (ref_lu_pipe.h: slip_dbg_*; e.g. the placement of the workgroups of the last launch: cu | sh | se | xcc) */
extern "C" int slip_hip_factor_debug_words(const slip_hip_factor *f, int64_t offset, int32_t count, int32_t *out)
{
    if (!f || !out || offset < 0 || count <= 0 || offset + count > slip_dbg_words(f->n)) return SLIP_HIP_INCORRECT_INPUT;
    CK(hipMemcpy(out, f->P.dbg + offset, (size_t) count * 4, hipMemcpyDeviceToHost));
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_factor_info(const slip_hip_factor *f, slip_hip_info *o)
{
    if (!f || !o) return SLIP_HIP_INCORRECT_INPUT;
    const SlipState *h = &f->hs;
    o->n = f->n; o->K = h->F; o->status = f->last_status; o->window_end = f->window_end;
    o->lnz = h->Lnz; o->unz = h->Unz; o->l_limbs = f->rescaled ? f->rsLexact : h->Lnl_exact; o->u_limbs = f->rescaled ? f->rsUexact : h->Unl_exact;
    o->n_upd = (int64_t) h->c_upd; o->b_read = (int64_t) h->c_read; o->b_write = (int64_t) h->c_write;
    o->n_src = (int64_t) h->c_src; o->l_streamed = (int64_t) h->c_streamed;
    o->max_limbs = (int64_t)((h->c_maxdig + 1) / 2);
    o->kernel_ms = f->kernel_ms; o->launches = f->launches; o->xcap_digits = f->P.xcap;
    o->limb_macs = (int64_t) h->c_macs; o->workers = f->nworkers; o->waves = f->waves; o->lds_bytes = f->lds_words * 4;
    o->short_commits = (int32_t)(uint32_t) h->c_short; o->committer_commits = (int32_t)(h->c_short >> 32);
    o->farm_jobs = (int32_t)(uint32_t) h->c_farm; o->farm_items = (int32_t)(h->c_farm >> 32);
    o->engine_commits = (int32_t)(uint32_t) h->c_eng; o->engine_sources = (int32_t)(h->c_eng >> 32);
    o->retractions = (int32_t)(uint32_t) h->c_retract; o->reexports = (int32_t)(h->c_retract >> 32); o->batch_commits = (int32_t) h->c_batch;
    o->raw_fills = (int64_t) h->c_raw;
    return SLIP_HIP_OK;
}

/* entry records -> signed 64-bit limb counts, and the limbs gathered entry by entry into the back-to-back layout
 * of the ABI (slots of rows multiplied straight into the slab may leave unused limbs behind them) */
/* entries' limbs, scattered over a slab with gaps (an early commit reserves a column's region from bounds), packed back
 * to back on the device: one wavefront per entry, coalesced; the host then copies exactly the limbs it was promised */
#ifndef SLIP_EMULATE
__global__ void __launch_bounds__(256) slip_gather_kernel(const SlipEnt *ent, const uint64_t *limbs, const int64_t *ooff, uint64_t *out, int64_t nz)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t) gridDim.x * blockDim.x) >> 6;
    for (int64_t t = wave; t < nz; t += nwaves) {
        const int64_t l = ooff[t + 1] - ooff[t];
        const uint64_t *src = limbs + ent[t].off; uint64_t *dst = out + ooff[t];
        for (int64_t c = lane; c < l; c += 64) dst[c] = src[c];
    }
}
#endif

/* `expect`: the limbs the device counted for these entries (SlipState.Lnl_exact / Unl_exact, or the rescaled totals);
 * `cap`: what the caller's limbs_out can hold.  Nothing is written to limbs_out unless the entry records are consistent
 * with both and every entry lies inside the slab (nl_alloc limbs): device state never sizes a write into host memory. */
static int fetch_factor(int32_t *len_out, uint64_t *limbs_out, const SlipEnt *dev_ent, const uint64_t *dev_limbs, int64_t nz, int64_t nl_alloc,
                        int64_t expect, int64_t cap, int64_t *written)
{
    if (written) *written = 0;
    if (nz <= 0) return 0;
    SlipEnt *ent = (SlipEnt *) malloc((size_t) nz * sizeof(SlipEnt));
    if (!ent) return SLIP_HIP_OUT_OF_MEMORY;
    if (hipMemcpy(ent, dev_ent, (size_t) nz * sizeof(SlipEnt), hipMemcpyDeviceToHost) != hipSuccess) { free(ent); return SLIP_HIP_DEVICE_ERROR; }
    /* the records first: lengths, offsets and the total against what the device counted */
    int64_t total = 0;
    for (int64_t t = 0; t < nz; t++) {
        const int64_t d = ent[t].len < 0 ? -(int64_t) ent[t].len : ent[t].len, l = (d + 1) >> 1;
        if (d > (int64_t) 1 << 30 || ent[t].off < 0 || (l > 0 && ent[t].off + l > nl_alloc)) {
            fprintf(stderr, "slip_hip: entry record %lld is inconsistent (off %lld, %lld digits, slab %lld limbs)\n", (long long) t, (long long) ent[t].off, (long long) d, (long long) nl_alloc);
            free(ent); return SLIP_HIP_DEVICE_ERROR;
        }
        total += l;
    }
    if (total != expect) {
        fprintf(stderr, "slip_hip: the entry records hold %lld limbs, the device counted %lld\n", (long long) total, (long long) expect);
        free(ent); return SLIP_HIP_DEVICE_ERROR;
    }
    if (limbs_out && total > cap) { free(ent); return SLIP_HIP_INCORRECT_INPUT; }
    if (len_out)
        for (int64_t t = 0; t < nz; t++) {
            int32_t d = ent[t].len, a = d < 0 ? -d : d;
            a = (a + 1) >> 1;
            len_out[t] = d < 0 ? -a : a;
        }
    int rc = 0;
    if (limbs_out && total > 0) {
#ifndef SLIP_EMULATE
        /* one pass on the device, then one copy of exactly the packed limbs */
        int64_t *ooff = (int64_t *) malloc(((size_t) nz + 1) * 8), *d_ooff = NULL; uint64_t *d_out = NULL;
        if (!ooff) { free(ent); return SLIP_HIP_OUT_OF_MEMORY; }
        ooff[0] = 0;
        for (int64_t t = 0; t < nz; t++) { const int32_t d = ent[t].len; ooff[t + 1] = ooff[t] + (((d < 0 ? -d : d) + 1) >> 1); }
        if (dev_alloc(&d_ooff, nz + 1) || dev_alloc(&d_out, total)) rc = SLIP_HIP_OUT_OF_MEMORY;
        else if (hipMemcpy(d_ooff, ooff, ((size_t) nz + 1) * 8, hipMemcpyHostToDevice) != hipSuccess) rc = SLIP_HIP_DEVICE_ERROR;
        else {
            int64_t blocks = (nz + 3) / 4; if (blocks > 4096) blocks = 4096; if (blocks < 1) blocks = 1;
            hipLaunchKernelGGL(slip_gather_kernel, dim3((unsigned) blocks), dim3(256), 0, 0, dev_ent, dev_limbs, d_ooff, d_out, nz);
            if (hipGetLastError() != hipSuccess || hipMemcpy(limbs_out, d_out, (size_t) total * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = SLIP_HIP_DEVICE_ERROR;
        }
        if (d_ooff) dev_free(d_ooff);
        if (d_out) dev_free(d_out);
        free(ooff);
#else
        uint64_t *raw = (uint64_t *) malloc((size_t)(nl_alloc > 0 ? nl_alloc : 1) * 8);
        if (!raw) rc = SLIP_HIP_OUT_OF_MEMORY;
        else if (hipMemcpy(raw, dev_limbs, (size_t) nl_alloc * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = SLIP_HIP_DEVICE_ERROR;
        else {
            int64_t o = 0;
            for (int64_t t = 0; t < nz; t++) {
                const int32_t d = ent[t].len;
                const int64_t l = ((d < 0 ? -d : d) + 1) >> 1;
                if (l) memcpy(limbs_out + o, raw + ent[t].off, (size_t) l * 8);
                o += l;
            }
        }
        free(raw);
#endif
    }
    if (!rc && written) *written = total;
    free(ent);
    return rc;
}

extern "C" int slip_hip_factor_download(const slip_hip_factor *f,
                                        int64_t *Lp, int32_t *Li, int32_t *Llen, uint64_t *Llimbs, int64_t *L_limbs_inout,
                                        int64_t *Up, int32_t *Ui, int32_t *Ulen, uint64_t *Ulimbs, int64_t *U_limbs_inout,
                                        int32_t *rholen, uint64_t *rholimbs, int64_t *rho_limbs_inout,
                                        int32_t *pinv)
{
    if (!f) return SLIP_HIP_INCORRECT_INPUT;
    /* a limb array without its capacity cannot be written safely */
    if ((Llimbs && !L_limbs_inout) || (Ulimbs && !U_limbs_inout) || (rholimbs && !rho_limbs_inout)) return SLIP_HIP_INCORRECT_INPUT;
    /* after a device error the columns between the ready frontier and the commit frontier may be half written: nothing is handed out */
    if (f->last_status == SLIP_HIP_DEVICE_ERROR) return SLIP_HIP_DEVICE_ERROR;
    const SlipParams *P = &f->P;
    const SlipState *h = &f->hs;
    const int32_t K = h->F;
    /* what is handed out: the resident factors, or their rescaled copy while it exists */
    const int rs = f->rescaled;
    const SlipEnt *Le = rs ? f->rsLe : P->Le, *Ue = rs ? f->rsUe : P->Ue;
    const uint64_t *Ll = rs ? f->rsLl : P->Llimbs, *Ul = rs ? f->rsUl : P->Ulimbs;
    const int64_t Lnl = rs ? f->rsLnl : P->Lcap_nl, Unl = rs ? f->rsUnl : P->Ucap_nl;
    const int64_t Lexact = rs ? f->rsLexact : h->Lnl_exact, Uexact = rs ? f->rsUexact : h->Unl_exact;
    int e;
    if (Lp) CK(hipMemcpy(Lp, P->Lp, ((size_t) K + 1) * 8, hipMemcpyDeviceToHost));
    if (Up) CK(hipMemcpy(Up, P->Up, ((size_t) K + 1) * 8, hipMemcpyDeviceToHost));
    if (Li && h->Lnz) CK(hipMemcpy(Li, P->Li, (size_t) h->Lnz * 4, hipMemcpyDeviceToHost));
    if (Ui && h->Unz) CK(hipMemcpy(Ui, P->Ui, (size_t) h->Unz * 4, hipMemcpyDeviceToHost));
    {
        int64_t wl = 0, wu = 0;
        if ((Llen || Llimbs) && (e = fetch_factor(Llen, Llimbs, Le, Ll, h->Lnz, Lnl, Lexact, L_limbs_inout ? *L_limbs_inout : 0, &wl))) return e;
        if ((Ulen || Ulimbs) && (e = fetch_factor(Ulen, Ulimbs, Ue, Ul, h->Unz, Unl, Uexact, U_limbs_inout ? *U_limbs_inout : 0, &wu))) return e;
        if (L_limbs_inout) *L_limbs_inout = wl;
        if (U_limbs_inout) *U_limbs_inout = wu;
    }
    if (pinv) CK(hipMemcpy(pinv, P->pinv.p_, (size_t) f->n * 4, hipMemcpyDeviceToHost));
    if ((rholen || rholimbs) && K > 0) {
        /* the pivots live in the L slab: gather them through the pivot records (a rescaled copy: through the pivot entries) */
        SlipPiv *pr = (SlipPiv *) malloc((size_t) K * sizeof(SlipPiv));
        if (!pr) return SLIP_HIP_OUT_OF_MEMORY;
        if (hipMemcpy(pr, P->piv.p_, (size_t) K * sizeof(SlipPiv), hipMemcpyDeviceToHost) != hipSuccess) { free(pr); return SLIP_HIP_DEVICE_ERROR; }
        if (rs) {
            int64_t *pi = (int64_t *) malloc((size_t) K * 8);
            SlipEnt pe;
            if (!pi) { free(pr); return SLIP_HIP_OUT_OF_MEMORY; }
            int bad = hipMemcpy(pi, f->rspiv, (size_t) K * 8, hipMemcpyDeviceToHost) != hipSuccess;
            for (int32_t k = 0; k < K && !bad; k++) {
                if (hipMemcpy(&pe, Le + pi[k], sizeof pe, hipMemcpyDeviceToHost) != hipSuccess) bad = 1;
                pr[k].off = pe.off; pr[k].len = pe.len;
            }
            free(pi);
            if (bad) { free(pr); return SLIP_HIP_DEVICE_ERROR; }
        }
        int64_t o = 0, capl = rho_limbs_inout ? *rho_limbs_inout : 0;
        int rc = 0;
        for (int32_t k = 0; k < K && !rc; k++) {
            int32_t d = pr[k].len, l = ((d < 0 ? -d : d) + 1) >> 1;
            if (rholen) rholen[k] = d < 0 ? -l : l;
            if (pr[k].off < 0 || pr[k].off + l > Lnl) { rc = SLIP_HIP_DEVICE_ERROR; break; }
            if (rholimbs) {
                if (o + l > capl) { rc = SLIP_HIP_INCORRECT_INPUT; break; }
                if (hipMemcpy(rholimbs + o, Ll + pr[k].off, (size_t) l * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = SLIP_HIP_DEVICE_ERROR;
            }
            o += l;
        }
        if (rho_limbs_inout) *rho_limbs_inout = o;
        free(pr);
        if (rc) return rc;
    } else if (rho_limbs_inout) *rho_limbs_inout = 0;
    return SLIP_HIP_OK;
}

extern "C" int slip_hip_wave_op_test(int32_t op, int32_t nops, int32_t la, int32_t lb, int32_t W,
                                     const uint32_t *a, const uint32_t *b, uint32_t *out)
{
    if (nops <= 0 || la <= 0 || W <= 0 || !a || !out || (op != 3 && op != 13 && op != 14 && (!b || lb <= 0))) return SLIP_HIP_INCORRECT_INPUT;
    if (op >= 10 && W > 256) return SLIP_HIP_INCORRECT_INPUT;
    if (slip_hip_device_count() <= 0) return SLIP_HIP_DEVICE_ERROR;
    uint32_t *da = NULL, *db = NULL, *dout = NULL, *ds = NULL;
    const int64_t lbb = (lb > 0 && op != 14) ? lb : 1;
    if (dev_alloc(&da, (int64_t) nops * la) || dev_alloc(&db, (int64_t) nops * lbb) ||
        dev_alloc(&dout, (int64_t) nops * W) || dev_alloc(&ds, (int64_t) nops * 2 * (W + 1))) return SLIP_HIP_OUT_OF_MEMORY;
    CK(hipMemcpy(da, a, (size_t) nops * la * 4, hipMemcpyHostToDevice));
    if (b && lb > 0 && op != 14) CK(hipMemcpy(db, b, (size_t) nops * lb * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dout, 0, (size_t) nops * W * 4));
#ifndef SLIP_EMULATE
    hipLaunchKernelGGL(slip_wave_op_kernel, dim3(nops), dim3(64), 0, 0, op, la, lb, W, da, db, dout, ds);
    CK(hipGetLastError());
#else
    emu::launch(nops, 64, [=]() {
        const int blk = slip_block();
        const uint32_t *A = da + (int64_t) blk * la, *B = db + (int64_t) blk * lbb;
        uint32_t *O = dout + (int64_t) blk * W, *s0 = ds + (int64_t) blk * 2 * (W + 1), *s1 = s0 + W + 1;
        if (op == 0) wb_mul_lo(O, A, la, B, lb, W);
        else if (op == 1) wb_addsub(O, A, la, B, lb, W, 0);
        else if (op == 2) wb_addsub(O, A, la, B, lb, W, 1);
        else if (op == 3) wb_inv_extend(O, 0, W, A, la, s0, s1);
        else slip_reg_op_test(op, A, la, B, lb, W, O, s0);
    }, 256 * 1024, 1);
#endif
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout, (size_t) nops * W * 4, hipMemcpyDeviceToHost));
    dev_free(da); dev_free(db); dev_free(dout); dev_free(ds);
    return SLIP_HIP_OK;
}

#ifndef SLIP_EMULATE
/* development aid: average shader cycles of one wave-level primitive (see slip_wave_bench_kernel) */
extern "C" int slip_hip_wave_op_bench(int32_t op, int32_t la, int32_t lb, int32_t W, int32_t iters, int32_t nwaves,
                                      int32_t out_in_lds, unsigned long long *cycles_out)
{
    uint32_t *da = NULL, *db = NULL, *dout = NULL; unsigned long long *dc = NULL;
    if (dev_alloc(&da, (int64_t) nwaves * la) || dev_alloc(&db, (int64_t) nwaves * lb) ||
        dev_alloc(&dout, (int64_t) nwaves * 2 * (W + 2)) || dev_alloc(&dc, nwaves)) return SLIP_HIP_OUT_OF_MEMORY;
    CK(hipMemset(da, 0x5A, (size_t) nwaves * la * 4));
    CK(hipMemset(db, 0xC3, (size_t) nwaves * lb * 4));
    const size_t lds = (size_t) nwaves * 2 * (W + 2) * 4;
    CK(hipFuncSetAttribute((const void *) slip_wave_bench_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
    hipLaunchKernelGGL(slip_wave_bench_kernel, dim3(1), dim3(64 * nwaves), lds, 0, op, la, lb, W, iters, out_in_lds, da, db, dout, dc);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(cycles_out, dc, (size_t) nwaves * 8, hipMemcpyDeviceToHost));
    dev_free(da); dev_free(db); dev_free(dout); dev_free(dc);
    return SLIP_HIP_OK;
}
#endif
