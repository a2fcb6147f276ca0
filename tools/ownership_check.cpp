/* Ownership check of the exact services' host layer, on the CPU: every handle-less service entry once on a 3 x 3 problem, the
 * matrix product once in two staging groups and once refused, as ONE executable with the emulated kernel source, so that the
 * host sanitizers see every "device" buffer (the emulator's hipMalloc is malloc).  From the repository's root:
 *
 *   clang++ -O1 -g -DSLIP_EMULATE -fsanitize=address,undefined -fno-sanitize-recover=undefined -Itests/emu -Islip_lu_amd/csrc \
 *       -x c++ slip_lu_amd/csrc/slip_hip.hip tools/ownership_check.cpp -o ownership_check && ./ownership_check
 *
 * It prints "ownership_check ok" and ends with status 0 when every call answered as expected; a leak, an overrun or a double
 * free is the sanitizers' report and a nonzero status. */
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>
#include "../include/slip_hip.h"
#include "fiber_emu.h"

struct Slab { std::vector<int32_t> len; std::vector<uint64_t> limbs; };
static Slab slab(std::initializer_list<long> v)
{
    Slab s;
    for (long x : v) { s.len.push_back(x < 0 ? -1 : x > 0); if (x) s.limbs.push_back((uint64_t)(x < 0 ? -x : x)); }
    return s;
}
#define L(s) (s).len.data(), (s).limbs.data(), (int64_t)(s).limbs.size()

static int failures = 0;
static void expect(const char *what, int rc, int want)
{
    if (rc != want) { fprintf(stderr, "%s: status %d, expected %d\n", what, rc, want); failures++; }
}

int main()
{
    setenv("SLIP_HIP_POOL_MB", "0", 1);
    const int32_t n = 3;
    const Slab x = slab({5, -7, 9}), a = slab({2, 3, -4}), d = slab({6}), lo = slab({-1, 0, 1}), hi = slab({4, 5, 6});
    const Slab p = slab({3}), t = slab({-2}), w = slab({1, 2, 3});
    const int32_t kind[3] = {1, 2, 3}, state[3] = {1, 2, 3}, place[1] = {1};
    const slip_hip_bounds B = {kind, lo.len.data(), lo.limbs.data(), (int64_t) lo.limbs.size(), hi.len.data(), hi.limbs.data(),
                               (int64_t) hi.limbs.size(), 0, NULL};
    int32_t r0[1], r1[1], r2[1], r3[1], *wl = NULL; uint64_t *wv = NULL; int64_t wn = 0;

    expect("ratio_test", slip_hip_ratio_test(n, 1, L(x), L(a), 1, NULL, r0, r1, r2, NULL), SLIP_HIP_OK);
    expect("ratio_test_bounded", slip_hip_ratio_test_bounded(n, 1, L(x), L(a), L(d), &B, 1, NULL, r0, r1, r2, r3, &wl, &wv, &wn, NULL), SLIP_HIP_OK);
    slip_hip_free(wl); slip_hip_free(wv);
    expect("bound_test", slip_hip_bound_test(n, 1, L(x), L(d), &B, NULL, r0, r1, r2, r3, &wl, &wv, &wn, NULL), SLIP_HIP_OK);
    slip_hip_free(wl); slip_hip_free(wv);
    expect("price_select", slip_hip_price_select(n, 1, 1, L(x), NULL, NULL, 0, L(d), state, NULL, NULL, 0, 1, NULL, r0, r1, r2, r3, &wl, &wv, &wn, NULL),
           SLIP_HIP_OK);
    slip_hip_free(wl); slip_hip_free(wv);
    expect("price_select, weighted", slip_hip_price_select(n, 1, 1, L(x), NULL, NULL, 0, L(d), state, L(w), 1, NULL, r0, r1, r2, r3, &wl, &wv, &wn, NULL),
           SLIP_HIP_OK);
    slip_hip_free(wl); slip_hip_free(wv);
    expect("pivot_update, d and place", slip_hip_pivot_update(n, 1, L(x), L(a), L(p), L(t), L(d), place, r0, &wl, &wv, &wn, NULL), SLIP_HIP_OK);
    slip_hip_free(wl); slip_hip_free(wv);
    expect("pivot_update", slip_hip_pivot_update(n, 1, L(x), L(a), L(p), L(t), NULL, NULL, 0, NULL, r0, &wl, &wv, &wn, NULL), SLIP_HIP_OK);
    slip_hip_free(wl); slip_hip_free(wv);

    /* the product of a 3 x 3 matrix with two vectors of 30-limb entries: under a staging bound of 1 KiB one vector a group */
    const int64_t Ap[4] = {0, 2, 3, 5}; const int32_t Ai[5] = {0, 2, 1, 0, 2};
    const Slab A = slab({2, -1, 3, 4, 5});
    Slab X;
    for (int e = 0; e < 6; e++) { X.len.push_back(e & 1 ? -30 : 30); for (int l = 0; l < 30; l++) X.limbs.push_back(~(uint64_t) 0 - (uint64_t)(e + l)); }
    slip_hip_matrix *M = NULL;
    expect("matrix_create", slip_hip_matrix_create(&M, n, n, Ap, Ai, A.len.data(), A.limbs.data()), SLIP_HIP_OK);
    setenv("SLIP_HIP_PRODUCT_STAGE_KB", "1", 1);
    wl = NULL; wv = NULL;
    expect("matrix_multiply, two groups", slip_hip_matrix_multiply(M, 0, 2, L(X), NULL, NULL, 0, NULL, NULL, 0, &wl, &wv, &wn, NULL), SLIP_HIP_OK);
    slip_hip_free(wl); slip_hip_free(wv);
    wl = NULL; wv = NULL;
    expect("matrix_multiply, x longer than its capacity",
           slip_hip_matrix_multiply(M, 0, 2, X.len.data(), X.limbs.data(), 179, NULL, NULL, 0, NULL, NULL, 0, &wl, &wv, &wn, NULL), SLIP_HIP_INCORRECT_INPUT);
    slip_hip_free(wl); slip_hip_free(wv);
    slip_hip_matrix_destroy(M);
    /* the emulator keeps its fibers' stacks for the life of the process: they are not the host layer's */
    for (char *s : emu::S().stacks) free(s);
    emu::S().stacks.clear();
    if (!failures) printf("ownership_check ok\n");
    return failures != 0;
}
