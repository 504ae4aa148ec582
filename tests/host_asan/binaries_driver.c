/* tests/host_asan/binaries_driver.c -- nbody_binary_finish (csrc/nbody_binaries.c) under AddressSanitizer + UBSan: buffers
 * of exactly `count` records on the heap, so a read or write past either end is caught; the order and the values are
 * checked too, with raw values on both sides of the eps and e2 guards, NaN and zero among them.  Host code only. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nbody.h"

static unsigned long long lcg(unsigned long long* s) { return *s = *s * 6364136223846793005ull + 1442695040888963407ull; }
static double unit(unsigned long long* s) { return (double)(lcg(s) >> 11) / 9007199254740992.0; }

static int run(int count, unsigned long long seed) {
    nbody_binary_raw* raw = (nbody_binary_raw*)malloc((size_t)(count ? count : 1) * sizeof(*raw));
    nbody_binary* out = (nbody_binary*)malloc((size_t)(count ? count : 1) * sizeof(*out));
    if (!raw || !out) return 2;
    for (int k = 0; k < count; ++k) {
        raw[k].i = (int32_t)(lcg(&seed) % 1000u);
        raw[k].j = raw[k].i + 1 + (int32_t)(lcg(&seed) % 1000u);
        if (lcg(&seed) & 1) { int32_t t = raw[k].i; raw[k].i = raw[k].j; raw[k].j = t; }
        raw[k].flags = (uint32_t)(lcg(&seed) % 4u) | 0x100u;
        raw[k].reserved = 0;
        raw[k].d2 = k % 11 == 0 ? 0.0 : 400.0 * unit(&seed);
        raw[k].v2 = k % 7 == 0 ? NAN : 3000.0 * unit(&seed);          /* about half above 2 gm / r: eps >= 0 */
        raw[k].mu = k % 13 == 0 ? 0.0 : 40000.0 * unit(&seed);
        raw[k].hz = k % 5 == 0 ? 1e9 : 400.0 * unit(&seed) - 200.0;   /* 1e9: e2 far below 0 */
    }
    int rc = nbody_binary_finish(count ? raw : NULL, count, count ? out : NULL);
    if (rc != NBODY_OK) { printf("finish rc=%d\n", rc); return 1; }
    for (int k = 0; k < count; ++k) {
        const nbody_binary* e = out + k;
        if (!(e->i < e->j) || e->reserved != 0 || (e->flags & ~3u)) { printf("record %d\n", k); return 1; }
        /* the guards: whatever the raw values are, a and period are never NaN or negative, ecc is never NaN */
        if (!(e->a >= 0.0) || !(e->period >= 0.0) || !(e->ecc >= 0.0) || (isinf(e->a) && !isinf(e->period))) { printf("orbit %d\n", k); return 1; }
        if (k && (out[k - 1].i > e->i || (out[k - 1].i == e->i && out[k - 1].j > e->j))) {
            printf("order %d\n", k);
            return 1;
        }
    }
    free(raw);
    free(out);
    return 0;
}

int main(void) {
    const int counts[] = {0, 1, 2, 3, 64, 1000, 4097};
    for (size_t a = 0; a < sizeof(counts) / sizeof(counts[0]); ++a)
        for (unsigned b = 0; b < 4; ++b)
            if (run(counts[a], 17u + a * 31u + b)) return 1;
    if (nbody_binary_finish(NULL, 3, NULL) != NBODY_ERR_INVALID || nbody_binary_finish(NULL, -1, NULL) != NBODY_ERR_INVALID) return 1;
    printf("binaries ok\n");
    return 0;
}
