/*
 * levels_selftest.c -- stand-alone memory-safety run of the oracle's encoders (test infrastructure, host code only).
 *
 * `make -C oracle selftest` builds this file together with fdeflate_oracle.c under AddressSanitizer and UBSan and runs
 * it: fdo_compress_level at every level 0..9 (and 12, which is 7) over generated inputs -- every length 0..300 of three
 * kinds, and longer streams of noise over small alphabets, words, motifs with runs, an incompressible stretch with a
 * late copy, and a stream long enough to cut a block and to start the second pass past the window --, each stream into
 * a buffer of exactly fdo_compress_bound bytes, decoded again with fdo_decompress_bounded and compared; then the same
 * through fdo_deflate_level_batch on 4 threads, and slots too small.  Exit status 0: everything round-tripped.
 * It loads nothing into Python and is not part of the pytest suite.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fdeflate_oracle.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void) { /* xorshift64* */
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static void fill(uint8_t *p, size_t n, int kind) {
    static const char *words[8] = {"the", "then", "there", "thereof", "lazy", "laze", "match", "matches"};
    size_t i = 0;
    switch (kind) {
    case 0: /* noise over 2 symbols */
    case 1: /* over 4 */
    case 2: /* over 256 */
        for (; i < n; i++) {
            p[i] = (uint8_t)(rnd() % (kind == 0 ? 2 : kind == 1 ? 4 : 256));
        }
        break;
    case 3: /* words */
        while (i < n) {
            const char *w = words[rnd() % 8];
            for (size_t k = 0; w[k] && i < n; k++) {
                p[i++] = (uint8_t)w[k];
            }
        }
        break;
    case 4: /* motifs of period 2..9 and runs */
        while (i < n) {
            uint8_t motif[9];
            size_t period = 2 + rnd() % 8, len = 20 + rnd() % 180;
            for (size_t k = 0; k < period; k++) {
                motif[k] = (uint8_t)rnd();
            }
            for (size_t k = 0; k < len && i < n; k++) {
                p[i++] = motif[k % period];
            }
            size_t run = 4 + rnd() % 300;
            uint8_t v = (uint8_t)rnd();
            for (size_t k = 0; k < run && i < n; k++) {
                p[i++] = v;
            }
        }
        break;
    default: /* incompressible, then a copy of an earlier part */
        for (; i < n; i++) {
            p[i] = (uint8_t)rnd();
        }
        if (n > 600) {
            memcpy(p + n - 200, p + 100, 200);
        }
        break;
    }
}

static int check(const uint8_t *in, size_t len, unsigned level, const uint8_t *comp, size_t clen, uint8_t *back) {
    size_t n = 0;
    int st = fdo_decompress_bounded(comp, clen, back, len, &n, 0, NULL);
    if (clen == 0 || st != FDO_OK || n != len || (len && memcmp(in, back, len) != 0)) {
        fprintf(stderr, "FAIL: level %u, %zu bytes: %zu compressed, status %d, %zu decoded\n", level, len, clen, st, n);
        return 1;
    }
    return 0;
}

int main(void) {
    enum { MAXLEN = 200000 };
    const unsigned levels[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12};
    const size_t nlevels = sizeof(levels) / sizeof(levels[0]);
    uint8_t *in = (uint8_t *)malloc(MAXLEN);
    uint8_t *back = (uint8_t *)malloc(MAXLEN + 1);
    int failures = 0;
    size_t streams = 0;
    if (!in || !back) {
        return 2;
    }
    for (int kind = 0; kind < 6; kind++) {
        size_t lens[340];
        size_t nl = 0;
        if (kind == 0 || kind == 3 || kind == 4) {
            for (size_t n = 0; n <= 300; n++) {
                lens[nl++] = n;
            }
        }
        lens[nl++] = 4000;
        lens[nl++] = 33000;
        lens[nl++] = 70001;
        if (kind == 3 || kind == 1) {
            lens[nl++] = MAXLEN;
        }
        for (size_t k = 0; k < nl; k++) {
            size_t len = lens[k];
            /* exactly len bytes, so that a read past the input is a read past the allocation */
            uint8_t *x = (uint8_t *)malloc(len ? len : 1);
            fill(in, len, kind);
            memcpy(x, in, len);
            for (size_t l = 0; l < nlevels; l++) {
                size_t cap = fdo_compress_bound(len);
                uint8_t *comp = (uint8_t *)malloc(cap);
                size_t clen = fdo_compress_level(x, len, levels[l], comp, cap);
                failures += check(x, len, levels[l], comp, clen, back);
                if (clen > 8 && fdo_compress_level(x, len, levels[l], comp, clen - 1) != 0) {
                    fprintf(stderr, "FAIL: level %u, %zu bytes: a slot one byte short was not refused\n", levels[l], len);
                    failures++;
                }
                free(comp);
                streams++;
            }
            free(x);
        }
    }
    /* the batch call: 64 streams of ragged lengths, 4 threads */
    {
        enum { N = 64 };
        uint64_t in_off[N + 1], out_off[N + 1];
        uint32_t out_len[N];
        in_off[0] = out_off[0] = 0;
        for (int i = 0; i < N; i++) {
            size_t len = (i % 8 == 7) ? 0 : 1 + rnd() % 3000;
            in_off[i + 1] = in_off[i] + len;
            out_off[i + 1] = out_off[i] + fdo_compress_bound(len);
        }
        uint8_t *bin = (uint8_t *)malloc(in_off[N] ? in_off[N] : 1);
        uint8_t *bout = (uint8_t *)malloc(out_off[N]);
        for (int i = 0; i < N; i++) {
            fill(bin + in_off[i], (size_t)(in_off[i + 1] - in_off[i]), i % 6);
        }
        for (size_t l = 0; l < nlevels; l++) {
            fdo_level_counters_reset();
            fdo_deflate_level_batch(bin, in_off, bout, out_off, out_len, N, levels[l], 4);
            for (int i = 0; i < N; i++) {
                failures += check(bin + in_off[i], (size_t)(in_off[i + 1] - in_off[i]), levels[l], bout + out_off[i], out_len[i], back);
                streams++;
            }
        }
        uint64_t c[FDO_LEVEL_COUNTERS];
        fdo_level_counters(c, FDO_LEVEL_COUNTERS);
        if (c[0] == 0) { /* steps2 of the last level's batch */
            fprintf(stderr, "FAIL: the batch left no counters\n");
            failures++;
        }
        free(bin);
        free(bout);
    }
    free(in);
    free(back);
    printf("levels_selftest: %zu streams, %d failures\n", streams, failures);
    return failures ? 1 : 0;
}
