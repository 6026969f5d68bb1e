/* The host latency histogram (upe_latency_*, upe_amd/csrc/upe_host.c) on the CPU, stand-alone:
 * `make -C upe_amd/csrc latency-san` builds this file with upe_host.c under the host sanitizers
 * (-fsanitize=address,undefined) and runs it.  Expected values come from a loop written here in
 * integer arithmetic only: at 2 cycles per ns and cycle counts below 2^53 the library's double
 * arithmetic is exact and ns = cycles / 2; the few samples beyond that (the conversion's
 * rounding, saturation, the wrapping sum) are worked out by hand.  The batch arrays are heap
 * blocks of exactly n entries, so a read past either end is reported. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/upe_gpu.h"

static int g_bad = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "latency_san:%d: %s\n", __LINE__, #cond);        \
            ++g_bad;                                                         \
        }                                                                    \
    } while (0)

static const uint64_t kBounds[UPE_LATENCY_BUCKETS] = {UPE_LATENCY_BOUNDS};

/* one sample of `ns` into a histogram kept by hand */
static void hand(upe_latency_hist_t *h, uint64_t ns) {
    int b = 0;
    while (b < UPE_LATENCY_BUCKETS - 1 && ns >= kBounds[b]) b++;
    h->buckets[b] += 1;
    h->total_count += 1;
    h->sum_ns += ns;
    if (ns < h->min_ns) h->min_ns = ns;
    if (ns > h->max_ns) h->max_ns = ns;
}

static void hand_init(upe_latency_hist_t *h) {
    memset(h, 0, sizeof *h);
    h->min_ns = 1000000;
}

static int same(const upe_latency_hist_t *a, const upe_latency_hist_t *b) {
    return memcmp(a, b, sizeof *a) == 0;
}

static void bucket_edges(void) {
    upe_latency_hist_t got, want;
    upe_latency_init(&got);
    hand_init(&want);
    CHECK(same(&got, &want));
    for (int i = 0; i < UPE_LATENCY_BUCKETS; i++)
        for (int d = -3; d <= 3; d++) {
            const uint64_t cycles = 2 * kBounds[i] + (uint64_t)(int64_t)d;
            CHECK(upe_latency_record(&got, cycles, 2.0) == 0);
            hand(&want, cycles / 2);
        }
    CHECK(same(&got, &want));
    /* by hand: around each bound, ns = bound - 2 and bound - 1 (twice) below it, bound (twice)
     * and bound + 1 (twice) at or above it */
    CHECK(got.buckets[0] == 3 && got.buckets[1] == 7 && got.buckets[6] == 7);
    CHECK(got.buckets[7] == 4 + 7 && got.total_count == 56);
    CHECK(got.min_ns == 98 && got.max_ns == 1000001);
    CHECK(upe_latency_record(&got, 0, 2.0) == 0);
    CHECK(got.min_ns == 0 && got.buckets[0] == 4);
}

static void rounding_saturation_and_wrap(void) {
    upe_latency_hist_t got, want;
    upe_latency_init(&got);
    hand_init(&want);
    /* (double)(2^53 + 1) is a tie: to even, 2^53; (double)(2^53 + 3) = 2^53 + 4 */
    CHECK(upe_latency_record(&got, (1ull << 53) + 1, 1.0) == 0);
    hand(&want, 1ull << 53);
    CHECK(upe_latency_record(&got, (1ull << 53) + 3, 1.0) == 0);
    hand(&want, (1ull << 53) + 4);
    CHECK(same(&got, &want));
    /* (double)(2^64 - 1) = 2^64: at 2 cycles per ns that is 2^63, and two of them wrap the sum
     * back to what it was */
    const uint64_t before = got.sum_ns;
    CHECK(upe_latency_record(&got, UINT64_MAX, 2.0) == 0);
    CHECK(got.max_ns == 1ull << 63 && got.sum_ns == before + (1ull << 63));
    CHECK(upe_latency_record(&got, UINT64_MAX, 2.0) == 0);
    CHECK(got.sum_ns == before && got.total_count == 4 && got.buckets[7] == 4);
    /* quotients of 2^64 or more saturate; the largest double below 2^64 does not */
    upe_latency_init(&got);
    CHECK(upe_latency_record(&got, UINT64_MAX, 1.0) == 0 && got.max_ns == UINT64_MAX);
    upe_latency_init(&got);
    CHECK(upe_latency_record(&got, UINT64_MAX - 1024, 1.0) == 0);
    CHECK(got.max_ns == UINT64_MAX - 2047 && got.sum_ns == UINT64_MAX - 2047);
    upe_latency_init(&got);
    CHECK(upe_latency_record(&got, 1ull << 63, 0.5) == 0 && got.max_ns == UINT64_MAX);
    CHECK(upe_latency_record(&got, 1, 1e-300) == 0 && got.total_count == 2);
    CHECK(upe_latency_record(&got, 7, 4.9406564584124654e-324) == 0); /* a subnormal: +inf */
    CHECK(got.sum_ns == UINT64_MAX - 2 && got.min_ns == 1000000 && got.buckets[7] == 3);
    CHECK(upe_latency_record(&got, 0, 4.9406564584124654e-324) == 0 && got.min_ns == 0);
}

static void refusals(void) {
    upe_latency_hist_t got, want;
    upe_latency_init(&got);
    CHECK(upe_latency_record(&got, 1000, 2.0) == 0);
    want = got;
    const double bad[] = {0.0, -0.0, -1.5, NAN, INFINITY, -INFINITY};
    const uint64_t ts[2] = {5, 6};
    for (size_t i = 0; i < sizeof bad / sizeof bad[0]; i++) {
        CHECK(upe_latency_record(&got, 1000, bad[i]) == -1);
        CHECK(upe_latency_record_batch(&got, ts, NULL, 2, 100, bad[i]) == -1);
        CHECK(upe_host_last_error()[0] != '\0');
    }
    CHECK(upe_latency_record(NULL, 1, 2.0) == -1);
    CHECK(upe_latency_record_batch(&got, NULL, NULL, 2, 100, 2.0) == -1);
    CHECK(upe_latency_record_batch(NULL, ts, NULL, 2, 100, 2.0) == -1);
    CHECK(upe_latency_record_batch(&got, NULL, NULL, 0, 100, 2.0) == 0);
    CHECK(same(&got, &want));
}

static void batch(void) {
    enum { N = 1000 };
    uint64_t *ts = malloc(N * sizeof *ts);
    uint32_t *v = malloc(N * sizeof *v);
    if (!ts || !v) abort();
    const uint64_t now = 1ull << 40;
    upe_latency_hist_t want, want_all;
    hand_init(&want);
    hand_init(&want_all);
    uint64_t x = 88172645463325252ull; /* xorshift64 */
    for (int k = 0; k < N; k++) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        const uint64_t cycles = (x >> 24) >> (x % 37);   /* below 2^40, every magnitude */
        const uint32_t code = (uint32_t)(k % 7), flags = (uint32_t)((x >> 8) & 0xF0);
        v[k] = code | flags | (uint32_t)(k << 8);
        ts[k] = k % 5 == 3 ? 0 : now - cycles;           /* now - cycles > 0 */
        if (ts[k] == 0) continue;
        hand(&want_all, cycles / 2);
        if (code != UPE_V_CONSUMED) hand(&want, cycles / 2);
    }
    upe_latency_hist_t got, one;
    upe_latency_init(&got);
    CHECK(upe_latency_record_batch(&got, ts, v, N, now, 2.0) == 0);
    CHECK(same(&got, &want));
    CHECK(want.total_count < want_all.total_count && want_all.total_count < N);
    upe_latency_init(&got);
    CHECK(upe_latency_record_batch(&got, ts, NULL, N, now, 2.0) == 0);
    CHECK(same(&got, &want_all));
    /* in two halves, and merged from two histograms */
    upe_latency_init(&got);
    upe_latency_init(&one);
    CHECK(upe_latency_record_batch(&got, ts, v, N / 2, now, 2.0) == 0);
    CHECK(upe_latency_record_batch(&one, ts + N / 2, v + N / 2, N - N / 2, now, 2.0) == 0);
    upe_latency_merge(&got, &one);
    CHECK(same(&got, &want));
    /* a timestamp later than now wraps: 2^64 - 2 cycles, 2^63 ns */
    const uint64_t late = now + 2;
    upe_latency_init(&got);
    CHECK(upe_latency_record_batch(&got, &late, NULL, 1, now, 2.0) == 0);
    CHECK(got.max_ns == 1ull << 63 && got.total_count == 1);
    /* percentile: the first bucket at which the cumulative count reaches (uint64)(p * total) */
    for (int p = 0; p <= 1000; p++) {
        const double pc = p / 1000.0;
        const uint64_t target = (uint64_t)(pc * (double)want.total_count);
        uint64_t cum = 0, exp = kBounds[UPE_LATENCY_BUCKETS - 1];
        for (int i = 0; i < UPE_LATENCY_BUCKETS; i++) {
            cum += want.buckets[i];
            if (cum >= target) {
                exp = kBounds[i];
                break;
            }
        }
        CHECK(upe_latency_percentile(&want, pc) == exp);
    }
    upe_latency_init(&got);
    CHECK(upe_latency_percentile(&got, 0.5) == 0);
    CHECK(upe_latency_percentile(&want, -1.0) == 100 && upe_latency_percentile(&want, NAN) == 100);
    CHECK(upe_latency_percentile(&want, 1e300) == 1000000);
    free(ts);
    free(v);
}

int main(void) {
    bucket_edges();
    rounding_saturation_and_wrap();
    refusals();
    batch();
    if (g_bad) {
        fprintf(stderr, "latency_san: %d checks failed\n", g_bad);
        return 1;
    }
    printf("latency_san: ok\n");
    return 0;
}
