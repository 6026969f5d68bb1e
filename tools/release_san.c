/* The release order's host side (upe_release_order_host, upe_release_flush,
 * upe_amd/csrc/upe_host.c) on the CPU, stand-alone: `make -C upe_amd/csrc release-san` builds this
 * file with upe_host.c under the host sanitizers (-fsanitize=address,undefined) and runs it.
 * Expected values come from a sequential loop over the packets written out here, in the order of
 * the reference's worker_main (src/worker.c:280-303).  Every array is a heap block of exactly the
 * entries the contract names, so a read or a write past them is reported. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/upe_gpu.h"

static int g_bad = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "release_san:%d: %s\n", __LINE__, #cond);     \
            ++g_bad;                                                      \
        }                                                                 \
    } while (0)

#define POISON 0xA5A5A5A5u

static uint32_t *block(size_t count, uint32_t fill) {
    uint32_t *p = malloc(count ? count * sizeof *p : 1);
    if (!p) abort();
    for (size_t k = 0; k < count; k++) p[k] = fill;
    return p;
}

/* verdict words: every code, the reply flag on some packets of any code, rule bits */
static uint32_t word(size_t i, uint32_t seed) {
    uint32_t x = (uint32_t)i * 2654435761u + seed * 40503u;
    x ^= x >> 13;
    uint32_t v = (x % 3 == 0) ? UPE_V_FWD : x % 7;
    if (x % 11 == 0) v |= UPE_VF_ARP_REPLY;
    return v | (1 + i % 5) << 8;
}

/* an event log the callbacks write and the expectation is compared with */
enum { EV_SEND_ONE = 1, EV_RELEASE, EV_SEND };
typedef struct {
    uint32_t *ev;   /* kind, value pairs */
    size_t count, cap;
    const uint8_t *frames;
} log_t;

static void put(log_t *l, uint32_t kind, uint32_t value) {
    if (l->count == l->cap) abort();
    l->ev[2 * l->count] = kind;
    l->ev[2 * l->count + 1] = value;
    l->count++;
}

static int cb_send_one(void *user, const uint8_t *frame, size_t len) {
    log_t *l = user;
    put(l, EV_SEND_ONE, (uint32_t)((frame - l->frames) / 64));
    CHECK(len == 16 + (size_t)((frame - l->frames) / 64) % 48);
    return 0;
}

static int cb_send(void *user, const uint8_t *const *frames, const size_t *lens, int count) {
    log_t *l = user;
    for (int k = 0; k < count; k++) {
        put(l, EV_SEND, (uint32_t)((frames[k] - l->frames) / 64));
        CHECK(lens[k] == 16 + (size_t)((frames[k] - l->frames) / 64) % 48);
    }
    put(l, EV_SEND, POISON); /* the end of one call */
    return count - 1;        /* one frame not sent */
}

static void cb_release(void *user, const uint32_t *handles, size_t count) {
    log_t *l = user;
    CHECK(count > 0);
    for (size_t k = 0; k < count; k++) put(l, EV_RELEASE, handles[k]);
}

static const upe_release_ops_t kOps = {cb_send_one, cb_send, cb_release};

/* One batch: n packets, bursts by `first` (nb + 1 offsets) and, when burst != 0, passed as that
 * fixed size. */
static void run(size_t n, const uint32_t *first, size_t nb, uint32_t burst, uint32_t seed,
                int with_slot) {
    uint32_t *v = block(n, 0), *slot = with_slot ? block(n, 0) : NULL;
    for (size_t i = 0; i < n; i++) {
        v[i] = word(i, seed);
        if (slot) slot[i] = 1000u + (uint32_t)((i * 7) % 13);
    }
    uint32_t *order = block(n, POISON), *handle = with_slot ? block(n, POISON) : NULL;
    uint32_t *bf = block(nb, POISON);
    /* the loop: per burst, the exits' frees in packet order, then tx_bufs[] */
    uint32_t *e_order = block(n, 0), *e_bf = block(nb, 0), *e_reply = block(n, 0);
    upe_release_info_t want;
    memset(&want, 0, sizeof want);
    want.packets = n, want.bursts = nb, want.first_reply = UINT64_MAX;
    size_t k = 0, replies = 0;
    for (size_t b = 0; b < nb; b++) {
        uint32_t tx_bufs[UPE_TX_BATCH_MAX], tx_count = 0;
        for (uint32_t i = first[b]; i < first[b + 1]; i++) {
            const uint32_t code = UPE_VERDICT_CODE(v[i]);
            if (v[i] & UPE_VF_ARP_REPLY) {
                if (replies == 0) want.first_reply = i;
                e_reply[replies++] = i;
            }
            if (code == UPE_V_FWD) {
                tx_bufs[tx_count++] = i;
                want.forwarded++;
            } else {
                e_order[k++] = i;
                if (code == UPE_V_CONSUMED) want.consumed++;
                else want.dropped++;
            }
        }
        for (uint32_t j = 0; j < tx_count; j++) e_order[k++] = tx_bufs[j];
        e_bf[b] = tx_count;
    }
    want.replies = replies;
    CHECK(k == n);
    uint32_t *reply = block(replies, POISON); /* exactly the entries the call may write */
    upe_release_info_t info;
    memset(&info, 0x5A, sizeof info);
    const int rc = upe_release_order_host(v, n, burst ? NULL : first, burst ? 12345 : nb, burst,
                                          slot, order, handle, bf, reply, &info);
    CHECK(rc == 0);
    CHECK(memcmp(&info, &want, sizeof info) == 0);
    CHECK(memcmp(order, e_order, n * sizeof *order) == 0);
    CHECK(memcmp(bf, e_bf, nb * sizeof *bf) == 0);
    CHECK(memcmp(reply, e_reply, replies * sizeof *reply) == 0);
    if (slot)
        for (size_t j = 0; j < n; j++) CHECK(handle[j] == slot[order[j]]);

    /* the flush: replies of the burst, the exits' frees, the batch, its frees */
    uint8_t *frames = malloc(64 * n + 96);
    uint64_t *desc = malloc(n ? n * sizeof *desc : 1);
    if (!frames || !desc) abort();
    memset(frames, 0x11, 64 * n + 96);
    for (size_t i = 0; i < n; i++) desc[i] = (uint64_t)(64 * i) << 16 | (16 + i % 48);
    log_t got = {block(2 * (3 * n + nb + 1), 0), 0, 3 * n + nb + 1, frames};
    log_t exp = {block(2 * (3 * n + nb + 1), 0), 0, 3 * n + nb + 1, frames};
    uint64_t e_fwd = 0, e_drp = 0;
    size_t q = 0;
    for (size_t b = 0; b < nb; b++) {
        const size_t s = first[b], e = first[b + 1], r = e - s - e_bf[b];
        for (; q < replies && e_reply[q] < e; q++) put(&exp, EV_SEND_ONE, e_reply[q]);
        for (size_t j = s; j < s + r; j++)
            put(&exp, EV_RELEASE, slot ? slot[e_order[j]] : e_order[j]);
        if (!e_bf[b]) continue;
        for (size_t j = s + r; j < e; j++) put(&exp, EV_SEND, e_order[j]);
        put(&exp, EV_SEND, POISON);
        e_fwd += e_bf[b] - 1, e_drp += 1;
        for (size_t j = s + r; j < e; j++)
            put(&exp, EV_RELEASE, slot ? slot[e_order[j]] : e_order[j]);
    }
    uint64_t fwd = 0, drp = 0;
    CHECK(upe_release_flush(frames, desc, order, handle, burst ? NULL : first, nb, burst, n, bf,
                            reply, replies, &kOps, &got, &fwd, &drp) == 0);
    CHECK(got.count == exp.count);
    CHECK(memcmp(got.ev, exp.ev, 2 * exp.count * sizeof *exp.ev) == 0);
    CHECK(fwd == e_fwd && drp == e_drp);

    /* refused lists: nothing is called */
    if (n >= 4 && nb >= 2) {
        got.count = 0;
        const uint32_t keep = bf[0];
        bf[0] = first[1] + 1;
        CHECK(upe_release_flush(frames, desc, order, handle, burst ? NULL : first, nb, burst, n,
                                bf, reply, replies, &kOps, &got, NULL, NULL) == -1);
        bf[0] = keep;
        const uint32_t o = order[0];
        order[0] = first[1]; /* the next burst's */
        CHECK(upe_release_flush(frames, desc, order, handle, burst ? NULL : first, nb, burst, n,
                                bf, reply, replies, &kOps, &got, NULL, NULL) == -1);
        order[0] = o;
        if (replies >= 2) {
            const uint32_t r1 = reply[1];
            reply[1] = reply[0];
            CHECK(upe_release_flush(frames, desc, order, handle, burst ? NULL : first, nb, burst,
                                    n, bf, reply, replies, &kOps, &got, NULL, NULL) == -1);
            reply[1] = (uint32_t)n;
            CHECK(upe_release_flush(frames, desc, order, handle, burst ? NULL : first, nb, burst,
                                    n, bf, reply, replies, &kOps, &got, NULL, NULL) == -1);
            reply[1] = r1;
        }
        CHECK(got.count == 0);
    }
    free(v), free(slot), free(order), free(handle), free(bf), free(e_order), free(e_bf);
    free(e_reply), free(reply), free(frames), free(desc), free(got.ev), free(exp.ev);
}

/* offset arrays that are not valid: *info in full, nothing else touched, the flush refuses */
static void run_bad(size_t n) {
    const size_t nb = (n + 63) / 64;
    uint32_t *v = block(n, 0), *good = block(nb + 2, 0);
    for (size_t i = 0; i < n; i++) v[i] = word(i, 9);
    for (size_t b = 0; b <= nb; b++) good[b] = b * 64 < n ? (uint32_t)(b * 64) : (uint32_t)n;
    for (int kind = 0; kind < 5; kind++) {
        uint32_t *f = block(nb + 2, 0);
        size_t cnt = nb;
        memcpy(f, good, (nb + 1) * sizeof *f);
        uint64_t bad = 1;
        if (kind == 0) f[0] = 1;
        else if (kind == 1) f[nb] = (uint32_t)n + 1, bad = n % 64 == 0 ? 2 : 1;
        else if (kind == 2) { /* a zero-length burst */
            memmove(f + 2, f + 1, nb * sizeof *f);
            cnt = nb + 1;
        } else if (kind == 3) f[1] = 65;
        else f[1] = good[2], f[2] = good[1], bad = 3; /* descending */
        uint32_t *order = block(n, POISON), *bf = block(cnt, POISON), *reply = block(n, POISON);
        upe_release_info_t info, fixed;
        CHECK(upe_release_order_host(v, n, f, cnt, 0, NULL, order, NULL, bf, reply, &info) == 0);
        CHECK(upe_release_order_host(v, n, NULL, 0, 64, NULL, order, NULL, bf, NULL, &fixed) == 0);
        CHECK(info.bad_bursts == bad && info.bursts == cnt && info.packets == n);
        CHECK(info.forwarded == fixed.forwarded && info.consumed == fixed.consumed &&
              info.dropped == fixed.dropped && info.replies == fixed.replies &&
              info.first_reply == fixed.first_reply);
        /* the fixed call wrote order and bf[0 .. nb); the bad one before it nothing */
        for (size_t k = 0; k < n; k++) order[k] = POISON;
        for (size_t k = 0; k < cnt; k++) bf[k] = POISON;
        CHECK(upe_release_order_host(v, n, f, cnt, 0, NULL, order, NULL, bf, reply, &info) == 0);
        for (size_t k = 0; k < n; k++) CHECK(order[k] == POISON && reply[k] == POISON);
        for (size_t k = 0; k < cnt; k++) CHECK(bf[k] == POISON);
        log_t got = {block(2, 0), 0, 0, NULL}; /* any callback aborts */
        uint8_t frames[8] = {0};
        uint64_t *desc = calloc(n, sizeof *desc);
        for (size_t k = 0; k < n; k++) order[k] = (uint32_t)k;
        for (size_t k = 0; k < cnt; k++) bf[k] = 0;
        CHECK(upe_release_flush(frames, desc, order, NULL, f, cnt, 0, n, bf, NULL, 0, &kOps, &got,
                                NULL, NULL) == -1);
        free(f), free(order), free(bf), free(reply), free(got.ev), free(desc);
    }
    free(v), free(good);
}

static void run_refused(void) {
    uint32_t v[8] = {4, 0, 4, 5, 1, 4, 2, 4}, first[3] = {0, 3, 8}, out[8], bf[8];
    upe_release_info_t info;
    memset(&info, 0, sizeof info);
    CHECK(upe_release_order_host(v, 8, NULL, 0, 0, NULL, out, NULL, bf, NULL, &info) == -1);
    CHECK(upe_release_order_host(v, 8, NULL, 0, 65, NULL, out, NULL, bf, NULL, &info) == -1);
    CHECK(upe_release_order_host(v, 8, first, 0, 0, NULL, out, NULL, bf, NULL, &info) == -1);
    CHECK(upe_release_order_host(v, 8, first, 9, 0, NULL, out, NULL, bf, NULL, &info) == -1);
    CHECK(upe_release_order_host(v, 8, first, 2, 0, v, out, NULL, bf, NULL, &info) == -1);
    CHECK(upe_release_order_host(v, 8, first, 2, 0, NULL, out, out, bf, NULL, &info) == -1);
    CHECK(upe_release_order_host(v, 8, first, 2, 0, NULL, out, NULL, bf, NULL, NULL) == -1);
    CHECK(upe_release_order_host(NULL, 8, first, 2, 0, NULL, out, NULL, bf, NULL, &info) == -1);
    CHECK(upe_release_order_host(v, 8, first, 2, 0, NULL, NULL, NULL, bf, NULL, &info) == -1);
    CHECK(upe_release_order_host(v, 8, first, 2, 0, NULL, out, NULL, NULL, NULL, &info) == -1);
    CHECK(upe_release_order_host(v, 0xFFFFFFFFull - UPE_RELEASE_BLOCK + 1, NULL, 0, 32, NULL, out,
                                 NULL, bf, NULL, &info) == -1);
    CHECK(upe_host_last_error()[0] != 0);
    CHECK(info.packets == 0 && info.first_reply == 0);
    CHECK(upe_release_order_host(NULL, 0, NULL, 0, 32, NULL, NULL, NULL, NULL, NULL, &info) == 0);
    CHECK(info.packets == 0 && info.bursts == 0 && info.first_reply == UINT64_MAX &&
          info.bad_bursts == 0 && info.replies == 0);
    CHECK(upe_release_flush(NULL, NULL, NULL, NULL, NULL, 0, 32, 0, NULL, NULL, 0, NULL, NULL,
                            NULL, NULL) == 0);
    CHECK(upe_release_flush(NULL, NULL, NULL, NULL, NULL, 0, 0, 0, NULL, NULL, 0, NULL, NULL,
                            NULL, NULL) == -1);
}

int main(void) {
    static const uint32_t kFixed[] = {1, 31, 32, 33, 48, 63, 64};
    static const size_t kSizes[] = {1, 63, 64, 65, 257, 1025, 4133};
    for (size_t a = 0; a < sizeof kSizes / sizeof *kSizes; a++) {
        const size_t n = kSizes[a];
        for (size_t j = 0; j < sizeof kFixed / sizeof *kFixed; j++) {
            const uint32_t burst = kFixed[j];
            const size_t nb = (n + burst - 1) / burst;
            uint32_t *first = block(nb + 1, 0);
            for (size_t b = 0; b <= nb; b++)
                first[b] = b * burst < n ? (uint32_t)(b * burst) : (uint32_t)n;
            run(n, first, nb, burst, (uint32_t)(a * 8 + j), (int)(j & 1));
            free(first);
        }
        /* lengths cycling 1..64, and all ones */
        uint32_t *first = block(n + 1, 0);
        size_t nb = 0;
        while (first[nb] < n) {
            const size_t next = first[nb] + 1 + nb % 64;
            first[nb + 1] = next < n ? (uint32_t)next : (uint32_t)n;
            nb++;
        }
        run(n, first, nb, 0, 77, 1);
        for (size_t b = 0; b <= n; b++) first[b] = (uint32_t)b;
        run(n, first, n, 0, 78, 0);
        free(first);
    }
    run_bad(130);
    run_bad(1024);
    run_refused();
    if (g_bad) {
        fprintf(stderr, "release_san: %d checks failed\n", g_bad);
        return 1;
    }
    printf("release_san: OK\n");
    return 0;
}
