/* upe_neigh_learn_host (upe_rules.cpp) on the CPU, stand-alone: `make -C upe_amd/csrc learn-san`
 * builds this file with upe_rules.cpp and upe_host.c under the host sanitizers
 * (-fsanitize=address,undefined) and runs it.  Slot arrays filled through upe_neigh_apply_writes
 * (so every entry is one a probe reaches): no table, 8 slots with 0, 1 and 2 of them free, 1024
 * slots a third full; each compiled with room 0, 3 and 4096 (upe_neigh_compile_room) and taught
 * batches of 0, 1, 700 and 2500 records: new addresses (some twice, the MAC changing), refreshes,
 * records of no kind.  Checked: the contract's loop (include/upe_gpu.h), written out below over the
 * image read back with upe_neigh_image_read and with the slot hashes restated here, gives the same
 * index bytes, deferred ranks and info; and, where nothing is deferred, the learnt image answers
 * every taught address as the image compiled from the arrays with the records applied does.  The
 * records, ranks, answers and slot copies are heap blocks of exactly their size, so a read or write
 * past either end is reported.  C: the ABI as a C caller sees it. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/upe_gpu.h"

/* the library's error slot, which upe_gpu.hip owns in the library */
static char g_msg[256];
int upe_gpu_set_last_error(const char *msg) {
    snprintf(g_msg, sizeof g_msg, "%s", msg ? msg : "");
    return -1;
}

static uint32_t g_x = 0x2545F491u;
static uint32_t rnd(void) { g_x ^= g_x << 13; g_x ^= g_x >> 17; g_x ^= g_x << 5; return g_x; }

static void *block(size_t n, size_t size) {
    void *p = calloc(n ? n : 1, size);
    if (!p) abort();
    return p;
}
#define CHECK(c) do { if (!(c)) { printf("learn_san: line %d: %s (%s)\n", __LINE__, #c, g_msg); exit(1); } } while (0)

/* slot1 / slot2 / slot3 and fold_v6 of csrc/upe_dev.h, restated */
static void cands(uint32_t k, uint32_t seed, uint32_t bits, uint32_t c[3]) {
    uint32_t x;
    c[0] = ((k ^ seed) * 0x9E3779B1u) >> (32 - bits);
    x = (k ^ seed) * 0x85EBCA77u;
    c[1] = ((x ^ (x >> 16)) * 0xC2B2AE3Du) >> (32 - bits);
    x = (k ^ (seed * 0x9E3779B9u)) * 0x27D4EB2Fu;
    c[2] = ((x ^ (x >> 15)) * 0x165667B1u) >> (32 - bits);
}
static uint32_t le32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
static uint32_t fold(const uint32_t w[4]) {
    return (w[0] * 0x9E3779B1u) ^ (w[1] * 0x85EBCA77u) ^ (w[2] * 0xC2B2AE3Du) ^ (w[3] * 0x27D4EB2Fu);
}

static upe_ctrl_write_t record(int kind, uint32_t tag, uint32_t rank) {
    upe_ctrl_write_t w;
    memset(&w, 0, sizeof w);
    w.index = 2 * rank + 1;
    w.kind = (uint8_t)kind;
    w.mac_off = 22;
    for (int j = 0; j < 6; j++) w.mac[j] = (uint8_t)(0x10 * j + rank + (rank >> 8));
    const uint32_t a = 0x0A000000u + tag * 2654435761u;
    for (int j = 0; j < (kind == UPE_CW_ARP ? 4 : 16); j++)
        w.ip[j] = (uint8_t)((a >> (8 * (j % 4))) + (j / 4) * (tag + 1));
    return w;
}

/* The contract's loop on one read-back index. */
typedef struct {
    upe_neigh_image_info_t m;
    uint32_t *arp, *ndp; /* 4 and 8 words per slot */
    size_t arp_slots, ndp_slots;
} index_t;

static index_t index_read(const upe_neigh_image_t *im) {
    index_t x;
    CHECK(upe_neigh_image_read(im, &x.m, NULL, 0, NULL, 0) == 0);
    x.arp_slots = x.m.arp_bits ? (size_t)1 << x.m.arp_bits : 1;
    x.ndp_slots = x.m.ndp_bits ? (size_t)1 << x.m.ndp_bits : 1;
    x.arp = block(x.arp_slots, 16);
    x.ndp = block(x.ndp_slots, 32);
    CHECK(upe_neigh_image_read(im, NULL, x.arp, x.arp_slots * 16, x.ndp, x.ndp_slots * 32) == 0);
    CHECK(upe_neigh_image_read(im, NULL, x.arp, x.arp_slots * 16 + 16, NULL, 0) == -1);
    return x;
}
static void index_free(index_t *x) { free(x->arp); free(x->ndp); }

static void loop(index_t *x, const upe_ctrl_write_t *w, size_t n, uint32_t *defer,
                 upe_neigh_learn_info_t *info) {
    memset(info, 0, sizeof *info);
    info->records = n;
    info->first_defer = UINT64_MAX;
    for (size_t i = 0; i < n; i++) {
        const int v6 = w[i].kind == UPE_CW_NDP;
        int done = 0, put_off = !(v6 || w[i].kind == UPE_CW_ARP);
        if (!put_off) {
            const uint32_t bits = v6 ? x->m.ndp_bits : x->m.arp_bits;
            const uint32_t seed = v6 ? x->m.ndp_seed : x->m.arp_seed;
            uint32_t *free_slots = v6 ? &x->m.ndp_free : &x->m.arp_free;
            uint32_t *t = v6 ? x->ndp : x->arp;
            const size_t stride = v6 ? 8 : 4, nw = v6 ? 4 : 1, mw = v6 ? 4 : 1;
            uint32_t a[4] = {le32(w[i].ip), le32(w[i].ip + 4), le32(w[i].ip + 8), le32(w[i].ip + 12)};
            const uint32_t lo = le32(w[i].mac), hi = (uint32_t)w[i].mac[4] | (uint32_t)w[i].mac[5] << 8;
            uint32_t c[3] = {0, 0, 0};
            if (bits) cands(v6 ? fold(a) : a[0], seed, bits, c);
            for (int q = 0; bits && q < 3 && !done; q++) {
                uint32_t *s = t + stride * c[q];
                if (((s[mw + 1] >> 16) & 1u) && memcmp(s, a, 4 * nw) == 0) {
                    s[mw] = lo;
                    s[mw + 1] = (s[mw + 1] & 0xFFFF0000u) | hi;
                    info->patched++;
                    done = 1;
                }
            }
            if (!done && !(v6 ? x->m.ndp_insertable : x->m.arp_insertable)) put_off = 1;
            if (!done && !put_off && *free_slots == 0) {
                info->dropped++;
                done = 1;
            }
            for (int q = 0; !done && !put_off && q < 3; q++) {
                uint32_t *s = t + stride * c[q];
                if ((s[mw + 1] >> 16) & 1u) continue;
                memset(s, 0, 4 * stride);
                memcpy(s, a, 4 * nw);
                s[mw] = lo;
                s[mw + 1] = hi | 1u << 16;
                --*free_slots;
                info->inserted++;
                done = 1;
            }
            if (!done) put_off = 1;
        }
        if (put_off) {
            if (info->deferred == 0) info->first_defer = i;
            defer[info->deferred++] = (uint32_t)i;
        }
    }
    info->arp_free = x->m.arp_free;
    info->ndp_free = x->m.ndp_free;
}

static size_t g_checks;

static void run(upe_arp_entry_t *arp, size_t acap, upe_ndp_entry_t *ndp, size_t ncap, size_t room,
                size_t n, uint32_t known) {
    upe_neigh_image_t *im = upe_neigh_compile_room(arp, acap, ndp, ncap, room, room);
    CHECK(im);
    if (room == 0) { /* byte for byte upe_neigh_compile's image */
        upe_neigh_image_t *plain = upe_neigh_compile(arp, acap, ndp, ncap);
        CHECK(plain);
        index_t p = index_read(plain), q = index_read(im);
        CHECK(memcmp(&p.m, &q.m, sizeof p.m) == 0 && p.arp_slots == q.arp_slots &&
              p.ndp_slots == q.ndp_slots && memcmp(p.arp, q.arp, 16 * p.arp_slots) == 0 &&
              memcmp(p.ndp, q.ndp, 32 * p.ndp_slots) == 0);
        index_free(&p), index_free(&q);
        upe_neigh_image_free(plain);
    }
    upe_ctrl_write_t *w = block(n, sizeof *w);
    for (size_t i = 0; i < n; i++) {
        const uint32_t r = rnd();
        const int kind = r % 29 == 0 ? (int)(r % 3) * 5 : (r & 1) ? UPE_CW_ARP : UPE_CW_NDP;
        /* a third refresh the table's addresses (tags below `known`), the rest are new, from a
         * pool small enough that some come twice */
        const uint32_t tag = (r >> 8) % 3 == 0 && known ? (r >> 12) % known
                                                        : 100000u + (r >> 12) % (uint32_t)(n + 1);
        w[i] = record(kind, tag, (uint32_t)i);
    }
    index_t x = index_read(im);
    uint32_t *want_defer = block(n, 4), *defer = block(n, 4);
    upe_neigh_learn_info_t want, info;
    loop(&x, w, n, want_defer, &want);
    memset(defer, 0xEE, 4 * (n ? n : 1));
    CHECK(upe_neigh_learn_host(im, n ? w : NULL, n, defer, &info) == 0);
    CHECK(memcmp(&info, &want, sizeof info) == 0);
    CHECK(info.patched + info.inserted + info.dropped + info.deferred == n);
    CHECK(memcmp(defer, want_defer, 4 * info.deferred) == 0);
    for (size_t i = info.deferred; i < n; i++) CHECK(defer[i] == 0xEEEEEEEEu);
    index_t y = index_read(im);
    CHECK(memcmp(&x.m, &y.m, sizeof x.m) == 0);
    CHECK(memcmp(x.arp, y.arp, 16 * x.arp_slots) == 0 && memcmp(x.ndp, y.ndp, 32 * x.ndp_slots) == 0);
    if (info.deferred == 0) {
        /* the records through the reference's update, compiled again: the same answers */
        upe_arp_entry_t *a2 = block(acap, sizeof *a2);
        upe_ndp_entry_t *n2 = block(ncap, sizeof *n2);
        if (acap) memcpy(a2, arp, acap * sizeof *a2);
        if (ncap) memcpy(n2, ndp, ncap * sizeof *n2);
        CHECK(upe_neigh_apply_writes(acap ? a2 : NULL, acap, ncap ? n2 : NULL, ncap, n ? w : NULL, n,
                                     5, NULL) == 0);
        upe_neigh_image_t *again = upe_neigh_compile(acap ? a2 : NULL, acap, ncap ? n2 : NULL, ncap);
        CHECK(again);
        upe_flow_key_t *k = block(n, sizeof *k);
        uint64_t *got = block(n, 8), *exp = block(n, 8);
        for (size_t i = 0; i < n; i++) {
            k[i].ip_ver = w[i].kind;
            memcpy(k[i].dst_ip.v6, w[i].ip, 16);
        }
        CHECK(upe_neigh_image_lookup_host(im, n ? k : NULL, n, got) == 0);
        CHECK(upe_neigh_image_lookup_host(again, n ? k : NULL, n, exp) == 0);
        CHECK(memcmp(got, exp, 8 * n) == 0);
        upe_neigh_image_info_t m2;
        CHECK(upe_neigh_image_read(again, &m2, NULL, 0, NULL, 0) == 0);
        CHECK(m2.arp_free == info.arp_free && m2.ndp_free == info.ndp_free);
        free(k), free(got), free(exp), free(a2), free(n2);
        upe_neigh_image_free(again);
    }
    index_free(&x), index_free(&y);
    free(w), free(want_defer), free(defer);
    upe_neigh_image_free(im);
    g_checks++;
}

/* `cap` slots with `fill` entries of tags 0 .. fill - 1, put in by the reference's update */
static void tables(size_t cap, uint32_t fill, upe_arp_entry_t **arp, upe_ndp_entry_t **ndp) {
    *arp = block(cap, sizeof **arp);
    *ndp = block(cap, sizeof **ndp);
    upe_ctrl_write_t *w = block(2 * fill, sizeof *w);
    for (uint32_t j = 0; j < fill; j++) {
        w[2 * j] = record(UPE_CW_ARP, j, j);
        w[2 * j + 1] = record(UPE_CW_NDP, j, j);
    }
    if (cap)
        CHECK(upe_neigh_apply_writes(*arp, cap, *ndp, cap, w, 2 * fill, 1, NULL) == 0);
    free(w);
}

int main(void) {
    static const size_t caps[] = {0, 8, 8, 8, 1024};
    static const uint32_t fills[] = {0, 8, 7, 6, 340};
    static const size_t rooms[] = {0, 3, 4096}, counts[] = {0, 1, 700, 2500};
    for (size_t t = 0; t < sizeof caps / sizeof *caps; t++) {
        upe_arp_entry_t *arp;
        upe_ndp_entry_t *ndp;
        tables(caps[t], fills[t], &arp, &ndp);
        for (size_t r = 0; r < 3; r++)
            for (size_t c = 0; c < 4; c++)
                run(caps[t] ? arp : NULL, caps[t], caps[t] ? ndp : NULL, caps[t], rooms[r],
                    counts[c], fills[t]);
        free(arp), free(ndp);
    }
    upe_neigh_learn_info_t info;
    CHECK(upe_neigh_learn_host(NULL, NULL, 0, NULL, &info) == -1);
    CHECK(upe_neigh_compile_room(NULL, 0, NULL, 0, ((size_t)1 << 30) + 1, 0) == NULL);
    printf("learn_san: ok (%zu runs)\n", g_checks);
    return 0;
}
