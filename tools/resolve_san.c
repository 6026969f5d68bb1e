/* The host side of the neighbour snapshot's two halves on the CPU, stand-alone: `make -C
 * upe_amd/csrc resolve-san` builds this file with upe_rules.cpp and upe_host.c under the host
 * sanitizers (-fsanitize=address,undefined) and runs it.  The slot arrays are the shapes of
 * tools/neigh_san.cpp (a table of no slots, one slot, a full table, a chain that wraps, an entry
 * behind an invalid slot, one address in two slots, the zero address, 4096 slots at about 0.7 with
 * holes, addresses of one fold_v6 and of one home slot).  Each goes through upe_neigh_compile (it
 * must succeed, or fail with a message where four addresses share a fold) and, with every stored
 * address, as many absent ones and the zero address as keys, through upe_neigh_lookup_host, whose
 * answers must equal a probe written out here (arp_get_mac, src/arp_table.c:55-80; ndp_get_mac,
 * src/ndp_table.c:67-86).  Tables, keys and results are heap blocks of exactly their size, so a
 * read or write past either end is reported.  C: the ABI as a C caller sees it. */
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

/* An address as words: ARP word 0 = the IPv4 address, NDP the 16 bytes as four LE words. */
typedef struct { uint32_t w[4]; } addr_t;

typedef struct {
    int v6;
    size_t cap;
    upe_arp_entry_t *arp; /* cap entries of the family's, the other NULL */
    upe_ndp_entry_t *ndp;
} table_t;

static table_t table_new(int v6, size_t cap) {
    table_t t = {v6, cap, NULL, NULL};
    if (cap && v6) t.ndp = calloc(cap, sizeof *t.ndp);
    if (cap && !v6) t.arp = calloc(cap, sizeof *t.arp);
    if (cap && !t.arp && !t.ndp) abort();
    return t;
}
static void table_free(table_t *t) { free(t->arp); free(t->ndp); }

static addr_t clip(int v6, addr_t k) {
    if (!v6) k.w[1] = k.w[2] = k.w[3] = 0;
    return k;
}
static size_t home(int v6, addr_t k) { return v6 ? k.w[0] ^ k.w[1] ^ k.w[2] ^ k.w[3] : k.w[0]; }
static int slot_valid(const table_t *t, size_t s) { return t->v6 ? t->ndp[s].valid : t->arp[s].valid; }
static const uint8_t *slot_mac(const table_t *t, size_t s) { return t->v6 ? t->ndp[s].mac : t->arp[s].mac; }
static addr_t slot_addr(const table_t *t, size_t s) {
    addr_t k = {{0, 0, 0, 0}};
    if (!t->v6) {
        k.w[0] = t->arp[s].ip;
    } else {
        for (int j = 0; j < 16; j++) k.w[j / 4] |= (uint32_t)t->ndp[s].ip[j] << (8 * (j % 4));
    }
    return k;
}
static int same(addr_t a, addr_t b) { return memcmp(a.w, b.w, sizeof a.w) == 0; }

/* An entry written straight into a slot; its MAC names the slot. */
static void put(table_t *t, size_t s, addr_t k, int valid) {
    const uint8_t mac[6] = {2, t->v6 ? 'n' : 'a', (uint8_t)(s >> 16), (uint8_t)(s >> 8), (uint8_t)s,
                            (uint8_t)rnd()};
    k = clip(t->v6, k);
    if (!t->v6) {
        t->arp[s].ip = k.w[0];
        memcpy(t->arp[s].mac, mac, 6);
        t->arp[s].valid = valid;
    } else {
        for (int j = 0; j < 16; j++) t->ndp[s].ip[j] = (uint8_t)(k.w[j / 4] >> (8 * (j % 4)));
        memcpy(t->ndp[s].mac, mac, 6);
        t->ndp[s].valid = valid;
    }
}
/* The reference's update: the first slot from the home slot that is invalid or holds the key. */
static void insert(table_t *t, addr_t k) {
    k = clip(t->v6, k);
    for (size_t i = 0; i < t->cap; i++) {
        const size_t s = (home(t->v6, k) + i) & (t->cap - 1);
        if (!slot_valid(t, s) || same(slot_addr(t, s), k)) {
            put(t, s, k, 1);
            return;
        }
    }
}
/* The reference's probe, as a d_mac word. */
static uint64_t probe(const table_t *t, addr_t k) {
    for (size_t i = 0; i < t->cap; i++) {
        const size_t s = (home(t->v6, k) + i) & (t->cap - 1);
        if (!slot_valid(t, s)) return 0;
        if (same(slot_addr(t, s), k)) {
            uint64_t v = 0;
            memcpy(&v, slot_mac(t, s), 6); /* a little-endian host, as the library's */
            return v | UPE_MAC_FOUND;
        }
    }
    return 0;
}
static addr_t homed(int v6, size_t cap, uint32_t h, uint32_t tag) {
    addr_t k = {{0, tag << 8, tag * 0x01010101u, 0}};
    k = clip(v6, k);
    k.w[0] = (uint32_t)((tag + 1) * cap) | h;
    k.w[0] ^= (k.w[1] ^ k.w[2] ^ k.w[3]) & (uint32_t)(cap - 1);
    return k;
}

static void set_key(upe_flow_key_t *key, int v6, addr_t k) {
    memset(key, 0xA7, sizeof *key); /* what is not asked for is noise */
    key->ip_ver = v6 ? 6 : 4;
    for (int j = 0; j < (v6 ? 16 : 4); j++) key->dst_ip.v6[j] = (uint8_t)(k.w[j / 4] >> (8 * (j % 4)));
}

/* compile (want_ok: it must succeed) and look every address up */
static int check(const char *what, const table_t *t, int want_ok) {
    g_msg[0] = 0;
    upe_neigh_image_t *im = upe_neigh_compile(t->arp, t->v6 ? 0 : t->cap, t->ndp, t->v6 ? t->cap : 0);
    if ((im != NULL) != (want_ok != 0) || (!im && !strstr(g_msg, "placement")))
        return fprintf(stderr, "%s %s: upe_neigh_compile %s (%s)\n", t->v6 ? "ndp" : "arp", what,
                       im ? "succeeded" : "failed", g_msg), 1;
    upe_neigh_image_free(im);
    size_t stored = 0;
    for (size_t s = 0; s < t->cap; s++) {
        const addr_t k = slot_addr(t, s);
        stored += slot_valid(t, s) || k.w[0] || k.w[1] || k.w[2] || k.w[3];
    }
    const size_t n = 2 * stored + 8 + 1 + 3;
    upe_flow_key_t *keys = malloc(n * sizeof *keys);
    uint64_t *want = malloc(n * sizeof *want), *got = malloc(n * sizeof *got);
    if (!keys || !want || !got) abort();
    size_t q = 0;
    for (size_t s = 0; s < t->cap; s++) {
        const addr_t k = slot_addr(t, s);
        if (!(slot_valid(t, s) || k.w[0] || k.w[1] || k.w[2] || k.w[3])) continue;
        set_key(&keys[q], t->v6, k);
        want[q++] = probe(t, k);
    }
    /* stored ones with a bit flipped (same chain, or the next) and random ones: whatever the
     * probe says of them */
    while (q < 2 * stored + 8) {
        addr_t k = stored && rnd() % 2 ? slot_addr(t, rnd() % t->cap)
                                       : (addr_t){{rnd(), rnd(), rnd(), rnd()}};
        if (rnd() % 4) k.w[rnd() % 4] ^= 1u << (rnd() % 32);
        k = clip(t->v6, k);
        set_key(&keys[q], t->v6, k);
        want[q++] = probe(t, k);
    }
    const addr_t zero = {{0, 0, 0, 0}};
    set_key(&keys[q], t->v6, zero);
    want[q++] = probe(t, zero);
    /* the other family's table is absent, and an ip_ver that is neither finds nothing */
    set_key(&keys[q], !t->v6, t->cap ? slot_addr(t, 0) : zero);
    want[q++] = 0;
    for (int ver = 0; ver <= 5; ver += 5) {
        set_key(&keys[q], t->v6, t->cap ? slot_addr(t, 0) : zero);
        keys[q].ip_ver = (uint8_t)ver;
        want[q++] = 0;
    }
    memset(got, 0x5C, n * sizeof *got);
    int bad = 0;
    if (q != n || upe_neigh_lookup_host(t->arp, t->v6 ? 0 : t->cap, t->ndp, t->v6 ? t->cap : 0, keys,
                                        n, got) != 0) {
        bad = fprintf(stderr, "%s %s: upe_neigh_lookup_host: %s\n", t->v6 ? "ndp" : "arp", what,
                      upe_host_last_error());
    } else {
        size_t hits = 0;
        for (size_t i = 0; i < n && !bad; i++) {
            hits += got[i] != 0;
            if (got[i] != want[i])
                bad = fprintf(stderr, "%s %s: key %zu: %016llx, the probe says %016llx\n",
                              t->v6 ? "ndp" : "arp", what, i, (unsigned long long)got[i],
                              (unsigned long long)want[i]);
        }
        if (!bad)
            printf("%s %s: %zu slots, %zu keys agree with the probe (%zu hit)\n",
                   t->v6 ? "ndp" : "arp", what, t->cap, n, hits);
    }
    free(keys);
    free(want);
    free(got);
    return bad != 0;
}

static int family(int v6) {
    int bad = 0;
    table_t t;
#define CASE(cap, what, ...)          \
    do {                              \
        t = table_new(v6, cap);       \
        __VA_ARGS__;                  \
        bad |= check(what, &t, 1);    \
        table_free(&t);               \
    } while (0)
    CASE(0, "capacity 0", (void)0);
    CASE(1, "capacity 1, empty", (void)0);
    CASE(1, "capacity 1, full", put(&t, 0, homed(v6, 1, 0, 5), 1));
    CASE(8, "full table", for (uint32_t j = 0; j < 8; j++) insert(&t, homed(v6, 8, j % 3, j)));
    CASE(8, "chain wraps past the end",
         for (uint32_t j = 0; j < 4; j++) insert(&t, homed(v6, 8, 6, j)));
    CASE(8, "entry behind an invalid slot", put(&t, 2, homed(v6, 8, 2, 1), 1);
         put(&t, 3, homed(v6, 8, 2, 2), 0); put(&t, 4, homed(v6, 8, 2, 3), 1));
    CASE(8, "one address in two valid slots", put(&t, 2, homed(v6, 8, 2, 1), 1);
         put(&t, 3, homed(v6, 8, 2, 2), 1); put(&t, 4, homed(v6, 8, 2, 2), 1);
         put(&t, 5, homed(v6, 8, 2, 3), 1));
    CASE(8, "the zero address alone", insert(&t, (addr_t){{0, 0, 0, 0}}));
    CASE(8, "the zero address inside a chain", insert(&t, homed(v6, 8, 7, 1));
         insert(&t, homed(v6, 8, 7, 2)); insert(&t, (addr_t){{0, 0, 0, 0}});
         insert(&t, homed(v6, 8, 0, 3)));
    /* 4096 slots at about 0.7: inserted as the reference does, holes knocked into the chains,
     * some of the keys behind them inserted again */
    CASE(4096, "4096 slots at about 0.7", {
        addr_t *keys = malloc(3000 * sizeof *keys);
        if (!keys) abort();
        for (int j = 0; j < 3000; j++) {
            addr_t k = clip(v6, (addr_t){{rnd(), rnd(), rnd(), rnd()}});
            if (j % 2)
                k.w[0] = (k.w[0] & ~0xFFFu) | ((home(v6, k) ^ k.w[0] ^ (rnd() % 2048)) & 0xFFFu);
            keys[j] = k;
            insert(&t, k);
        }
        for (size_t s = 0; s < 4096; s++)
            if (slot_valid(&t, s) && rnd() % 16 == 0) {
                if (v6) t.ndp[s].valid = 0; else t.arp[s].valid = 0;
            }
        for (int j = 0; j < 60; j++) insert(&t, keys[rnd() % 3000]);
        free(keys);
    });
#undef CASE
    return bad;
}

/* fold_v6 (upe_dev.h), restated: the index's 32-bit key of an NDP address */
static uint32_t fold(const uint32_t w[4]) {
    return (w[0] * 0x9E3779B1u) ^ (w[1] * 0x85EBCA77u) ^ (w[2] * 0xC2B2AE3Du) ^ (w[3] * 0x27D4EB2Fu);
}

/* NDP only: three addresses of one fold_v6 compile, a fourth cannot be placed; five addresses of
 * one home slot make one chain */
static int ndp_collisions(void) {
    const uint32_t c0 = 0x9E3779B1u;
    uint32_t inv = c0;
    for (int j = 0; j < 5; j++) inv *= 2u - c0 * inv;
    if (c0 * inv != 1u) return fprintf(stderr, "no inverse\n"), 1;
    int bad = 0;
    const addr_t a = {{0x20010DB8u, 0x11111111u, 0x22222222u, 0x33333333u}};
    for (uint32_t count = 3; count <= 4; count++) {
        table_t t = table_new(1, 16);
        insert(&t, a);
        for (uint32_t j = 1; j < count; j++) {
            addr_t b = {{0, a.w[1] + j, a.w[2] ^ (j << 8), a.w[3] + 7 * j}};
            b.w[0] = (fold(a.w) ^ fold(b.w)) * inv;
            if (fold(b.w) != fold(a.w)) return fprintf(stderr, "the folds differ\n"), 1;
            insert(&t, b);
        }
        bad |= check(count == 3 ? "three addresses of one fold_v6" : "four addresses of one fold_v6",
                     &t, count == 3);
        table_free(&t);
    }
    table_t x = table_new(1, 16);
    const uint32_t w[4] = {0x20010DB8u, 0x00000001u, 0xA5A50000u, 0x0000C3C3u};
    for (int r = 0; r < 4; r++)
        insert(&x, (addr_t){{w[r], w[(r + 1) % 4], w[(r + 2) % 4], w[(r + 3) % 4]}});
    insert(&x, (addr_t){{w[1], w[0], w[3], w[2]}});
    bad |= check("addresses of one home slot", &x, 1);
    table_free(&x);
    return bad;
}

/* what the two calls refuse */
static int arguments(void) {
    upe_arp_entry_t *t = calloc(4, sizeof *t);
    upe_flow_key_t key;
    uint64_t out = 0;
    memset(&key, 0, sizeof key);
    if (!t) abort();
    int bad = 0;
    bad |= upe_neigh_compile(t, 3, NULL, 0) != NULL || !strstr(g_msg, "power of two");
    bad |= upe_neigh_compile(NULL, 4, NULL, 0) != NULL || !strstr(g_msg, "null table");
    bad |= upe_neigh_lookup_host(t, 3, NULL, 0, &key, 1, &out) != -1;
    bad |= upe_neigh_lookup_host(NULL, 4, NULL, 0, &key, 1, &out) != -1;
    bad |= upe_neigh_lookup_host(t, 4, NULL, 0, NULL, 1, &out) != -1;
    bad |= upe_neigh_lookup_host(t, 4, NULL, 0, &key, 1, NULL) != -1;
    bad |= upe_neigh_lookup_host(NULL, 0, NULL, 0, NULL, 0, NULL) != 0;
    upe_neigh_image_free(NULL);
    free(t);
    if (bad) fprintf(stderr, "argument checks\n");
    return bad;
}

int main(void) {
    const int bad = family(0) | family(1) | ndp_collisions() | arguments();
    if (!bad) printf("resolve_san: ok\n");
    return bad;
}
