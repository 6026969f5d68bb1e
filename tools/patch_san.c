/* upe_neigh_patch_host (upe_rules.cpp) on the CPU, stand-alone: `make -C upe_amd/csrc patch-san`
 * builds this file with upe_rules.cpp and upe_host.c under the host sanitizers
 * (-fsanitize=address,undefined) and runs it.  Per family, slot arrays of the shapes of
 * tools/resolve_san.c (no slots, one slot, a full table, a chain that wraps, an entry behind an
 * invalid slot, a stale address, one address in two slots, the zero address, 4096 slots at about
 * 0.7 with holes) and a batch of records over each: every stored address refreshed with a MAC of
 * its own, one address three times, absent addresses (the zero address among them), a record of
 * no kind, a record of the other family, whose table has no slots.  Checked: the missed ranks are
 * the records whose address upe_neigh_lookup_host misses before the batch, info adds up, and the
 * patched image answers every stored, taught and absent address as the image compiled from the
 * slot arrays with the held records applied (upe_neigh_apply_writes) does.  Records, ranks and
 * answers are heap blocks of exactly their size, so a read or write past either end is reported.
 * C: the ABI as a C caller sees it. */
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

typedef struct { uint8_t b[16]; } addr_t; /* ARP: bytes 0-3 the address (LE word), the rest 0 */

typedef struct {
    int v6;
    size_t cap;
    upe_arp_entry_t *arp;
    upe_ndp_entry_t *ndp;
} table_t;

static void *block(size_t n, size_t size) {
    void *p = calloc(n ? n : 1, size);
    if (!p) abort();
    return p;
}
static table_t table_new(int v6, size_t cap) {
    table_t t = {v6, cap, NULL, NULL};
    if (cap && v6) t.ndp = block(cap, sizeof *t.ndp);
    if (cap && !v6) t.arp = block(cap, sizeof *t.arp);
    return t;
}
static table_t table_copy(const table_t *t) {
    table_t c = table_new(t->v6, t->cap);
    if (t->arp) memcpy(c.arp, t->arp, t->cap * sizeof *t->arp);
    if (t->ndp) memcpy(c.ndp, t->ndp, t->cap * sizeof *t->ndp);
    return c;
}
static void table_free(table_t *t) { free(t->arp); free(t->ndp); }

static uint32_t word(addr_t k, int j) {
    return (uint32_t)k.b[4 * j] | (uint32_t)k.b[4 * j + 1] << 8 | (uint32_t)k.b[4 * j + 2] << 16 |
           (uint32_t)k.b[4 * j + 3] << 24;
}
static addr_t addr(int v6, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    const uint32_t w[4] = {w0, v6 ? w1 : 0, v6 ? w2 : 0, v6 ? w3 : 0};
    addr_t k;
    for (int j = 0; j < 16; j++) k.b[j] = (uint8_t)(w[j / 4] >> (8 * (j % 4)));
    return k;
}
/* An address whose home slot (ip & (cap - 1); the XOR of the words) is h. */
static addr_t homed(int v6, size_t cap, uint32_t h, uint32_t tag) {
    const uint32_t w1 = tag << 8, w2 = tag * 0x01010101u;
    uint32_t w0 = (uint32_t)((tag + 1) * cap) | h;
    if (v6) w0 ^= (w1 ^ w2) & (uint32_t)(cap - 1);
    return addr(v6, w0, w1, w2, 0);
}
static size_t home(int v6, addr_t k) {
    return v6 ? word(k, 0) ^ word(k, 1) ^ word(k, 2) ^ word(k, 3) : word(k, 0);
}
static addr_t slot_addr(const table_t *t, size_t s) {
    addr_t k;
    memset(&k, 0, sizeof k);
    if (t->v6) memcpy(k.b, t->ndp[s].ip, 16);
    else memcpy(k.b, &t->arp[s].ip, 4); /* a little-endian host, as the library's */
    return k;
}
static int slot_valid(const table_t *t, size_t s) { return t->v6 ? t->ndp[s].valid : t->arp[s].valid; }
static void put(table_t *t, size_t s, addr_t k, int valid) {
    const uint8_t mac[6] = {2, t->v6 ? 'n' : 'a', (uint8_t)(s >> 16), (uint8_t)(s >> 8), (uint8_t)s,
                            (uint8_t)rnd()};
    if (t->v6) {
        memcpy(t->ndp[s].ip, k.b, 16);
        memcpy(t->ndp[s].mac, mac, 6);
        t->ndp[s].valid = valid;
    } else {
        memcpy(&t->arp[s].ip, k.b, 4);
        memcpy(t->arp[s].mac, mac, 6);
        t->arp[s].valid = valid;
    }
}
static void insert(table_t *t, addr_t k) {
    for (size_t i = 0; i < t->cap; i++) {
        const size_t s = (home(t->v6, k) + i) & (t->cap - 1);
        if (!slot_valid(t, s) || memcmp(slot_addr(t, s).b, k.b, 16) == 0) {
            put(t, s, k, 1);
            return;
        }
    }
}

static void set_key(upe_flow_key_t *key, int v6, addr_t k) {
    memset(key, 0xA7, sizeof *key); /* what is not asked for is noise */
    key->ip_ver = v6 ? 6 : 4;
    memcpy(key->dst_ip.v6, k.b, v6 ? 16 : 4);
}
static void set_rec(upe_ctrl_write_t *r, size_t rank, int kind, addr_t k) {
    memset(r, 0, sizeof *r);
    r->index = (uint32_t)(7 * rank + 3);
    r->kind = (uint8_t)kind;
    r->mac_off = 22;
    r->mac[0] = 0x0A;
    r->mac[1] = (uint8_t)kind;
    r->mac[2] = (uint8_t)(rank >> 16);
    r->mac[3] = (uint8_t)(rank >> 8);
    r->mac[4] = (uint8_t)rank;
    r->mac[5] = (uint8_t)rnd();
    memcpy(r->ip, k.b, 16);
}

#define FAIL(...) return fprintf(stderr, __VA_ARGS__), fputc('\n', stderr), 1

static int check(const char *what, const table_t *t) {
    const int v6 = t->v6, kind = v6 ? UPE_CW_NDP : UPE_CW_ARP;
    const size_t absent = 64;
    /* the records */
    const size_t count = t->cap + 3 + absent + 3;
    upe_ctrl_write_t *w = block(count, sizeof *w);
    size_t n = 0;
    for (size_t s = 0; s < t->cap; s++) set_rec(&w[n], n, kind, slot_addr(t, s)), n++;
    for (int j = 0; j < 3; j++) /* one address three times: the last must win */
        set_rec(&w[n], n, kind, t->cap ? slot_addr(t, t->cap / 2) : addr(v6, 9, 9, 9, 9)), n++;
    for (size_t j = 0; j < absent; j++)
        set_rec(&w[n], n, kind, j ? addr(v6, rnd() | 1u << 31, rnd(), rnd(), rnd()) : addr(v6, 0, 0, 0, 0)), n++;
    set_rec(&w[n], n, 0, t->cap ? slot_addr(t, 0) : addr(v6, 1, 2, 3, 4)), n++;    /* no kind */
    set_rec(&w[n], n, 5, t->cap ? slot_addr(t, 0) : addr(v6, 1, 2, 3, 4)), n++;
    set_rec(&w[n], n, v6 ? UPE_CW_ARP : UPE_CW_NDP, addr(!v6, 5, 6, 7, 8)), n++;   /* no table */
    if (n != count) FAIL("%s: record count", what);
    /* held, by the probe over the slot arrays before the batch */
    upe_flow_key_t *keys = block(count, sizeof *keys);
    uint64_t *before = block(count, sizeof *before);
    for (size_t i = 0; i < count; i++) set_key(&keys[i], w[i].kind == UPE_CW_NDP, *(const addr_t *)w[i].ip);
    if (upe_neigh_lookup_host(t->arp, v6 ? 0 : t->cap, t->ndp, v6 ? t->cap : 0, keys, count, before))
        FAIL("%s: upe_neigh_lookup_host: %s", what, upe_host_last_error());
    size_t want_miss = 0;
    for (size_t i = 0; i < count; i++)
        if (!before[i] || (w[i].kind != UPE_CW_ARP && w[i].kind != UPE_CW_NDP)) want_miss++;
    /* the patch */
    upe_neigh_image_t *im = upe_neigh_compile(t->arp, v6 ? 0 : t->cap, t->ndp, v6 ? t->cap : 0);
    if (!im) FAIL("%s: upe_neigh_compile: %s", what, g_msg);
    uint32_t *miss = block(count, sizeof *miss);
    memset(miss, 0xEE, count * sizeof *miss);
    upe_neigh_patch_info_t info;
    if (upe_neigh_patch_host(im, w, count, miss, &info)) FAIL("%s: patch: %s", what, g_msg);
    if (info.records != count || info.missed != want_miss || info.patched != count - want_miss)
        FAIL("%s: info %llu %llu %llu, want %zu misses of %zu", what, (unsigned long long)info.records,
             (unsigned long long)info.patched, (unsigned long long)info.missed, want_miss, count);
    size_t m = 0;
    for (size_t i = 0; i < count; i++) {
        const int held = before[i] && (w[i].kind == UPE_CW_ARP || w[i].kind == UPE_CW_NDP);
        if (!held && miss[m++] != i) FAIL("%s: miss[%zu] = %u, want %zu", what, m - 1, miss[m - 1], i);
    }
    for (size_t i = m; i < count; i++)
        if (miss[i] != 0xEEEEEEEEu) FAIL("%s: miss[%zu] written", what, i);
    if (info.first_miss != (want_miss ? miss[0] : UINT64_MAX)) FAIL("%s: first_miss", what);
    /* the invariant: the held records through upe_neigh_apply_writes, compiled again */
    table_t u = table_copy(t);
    upe_ctrl_write_t *held = block(count, sizeof *held);
    size_t nh = 0;
    for (size_t i = 0; i < count; i++)
        if (before[i] && (w[i].kind == UPE_CW_ARP || w[i].kind == UPE_CW_NDP)) held[nh++] = w[i];
    if (upe_neigh_apply_writes(u.arp, v6 ? 0 : u.cap, u.ndp, v6 ? u.cap : 0, held, nh, 77, NULL))
        FAIL("%s: upe_neigh_apply_writes: %s", what, upe_host_last_error());
    upe_neigh_image_t *ref = upe_neigh_compile(u.arp, v6 ? 0 : u.cap, u.ndp, v6 ? u.cap : 0);
    if (!ref) FAIL("%s: upe_neigh_compile (applied): %s", what, g_msg);
    uint64_t *got = block(count, sizeof *got), *want = block(count, sizeof *want);
    if (upe_neigh_image_lookup_host(im, keys, count, got) ||
        upe_neigh_image_lookup_host(ref, keys, count, want))
        FAIL("%s: upe_neigh_image_lookup_host: %s", what, g_msg);
    for (size_t i = 0; i < count; i++)
        if (got[i] != want[i])
            FAIL("%s: record %zu's address answers %llx, want %llx", what, i,
                 (unsigned long long)got[i], (unsigned long long)want[i]);
    /* a patch without a miss list, and an empty one */
    upe_neigh_patch_info_t again;
    if (upe_neigh_patch_host(im, w, count, NULL, &again) || memcmp(&again, &info, sizeof info))
        FAIL("%s: patch without a miss list", what);
    if (upe_neigh_patch_host(im, NULL, 0, NULL, &again) || again.records || again.patched ||
        again.missed || again.first_miss != UINT64_MAX)
        FAIL("%s: empty patch", what);
    free(got), free(want), free(held), free(miss), free(before), free(keys), free(w);
    table_free(&u);
    upe_neigh_image_free(im), upe_neigh_image_free(ref);
    return 0;
}

static int family(int v6) {
    int bad = 0;
    table_t t = table_new(v6, 0);
    bad |= check("no slots", &t);
    t = table_new(v6, 1);
    bad |= check("one empty slot", &t);
    put(&t, 0, homed(v6, 1, 0, 5), 1);
    bad |= check("one full slot", &t);
    table_free(&t);
    t = table_new(v6, 8);
    for (uint32_t j = 0; j < 8; j++) insert(&t, homed(v6, 8, j % 3, j));
    bad |= check("full", &t);
    table_free(&t);
    t = table_new(v6, 16);
    for (uint32_t j = 0; j < 4; j++) insert(&t, homed(v6, 16, 14, j));
    bad |= check("wrap", &t);
    table_free(&t);
    t = table_new(v6, 16); /* slot 4 hidden behind the invalid, stale slot 3 */
    put(&t, 2, homed(v6, 16, 2, 1), 1);
    put(&t, 3, homed(v6, 16, 2, 2), 0);
    put(&t, 4, homed(v6, 16, 2, 3), 1);
    bad |= check("hidden and stale", &t);
    table_free(&t);
    t = table_new(v6, 16); /* one address in slots 3 and 4: slot 3 answers */
    put(&t, 2, homed(v6, 16, 2, 1), 1);
    put(&t, 3, homed(v6, 16, 2, 2), 1);
    put(&t, 4, homed(v6, 16, 2, 2), 1);
    put(&t, 5, homed(v6, 16, 2, 3), 1);
    bad |= check("dup", &t);
    table_free(&t);
    t = table_new(v6, 16);
    insert(&t, homed(v6, 16, 15, 1));
    insert(&t, homed(v6, 16, 15, 2));
    insert(&t, addr(v6, 0, 0, 0, 0));
    insert(&t, homed(v6, 16, 0, 3));
    bad |= check("zero address", &t);
    table_free(&t);
    t = table_new(v6, 4096);
    for (int j = 0; j < 3000; j++) insert(&t, addr(v6, rnd(), rnd(), rnd(), rnd()));
    for (size_t s = 0; s < 4096; s++)
        if (rnd() % 16 == 0) {
            if (v6) t.ndp[s].valid = 0;
            else t.arp[s].valid = 0;
        }
    bad |= check("4096 with holes", &t);
    table_free(&t);
    return bad;
}

static int arguments(void) {
    upe_neigh_patch_info_t info;
    upe_ctrl_write_t w;
    memset(&w, 0, sizeof w);
    upe_neigh_image_t *im = upe_neigh_compile(NULL, 0, NULL, 0);
    int bad = !im;
    bad |= upe_neigh_patch_host(NULL, &w, 1, NULL, &info) != -1;
    bad |= upe_neigh_patch_host(im, &w, 1, NULL, NULL) != -1;
    bad |= upe_neigh_patch_host(im, NULL, 1, NULL, &info) != -1;
    bad |= upe_neigh_patch_host(im, &w, (size_t)0xFFFFFFFFu - UPE_PATCH_BLOCK + 1, NULL, &info) != -1;
    bad |= upe_neigh_image_lookup_host(NULL, NULL, 0, NULL) != -1;
    bad |= upe_neigh_image_lookup_host(im, NULL, 0, NULL) != 0;
    upe_neigh_image_free(im);
    if (bad) fprintf(stderr, "arguments\n");
    return bad;
}

int main(void) {
    const int bad = family(0) | family(1) | arguments();
    printf(bad ? "patch_san: FAILED\n" : "patch_san: ok\n");
    return bad;
}
