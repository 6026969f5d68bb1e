/* The control writes' host side (upe_ctrl_writes_host, upe_neigh_apply_writes,
 * upe_amd/csrc/upe_host.c) on the CPU, stand-alone: `make -C upe_amd/csrc ctrl-san` builds this
 * file with upe_host.c under the host sanitizers (-fsanitize=address,undefined) and runs it.
 * Expected values come from a walk (reference src/worker.c:68-95) and two probes
 * (src/arp_table.c:26-53, src/ndp_table.c:39-65) written out here.  Every frame is a heap block
 * of exactly len bytes and every record array one of exactly cap entries, so a read at or past
 * len, or a write at or past cap, is reported. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/upe_gpu.h"

static int g_bad = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "ctrl_san:%d: %s\n", __LINE__, #cond);        \
            ++g_bad;                                                      \
        }                                                                 \
    } while (0)

static const uint8_t kMacA[6] = {0x0a, 0x1b, 0x2c, 0x3d, 0x4e, 0x5f};
static const uint8_t kMacB[6] = {0x0b, 1, 2, 3, 4, 5};

/* an NS (135) or NA (136) of `size` bytes: the first option at 78 = (type, lb, kMacA), a second
 * one of the same type 8 bytes on with kMacB, zeros after it */
static void build_nd(uint8_t *f, size_t size, int kind, int type, int lb) {
    memset(f, 0, size);
    f[12] = 0x86, f[13] = 0xDD;
    f[14] = 0x60, f[20] = 58, f[21] = 64;
    for (int j = 0; j < 16; j++) f[22 + j] = (uint8_t)(0xA0 + j), f[38 + j] = (uint8_t)(0xB0 + j);
    f[54] = (uint8_t)kind;
    for (int j = 0; j < 16; j++) f[62 + j] = (uint8_t)(0xC0 + j);
    f[78] = (uint8_t)type, f[79] = (uint8_t)lb;
    memcpy(f + 80, kMacA, 6);
    f[86] = (uint8_t)type, f[87] = 1;
    memcpy(f + 88, kMacB, 6);
}

static void build_arp(uint8_t *f, int op) {
    static const uint8_t hdr[8] = {0, 1, 8, 0, 6, 4, 0, 0};
    memset(f, 0xFF, 6);
    memset(f + 6, 0x66, 6);
    f[12] = 0x08, f[13] = 0x06;
    memcpy(f + 14, hdr, 8);
    f[21] = (uint8_t)op;
    memcpy(f + 22, kMacA, 6);
    f[28] = 0xE1, f[29] = 0xE2, f[30] = 0xE3, f[31] = 0xE4;
    memset(f + 32, 0, 6);
    f[38] = 10, f[39] = 128, f[40] = 0, f[41] = 1;
}

/* what the reference does with frame f of len bytes: 0 = not marked, 1 = marked and nothing
 * learned, 2 = *w is the record */
static int expect(const uint8_t *f, uint32_t len, uint32_t index, upe_ctrl_write_t *w) {
    uint8_t z[78] = {0}; /* the frame's first bytes in a zero-filled buffer */
    memcpy(z, f, len < sizeof z ? len : sizeof z);
    memset(w, 0, sizeof *w);
    w->index = index;
    if (z[12] == 0x08 && z[13] == 0x06) {
        static const uint8_t hdr[6] = {0, 1, 8, 0, 6, 4};
        if (memcmp(z + 14, hdr, 6) != 0) return 0;
        w->kind = UPE_CW_ARP, w->mac_off = 22;
        memcpy(w->mac, z + 22, 6);
        w->ip[0] = z[31], w->ip[1] = z[30], w->ip[2] = z[29], w->ip[3] = z[28];
        return 2;
    }
    if (!(z[12] == 0x86 && z[13] == 0xDD && len >= 78 && z[20] == 58 &&
          (z[54] == 135 || z[54] == 136)))
        return 0;
    size_t off = 78;
    while (off + 2 <= len) {
        const uint8_t ot = f[off];
        const uint8_t ol = (uint8_t)(f[off + 1] * 8);
        if (ol == 0 || off + ol > len) break;
        if ((z[54] == 135 && ot == 1) || (z[54] == 136 && ot == 2)) {
            w->kind = UPE_CW_NDP, w->mac_off = (uint16_t)(off + 2);
            memcpy(w->mac, f + off + 2, 6);
            memcpy(w->ip, z[54] == 135 ? z + 22 : z + 62, 16);
            return 2;
        }
        off += ol;
    }
    return 1;
}

/* one frame, in a heap block of exactly len bytes, as a batch of 1 */
static void one(const uint8_t *full, uint32_t len) {
    uint8_t *f = malloc(len ? len : 1);
    memcpy(f, full, len);
    const uint64_t desc = UPE_DESC(0, len);
    upe_ctrl_write_t want, *got = malloc(sizeof *got);
    upe_ctrl_info_t info;
    memset(got, 0xA7, sizeof *got);
    const int e = expect(f, len, 0, &want);
    CHECK(upe_ctrl_writes_host(f, &desc, 1, got, 1, &info) == 0);
    CHECK(info.ctrl == (e > 0) && info.writes == (e == 2) && info.stored == info.writes);
    CHECK(info.first_write == (e == 2 ? 0 : UINT64_MAX));
    if (e == 2) CHECK(memcmp(got, &want, sizeof want) == 0);
    free(got);
    free(f);
}

static void lengths(void) {
    uint8_t full[512];
    int learned = 0;
    for (int kind = 135; kind <= 136; kind++) {
        build_nd(full, sizeof full, kind, kind == 135 ? 1 : 2, 1);
        for (uint32_t len = 0; len <= 100; len++) one(full, len);
        upe_ctrl_write_t w;
        learned += expect(full, 85, 0, &w) == 1 && expect(full, 86, 0, &w) == 2;
        /* the length bytes: 0 and 32 and 64 stop the walk, 1 and 33 are 8 bytes */
        static const int lbs[5] = {0, 1, 32, 33, 64};
        for (int k = 0; k < 5; k++) {
            build_nd(full, sizeof full, kind, kind == 135 ? 1 : 2, lbs[k]);
            one(full, 400);
            CHECK(expect(full, 400, 0, &w) == (lbs[k] % 32 == 1 ? 2 : 1));
            CHECK(lbs[k] % 32 != 1 || memcmp(w.mac, kMacA, 6) == 0);
            /* the same length byte on another type's option: the walk steps over 8 bytes */
            build_nd(full, sizeof full, kind, 5, lbs[k]);
            full[86] = kind == 135 ? 1 : 2;
            one(full, 400);
            CHECK(expect(full, 400, 0, &w) == (lbs[k] % 32 == 1 ? 2 : 1));
            CHECK(lbs[k] % 32 != 1 || memcmp(w.mac, kMacB, 6) == 0);
        }
    }
    CHECK(learned == 2);
    build_arp(full, 1);
    for (uint32_t len = 0; len <= 60; len++) one(full, len);
}

/* a batch of several frames; cap 0, writes - 1, writes */
static void caps(void) {
    enum { N = 9, SLOT = 112 };
    uint8_t *frames = calloc(N, SLOT);
    uint64_t desc[N];
    upe_ctrl_write_t all[N], w;
    uint64_t writes = 0, ctrl = 0;
    for (int i = 0; i < N; i++) {
        uint8_t *f = frames + i * SLOT;
        uint32_t len = 86;
        if (i % 3 == 0) build_arp(f, 1 + i % 2), len = 42;
        else build_nd(f, 96, 135 + i % 2, i == 4 ? 7 : 1 + i % 2, 1), len = i == 7 ? 84 : 96;
        desc[i] = UPE_DESC((uint64_t)i * SLOT, len);
        const int e = expect(f, len, (uint32_t)i, &w);
        ctrl += e > 0;
        if (e == 2) all[writes++] = w;
    }
    CHECK(ctrl == N && writes >= 5 && writes < ctrl);
    const size_t tries[3] = {0, (size_t)writes - 1, (size_t)writes};
    for (int t = 0; t < 3; t++) {
        const size_t cap = tries[t];
        upe_ctrl_write_t *got = malloc(cap ? cap * sizeof *got : 1);
        upe_ctrl_info_t info;
        CHECK(upe_ctrl_writes_host(frames, desc, N, cap ? got : NULL, cap, &info) == 0);
        CHECK(info.ctrl == ctrl && info.writes == writes && info.stored == cap);
        CHECK(info.first_write == all[0].index);
        CHECK(memcmp(got, all, cap * sizeof *got) == 0);
        free(got);
    }
    /* refusals: nothing written */
    upe_ctrl_info_t info;
    memset(&info, 0xA7, sizeof info);
    CHECK(upe_ctrl_writes_host(NULL, desc, N, all, N, &info) == -1);
    CHECK(upe_ctrl_writes_host(frames, NULL, N, all, N, &info) == -1);
    CHECK(upe_ctrl_writes_host(frames, desc, N, NULL, 1, &info) == -1);
    CHECK(upe_ctrl_writes_host(frames, desc, N, all, N, NULL) == -1);
    CHECK(upe_ctrl_writes_host(frames, desc, 0xFFFFFFFFull - UPE_CTRL_BLOCK + 1, all, N, &info) == -1);
    CHECK(upe_host_last_error()[0] != 0 && info.ctrl == 0xA7A7A7A7A7A7A7A7ull);
    CHECK(upe_ctrl_writes_host(NULL, NULL, 0, NULL, 0, &info) == 0);
    CHECK(info.ctrl == 0 && info.writes == 0 && info.stored == 0 && info.first_write == UINT64_MAX);
    free(frames);
}

/* the probes, written out */
static void hand_arp(upe_arp_entry_t *t, size_t cap, uint32_t ip, const uint8_t *mac, int64_t now) {
    for (size_t i = 0; i < cap; i++) {
        upe_arp_entry_t *e = &t[((ip & (cap - 1)) + i) & (cap - 1)];
        if (e->valid && e->ip != ip) continue;
        if (!e->valid) e->valid = true, e->ip = ip;
        memcpy(e->mac, mac, 6);
        e->update_at = now;
        return;
    }
}

static void hand_ndp(upe_ndp_entry_t *t, size_t cap, const uint8_t *ip, const uint8_t *mac, int64_t now) {
    uint32_t h = 0, c;
    for (int i = 0; i < 4; i++) memcpy(&c, ip + 4 * i, 4), h ^= c;
    for (size_t i = 0; i < cap; i++) {
        upe_ndp_entry_t *e = &t[((h & (cap - 1)) + i) & (cap - 1)];
        if (e->valid && memcmp(e->ip, ip, 16) != 0) continue;
        if (!e->valid) e->valid = true, memcpy(e->ip, ip, 16);
        memcpy(e->mac, mac, 6);
        e->update_at = now;
        return;
    }
}

static void apply(void) {
    enum { N = 40, CA = 8, CN = 4 };
    upe_ctrl_write_t *w = calloc(N, sizeof *w);
    for (int i = 0; i < N; i++) {
        w[i].index = (uint32_t)i;
        w[i].kind = i % 2 ? UPE_CW_NDP : UPE_CW_ARP;
        w[i].mac[0] = (uint8_t)i, w[i].mac[5] = 0x77;
        /* few addresses, colliding homes: updates of a held address, probes that wrap, and from
         * record 24 on new addresses for tables that are full by then */
        const uint8_t a = (uint8_t)(i < 24 ? (i / 2) % 5 : 100 + i);
        if (i % 2) w[i].ip[15] = a, w[i].ip[0] = 0x20, w[i].ip[3] = (uint8_t)(a * 4);
        else w[i].ip[0] = (uint8_t)(a * 8), w[i].ip[1] = a;
    }
    upe_arp_entry_t *ga = calloc(CA, sizeof *ga), *ha = calloc(CA, sizeof *ha);
    upe_ndp_entry_t *gn = calloc(CN, sizeof *gn), *hn = calloc(CN, sizeof *hn);
    size_t applied = 99;
    CHECK(upe_neigh_apply_writes(ga, CA, gn, CN, w, N, 1234, &applied) == 0 && applied == N);
    for (int i = 0; i < N; i++) {
        uint32_t ip;
        memcpy(&ip, w[i].ip, 4);
        if (i % 2) hand_ndp(hn, CN, w[i].ip, w[i].mac, 1234);
        else hand_arp(ha, CA, ip, w[i].mac, 1234);
    }
    int full = 1;
    for (int s = 0; s < CA; s++) {
        CHECK(ga[s].valid == ha[s].valid && ga[s].ip == ha[s].ip && ga[s].update_at == ha[s].update_at &&
              memcmp(ga[s].mac, ha[s].mac, 6) == 0);
        full &= s >= 5 || ga[s].valid;
    }
    for (int s = 0; s < CN; s++) {
        CHECK(gn[s].valid && hn[s].valid && gn[s].update_at == 1234 &&
              memcmp(gn[s].ip, hn[s].ip, 16) == 0 && memcmp(gn[s].mac, hn[s].mac, 6) == 0);
    }
    CHECK(full);
    /* a full NDP table and new addresses: left alone, still counted; ARP has no table */
    memcpy(hn, gn, CN * sizeof *gn);
    CHECK(upe_neigh_apply_writes(NULL, 0, gn, CN, w + 24, N - 24, 5678, &applied) == 0);
    CHECK(applied == (N - 24) / 2 && memcmp(gn, hn, CN * sizeof *gn) == 0);
    /* refusals: checked before the first write */
    memcpy(ha, ga, CA * sizeof *ga);
    w[N - 1].kind = 5;
    applied = 99;
    CHECK(upe_neigh_apply_writes(ga, CA, gn, CN, w, N, 9, &applied) == -1);
    CHECK(upe_neigh_apply_writes(ga, 6, gn, CN, w, N - 1, 9, &applied) == -1);
    CHECK(upe_neigh_apply_writes(NULL, CA, gn, CN, w, N - 1, 9, &applied) == -1);
    CHECK(upe_neigh_apply_writes(ga, CA, NULL, CN, w, N - 1, 9, &applied) == -1);
    CHECK(upe_neigh_apply_writes(ga, CA, gn, CN, NULL, N - 1, 9, &applied) == -1);
    CHECK(applied == 99 && upe_host_last_error()[0] != 0);
    CHECK(memcmp(ga, ha, CA * sizeof *ga) == 0 && memcmp(gn, hn, CN * sizeof *gn) == 0);
    CHECK(upe_neigh_apply_writes(NULL, 0, NULL, 0, NULL, 0, 9, NULL) == 0);
    free(w), free(ga), free(ha), free(gn), free(hn);
}

int main(void) {
    lengths();
    caps();
    apply();
    if (g_bad) {
        fprintf(stderr, "ctrl_san: %d check(s) failed\n", g_bad);
        return 1;
    }
    printf("ctrl_san: ok\n");
    return 0;
}
