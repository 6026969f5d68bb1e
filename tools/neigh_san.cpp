// The neighbour snapshot builder (build_neigh_image, upe_amd/csrc/upe_rules.cpp) under the host
// sanitizers, stand-alone: `make -C upe_amd/csrc neigh-san` builds this file with it
// (-fsanitize=address,undefined) and runs it.  Deterministic slot arrays go through the builder;
// every stored address, as many absent ones and the all-zero address are then looked up in the image the way the
// kernels do (the key's three candidate slots; a slot hits when it is used and holds the key) and
// in the slot array the way the reference does (arp_get_mac, src/arp_table.c:55-80, ndp_get_mac,
// src/ndp_table.c:67-86: from the home slot, linearly, the first valid entry of the key, nothing
// past the first invalid slot).  Hit or miss and the MAC must agree for every query.
#include <stdio.h>
#include <string.h>

#include <array>
#include <set>
#include <vector>

#include "../upe_amd/csrc/upe_rules.h"

using namespace upe;

// the library's error slot, which upe_gpu.hip owns in the library
static char g_msg[256];
extern "C" int upe_gpu_set_last_error(const char* msg) {
    snprintf(g_msg, sizeof g_msg, "%s", msg ? msg : "");
    return -1;
}

static uint32_t g_x = 0x2545F491u;
static uint32_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 17; g_x ^= g_x << 5; return g_x; }

// An address as words: ARP word 0 = the IPv4 address, NDP the 16 bytes as four LE words.
using Key = std::array<uint32_t, 4>;
struct Mac {
    uint8_t b[6];
};

static bool image_mac(bool used, uint32_t lo, uint32_t hi, Mac& m) {
    if (!used) return false;
    for (int j = 0; j < 4; ++j) m.b[j] = (uint8_t)(lo >> (8 * j));
    m.b[4] = (uint8_t)hi, m.b[5] = (uint8_t)(hi >> 8);
    return true;
}

struct Arp {
    using Entry = upe_arp_entry_t;
    static constexpr const char* name = "arp";
    static Key key(const Entry& e) { return {e.ip, 0, 0, 0}; }
    static void set_key(Entry& e, const Key& k) { e.ip = k[0]; }
    static Key clip(const Key& k) { return {k[0], 0, 0, 0}; }
    static size_t home(const Key& k) { return k[0]; }
    static int build(const Entry* t, size_t cap, NeighImage& im) {
        return build_neigh_image(t, cap, nullptr, 0, im);
    }
    static bool shape_ok(const NeighImage& im) {
        return im.arp.size() == (im.arp_bits ? (size_t)1 << im.arp_bits : 1);
    }
    static bool find(const NeighImage& im, const Key& k, Mac& m) {
        if (im.arp_bits == 0) return false;
        for (uint32_t s : {slot1(k[0], im.arp_seed, im.arp_bits), slot2(k[0], im.arp_seed, im.arp_bits),
                           slot3(k[0], im.arp_seed, im.arp_bits)}) {
            const uint4& e = im.arp.at(s);
            if (e.x == k[0] && image_mac((e.z >> 16) & 1u, e.y, e.z & 0xFFFFu, m)) return true;
        }
        return false;
    }
};

struct Ndp {
    using Entry = upe_ndp_entry_t;
    static constexpr const char* name = "ndp";
    static Key key(const Entry& e) { return {le32(e.ip), le32(e.ip + 4), le32(e.ip + 8), le32(e.ip + 12)}; }
    static void set_key(Entry& e, const Key& k) {
        for (int j = 0; j < 16; ++j) e.ip[j] = (uint8_t)(k[j / 4] >> (8 * (j % 4)));
    }
    static Key clip(const Key& k) { return k; }
    static size_t home(const Key& k) { return k[0] ^ k[1] ^ k[2] ^ k[3]; }
    static int build(const Entry* t, size_t cap, NeighImage& im) {
        return build_neigh_image(nullptr, 0, t, cap, im);
    }
    static bool shape_ok(const NeighImage& im) {
        return im.ndp.size() == 2 * (im.ndp_bits ? (size_t)1 << im.ndp_bits : 1);
    }
    static bool find(const NeighImage& im, const Key& k, Mac& m) {
        if (im.ndp_bits == 0) return false;
        const uint32_t f = fold_v6(k.data());
        for (uint32_t s : {slot1(f, im.ndp_seed, im.ndp_bits), slot2(f, im.ndp_seed, im.ndp_bits),
                           slot3(f, im.ndp_seed, im.ndp_bits)}) {
            const uint4& a = im.ndp.at(2 * (size_t)s);
            const uint4& d = im.ndp.at(2 * (size_t)s + 1);
            if (a.x == k[0] && a.y == k[1] && a.z == k[2] && a.w == k[3] &&
                image_mac((d.y >> 16) & 1u, d.x, d.y & 0xFFFFu, m))
                return true;
        }
        return false;
    }
};

// The reference's probe over the slot array.
template <class F>
static bool probe(const std::vector<typename F::Entry>& t, const Key& k, Mac& m) {
    const size_t cap = t.size();
    for (size_t i = 0; i < cap; ++i) {
        const typename F::Entry& e = t[(F::home(k) + i) & (cap - 1)];
        if (!e.valid) return false;
        if (F::key(e) == k) {
            memcpy(m.b, e.mac, 6);
            return true;
        }
    }
    return false;
}

template <class F>
struct Table {
    std::vector<typename F::Entry> t;
    explicit Table(size_t cap) : t(cap) {
        if (cap) memset(t.data(), 0, cap * sizeof t[0]);
    }
    // An entry written straight into a slot (wherever a probe would have put it); its MAC names
    // the slot, so that two entries of one address answer differently.
    void put(size_t slot, const Key& k, bool valid = true) {
        typename F::Entry& e = t[slot];
        F::set_key(e, F::clip(k));
        const uint8_t mac[6] = {2, (uint8_t)F::name[0], (uint8_t)(slot >> 16), (uint8_t)(slot >> 8),
                                (uint8_t)slot, (uint8_t)rnd()};
        memcpy(e.mac, mac, 6);
        e.valid = valid;
    }
    // The reference's update: the first slot from the home slot that is invalid or holds the key.
    void insert(const Key& key) {
        const Key k = F::clip(key);
        for (size_t i = 0; i < t.size(); ++i) {
            const size_t s = (F::home(k) + i) & (t.size() - 1);
            if (!t[s].valid || F::key(t[s]) == k) return put(s, k);
        }
    }
};

template <class F>
static int check(const char* what, const Table<F>& tab) {
    NeighImage im;
    if (F::build(tab.t.data(), tab.t.size(), im) != 0)
        return fprintf(stderr, "%s %s: build_neigh_image: %s\n", F::name, what, g_msg), 1;
    if (!F::shape_ok(im) || im.arp.empty() || im.ndp.size() < 2)
        return fprintf(stderr, "%s %s: slot array and bits disagree\n", F::name, what), 1;
    // every stored address (an invalid slot's too), then as many that are stored nowhere: stored
    // ones with a bit flipped (same chain, or the next) and random ones
    std::vector<Key> q;
    std::set<Key> stored;
    for (const auto& e : tab.t) {
        const Key k = F::key(e);
        if (k != Key{} || e.valid) q.push_back(k), stored.insert(k);
    }
    const size_t nstored = q.size();
    for (size_t absent = 0; absent < nstored + 8;) {
        Key k = nstored && rnd() % 2 ? q[rnd() % nstored] : F::clip(Key{rnd(), rnd(), rnd(), rnd()});
        if (rnd() % 4) k[rnd() % 4] ^= 1u << (rnd() % 32);
        k = F::clip(k);
        if (stored.count(k)) continue;
        q.push_back(k);
        ++absent;
    }
    // the all-zero address (0.0.0.0 / ::) where the table lacks it: the key every empty slot of
    // the image holds, so only the slots' used bit makes it miss
    if (!stored.count(Key{})) q.push_back(Key{});
    size_t hits = 0;
    for (size_t i = 0; i < q.size(); ++i) {
        Mac got = {}, want = {};
        const bool g = F::find(im, q[i], got), w = probe<F>(tab.t, q[i], want);
        if (g != w || (g && memcmp(got.b, want.b, 6) != 0))
            return fprintf(stderr, "%s %s: query %zu (%08x %08x %08x %08x): image %s, probe %s\n",
                           F::name, what, i, q[i][0], q[i][1], q[i][2], q[i][3],
                           g ? "hit" : "miss", w ? (g ? "hit, another MAC" : "hit") : "miss"), 1;
        hits += g;
        if (i >= nstored && g) return fprintf(stderr, "%s %s: an absent address hit\n", F::name, what), 1;
    }
    printf("%s %s: %zu slots, %zu queries agree with the probe (%zu hit)\n", F::name, what,
           tab.t.size(), q.size(), hits);
    return 0;
}

// A key of home slot `home` in a table of `cap` slots; `tag` tells keys of one home apart.
template <class F>
static Key homed(size_t cap, uint32_t home, uint32_t tag) {
    Key k = F::clip(Key{0, tag << 8, tag * 0x01010101u, 0});
    k[0] = (uint32_t)((tag + 1) * cap) | home;   // word 0's low bits are free: fix the XOR with them
    k[0] ^= (k[1] ^ k[2] ^ k[3]) & (uint32_t)(cap - 1);
    return k;
}

template <class F>
static int family() {
    int bad = 0;
    bad |= check("capacity 0", Table<F>(0));
    bad |= check("capacity 1, empty", Table<F>(1));
    {
        Table<F> t(1);
        t.put(0, homed<F>(1, 0, 5));
        bad |= check("capacity 1, full", t);
    }
    {   // every slot valid: a probe of an absent key ends only after a whole turn
        Table<F> t(8);
        for (uint32_t j = 0; j < 8; ++j) t.insert(homed<F>(8, j % 3, j));
        bad |= check("full table", t);
    }
    {
        Table<F> t(8);
        for (uint32_t j = 0; j < 4; ++j) t.insert(homed<F>(8, 6, j));   // slots 6, 7, 0, 1
        if (!t.t[1].valid || t.t[2].valid) return fprintf(stderr, "the chain does not wrap\n"), 1;
        bad |= check("chain wraps past the end", t);
    }
    {   // slot 2 valid, slot 3 invalid, the key of home 2 at slot 4: no probe reaches it
        Table<F> t(8);
        t.put(2, homed<F>(8, 2, 1));
        t.put(3, homed<F>(8, 2, 2), false);
        t.put(4, homed<F>(8, 2, 3));
        Mac m;
        if (probe<F>(t.t, homed<F>(8, 2, 3), m)) return fprintf(stderr, "the entry is reachable\n"), 1;
        bad |= check("entry behind an invalid slot", t);
    }
    {   // one address twice in a chain: the probe answers with slot 3's MAC
        Table<F> t(8);
        t.put(2, homed<F>(8, 2, 1));
        t.put(3, homed<F>(8, 2, 2));
        t.put(4, homed<F>(8, 2, 2));
        t.put(5, homed<F>(8, 2, 3));
        bad |= check("one address in two valid slots", t);
    }
    {   // a valid entry for 0.0.0.0 / :: (an ARP probe makes the reference call arp_update(0, sha)):
        // alone, and inside a chain that wraps (homes 7, 7, 0 = the zero address, 0)
        Table<F> t(8);
        t.insert(Key{});
        if (!t.t[0].valid) return fprintf(stderr, "the zero address is not at slot 0\n"), 1;
        bad |= check("the zero address alone", t);
        Table<F> c(8);
        c.insert(homed<F>(8, 7, 1));
        c.insert(homed<F>(8, 7, 2));
        c.insert(Key{});
        c.insert(homed<F>(8, 0, 3));
        if (!c.t[1].valid || F::key(c.t[1]) != Key{} || !c.t[2].valid)
            return fprintf(stderr, "the zero address is not inside the chain\n"), 1;
        bad |= check("the zero address inside a chain", c);
    }
    {   // 4096 slots at about 0.7: inserted as the reference does, then holes knocked into the
        // chains (entries behind them become unreachable) and some of those keys inserted again
        // (the copy in the hole shadows the one behind it)
        Table<F> t(4096);
        std::vector<Key> keys;
        for (int j = 0; j < 3000; ++j) {
            // half the keys in a range of 2048 homes, so that chains grow long and merge
            Key k = F::clip(Key{rnd(), rnd(), rnd(), rnd()});
            if (j % 2) k[0] = (k[0] & ~0xFFFu) | ((F::home(k) ^ k[0] ^ (rnd() % 2048)) & 0xFFFu);
            keys.push_back(k);
            t.insert(k);
        }
        for (auto& e : t.t)
            if (e.valid && rnd() % 16 == 0) e.valid = false;
        for (int j = 0; j < 60; ++j) t.insert(keys[rnd() % keys.size()]);
        size_t valid = 0;
        for (const auto& e : t.t) valid += e.valid;
        if (valid < 2700 || valid > 3000) return fprintf(stderr, "fill %zu / 4096\n", valid), 1;
        bad |= check("4096 slots at about 0.7", t);
    }
    return bad;
}

// NDP only: addresses that differ and share the 32-bit key the index is placed by, or the home
// slot of the reference's table.
static int ndp_collisions() {
    // fold_v6 multiplies word 0 by an odd constant, which has an inverse modulo 2^32 (Newton:
    // each step doubles the correct low bits): pick words 1-3, solve word 0 for the same fold
    const uint32_t c0 = 0x9E3779B1u;
    uint32_t inv = c0;
    for (int j = 0; j < 5; ++j) inv *= 2u - c0 * inv;
    if (c0 * inv != 1u) return fprintf(stderr, "no inverse\n"), 1;
    Table<Ndp> t(16);
    const Key a = {0x20010DB8u, 0x11111111u, 0x22222222u, 0x33333333u};
    t.insert(a);
    // (three in all: keys of one fold share their three candidate slots, so the placement has
    // room for no more and the load of a table with a fourth fails)
    for (uint32_t j = 1; j <= 2; ++j) {
        Key b = {0, a[1] + j, a[2] ^ (j << 8), a[3] + 7 * j};
        const uint32_t zero[4] = {0, b[1], b[2], b[3]};
        b[0] = (fold_v6(a.data()) ^ fold_v6(zero)) * inv;
        if (b == a || fold_v6(b.data()) != fold_v6(a.data()))
            return fprintf(stderr, "the folds differ\n"), 1;
        t.insert(b);
    }
    int bad = check("addresses of one fold_v6", t);
    {   // a fourth: the load fails, at once (not after a search through every size and seed)
        Table<Ndp> f = t;
        Key b = {0, a[1] + 3, a[2] ^ (3u << 8), a[3] + 21};
        const uint32_t zero[4] = {0, b[1], b[2], b[3]};
        b[0] = (fold_v6(a.data()) ^ fold_v6(zero)) * inv;
        f.insert(b);
        size_t valid = 0;
        for (const auto& e : f.t) valid += e.valid;
        NeighImage im;
        g_msg[0] = 0;
        if (valid != 4 || fold_v6(b.data()) != fold_v6(a.data()) ||
            Ndp::build(f.t.data(), f.t.size(), im) == 0 || !strstr(g_msg, "placement"))
            return fprintf(stderr, "four addresses of one fold_v6: no placement error (%s)\n", g_msg), 1;
        printf("ndp four addresses of one fold_v6: %s\n", g_msg);
    }
    // the same words in another order: equal XOR, so one home slot, one chain
    Table<Ndp> x(16);
    const uint32_t w[4] = {0x20010DB8u, 0x00000001u, 0xA5A50000u, 0x0000C3C3u};
    for (int r = 0; r < 4; ++r) x.insert(Key{w[r], w[(r + 1) % 4], w[(r + 2) % 4], w[(r + 3) % 4]});
    x.insert(Key{w[1], w[0], w[3], w[2]});
    for (size_t s = 0; s < 16; ++s)
        if (x.t[s].valid && (Ndp::home(Ndp::key(x.t[s])) & 15) != (Ndp::home(Key{w[0], w[1], w[2], w[3]}) & 15))
            return fprintf(stderr, "the home slots differ\n"), 1;
    return bad | check("addresses of one home slot", x);
}

int main() { return family<Arp>() | family<Ndp>() | ndp_collisions(); }
