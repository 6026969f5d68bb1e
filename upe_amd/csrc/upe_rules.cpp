// upe_rules.cpp — the rule compiler of libupe_gpu: rule_t tables -> the images the classify
// kernels read (upe_dev.h): the RuleV4 / RuleV6 words, the family lists, the tuple-space index,
// the decision-tree forest; and the host walk of the tree (upe_rules_match_host).  Also the
// neighbour snapshot upe_gpu_load_neigh uploads (build_neigh_image; upe_neigh_compile hands it
// out as a value, as upe_rules_compile hands out the rule image).  Plain C++, host memory
// only: no context, no GPU, any thread.  tools/rules_san.cpp and tools/neigh_san.cpp run it under
// the host sanitizers (`make rules-san`, `make neigh-san`).
#include "upe_rules.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <deque>
#include <map>
#include <new>
#include <utility>

namespace upe {

// (upe_rules.h)
int cuckoo3_place(const std::vector<uint32_t>& key, uint32_t& bits, uint32_t& seed,
                  std::vector<int32_t>& slot, size_t room) {
    const size_t n = key.size();
    slot.clear();
    bits = 0;
    seed = 0;
    if (n + room == 0) return 0;
    // Equal keys share their three candidate slots under every seed and at every size: a fourth
    // can never be placed.  Fail now: the search below would try every seed at every size up to
    // 2^31 slots first (terabytes of slot-array clears) before it gave up.
    {
        std::vector<uint32_t> sorted(key);
        std::sort(sorted.begin(), sorted.end());
        for (size_t j = 3; j < n; ++j)
            if (sorted[j] == sorted[j - 3]) return -1;
    }
    bits = 1;
    while (((size_t)1 << bits) * 4 < (n + room) * 5) ++bits;   // (n + room <= 2^31)
    for (; bits <= 31; ++bits) {
        const size_t m = (size_t)1 << bits;
        for (uint32_t attempt = 0; attempt < 64; ++attempt) {
            const uint32_t sd = attempt * 0x6D2B79F5u + bits;
            slot.assign(m, -1);
            uint32_t rnd = sd | 1u;
            bool ok = true;
            for (size_t j = 0; j < n && ok; ++j) {
                int32_t cur = (int32_t)j;
                uint32_t from = ~0u;
                for (int kick = 0;; ++kick) {
                    const uint32_t c[3] = {slot1(key[cur], sd, bits), slot2(key[cur], sd, bits),
                                           slot3(key[cur], sd, bits)};
                    int placed = -1;
                    for (int q = 0; q < 3 && placed < 0; ++q)
                        if (slot[c[q]] < 0) placed = q;
                    if (placed >= 0) {
                        slot[c[placed]] = cur;
                        break;
                    }
                    if (kick >= 1000) {
                        ok = false;
                        break;
                    }
                    // evict a random choice other than the slot the key was just evicted from
                    rnd ^= rnd << 13; rnd ^= rnd >> 17; rnd ^= rnd << 5;
                    uint32_t q = rnd % 3u;
                    if (c[q] == from) q = (q + 1) % 3u;
                    std::swap(cur, slot[c[q]]);
                    from = c[q];
                }
            }
            if (ok) {
                seed = sd;
                return 0;
            }
        }
    }
    return -1;
}

namespace {
// The slots a reference probe reaches (arp_get_mac, src/arp_table.c:55-80; ndp_get_mac,
// src/ndp_table.c:67-86): from the key's home slot, a linear probe answers with the first valid
// entry of the same key and stops at the first invalid slot.
template <class E, class Home, class Same>
std::vector<uint32_t> reachable(const E* e, size_t cap, Home home, Same same) {
    std::vector<uint32_t> keep;
    const size_t mask = cap - 1;
    for (size_t s0 = 0; s0 < cap; ++s0) {
        if (!e[s0].valid) continue;
        for (size_t i = 0, t = home(e[s0]) & mask; i < cap; ++i, t = (t + 1) & mask) {
            if (!e[t].valid) break;
            if (same(e[t], e[s0])) {
                if (t == s0) keep.push_back((uint32_t)s0);
                break;
            }
        }
    }
    return keep;
}
}  // namespace

// (upe_rules.h)
int build_neigh_image(const upe_arp_entry_t* arp, size_t arp_cap, const upe_ndp_entry_t* ndp,
                      size_t ndp_cap, NeighImage& im, size_t arp_room, size_t ndp_room) {
    const std::vector<uint32_t> arp_keep = reachable(
        arp, arp_cap, [](const upe_arp_entry_t& e) { return (size_t)e.ip; },
        [](const upe_arp_entry_t& a, const upe_arp_entry_t& b) { return a.ip == b.ip; });
    // ndp_hash (src/ndp_table.c:6-17): home slot = XOR of the LE words
    const std::vector<uint32_t> ndp_keep = reachable(
        ndp, ndp_cap,
        [](const upe_ndp_entry_t& e) {
            return (size_t)(le32(e.ip) ^ le32(e.ip + 4) ^ le32(e.ip + 8) ^ le32(e.ip + 12));
        },
        [](const upe_ndp_entry_t& a, const upe_ndp_entry_t& b) { return memcmp(a.ip, b.ip, 16) == 0; });
    // Place the reachable entries by three-choice cuckoo hashing at load factor <= 0.8.
    std::vector<uint32_t> akey(arp_keep.size()), nkey(ndp_keep.size());
    for (size_t j = 0; j < arp_keep.size(); ++j) akey[j] = arp[arp_keep[j]].ip;
    std::vector<std::array<uint32_t, 4>> nwords(ndp_keep.size());
    for (size_t j = 0; j < ndp_keep.size(); ++j) {
        const uint8_t* ip = ndp[ndp_keep[j]].ip;
        nwords[j] = {le32(ip), le32(ip + 4), le32(ip + 8), le32(ip + 12)};
        nkey[j] = fold_v6(nwords[j].data());
    }
    std::vector<int32_t> aslot, nslot;   // slot -> entry (index into *_keep), -1 empty
    if (cuckoo3_place(akey, im.arp_bits, im.arp_seed, aslot, arp_room) != 0 ||
        cuckoo3_place(nkey, im.ndp_bits, im.ndp_seed, nslot, ndp_room) != 0)
        return fail("neighbour index: cuckoo placement failed (at most three reachable IPv6 "
                    "addresses may share one fold_v6)");
    im.arp.assign(aslot.size(), make_uint4(0, 0, 0, 0));
    for (size_t t = 0; t < aslot.size(); ++t) {
        if (aslot[t] < 0) continue;
        const upe_arp_entry_t& e = arp[arp_keep[aslot[t]]];
        im.arp[t] = make_uint4(e.ip, mac_lo(e.mac), mac_hi(e.mac) | (1u << 16), 0);
    }
    im.ndp.assign(2 * nslot.size(), make_uint4(0, 0, 0, 0));
    for (size_t t = 0; t < nslot.size(); ++t) {
        if (nslot[t] < 0) continue;
        const upe_ndp_entry_t& e = ndp[ndp_keep[nslot[t]]];
        const auto& w = nwords[nslot[t]];
        im.ndp[2 * t] = make_uint4(w[0], w[1], w[2], w[3]);
        im.ndp[2 * t + 1] = make_uint4(mac_lo(e.mac), mac_hi(e.mac) | (1u << 16), 0, 0);
    }
    if (im.arp.empty()) im.arp.push_back(make_uint4(0, 0, 0, 0));   // keep a valid allocation
    if (im.ndp.empty()) im.ndp.resize(2, make_uint4(0, 0, 0, 0));
    // what upe_gpu_neigh_learn needs to know of the arrays (capacities <= 2^30)
    size_t avalid = 0, nvalid = 0;
    for (size_t s = 0; s < arp_cap; ++s) avalid += arp[s].valid ? 1u : 0u;
    for (size_t s = 0; s < ndp_cap; ++s) nvalid += ndp[s].valid ? 1u : 0u;
    im.arp_free = (uint32_t)(arp_cap - avalid);
    im.ndp_free = (uint32_t)(ndp_cap - nvalid);
    im.arp_insertable = im.arp_bits != 0 && arp_keep.size() == avalid;
    im.ndp_insertable = im.ndp_bits != 0 && ndp_keep.size() == nvalid;
    return 0;
}

// (upe_rules.h)
int compile_neigh(const upe_arp_entry_t* arp, size_t arp_cap, const upe_ndp_entry_t* ndp,
                  size_t ndp_cap, NeighImage& im, size_t arp_room, size_t ndp_room) {
    auto pow2 = [](size_t x) { return x == 0 || (x & (x - 1)) == 0; };
    if (!pow2(arp_cap) || !pow2(ndp_cap))
        return fail("neighbour table capacity must be a power of two (arp_table_init)");
    if ((arp_cap && !arp) || (ndp_cap && !ndp)) return fail("null table");
    if (arp_cap > (1u << 30) || ndp_cap > (1u << 30)) return fail("table too large");
    if (arp_room > (1u << 30) || ndp_room > (1u << 30)) return fail("room too large");
    return build_neigh_image(arp, arp_cap, ndp, ndp_cap, im, arp_room, ndp_room);
}

}  // namespace upe

using namespace upe;

namespace {

uint32_t act_code(int32_t type) { return type == UPE_ACT_DROP ? 0u : type == UPE_ACT_FWD ? 1u : 2u; }

// Two-choice cuckoo placement of distinct keys by a seed-dependent 32-bit hash per key,
// hfn(j, seed) (different entries may share a hash key, the device compares the full key).
// Starts at 2^bits >= ratio_x2 / 2 x n slots and tries seeds, then doubles, until every key sits
// in slot1 or slot2.  bits = 0 for no keys.
template <class H>
int cuckoo_place_fn(size_t n, H hfn, uint32_t& bits, uint32_t& seed, std::vector<int32_t>& slot,
                    uint32_t ratio_x2 = 5) {
    std::vector<uint32_t> key(n);
    slot.clear();
    bits = 0;
    seed = 0;
    if (n == 0) return 0;
    bits = 1;
    while (((size_t)1 << bits) * 2 < n * ratio_x2) ++bits;
    for (; bits <= 31; ++bits) {
        const size_t m = (size_t)1 << bits;
        for (uint32_t attempt = 0; attempt < 64; ++attempt) {
            const uint32_t sd = attempt * 0x6D2B79F5u + bits;
            for (size_t j = 0; j < n; ++j) key[j] = hfn(j, sd);
            slot.assign(m, -1);
            bool ok = true;
            for (size_t j = 0; j < n && ok; ++j) {
                int32_t cur = (int32_t)j;
                uint32_t t = slot1(key[cur], sd, bits);
                for (int kick = 0;; ++kick) {
                    if (slot[t] < 0) {
                        slot[t] = cur;
                        break;
                    }
                    if (kick >= 500) {
                        ok = false;
                        break;
                    }
                    std::swap(cur, slot[t]);   // evict; the evicted key moves to its other slot
                    const uint32_t s1 = slot1(key[cur], sd, bits), s2 = slot2(key[cur], sd, bits);
                    t = t == s1 ? s2 : s1;
                }
            }
            if (ok) {
                seed = sd;
                return 0;
            }
        }
    }
    return -1;
}

// Tuple-space index of the compiled rules (see TssGroup).  Returns false when the table is
// better served by the linear scan: small tables, or too many distinct mask signatures.
bool build_tss_family(int F, const std::vector<RuleV4>& v4, const std::vector<RuleV6>& v6,
                      const upe_rule_t* rules, size_t count, TssFamily& out) {
    const int nw = F == 4 ? 4 : 10;
    using Sig = std::array<uint32_t, 10>;
    using Key = std::array<uint32_t, 10>;
    struct Grp {
        uint32_t minidx = kNone;
        std::map<Key, uint32_t> keys;   // masked key -> smallest sorted index
    };
    std::map<Sig, Grp> groups;
    for (size_t i = 0; i < count; ++i) {
        const uint8_t ver = rules[i].ip_ver;
        if (ver != 0 && ver != F) continue;
        const RuleV4& r = v4[i];
        const RuleV6& q = v6[i];
        Sig sg{};
        Key k{};
        sg[0] = r.m0 & ~0xFFu;
        sg[1] = r.m1 & 0xFFFFu;
        sg[2] = r.sm0;
        sg[3] = r.dm0;
        k[0] = r.x0 & sg[0];
        k[1] = r.x1 & sg[1];
        k[2] = r.s0;
        if (F == 4) {
            k[3] = r.d0;
        } else {
            for (int j = 0; j < 3; ++j) {
                sg[4 + j] = q.sm[j];
                sg[7 + j] = q.dm[j];
            }
            k[3] = q.s[0]; k[4] = q.s[1]; k[5] = q.s[2];
            k[6] = r.d0;
            k[7] = q.d[0]; k[8] = q.d[1]; k[9] = q.d[2];
        }
        Grp& g = groups[sg];
        if (g.minidx == kNone) g.minidx = (uint32_t)i;
        g.keys.emplace(k, (uint32_t)i);   // first insertion = smallest sorted index
    }
    std::vector<std::pair<uint32_t, const std::pair<const Sig, Grp>*>> order;
    for (const auto& kv : groups) order.push_back({kv.second.minidx, &kv});
    std::sort(order.begin(), order.end(),
              [](const auto& x, const auto& y) { return x.first < y.first; });
    const int per = F == 4 ? kTssSlot4 : kTssSlot6;
    out.groups.clear();
    out.slots.clear();
    for (const auto& o : order) {
        const Sig& sg = o.second->first;
        const Grp& g = o.second->second;
        std::vector<Key> keys;
        std::vector<uint32_t> idx;
        for (const auto& kv : g.keys) {
            keys.push_back(kv.first);
            idx.push_back(kv.second);
        }
        uint32_t bits = 0, seed = 0;
        std::vector<int32_t> slot;
        if (cuckoo_place_fn(keys.size(),
                            [&](size_t j, uint32_t sd) { return tss_hash(keys[j].data(), nw, sd); },
                            bits, seed, slot, kTssRatioX2) != 0)
            return false;
        TssGroup d;
        memset(&d, 0, sizeof d);
        for (int j = 0; j < 10; ++j) d.w[j] = sg[j];
        d.w[10] = g.minidx;
        d.w[11] = bits;
        d.w[12] = seed;
        d.w[13] = (uint32_t)(out.slots.size() / per);
        bool wild = true;
        for (int j = 0; j < 10; ++j) wild = wild && sg[j] == 0;
        if (wild && idx.size() == 1)
            d.w[14] = 1u | (act_code(rules[idx[0]].action.type) << 8);
        out.groups.push_back(d);
        const size_t base = out.slots.size();
        out.slots.resize(base + slot.size() * per, make_uint4(0, 0, 0, 0));
        const size_t fbase = out.fp.size();
        out.fp.resize(fbase + slot.size(), 0);
        for (size_t t = 0; t < slot.size(); ++t) {
            if (slot[t] < 0) continue;
            const Key& k = keys[slot[t]];
            out.fp[fbase + t] = tss_tag(tss_hash(k.data(), nw, seed));
            uint4* e = &out.slots[base + t * per];
            const uint32_t act = act_code(rules[idx[slot[t]]].action.type);
            if (F == 4) {
                const uint32_t v = (idx[slot[t]] + 1u) | act << 22;
                e[0] = make_uint4(k[0] | (v & 0xFFu), k[1] | ((v >> 8) << 16), k[2], k[3]);
            } else {
                e[0] = make_uint4(k[0], k[1], k[2], k[3]);
                e[1] = make_uint4(k[4], k[5], k[6], k[7]);
                e[2] = make_uint4(k[8], k[9], idx[slot[t]], 1u | (act << 8));
            }
        }
    }
    return true;
}

// ---- decision-tree index (round 5; TreeNode comment) ----------------------------------------
// The conservative range of one rule of a family list on one key word: lo = x & m, hi = x | ~m
// (within the word's width); `exact` when ~m is a run of low bits (prefix, exact value or
// wildcard), so that the range is exactly the set of values the rule accepts on that word.
struct TreeRule {
    uint32_t lo[kTreeDims], hi[kTreeDims];
    uint16_t exact;   // bit d: word d's range is exact
};
constexpr uint32_t kTreeWidth[kTreeDims] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu,
                                            0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu,
                                            0xFFFFu, 0xFFFFu, 0xFFu};
// A family list entry (RuleV4 words, plus the IPv6 words for family 6) as key-word ranges.  IPv4
// word 0 is host order already (src/parser.c:40-41) and its other address words are 0 in the key.
// An IPv6 address word is compared big-endian (a prefix is then a range) when bit j (source word
// j) or 4 + j (destination word j) of swap6 is set, else as loaded: a version-agnostic rule's
// IPv4 prefix (host order, src/rule_config.c:60-66) is a range only that way (tree_swap6).
uint32_t word_of(uint32_t v, uint32_t swap6, int j) { return (swap6 >> j & 1u) ? bswap32(v) : v; }
TreeRule tree_rule(int F, const RuleV4& r, const RuleV6* q, uint32_t swap6 = 0xFFu) {
    TreeRule t;
    uint32_t x[kTreeDims] = {}, m[kTreeDims] = {};
    if (F == 4) {
        x[0] = r.s0; m[0] = r.sm0;
        x[4] = r.d0; m[4] = r.dm0;
    } else {
        for (int j = 0; j < 4; ++j) {
            const uint32_t xs = j ? q->s[j - 1] : r.s0, ms = j ? q->sm[j - 1] : r.sm0;
            const uint32_t xd = j ? q->d[j - 1] : r.d0, md = j ? q->dm[j - 1] : r.dm0;
            x[j] = word_of(xs, swap6, j); m[j] = word_of(ms, swap6, j);
            x[4 + j] = word_of(xd, swap6, 4 + j); m[4 + j] = word_of(md, swap6, 4 + j);
        }
    }
    x[8] = r.x0 >> 16; m[8] = r.m0 >> 16;
    x[9] = r.x1 & 0xFFFFu; m[9] = r.m1 & 0xFFFFu;
    x[10] = (r.x0 >> 8) & 0xFFu; m[10] = (r.m0 >> 8) & 0xFFu;
    t.exact = 0;
    for (int d = 0; d < kTreeDims; ++d) {
        const uint32_t w = kTreeWidth[d], inv = ~m[d] & w;
        t.lo[d] = x[d] & m[d] & w;
        t.hi[d] = (x[d] & w) | inv;
        if ((inv & (inv + 1u)) == 0) t.exact |= (uint16_t)(1u << d);
    }
    return t;
}

// The byte order of each IPv6 address word under which more of the family's rules are ranges
// (exact): big-endian for IPv6 prefixes, as loaded for version-agnostic IPv4 prefixes in the
// IPv6 list (config C's 10 %); ties big-endian.
uint32_t tree_swap6(const std::vector<RuleV4>& v4, const std::vector<RuleV6>& v6,
                    const std::vector<uint32_t>& l6) {
    auto exact = [](uint32_t m) { const uint32_t inv = ~m; return (inv & (inv + 1u)) == 0; };
    uint32_t swap6 = 0;
    for (int w = 0; w < 8; ++w) {
        const int j = w & 3;
        long votes = 0;
        for (uint32_t i : l6) {
            const uint32_t m = w < 4 ? (j ? v6[i].sm[j - 1] : v4[i].sm0)
                                     : (j ? v6[i].dm[j - 1] : v4[i].dm0);
            votes += (long)exact(bswap32(m)) - (long)exact(m);
        }
        if (votes >= 0) swap6 |= 1u << w;
    }
    return swap6;
}

// HyperSplit-style build of one family's tree into img (breadth first, so the top levels are
// contiguous).  rules: the family list's entries in list order.  Returns false when the node
// budget or the leaf-length limit is exceeded (the table then keeps the linear scan).
bool build_tree_family(const std::vector<TreeRule>& R, const std::vector<uint32_t>& members,
                       int fam_slot, uint32_t binth, size_t node_budget, TreeImage& img,
                       uint32_t dims = (1u << kTreeDims) - 1u) {
    struct Task {
        uint32_t node;
        uint32_t depth;
        std::array<uint32_t, kTreeDims> lo, hi;
        std::vector<uint32_t> list;
    };
    const uint32_t root = (uint32_t)img.nodes.size();
    img.nodes.push_back(make_uint2(0, 0));
    std::deque<Task> q;
    Task t0;
    t0.node = root;
    t0.depth = 0;
    for (int d = 0; d < kTreeDims; ++d) {
        t0.lo[d] = 0;
        t0.hi[d] = kTreeWidth[d];
    }
    t0.list = members;
    q.push_back(std::move(t0));
    std::vector<uint32_t> los, his, cand;
    while (!q.empty()) {
        Task t = std::move(q.front());
        q.pop_front();
        // keep the rules up to the first one that matches every key of the box
        std::vector<uint32_t>& L = t.list;
        std::vector<uint8_t> covers(L.size(), 0);
        for (size_t j = 0; j < L.size(); ++j) {
            const TreeRule& r = R[L[j]];
            bool cov = true;
            for (int d = 0; d < kTreeDims && cov; ++d)
                cov = (r.exact >> d & 1u) && r.lo[d] <= t.lo[d] && r.hi[d] >= t.hi[d];
            if (cov) {
                covers[j] = 1;
                L.resize(j + 1);
                covers.resize(j + 1);
                break;
            }
        }
        const uint32_t n = (uint32_t)L.size();
        int best_d = -1;
        uint32_t best_t = 0, best_max = n, best_sum = 2 * n;
        if (n > binth && !covers[0]) {
            for (int d = 0; d < kTreeDims; ++d) {
                if (!(dims >> d & 1u)) continue;
                los.clear();
                his.clear();
                bool split = false;
                for (uint32_t j : L) {
                    const uint32_t lo = std::max(R[j].lo[d], t.lo[d]);
                    const uint32_t hi = std::min(R[j].hi[d], t.hi[d]);
                    los.push_back(lo);
                    his.push_back(hi);
                    split |= lo > t.lo[d] || hi < t.hi[d];
                }
                if (!split) continue;
                std::sort(los.begin(), los.end());
                std::sort(his.begin(), his.end());
                cand.clear();
                for (uint32_t v : los)
                    if (v > t.lo[d]) cand.push_back(v);
                for (uint32_t v : his)
                    if (v < t.hi[d]) cand.push_back(v + 1u);
                std::sort(cand.begin(), cand.end());
                cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
                size_t il = 0, ih = 0;
                for (uint32_t c : cand) {
                    while (il < los.size() && los[il] < c) ++il;   // rules reaching below c
                    while (ih < his.size() && his[ih] < c) ++ih;   // rules ending below c
                    const uint32_t nl = (uint32_t)il, nr = n - (uint32_t)ih;
                    const uint32_t mx = std::max(nl, nr), sm = nl + nr;
                    if (mx < best_max || (mx == best_max && sm < best_sum)) {
                        best_max = mx;
                        best_sum = sm;
                        best_d = d;
                        best_t = c;
                    }
                }
            }
        }
        if (best_d < 0 || best_max >= n) {
            // a leaf: its rules in list order, the covering one flagged
            if (n >= (1u << 11)) return false;
            img.nodes[t.node] = make_uint2(16u | n << 5, (uint32_t)img.leaves.size());
            for (uint32_t j = 0; j < n; ++j)
                img.leaves.push_back(L[j] | (covers[j] ? 0x80000000u : 0u));
            img.max_leaf = std::max(img.max_leaf, n);
            img.depth[fam_slot] = std::max(img.depth[fam_slot], t.depth);
            std::vector<uint32_t>().swap(L);
            continue;
        }
        if (img.nodes.size() + 2 > node_budget || img.nodes.size() + 2 >= (1u << 27)) return false;
        const uint32_t child = (uint32_t)img.nodes.size();
        img.nodes.push_back(make_uint2(0, 0));
        img.nodes.push_back(make_uint2(0, 0));
        img.nodes[t.node] = make_uint2((uint32_t)best_d | child << 5, best_t);
        Task a, b;
        a.node = child;
        b.node = child + 1;
        a.depth = b.depth = t.depth + 1;
        a.lo = b.lo = t.lo;
        a.hi = b.hi = t.hi;
        a.hi[best_d] = best_t - 1u;
        b.lo[best_d] = best_t;
        for (uint32_t j : L) {
            if (std::max(R[j].lo[best_d], t.lo[best_d]) < best_t) a.list.push_back(j);
            if (std::min(R[j].hi[best_d], t.hi[best_d]) >= best_t) b.list.push_back(j);
        }
        std::vector<uint32_t>().swap(L);
        q.push_back(std::move(a));
        q.push_back(std::move(b));
    }
    return true;
}

// One family's forest: its rules grouped by the key field (source address, destination address,
// source port, destination port, protocol) whose range overlaps the fewest other rules of the
// list (EffiCuts-style separation: a rule narrow only in its destination port is not copied into
// every leaf of a tree that splits on addresses), one tree per field, each split on its own field's
// words (an address tree also on the ports and the protocol) only, so that a walk level selects
// among few key words prepared before the walk (tree_match), every tree's
// rules in list order; a field no rule is narrowest in gets an empty tree.  A key's first match
// is the smallest of its first matches in the trees (the groups partition the list).  The
// family's first rule that matches every key is no tree's, nor is any rule after it: it is the
// answer when no tree has one (*def, its list position, else kNone).  roots: kTreeFields entries.
int tree_field(int d) { return d < 4 ? 0 : d < 8 ? 1 : d - 6; }
constexpr uint32_t kTreeFieldDims[kTreeFields] = {0x70Fu, 0x7F0u, 1u << 8, 1u << 9, 1u << 10};
bool build_forest_family(const std::vector<TreeRule>& R, int fam_slot, uint32_t binth,
                         size_t node_budget, TreeImage& img, std::vector<uint32_t>& roots,
                         uint32_t* def, const std::vector<TreeRule>* RG = nullptr) {
    const size_t n = R.size();
    const std::vector<TreeRule>& G = RG ? *RG : R;
    roots.clear();
    *def = kNone;
    std::vector<int> grp(n, -1);
    std::vector<uint32_t> best(n, 0xFFFFFFFFu);
    std::vector<uint32_t> los(n), his(n);
    for (int d = 0; d < kTreeDims && n > 0; ++d) {
        for (size_t i = 0; i < n; ++i) {
            los[i] = G[i].lo[d];
            his[i] = G[i].hi[d];
        }
        std::sort(los.begin(), los.end());
        std::sort(his.begin(), his.end());
        for (size_t i = 0; i < n; ++i) {
            // rules whose range meets rule i's on word d: lo <= hi_i, minus those ending below lo_i
            const size_t a = (size_t)(std::upper_bound(los.begin(), los.end(), G[i].hi[d]) - los.begin());
            const size_t b = (size_t)(std::lower_bound(his.begin(), his.end(), G[i].lo[d]) - his.begin());
            const uint32_t ov = (uint32_t)(a - b);
            if (ov < best[i]) {
                best[i] = ov;
                grp[i] = tree_field(d);
            }
        }
    }
    for (size_t i = 0; i < n; ++i) {
        bool all = true;
        for (int d = 0; d < kTreeDims && all; ++d)
            all = (R[i].exact >> d & 1u) && R[i].lo[d] == 0 && R[i].hi[d] == kTreeWidth[d];
        if (all) {   // matches every key of the family
            grp[i] = -1;
            if (*def == kNone) *def = (uint32_t)i;
        }
    }
    // rules after the family's first catch-all are never a first match: no tree's
    std::vector<std::vector<uint32_t>> groups(kTreeFields);
    for (size_t i = 0; i < n && i < *def; ++i)
        if (grp[i] >= 0) groups[grp[i]].push_back((uint32_t)i);
    for (int g = 0; g < kTreeFields; ++g) {
        const std::vector<uint32_t>& members = groups[g];
        roots.push_back((uint32_t)img.nodes.size());
        if (members.empty()) {   // an empty leaf
            img.nodes.push_back(make_uint2(16u, 0u));
            continue;
        }
        const size_t n0 = img.nodes.size(), e0 = img.leaves.size();
        // (large groups: longer leaves, or nested prefixes multiply the leaves)
        const uint32_t bt = members.size() > 4096 ? std::max(binth, 16u) : binth;
        const bool ok = build_tree_family(R, members, fam_slot, bt, node_budget, img,
                                          kTreeFieldDims[g]);
        if (getenv("UPE_GPU_VERBOSE"))
            fprintf(stderr, "upe_gpu: tree family %d field %d: %zu rules, %zu nodes, %zu leaf entries%s\n",
                    fam_slot ? 6 : 4, g, members.size(), img.nodes.size() - n0,
                    img.leaves.size() - e0, ok ? "" : " (over budget)");
        if (!ok) return false;
    }
    return true;
}

// Binary nodes (build_tree_family: inner {dim | child << 5, threshold}, leaf {16 | count << 5,
// first entry}) -> the walk's two-level nodes (Args::tree comment), breadth first from the roots
// (roots[k] -> node first + k).  False when an index outgrows its bits.
bool pack_two_level(const std::vector<uint2>& bin, const std::vector<uint32_t>& roots,
                    uint32_t first, std::vector<uint4>& out) {
    auto is_leaf = [&](uint32_t b) { return (bin[b].x & 16u) != 0u; };
    auto leaf_word = [&](uint32_t b, bool& ok) {
        const uint32_t cnt = bin[b].x >> 5, off = bin[b].y;
        ok = ok && cnt < (1u << 11) && off < (1u << 21);
        return cnt << 21 | off;
    };
    out.resize(first + roots.size(), make_uint4(0, 0, 0, 0));
    std::deque<std::pair<uint32_t, uint32_t>> q;   // (binary node, packed node)
    for (size_t k = 0; k < roots.size(); ++k) q.emplace_back(roots[k], first + (uint32_t)k);
    bool ok = true;
    while (!q.empty() && ok) {
        const auto [b, o] = q.front();
        q.pop_front();
        if (is_leaf(b)) {
            out[o] = make_uint4(1u << 12, leaf_word(b, ok), 0, 0);
            continue;
        }
        const uint32_t l = bin[b].x >> 5, r = l + 1;
        const bool ll = is_leaf(l), rl = is_leaf(r);
        const uint32_t base = (ll && rl) ? 0u : (uint32_t)out.size();
        ok = ok && base < (1u << 17);
        uint4 nd;
        nd.x = (bin[b].x & 15u) | (bin[l].x & 15u) << 4 | (bin[r].x & 15u) << 8 |
               (ll ? 1u : 0u) << 13 | (rl ? 1u : 0u) << 14 | base << 15;
        nd.y = bin[b].y;
        nd.z = ll ? leaf_word(l, ok) : bin[l].y;
        nd.w = rl ? leaf_word(r, ok) : bin[r].y;
        out[o] = nd;
        uint32_t next = base;
        for (const uint32_t c : {l, r}) {
            if (is_leaf(c)) continue;
            out.resize(out.size() + 2, make_uint4(0, 0, 0, 0));
            q.emplace_back(bin[c].x >> 5, next);
            q.emplace_back((bin[c].x >> 5) + 1u, next + 1u);
            next += 2;
        }
    }
    return ok;
}

// The forests of both family lists (l4 / l6: sorted indexes of the list entries), packed two
// levels to a node after the directory (Args::tree comment: node 0 = {trees of family 4, trees
// of family 6 | IPv6 byte orders << 16, the families' default answers (list positions, kNone =
// none)}, then the trees' roots, family 4's first, so that a walk starts without an indirection).
// group_be: the IPv6 rules grouped by their big-endian ranges whatever the words' byte order
// (build_tree's choice).
bool build_tree_as(const std::vector<RuleV4>& v4, const std::vector<RuleV6>& v6,
                   const std::vector<uint32_t>& l4, const std::vector<uint32_t>& l6, uint32_t binth,
                   size_t node_budget, bool group_be, TreeImage& img) {
    img = TreeImage();
    TreeImage body;
    std::vector<TreeRule> R;
    std::vector<uint32_t> r4, r6;
    uint32_t def4 = kNone, def6 = kNone;
    for (uint32_t i : l4) R.push_back(tree_rule(4, v4[i], nullptr));
    if (!build_forest_family(R, 0, binth, node_budget, body, r4, &def4)) return false;
    R.clear();
    const uint32_t swap6 = tree_swap6(v4, v6, l6);
    for (uint32_t i : l6) R.push_back(tree_rule(6, v4[i], &v6[i], swap6));
    std::vector<TreeRule> RG;
    if (group_be)
        for (uint32_t i : l6) RG.push_back(tree_rule(6, v4[i], &v6[i], 0xFFu));
    if (!build_forest_family(R, 1, binth, node_budget, body, r6, &def6, group_be ? &RG : nullptr))
        return false;
    std::vector<uint32_t> roots = r4;
    roots.insert(roots.end(), r6.begin(), r6.end());
    std::vector<uint4> packed;
    if (!pack_two_level(body.nodes, roots, 1u, packed)) return false;
    packed[0] = make_uint4((uint32_t)r4.size(), (uint32_t)r6.size() | swap6 << 16, def4, def6);
    img.nodes.resize(2 * packed.size());
    memcpy(img.nodes.data(), packed.data(), packed.size() * sizeof(uint4));
    img.leaves = std::move(body.leaves);
    img.depth[0] = body.depth[0];
    img.depth[1] = body.depth[1];
    img.max_leaf = body.max_leaf;
    img.trees[0] = (uint32_t)r4.size();
    img.trees[1] = (uint32_t)r6.size();
    img.swap6 = swap6;
    return true;
}

// Host walk of the image, bit for bit what tree_match does on the device: the list position of
// the key's first match (kNone = none).  kv: the key words (kTreeDims comment).
uint32_t tree_walk_host(const TreeImage& img, const std::vector<RuleV4>& v4,
                        const std::vector<RuleV6>& v6, const std::vector<uint32_t>& list, bool is6,
                        const uint32_t kv[kTreeDims], uint32_t k0, uint32_t k1, const uint32_t s[4],
                        const uint32_t d[4], uint8_t* prof_depth, uint8_t* prof_steps) {
    const uint2 dir = img.nodes[0], dflt = img.nodes[1];
    const uint32_t nt = is6 ? dir.y & 0xFFFFu : dir.x, first = 1u + (is6 ? dir.x : 0u);
    const uint4* S = reinterpret_cast<const uint4*>(img.nodes.data());
    uint32_t best = kNone;
    for (uint32_t t = 0; t < nt; ++t) {
        uint32_t idx = first + t, lw = 0, depth = 0;
        for (;;) {   // tree_match's step, two levels per node
            const uint4 q = S[idx];
            ++depth;
            if (q.x & 0x1000u) {
                lw = q.y;
                break;
            }
            const bool c1 = kv[q.x & 15u] >= q.y;
            const bool lleaf = (q.x >> 13) & 1u;
            const bool cl = c1 ? ((q.x >> 14) & 1u) != 0u : lleaf;
            const uint32_t ct = c1 ? q.w : q.z;
            if (cl) {
                lw = ct;
                break;
            }
            const uint32_t c2 = kv[c1 ? (q.x >> 8) & 15u : (q.x >> 4) & 15u] >= ct ? 1u : 0u;
            idx = (q.x >> 15) + ((c1 && !lleaf) ? 2u : 0u) + c2;
        }
        const uint32_t cnt = lw >> 21, off = lw & 0x1FFFFFu;
        if (prof_depth && t < 16) {
            prof_depth[t] = (uint8_t)std::min(depth, 255u);
            prof_steps[t] = 0;
        }
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t e = img.leaves[off + j];
            const uint32_t pos = e & 0x7FFFFFFFu;
            if (prof_steps && t < 16 && prof_steps[t] < 255) ++prof_steps[t];
            if (pos >= best) break;
            bool hit = (e >> 31) != 0;
            if (!hit) {
                const RuleV4& r = v4[list[pos]];
                uint32_t x = ((k0 ^ r.x0) & r.m0) | ((k1 ^ r.x1) & r.m1 & 0xFFFFu) |
                             ((s[0] ^ r.s0) & r.sm0) | ((d[0] ^ r.d0) & r.dm0);
                if (is6) {
                    const RuleV6& q6 = v6[list[pos]];
                    for (int w = 0; w < 3; ++w)
                        x |= ((s[w + 1] ^ q6.s[w]) & q6.sm[w]) | ((d[w + 1] ^ q6.d[w]) & q6.dm[w]);
                }
                hit = x == 0;
            }
            if (hit) {
                best = pos;
                break;
            }
        }
    }
    return best != kNone ? best : is6 ? dflt.y : dflt.x;
}

// Sampled walk cost of an image's IPv6 forest: nodes loaded plus leaf entries read (tree_walk_host's
// profile) over keys whose fields are drawn from the IPv6 rules' own constrained fields, a stand-in
// for traffic from the pools the rules were written for.
uint64_t tree_sample_cost6(const TreeImage& img, const std::vector<RuleV4>& v4,
                           const std::vector<RuleV6>& v6, const std::vector<uint32_t>& l6) {
    static constexpr int kFieldDims[5][2] = {{0, 4}, {4, 8}, {8, 9}, {9, 10}, {10, 11}};
    std::vector<TreeRule> R;
    for (uint32_t i : l6) R.push_back(tree_rule(6, v4[i], &v6[i], img.swap6));
    std::vector<uint32_t> by_field[5];
    for (uint32_t i = 0; i < (uint32_t)R.size(); ++i)
        for (int f = 0; f < 5; ++f)
            for (int dm = kFieldDims[f][0]; dm < kFieldDims[f][1]; ++dm)
                if (R[i].lo[dm] != 0 || R[i].hi[dm] != kTreeWidth[dm]) {
                    by_field[f].push_back(i);
                    break;
                }
    uint64_t x = 0x9E3779B97F4A7C15ull, cost = 0;
    auto rnd = [&]() {   // splitmix64
        uint64_t z = (x += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return (uint32_t)(z ^ (z >> 31));
    };
    const size_t n = std::min<size_t>(4096, 4 * R.size());
    for (size_t k = 0; k < n; ++k) {
        uint32_t kv[kTreeDims] = {};
        for (int f = 0; f < 5; ++f) {
            const TreeRule* r = by_field[f].empty() ? nullptr : &R[by_field[f][rnd() % by_field[f].size()]];
            for (int dm = kFieldDims[f][0]; dm < kFieldDims[f][1]; ++dm) {
                const uint32_t lo = r ? r->lo[dm] : 0u, hi = r ? r->hi[dm] : kTreeWidth[dm];
                const uint64_t span = (uint64_t)hi - lo + 1u;
                kv[dm] = lo + (uint32_t)(rnd() % span);
            }
        }
        uint32_t sw[4], dw[4];
        for (int j = 0; j < 4; ++j) {
            sw[j] = word_of(kv[j], img.swap6, j);
            dw[j] = word_of(kv[4 + j], img.swap6, 4 + j);
        }
        const uint32_t k0 = 6u | kv[10] << 8 | kv[8] << 16, k1 = kv[9];
        uint8_t dep[16] = {}, stp[16] = {};
        tree_walk_host(img, v4, v6, l6, true, kv, k0, k1, sw, dw, dep, stp);
        for (int t = 0; t < 16; ++t) cost += dep[t] + stp[t];
    }
    return cost;
}

// build_tree_as, and when the IPv6 words' byte orders differ from big-endian, also with the
// grouping by big-endian ranges: the one of lower sampled cost (tree_sample_cost6).  The byte
// order makes a version-agnostic IPv4 prefix a range (config C6: 75 -> 63 us per 1M), but the
// grouping its ranges imply can move rules into port and protocol trees with long leaves (the
// 16k-rule flow table: 269 -> 332 us; the big-endian grouping 260).
bool build_tree(const std::vector<RuleV4>& v4, const std::vector<RuleV6>& v6,
                const std::vector<uint32_t>& l4, const std::vector<uint32_t>& l6, uint32_t binth,
                size_t node_budget, TreeImage& img) {
    const bool ok = build_tree_as(v4, v6, l4, l6, binth, node_budget, false, img);
    if (!ok || img.swap6 == 0xFFu) return ok;
    TreeImage alt;
    if (!build_tree_as(v4, v6, l4, l6, binth, node_budget, true, alt)) return true;
    const uint64_t ca = tree_sample_cost6(img, v4, v6, l6), cb = tree_sample_cost6(alt, v4, v6, l6);
    if (getenv("UPE_GPU_VERBOSE"))
        fprintf(stderr, "upe_gpu: tree IPv6 byte orders %02x, sampled cost %llu (grouped as such) / %llu (grouped big-endian)\n",
                img.swap6, (unsigned long long)ca, (unsigned long long)cb);
    if (cb < ca) img = std::move(alt);
    return true;
}

size_t tree_node_budget(size_t count) {
    const char* e = getenv("UPE_GPU_TREE_BUDGET");   // diagnostic override
    if (e) return (size_t)strtoull(e, nullptr, 10);
    return std::max<size_t>(1u << 16, 64 * count);
}

// The tree of a table: the shortest leaves (at most 1, 2, 3, then kTreeBinth rules before a
// split) whose image still leaves room in LDS for both family lists (list_bytes), a 1k-rule
// rule_stats histogram and two 1k-slot neighbour indexes — the leaf tests read the lists from
// LDS, and a list left in memory costs more than longer leaves (round 5: CF 73.8 / 71.0 / 87.6 us
// at 4 / 3 / 2, whose image no longer fit; C6 83.7 / 79.2 / 76.6).  Tables whose lists cannot be
// staged anyway get kTreeBinth.  forced: UPE_GPU_TREE_BINTH (diagnostic), 0 = choose.
constexpr size_t kTreeLdsReserve = 56 * 1024;
// The list entries a scan of family F's list can reach: up to and including its first rule that
// matches every key of the family (build_forest_family's default answer), else the whole list.
size_t scan_reach(int F, const std::vector<RuleV4>& v4, const std::vector<RuleV6>& v6,
                  const std::vector<uint32_t>& list) {
    for (size_t j = 0; j < list.size(); ++j) {
        const TreeRule r = tree_rule(F, v4[list[j]], F == 6 ? &v6[list[j]] : nullptr);
        bool all = true;
        for (int d = 0; d < kTreeDims && all; ++d)
            all = (r.exact >> d & 1u) && r.lo[d] == 0 && r.hi[d] == kTreeWidth[d];
        if (all) return j + 1;
    }
    return list.size();
}
bool choose_tree(const std::vector<RuleV4>& v4, const std::vector<RuleV6>& v6,
                 const std::vector<uint32_t>& l4, const std::vector<uint32_t>& l6, size_t count,
                 uint32_t forced, TreeImage& t) {
    const size_t budget = tree_node_budget(count);
    if (forced) return build_tree(v4, v6, l4, l6, forced, budget, t);
    const size_t list_bytes = (2 * l4.size() + kFamV6Stride * l6.size()) * sizeof(uint4);
    if (list_bytes + kTreeLdsReserve >= kLdsDynMaxLarge) return build_tree(v4, v6, l4, l6, kTreeBinth, budget, t);
    for (uint32_t b : {1u, 2u, 3u}) {
        if (!build_tree(v4, v6, l4, l6, b, budget, t)) continue;
        const size_t img = 8 * t.nodes.size() + 4 * t.leaves.size();
        if (img + list_bytes + kTreeLdsReserve <= kLdsDynMaxLarge) return true;
    }
    return build_tree(v4, v6, l4, l6, kTreeBinth, budget, t);
}

// rule_t -> the compiled words: RuleV4 / RuleV6 (pre-masked) and rinfo, pad >= count entries (the
// padding never matches).  -1 (message set) on a rule_id outside [0, cap).
int compile_rules(const upe_rule_t* rules, size_t count, size_t cap, size_t pad,
                  std::vector<RuleV4>& v4, std::vector<RuleV6>& v6, std::vector<int2>& info) {
    v4.assign(pad, RuleV4{});
    v6.assign(pad, RuleV6{});
    info.assign(pad, make_int2(0, 0));
    for (size_t i = 0; i < pad; ++i) {
        RuleV4& a = v4[i];
        RuleV6& b = v6[i];
        memset(&a, 0, sizeof a);
        memset(&b, 0, sizeof b);
        if (i >= count) {
            // never matches: ip_ver byte 0xFF against a key version of 4 or 6
            a.x0 = 0xFF;
            a.m0 = 0xFF;
            continue;
        }
        const upe_rule_t& r = rules[i];
        if (r.rule_id >= cap) return fail("rule_id >= capacity (rule_stats index)");
        a.x0 = (uint32_t)r.ip_ver | ((uint32_t)r.protocol << 8) | ((uint32_t)r.src_port << 16);
        a.m0 = (r.ip_ver ? 0xFFu : 0u) | (r.protocol ? 0xFF00u : 0u) |
               (r.src_port ? 0xFFFF0000u : 0u);
        a.x1 = (uint32_t)r.dst_port | (act_code(r.action.type) << 16);
        a.m1 = r.dst_port ? 0xFFFFu : 0u;
        const uint8_t* si = r.src_ip.v6;
        const uint8_t* sm = r.src_mask.v6;
        const uint8_t* di = r.dst_ip.v6;
        const uint8_t* dm = r.dst_mask.v6;
        a.sm0 = le32(sm);
        a.s0 = le32(si) & a.sm0;
        a.dm0 = le32(dm);
        a.d0 = le32(di) & a.dm0;
        bool v6w = false;
        for (int j = 0; j < 3; ++j) {
            b.sm[j] = le32(sm + 4 * (j + 1));
            b.s[j] = le32(si + 4 * (j + 1)) & b.sm[j];
            b.dm[j] = le32(dm + 4 * (j + 1));
            b.d[j] = le32(di + 4 * (j + 1)) & b.dm[j];
            v6w |= b.sm[j] != 0 || b.dm[j] != 0;
        }
        if (v6w) a.m1 |= kRuleV6Words;   // IPv6 keys must test this rule's rv6 words
        info[i] = make_int2(r.action.type, (int)r.rule_id);
    }
    return 0;
}

// Does compiled rule i match every key of family 4 / 6?
bool matches_all4(const RuleV4& e) {
    return (e.m0 & 0xFFFFFF00u) == 0 && (e.m1 & 0xFFFFu) == 0 && e.sm0 == 0 && e.dm0 == 0;
}
bool matches_all6(const RuleV4& e, const RuleV6& q) {
    bool all = matches_all4(e);
    for (int j = 0; j < 3; ++j) all = all && q.sm[j] == 0 && q.dm[j] == 0;
    return all;
}

// The family lists (FamTable): the sorted indexes of the rules a key of each family can match
// (ip_ver 4 or 0, 6 or 0), each ending at its family's first rule that matches every key of the
// family (nothing after it can be a first match: seed-3 config C's IPv6 list is one entry long).
void family_lists(const upe_rule_t* rules, size_t count, const std::vector<RuleV4>& v4,
                  const std::vector<RuleV6>& v6, std::vector<uint32_t>& l4,
                  std::vector<uint32_t>& l6, bool& end4, bool& end6) {
    l4.clear();
    l6.clear();
    end4 = end6 = false;
    for (size_t i = 0; i < count; ++i) {
        const uint8_t ver = rules[i].ip_ver;
        if (!end4 && (ver == 0 || ver == 4)) {
            l4.push_back((uint32_t)i);
            end4 = matches_all4(v4[i]);
        }
        if (!end6 && (ver == 0 || ver == 6)) {
            l6.push_back((uint32_t)i);
            end6 = matches_all6(v4[i], v6[i]);
        }
    }
}

}  // namespace

// (upe_rules.h)
int upe::build_image(const upe_rule_t* rules, size_t count, size_t cap, upe_rule_image& im) {
    im.count = count;
    im.cap = cap;
    const size_t pad = ((count + kUnroll - 1) / kUnroll + 1) * kUnroll;  // >= 1 padding block
    im.pad = pad;
    std::vector<RuleV4>& v4 = im.v4;
    std::vector<RuleV6>& v6 = im.v6;
    std::vector<int2>& info = im.info;
    if (compile_rules(rules, count, cap, pad, v4, v6, info) != 0) return -1;
    // a family none of whose reachable rules forwards never consults or updates its L1 entry
    // (src/worker.c:155-244 run only for forwarded packets): its entry's agreement is moot
    bool& fwd4 = im.fwd4;
    bool& fwd6 = im.fwd6;
    {
        bool e4 = false, e6 = false;
        for (size_t i = 0; i < count && !(e4 && e6); ++i) {
            const uint8_t ver = rules[i].ip_ver;
            const bool all4 = matches_all4(v4[i]), all6 = matches_all6(v4[i], v6[i]);
            const bool fwd = rules[i].action.type == UPE_ACT_FWD;
            if (!e4 && (ver == 0 || ver == 4)) { fwd4 = fwd4 || fwd; e4 = all4; }
            if (!e6 && (ver == 0 || ver == 6)) { fwd6 = fwd6 || fwd; e6 = all6; }
        }
    }
    // linear-scan tables past the LDS copy: the per-family lists (FamTable)
    uint32_t& fam4 = im.fam4;
    uint32_t& fam6 = im.fam6;
    uint32_t& fam_all = im.fam_all;
    uint32_t& fam_x1idx = im.fam_x1idx;
    std::vector<uint32_t> l4, l6;   // the family lists' sorted indexes
    std::vector<uint4>& fimg = im.fimg;
    if (pad > (size_t)kSmallRules) {
        bool end4 = false, end6 = false;
        family_lists(rules, count, v4, v6, l4, l6, end4, end6);
        const size_t n4 = (l4.size() + kUnroll - 1) / kUnroll * kUnroll;
        const size_t n6 = (l6.size() + kUnroll - 1) / kUnroll * kUnroll;
        // (+1: the scalar scan loads an IPv6 entry's last 48 bytes as 64)
        fimg.assign(2 * n4 + kFamV6Stride * n6 + (n4 + n6 + 3) / 4 + 1, make_uint4(0, 0, 0, 0));
        RuleV4 never;
        memset(&never, 0, sizeof never);
        never.x0 = 0xFF;   // ip_ver byte 0xFF against a key version of 4 or 6
        never.m0 = 0xFF;
        uint32_t* idx = reinterpret_cast<uint32_t*>(fimg.data() + 2 * n4 + kFamV6Stride * n6);
        // tables below 8192 rules: the sorted index rides in x1 bits 18-30 (m1 keeps them clear,
        // so the match is unchanged) and comes back with the matched rule's words
        const bool x1idx = count < 8192;
        for (size_t j = 0; j < n4; ++j) {
            RuleV4 e = j < l4.size() ? v4[l4[j]] : never;
            if (x1idx && j < l4.size()) e.x1 |= l4[j] << 18;
            memcpy(&fimg[2 * j], &e, sizeof e);
            idx[j] = j < l4.size() ? l4[j] : 0u;
        }
        for (size_t j = 0; j < n6; ++j) {
            uint4* o = &fimg[2 * n4 + kFamV6Stride * j];
            if (j < l6.size()) {
                RuleV4 e = v4[l6[j]];
                if (x1idx) e.x1 |= l6[j] << 18;
                memcpy(o, &e, sizeof(RuleV4));
                memcpy(o + 2, &v6[l6[j]], 3 * sizeof(uint4));   // s, sm, d, dm (12 words)
            } else {
                memcpy(o, &never, sizeof never);
            }
            idx[n4 + j] = j < l6.size() ? l6[j] : 0u;
        }
        fam4 = (uint32_t)n4;
        fam6 = (uint32_t)n6;
        fam_all = (l4.size() == 1 && end4 ? 1u : 0u) | (l6.size() == 1 && end6 ? 2u : 0u);
        fam_x1idx = x1idx ? 1u : 0u;
    }
    // Large tables: a tuple-space index when the rules fall into few mask signatures (one hash
    // probe per signature instead of a test per rule).
    bool& tss = im.tss;
    TssFamily& f4 = im.f4;
    TssFamily& f6 = im.f6;
    std::vector<uint16_t>& fps = im.fps;   // the staged fingerprint image
    const char* force = getenv("UPE_GPU_TSS");   // diagnostic: 0 = never, 1 = always
    if (count > 0 && count < kTssMaxRules && !(force && force[0] == '0') &&
        build_tss_family(4, v4, v6, rules, count, f4) && build_tss_family(6, v4, v6, rules, count, f6)) {
        const size_t ng = f4.groups.size() + f6.groups.size();
        if ((force && force[0] == '1') || (count >= 1024 && ng * 16 <= count)) {
            // the staged fingerprint image: small groups, in probe order, while it fits
            const char* st = getenv("UPE_GPU_FP_STAGE");   // diagnostic: 0 = stage none
            for (TssFamily* f : {&f4, &f6})
                for (TssGroup& g : f->groups) {
                    if (st && st[0] == '0') break;
                    const uint32_t slots = 1u << g.w[11];
                    if ((g.w[14] & 1u) || slots > kFpStageGroup || fps.size() + slots > kFpStageMax)
                        continue;
                    g.w[15] = 1u + (uint32_t)fps.size();
                    fps.insert(fps.end(), f->fp.begin() + g.w[13], f->fp.begin() + g.w[13] + slots);
                }
            fps.resize((fps.size() + 7) & ~(size_t)7, 0);
            tss = true;
        }
    }
    // Linear-scan tables past kSmallRules without a tuple-space index: the decision tree over the
    // family lists (kTreeDims comment), unless it outgrows its node budget, or a scan never gets
    // far: both families' lists reach their first catch-all within kTreeMinReach entries (the
    // scan's cost is then bounded by that, and its wave-uniform scalar loads beat the walk:
    // seed-3 config C 38.1 vs 46.5 us).  UPE_GPU_TREE: 0 = never, 1 = whenever it builds
    // (diagnostics); UPE_GPU_TREE_BINTH: rules per leaf before a split.
    bool& tree_ok = im.tree_ok;
    std::vector<uint4>& timg = im.timg;
    TreeImage& t = im.t;
    const char* tf = getenv("UPE_GPU_TREE");
    // (the reach first, from the lists alone: a table a scan never walks far into is not built a
    // tree only to throw it away — ADVICE r05; a reload then costs the lists, not the forest)
    const size_t reach0 = std::max(scan_reach(4, v4, v6, l4), scan_reach(6, v4, v6, l6));
    if (!tss && pad > (size_t)kSmallRules && !(tf && tf[0] == '0') &&
        (reach0 > kTreeMinReach || (tf && tf[0] == '1'))) {
        const char* bt = getenv("UPE_GPU_TREE_BINTH");
        const uint32_t binth = bt ? (uint32_t)std::max(1, atoi(bt)) : 0u;
        if (choose_tree(v4, v6, l4, l6, count, binth, t)) {
            const size_t nw = 2 * t.nodes.size() + t.leaves.size();
            timg.assign((nw + 3) / 4, make_uint4(0, 0, 0, 0));
            memcpy(timg.data(), t.nodes.data(), t.nodes.size() * sizeof(uint2));
            memcpy(reinterpret_cast<uint32_t*>(timg.data()) + 2 * t.nodes.size(), t.leaves.data(),
                   t.leaves.size() * sizeof(uint32_t));
            // the list entries a scan can reach: up to the family's first catch-all (node 1)
            const uint2 dflt = t.nodes[1];
            const size_t reach = std::max(dflt.x == kNone ? l4.size() : (size_t)dflt.x + 1,
                                          dflt.y == kNone ? l6.size() : (size_t)dflt.y + 1);
            tree_ok = reach > kTreeMinReach || (tf && tf[0] == '1');
        }
    }
    return 0;
}

extern "C" upe_rule_image_t* upe_rules_compile(const upe_rule_t* rules, size_t count,
                                               size_t rule_capacity) {
    if (rule_capacity == 0 || rule_capacity > (1u << 24)) {
        fail("rule_capacity must be in [1, 2^24]");
        return nullptr;
    }
    if (count > rule_capacity || (count && !rules)) {
        fail(count > rule_capacity ? "rule count exceeds the capacity" : "null rules");
        return nullptr;
    }
    try {
        auto* im = new upe_rule_image;
        if (build_image(rules, count, rule_capacity, *im) != 0) {
            delete im;
            return nullptr;
        }
        return im;
    } catch (const std::bad_alloc&) {
        fail("out of memory (rule image)");
        return nullptr;
    }
}

extern "C" void upe_rules_image_free(upe_rule_image_t* im) { delete im; }

// The neighbour snapshot the same way: upe_gpu_load_neigh's build, apart from any context.
// (upe_neigh_image is a hidden type, as the NeighImage it holds; g++ would hide a function that
// names it along with it, so the two entry points say that they are exported.)
#define UPE_EXPORT __attribute__((visibility("default")))
extern "C" UPE_EXPORT upe_neigh_image_t* upe_neigh_compile(const upe_arp_entry_t* arp, size_t arp_capacity,
                                                const upe_ndp_entry_t* ndp, size_t ndp_capacity) {
    try {
        auto* im = new upe_neigh_image;
        if (compile_neigh(arp, arp_capacity, ndp, ndp_capacity, im->im) != 0) {
            delete im;
            return nullptr;
        }
        return im;
    } catch (const std::bad_alloc&) {
        fail("out of memory (neighbour image)");
        return nullptr;
    }
}

extern "C" UPE_EXPORT void upe_neigh_image_free(upe_neigh_image_t* im) { delete im; }

namespace {
// The device lookups (arp_lookup / ndp_lookup with arp_slot_of / ndp_slot_of, upe_neigh_lookup.h)
// on the host: the slot of the image's index that answers for an address — the first of its three
// candidates that is used and holds it — or kNone.
uint32_t arp_slot_host(const NeighImage& im, uint32_t ip) {
    if (im.arp_bits == 0) return kNone;
    const uint32_t c[3] = {slot1(ip, im.arp_seed, im.arp_bits), slot2(ip, im.arp_seed, im.arp_bits),
                           slot3(ip, im.arp_seed, im.arp_bits)};
    for (uint32_t t : c)
        if (((im.arp[t].z >> 16) & 1u) && im.arp[t].x == ip) return t;
    return kNone;
}
uint32_t ndp_slot_host(const NeighImage& im, const uint32_t ip[4]) {
    if (im.ndp_bits == 0) return kNone;
    const uint32_t k = fold_v6(ip);
    const uint32_t c[3] = {slot1(k, im.ndp_seed, im.ndp_bits), slot2(k, im.ndp_seed, im.ndp_bits),
                           slot3(k, im.ndp_seed, im.ndp_bits)};
    for (uint32_t t : c) {
        const uint4 &a = im.ndp[2 * (size_t)t], &m = im.ndp[2 * (size_t)t + 1];
        if (((m.y >> 16) & 1u) && a.x == ip[0] && a.y == ip[1] && a.z == ip[2] && a.w == ip[3])
            return t;
    }
    return kNone;
}
// A slot's MAC words in upe_gpu_resolve_keys' format.
uint64_t found(uint32_t lo, uint32_t hi) {
    return (uint64_t)lo | (uint64_t)((hi & 0xFFFFu) | 1u << 16) << 32;
}
}  // namespace

// upe_gpu_resolve_keys over an image on the host (include/upe_gpu.h).
extern "C" UPE_EXPORT int upe_neigh_image_lookup_host(const upe_neigh_image_t* image,
                                                      const upe_flow_key_t* keys, size_t n,
                                                      uint64_t* mac) {
    if (!image || (n && (!keys || !mac))) return fail("null argument");
    const NeighImage& im = image->im;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* d = keys[i].dst_ip.v6;
        mac[i] = 0;
        if (keys[i].ip_ver == 4) {
            const uint32_t t = arp_slot_host(im, le32(d));
            if (t != kNone) mac[i] = found(im.arp[t].y, im.arp[t].z);
        } else if (keys[i].ip_ver == 6) {
            const uint32_t ip[4] = {le32(d), le32(d + 4), le32(d + 8), le32(d + 12)};
            const uint32_t t = ndp_slot_host(im, ip);
            if (t != kNone) mac[i] = found(im.ndp[2 * (size_t)t + 1].x, im.ndp[2 * (size_t)t + 1].y);
        }
    }
    return 0;
}

// upe_gpu_neigh_patch's twin (include/upe_gpu.h; the kernels: upe_neigh_patch.hip).  "Held" is
// held before the call: a record rewrites MAC bytes only, which no lookup's hit depends on, so the
// records go in rank order, one after another, and the last one aimed at a slot stays.
extern "C" UPE_EXPORT int upe_neigh_patch_host(upe_neigh_image_t* image,
                                               const upe_ctrl_write_t* writes, size_t count,
                                               uint32_t* miss, upe_neigh_patch_info_t* info) {
    if (!image || !info || (count && !writes)) return fail("null argument");
    if (count > 0xFFFFFFFFull - UPE_PATCH_BLOCK) return fail("count must fit in 32 bits");
    NeighImage& im = image->im;
    uint64_t missed = 0, first = ~0ull;
    for (size_t i = 0; i < count; ++i) {
        const upe_ctrl_write_t& w = writes[i];
        const uint32_t lo = mac_lo(w.mac), hi = mac_hi(w.mac);
        uint32_t t = kNone;
        if (w.kind == UPE_CW_ARP) {
            t = arp_slot_host(im, le32(w.ip));
            if (t != kNone) {
                im.arp[t].y = lo;
                im.arp[t].z = (im.arp[t].z & 0xFFFF0000u) | hi;
            }
        } else if (w.kind == UPE_CW_NDP) {
            const uint32_t ip[4] = {le32(w.ip), le32(w.ip + 4), le32(w.ip + 8), le32(w.ip + 12)};
            t = ndp_slot_host(im, ip);
            if (t != kNone) {
                uint4& m = im.ndp[2 * (size_t)t + 1];
                m.x = lo;
                m.y = (m.y & 0xFFFF0000u) | hi;
            }
        }
        if (t == kNone) {
            if (missed == 0) first = i;
            if (miss) miss[missed] = (uint32_t)i;
            ++missed;
        }
    }
    info->records = count;
    info->patched = count - missed;
    info->missed = missed;
    info->first_miss = first;
    return 0;
}

// upe_neigh_compile with room for new addresses in each index (include/upe_gpu.h).
extern "C" UPE_EXPORT upe_neigh_image_t* upe_neigh_compile_room(
    const upe_arp_entry_t* arp, size_t arp_capacity, const upe_ndp_entry_t* ndp,
    size_t ndp_capacity, size_t arp_room, size_t ndp_room) {
    try {
        auto* im = new upe_neigh_image;
        if (compile_neigh(arp, arp_capacity, ndp, ndp_capacity, im->im, arp_room, ndp_room) != 0) {
            delete im;
            return nullptr;
        }
        return im;
    } catch (const std::bad_alloc&) {
        fail("out of memory (neighbour image)");
        return nullptr;
    }
}

// What an image holds (include/upe_gpu.h).
extern "C" UPE_EXPORT int upe_neigh_image_read(const upe_neigh_image_t* image,
                                               upe_neigh_image_info_t* info, void* arp,
                                               size_t arp_bytes, void* ndp, size_t ndp_bytes) {
    if (!image) return fail("null argument");
    const NeighImage& im = image->im;
    if ((arp && arp_bytes != im.arp.size() * sizeof(uint4)) ||
        (ndp && ndp_bytes != im.ndp.size() * sizeof(uint4)))
        return fail("slot array size does not match the image");
    if (info)
        *info = upe_neigh_image_info_t{im.arp_bits, im.arp_seed, im.ndp_bits, im.ndp_seed,
                                       im.arp_free, im.ndp_free, im.arp_insertable ? 1u : 0u,
                                       im.ndp_insertable ? 1u : 0u};
    if (arp) memcpy(arp, im.arp.data(), arp_bytes);
    if (ndp) memcpy(ndp, im.ndp.data(), ndp_bytes);
    return 0;
}

// upe_gpu_neigh_learn's twin (include/upe_gpu.h; the kernel: upe_neigh_learn.hip): the contract's
// loop as it stands there, one record after another on the image's index and free counts.
// arp_update (reference src/arp_table.c:26-53) / ndp_update (src/ndp_table.c:39-65) of a held
// address rewrite the MAC; of a new one they take a free slot when the table has one.
extern "C" UPE_EXPORT int upe_neigh_learn_host(upe_neigh_image_t* image,
                                               const upe_ctrl_write_t* writes, size_t count,
                                               uint32_t* defer, upe_neigh_learn_info_t* info) {
    if (!image || !info || (count && !writes)) return fail("null argument");
    if (count > 0xFFFFFFFFull - UPE_LEARN_CHUNK) return fail("count must fit in 32 bits");
    NeighImage& im = image->im;
    uint64_t patched = 0, inserted = 0, dropped = 0, deferred = 0, first = ~0ull;
    auto put_off = [&](size_t i) {
        if (deferred == 0) first = i;
        if (defer) defer[deferred] = (uint32_t)i;
        ++deferred;
    };
    for (size_t i = 0; i < count; ++i) {
        const upe_ctrl_write_t& w = writes[i];
        const uint32_t lo = mac_lo(w.mac), hi = mac_hi(w.mac);
        if (w.kind == UPE_CW_ARP) {
            const uint32_t ip = le32(w.ip);
            const uint32_t t = arp_slot_host(im, ip);
            if (t != kNone) {
                im.arp[t].y = lo;
                im.arp[t].z = (im.arp[t].z & 0xFFFF0000u) | hi;
                ++patched;
            } else if (!im.arp_insertable) {
                put_off(i);
            } else if (im.arp_free == 0) {
                ++dropped;
            } else {
                const uint32_t c[3] = {slot1(ip, im.arp_seed, im.arp_bits),
                                       slot2(ip, im.arp_seed, im.arp_bits),
                                       slot3(ip, im.arp_seed, im.arp_bits)};
                int q = 0;
                while (q < 3 && ((im.arp[c[q]].z >> 16) & 1u)) ++q;
                if (q == 3) {
                    put_off(i);
                } else {
                    im.arp[c[q]] = make_uint4(ip, lo, hi | (1u << 16), 0);
                    --im.arp_free;
                    ++inserted;
                }
            }
        } else if (w.kind == UPE_CW_NDP) {
            const uint32_t ip[4] = {le32(w.ip), le32(w.ip + 4), le32(w.ip + 8), le32(w.ip + 12)};
            const uint32_t t = ndp_slot_host(im, ip);
            if (t != kNone) {
                uint4& m = im.ndp[2 * (size_t)t + 1];
                m.x = lo;
                m.y = (m.y & 0xFFFF0000u) | hi;
                ++patched;
            } else if (!im.ndp_insertable) {
                put_off(i);
            } else if (im.ndp_free == 0) {
                ++dropped;
            } else {
                const uint32_t k = fold_v6(ip);
                const uint32_t c[3] = {slot1(k, im.ndp_seed, im.ndp_bits),
                                       slot2(k, im.ndp_seed, im.ndp_bits),
                                       slot3(k, im.ndp_seed, im.ndp_bits)};
                int q = 0;
                while (q < 3 && ((im.ndp[2 * (size_t)c[q] + 1].y >> 16) & 1u)) ++q;
                if (q == 3) {
                    put_off(i);
                } else {
                    im.ndp[2 * (size_t)c[q]] = make_uint4(ip[0], ip[1], ip[2], ip[3]);
                    im.ndp[2 * (size_t)c[q] + 1] = make_uint4(lo, hi | (1u << 16), 0, 0);
                    --im.ndp_free;
                    ++inserted;
                }
            }
        } else {
            put_off(i);
        }
    }
    *info = upe_neigh_learn_info_t{count, patched, inserted, dropped, deferred, first,
                                   im.arp_free, im.ndp_free};
    return 0;
}

// (diagnostic, not part of the ABI) the same, and per key and tree of its family (first 16):
// levels walked (prof_depth[16 * i + t]) and leaf entries read (prof_steps[16 * i + t])
extern "C" int upe_tree_profile_host(const upe_rule_t* rules, size_t count,
                                     const upe_flow_key_t* keys, size_t n, int64_t* out,
                                     upe_rule_index_info_t* info, uint8_t* prof_depth,
                                     uint8_t* prof_steps) {
    if ((count && !rules) || (n && (!keys || !out))) return fail("null argument");
    const size_t pad = ((count + kUnroll - 1) / kUnroll + 1) * kUnroll;
    std::vector<RuleV4> v4;
    std::vector<RuleV6> v6;
    std::vector<int2> rinfo;
    if (compile_rules(rules, count, 0xFFFFFFFFu, pad, v4, v6, rinfo) != 0) return -1;
    std::vector<uint32_t> l4, l6;
    bool end4 = false, end6 = false;
    family_lists(rules, count, v4, v6, l4, l6, end4, end6);
    const char* bt = getenv("UPE_GPU_TREE_BINTH");
    const uint32_t binth = bt ? (uint32_t)std::max(1, atoi(bt)) : 0u;
    TreeImage t;
    const bool tree = choose_tree(v4, v6, l4, l6, count, binth, t);
    if (info)
        *info = tree ? upe_rule_index_info_t{(uint64_t)t.nodes.size(), (uint64_t)t.leaves.size(),
                                             t.depth[0], t.depth[1], t.max_leaf,
                                             t.trees[0] | t.trees[1] << 16}
                     : upe_rule_index_info_t{};
    for (size_t i = 0; i < n; ++i) {
        const upe_flow_key_t& k = keys[i];
        if (k.ip_ver != 4 && k.ip_ver != 6) {
            out[i] = -1;
            continue;
        }
        const bool is6 = k.ip_ver == 6;
        const uint32_t k0 = (uint32_t)k.ip_ver | ((uint32_t)k.protocol << 8) |
                            ((uint32_t)k.src_port << 16);
        const uint32_t k1 = k.dst_port;
        uint32_t sw[4], dw[4], kv[kTreeDims] = {};
        for (int j = 0; j < 4; ++j) {
            sw[j] = le32(k.src_ip.v6 + 4 * j);
            dw[j] = le32(k.dst_ip.v6 + 4 * j);
        }
        if (is6) {
            for (int j = 0; j < 4; ++j) {
                kv[j] = word_of(sw[j], t.swap6, j);
                kv[4 + j] = word_of(dw[j], t.swap6, 4 + j);
            }
        } else {
            kv[0] = sw[0];
            kv[4] = dw[0];
        }
        kv[8] = k.src_port;
        kv[9] = k.dst_port;
        kv[10] = k.protocol;
        const std::vector<uint32_t>& list = is6 ? l6 : l4;
        uint32_t pos = kNone;
        if (tree) {
            pos = tree_walk_host(t, v4, v6, list, is6, kv, k0, k1, sw, dw,
                                 prof_depth ? prof_depth + 16 * i : nullptr,
                                 prof_steps ? prof_steps + 16 * i : nullptr);
        } else {
            for (size_t j = 0; j < list.size() && pos == kNone; ++j) {
                const RuleV4& r = v4[list[j]];
                uint32_t x = ((k0 ^ r.x0) & r.m0) | ((k1 ^ r.x1) & r.m1 & 0xFFFFu) |
                             ((sw[0] ^ r.s0) & r.sm0) | ((dw[0] ^ r.d0) & r.dm0);
                if (is6)
                    for (int w = 0; w < 3; ++w)
                        x |= ((sw[w + 1] ^ v6[list[j]].s[w]) & v6[list[j]].sm[w]) |
                             ((dw[w + 1] ^ v6[list[j]].d[w]) & v6[list[j]].dm[w]);
                if (x == 0) pos = (uint32_t)j;
            }
        }
        out[i] = pos == kNone ? -1 : (int64_t)list[pos];
    }
    return 0;
}

// rule_table_match (reference src/rule_table.c:163-176) for a batch of keys on the host, through
// the decision tree the GPU path builds for the same table (tree_walk_host: the device's walk bit
// for bit), or the family lists' linear first match when the table gets no tree.
extern "C" int upe_rules_match_host(const upe_rule_t* rules, size_t count,
                                    const upe_flow_key_t* keys, size_t n, int64_t* out,
                                    upe_rule_index_info_t* info) {
    return upe_tree_profile_host(rules, count, keys, n, out, info, nullptr, nullptr);
}
