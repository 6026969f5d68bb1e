// upe_match.h — rule_table_match on the device (reference src/rule_table.c:163-176 over match_rule
// :76-91): the four matchers over a key's words and the few helpers they need, for the units whose
// kernels match keys: upe_gpu.hip (upe_classify, per parsed packet) and upe_keys.hip
// (upe_match_keys, per flow key).  Device code only; internal linkage (an unnamed namespace, as
// upe_plan.h), so each unit compiles its own copies into its own kernels.
//
// A key is the words upe_classify has always handed its matchers:
//   k0 = ip_ver | protocol << 8 | src_port << 16      (RuleV4 x0 / m0, upe_dev.h)
//   k1 = dst_port                                     (RuleV4 x1 / m1)
//   s[4], d[4]: the address unions as little-endian words: IPv4 host order in word 0 (as
//   parse_flow_key stores it, src/parser.c:40-41), IPv6 the wire bytes.  No matcher reads words
//   1-3 of an IPv4 key.
// key_k0 / key_k1 are that packing's one definition.
//
// The matchers read the table through `a`, any struct with the fields of upe_gpu.hip's Args that
// they name (each unit passes its own kernel-argument struct; the bodies are one text):
//   scan_rules      rv4, rv6
//   scan_fam        fam, fam4, fam6, fam6_lds
//   tree_match      tree, tree_loff, fam, fam4, fam6, fam4_lds, fam6_lds
//   tss_match_both  tg4, tg6, tt4, tt6, ng4, ng6
// fam_sorted_index (a FamTable match's sorted index) also fam_x1idx.
#ifndef UPE_MATCH_H
#define UPE_MATCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "upe_dev.h"

namespace {

using namespace upe;

// The key words of (family, protocol, source port) and of the destination port.
__device__ __forceinline__ uint32_t key_k0(bool v6, uint32_t proto, uint32_t sport) {
    return (v6 ? 6u : 4u) | (proto << 8) | (sport << 16);
}
__device__ __forceinline__ uint32_t key_k1(uint32_t dport) { return dport; }

// v_bfi_b32 with a per-lane all-ones / all-zeros mask in a VGPR: a where m is set, else b (a
// select the compiler cannot turn into an indexed load of the array a and b come from, and one
// that needs no SGPR lane mask)
__device__ __forceinline__ uint32_t vsel(uint32_t m, uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b));
    return r;
}

// Rule words are read through the constant address space: the compiler may then use scalar
// (s_load) loads, which it will not do through a generic pointer it cannot prove unwritten.
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));

template <typename V, typename T>
__device__ __forceinline__ const __attribute__((address_space(4))) V* as_const(const T* p) {
    return (const __attribute__((address_space(4))) V*)p;
}

// First-match scan (reference src/rule_table.c:163-176 over match_rule :76-91).  Every lane of
// the wave walks the same rules in sorted order; rule words are wave-uniform loads.  `done`
// lanes (already matched, or not scanning) are ignored.  V6 = some lane holds an IPv6 key; rules
// without IPv6 address words skip the rv6 test (a scalar branch).
// Small tables are read from an LDS copy (staged at kernel entry, broadcast reads of a
// wave-uniform address: no scalar-cache round trip in the dependent chain); larger ones through
// the scalar unit from the constant address space.  (Staging the first 64 rules of larger
// tables in LDS too measured slower, profiles/r03/v8_rule_prefix_ab.txt: C's rule words already
// hit in the scalar cache.)
template <bool V6, bool kLdsRules, class Tab>
__device__ __forceinline__ uint32_t scan_rules(const Tab& a, bool done, bool is6, uint32_t k0,
                                               uint32_t k1, const uint32_t s[4],
                                               const uint32_t d[4], uint32_t& act,
                                               const u32x8* l4, const u32x16* l6,
                                               uint32_t b0, uint32_t b1) {
    uint32_t hit = kNone;
    static_assert(sizeof(RuleV4) == 32 && sizeof(RuleV6) == 64, "rule stream strides");
    const auto* rv4 = as_const<u32x8>(a.rv4);
    const auto* rv6 = as_const<u32x16>(a.rv6);
    for (uint32_t b = b0; b < b1; b += kUnroll) {
        // the rule index is wave-uniform: say so, so rule words come through the scalar unit
        const uint32_t base = __builtin_amdgcn_readfirstlane(b);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            // RuleV4 words: x0 m0 x1 m1 s0 sm0 d0 dm0
            const u32x8 r = kLdsRules ? l4[base + u] : rv4[base + u];
            uint32_t x = ((k0 ^ r[0]) & r[1]) | ((k1 ^ r[2]) & r[3]) | ((s[0] ^ r[4]) & r[5]) |
                         ((d[0] ^ r[6]) & r[7]);
            if (V6 && (__builtin_amdgcn_readfirstlane(r[3]) & kRuleV6Words)) {
                // RuleV6 words: s[3] sm[3] d[3] dm[3]
                const u32x16 q = kLdsRules ? l6[base + u] : rv6[base + u];
                const uint32_t y = ((s[1] ^ q[0]) & q[3]) | ((s[2] ^ q[1]) & q[4]) |
                                   ((s[3] ^ q[2]) & q[5]) | ((d[1] ^ q[6]) & q[9]) |
                                   ((d[2] ^ q[7]) & q[10]) | ((d[3] ^ q[8]) & q[11]);
                if (is6) x |= y;
            }
            if (!done && x == 0) {
                hit = base + u;
                act = r[2];   // the action code rides in x1 bits 16-17 (see RuleV4)
                done = true;
            }
        }
        if (__all(done)) break;
    }
    return hit;
}

// First match over the per-family lists (FamTable): the same rule tests as scan_rules, each lane
// against its own family's list; `pos` is the lane's position in its list, turned into the
// sorted index after the loop (reference src/rule_table.c:163-176: the first match in (priority,
// rule_id) order — a rule of the other family cannot match, so it is skipped, not reordered).
template <bool V6, class Tab>
__device__ __forceinline__ uint32_t scan_fam(const Tab& a, bool done, bool is6, uint32_t k0,
                                             uint32_t k1, const uint32_t s[4], const uint32_t d[4],
                                             uint32_t& act, const uint4* l6) {
    // the IPv4 lanes' list, then the IPv6 lanes' list (one loop after the other: interleaving
    // both in one loop held twice the rule words in SGPRs and spilled)
    const auto* f4 = as_const<u32x8>(a.fam);
    const uint4* f6 = a.fam + 2 * (size_t)a.fam4;
    uint32_t pos = kNone;
    bool dn = done || is6;
    for (uint32_t b = 0; b < a.fam4; b += kUnroll) {
        if (!__any(!dn)) break;
        const uint32_t base = __builtin_amdgcn_readfirstlane(b);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const u32x8 r = f4[base + u];
            const uint32_t x = ((k0 ^ r[0]) & r[1]) | ((k1 ^ r[2]) & r[3]) |
                               ((s[0] ^ r[4]) & r[5]) | ((d[0] ^ r[6]) & r[7]);
            if (!dn && x == 0) {
                pos = base + u;
                act = r[2];
                dn = true;
            }
        }
    }
    if (V6 && a.fam6_lds) {
        dn = done || !is6;
        for (uint32_t b = 0; b < a.fam6; b += kUnroll) {
            if (!__any(!dn)) break;
            const uint32_t base = __builtin_amdgcn_readfirstlane(b);
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const uint4* e = l6 + kFamV6Stride * (base + u);
                const uint4 e0 = e[0], e1 = e[1];
                uint32_t x = ((k0 ^ e0.x) & e0.y) | ((k1 ^ e0.z) & e0.w) |
                             ((s[0] ^ e1.x) & e1.y) | ((d[0] ^ e1.z) & e1.w);
                // (the IPv6 words only when some lane still looking passes the rest of the rule:
                // C6 136.6 -> 126.9 us; in the whole-table scan the same test cost C 0.5 us)
                if ((__builtin_amdgcn_readfirstlane(e0.w) & kRuleV6Words) && __any(!dn && x == 0)) {
                    const uint4 e2 = e[2], e3 = e[3], e4 = e[4];
                    // s1 s2 s3 sm1 | sm2 sm3 d1 d2 | d3 dm1 dm2 dm3
                    x |= ((s[1] ^ e2.x) & e2.w) | ((s[2] ^ e2.y) & e3.x) | ((s[3] ^ e2.z) & e3.y) |
                         ((d[1] ^ e3.z) & e4.y) | ((d[2] ^ e3.w) & e4.z) | ((d[3] ^ e4.x) & e4.w);
                }
                if (!dn && x == 0) {
                    pos = base + u;
                    act = e0.z;
                    dn = true;
                }
            }
        }
    } else if (V6) {
        // (two entries per step: four held 96 rule words in SGPRs and spilled)
        dn = done || !is6;
        for (uint32_t b = 0; b < a.fam6; b += 2) {
            if (!__any(!dn)) break;
            const uint32_t base = __builtin_amdgcn_readfirstlane(b);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const uint4* e = f6 + (size_t)kFamV6Stride * (base + u);
                const u32x8 r = *as_const<u32x8>(e);
                uint32_t x = ((k0 ^ r[0]) & r[1]) | ((k1 ^ r[2]) & r[3]) |
                             ((s[0] ^ r[4]) & r[5]) | ((d[0] ^ r[6]) & r[7]);
                if ((__builtin_amdgcn_readfirstlane(r[3]) & kRuleV6Words) && __any(!dn && x == 0)) {
                    const u32x16 q = *as_const<u32x16>(e + 2);
                    x |= ((s[1] ^ q[0]) & q[3]) | ((s[2] ^ q[1]) & q[4]) | ((s[3] ^ q[2]) & q[5]) |
                         ((d[1] ^ q[6]) & q[9]) | ((d[2] ^ q[7]) & q[10]) | ((d[3] ^ q[8]) & q[11]);
                }
                if (!dn && x == 0) {
                    pos = base + u;
                    act = r[2];
                    dn = true;
                }
            }
        }
    }
    // the lane's entry in the lists' index array (fam4 + position for the IPv6 list); the caller
    // loads the sorted index from it late, so the round trip overlaps the rest of the chunk
    return pos == kNone ? kNone : (is6 ? a.fam4 : 0u) + pos;
}

// The sorted index of a FamTable match (scan_fam's or tree_match's result `ri`, not kNone, with
// the matched entry's x1 word `act`): in the entry's x1 bits 18-30 for tables below 8192 rules
// (fam_x1idx), else loaded from the lists' index array behind the two lists.
template <class Tab>
__device__ __forceinline__ uint32_t fam_sorted_index(const Tab& a, uint32_t ri, uint32_t act) {
    return a.fam_x1idx ? (act >> 18) & 0x1FFFu
                       : reinterpret_cast<const uint32_t*>(a.fam + 2 * (size_t)a.fam4 +
                                                           (size_t)kFamV6Stride * a.fam6)[ri];
}

// First match through the decision-tree index (kTreeDims comment): for each of its family's five
// field trees a lane walks to a leaf, then tests the leaf's rules in list order against their
// FamTable entries (the flagged one without a test), stopping at its first match or at a
// position no better than the best so far.  A field's tree splits on that field's words only (an
// address tree also on the ports and the protocol), so each level compares one of a few key words
// prepared before the walk (an address tree: one of its field's four words or a port word, by
// the node's dimension bits).  Walks are per lane (divergent loads: LDS when
// the image is staged, else memory), two levels per 16-byte node load, the deep trees together
// (source and destination address, destination port), then the shallow ones (source port,
// protocol), node loads in flight together; the wave iterates as long as its deepest walk and
// its longest leaf, tree by tree.  Returns the
// lane's FamTable index-array entry, as scan_fam.
template <bool kLdsTree, class Tab>
__device__ __forceinline__ uint32_t tree_match(const Tab& a, bool active, bool is6, uint32_t k0,
                                               uint32_t k1, const uint32_t s[4], const uint32_t d[4],
                                               uint32_t& act, const uint2* lnodes, const uint4* l6,
                                               const uint4* l4) {
    const uint2* N = kLdsTree ? lnodes : a.tree;
    const uint32_t* E = reinterpret_cast<const uint32_t*>(N) + a.tree_loff;
    const uint2 dir = N[0];
    const uint32_t nt = active ? (is6 ? dir.y & 0xFFFFu : dir.x) : 0u, first = 1u + (is6 ? dir.x : 0u);
    const uint32_t sp = k0 >> 16, dp = k1, pr = (k0 >> 8) & 0xFFu;
    const uint4* g6 = a.fam + 2 * (size_t)a.fam4;
    uint32_t best = kNone, bact = 0;
    const bool fam_lds = (a.fam4_lds || a.fam4 == 0u) && (a.fam6_lds || a.fam6 == 0u);
    // The leaf of one tree: its rules in list order until a match or a position >= best.
    auto leaf_tests = [&](const uint32_t lw) {
        const uint32_t cnt = lw >> 21, off = lw & 0x1FFFFFu;
        bool look = cnt != 0u;
        for (uint32_t j = 0; __any(look); ++j) {
            if (look) {
                const uint32_t e = E[off + j];
                const uint32_t p = e & 0x7FFFFFFFu;
                if (p >= best) {
                    look = false;   // the lists ascend: nothing later in this leaf can win
                } else {
                    const bool cov = (e >> 31) != 0u;
                    if (fam_lds) {
                        // both lists in LDS (the usual case): one address, the first two words
                        // read for every lane, an IPv6 entry's other words in a masked block
                        // that updates x in place (no zeroed registers to merge)
                        const uint4* f = is6 ? l6 + kFamV6Stride * p : l4 + 2 * p;
                        const uint4 e0 = f[0], e1 = f[1];
                        uint32_t x6 = 0;
                        if (is6) {   // (issued with the first two reads: no second round trip)
                            const uint4 e2 = f[2], e3 = f[3], e4 = f[4];
                            x6 = ((s[1] ^ e2.x) & e2.w) | ((s[2] ^ e2.y) & e3.x) |
                                 ((s[3] ^ e2.z) & e3.y) | ((d[1] ^ e3.z) & e4.y) |
                                 ((d[2] ^ e3.w) & e4.z) | ((d[3] ^ e4.x) & e4.w);
                        }
                        const uint32_t x = ((k0 ^ e0.x) & e0.y) | ((k1 ^ e0.z) & e0.w) |
                                           ((s[0] ^ e1.x) & e1.y) | ((d[0] ^ e1.z) & e1.w) | x6;
                        if (cov || x == 0u) {
                            best = p;
                            bact = e0.z;
                            look = false;
                        } else if (j + 1u >= cnt) {
                            look = false;
                        }
                        continue;
                    }
                    uint4 e0, e1 = make_uint4(0, 0, 0, 0), e2 = e1, e3 = e1, e4 = e1;
                    if (is6 && a.fam6_lds) {
                        const uint4* f = l6 + kFamV6Stride * p;
                        e0 = f[0];
                        if (!cov) { e1 = f[1]; e2 = f[2]; e3 = f[3]; e4 = f[4]; }
                    } else if (is6) {
                        const uint4* f = g6 + (size_t)kFamV6Stride * p;
                        e0 = f[0];
                        if (!cov) { e1 = f[1]; e2 = f[2]; e3 = f[3]; e4 = f[4]; }
                    } else if (a.fam4_lds) {
                        const uint4* f = l4 + 2 * p;
                        e0 = f[0];
                        if (!cov) e1 = f[1];
                    } else {
                        const uint4* f = a.fam + 2 * (size_t)p;
                        e0 = f[0];
                        if (!cov) e1 = f[1];
                    }
                    uint32_t x = ((k0 ^ e0.x) & e0.y) | ((k1 ^ e0.z) & e0.w) |
                                 ((s[0] ^ e1.x) & e1.y) | ((d[0] ^ e1.z) & e1.w);
                    // s1 s2 s3 sm1 | sm2 sm3 d1 d2 | d3 dm1 dm2 dm3 (zero words for IPv4 entries)
                    x |= ((s[1] ^ e2.x) & e2.w) | ((s[2] ^ e2.y) & e3.x) | ((s[3] ^ e2.z) & e3.y) |
                         ((d[1] ^ e3.z) & e4.y) | ((d[2] ^ e3.w) & e4.z) | ((d[3] ^ e4.x) & e4.w);
                    if (cov || x == 0u) {
                        best = p;
                        bact = e0.z;
                        look = false;
                    } else if (j + 1u >= cnt) {
                        look = false;
                    }
                }
            }
        }
    };
    // an address tree's key word for a dimension: one of its field's words (big-endian for IPv6
    // where the image says so, so that a prefix is a range; IPv4's host-order word 0 and zeros),
    // or a port or the protocol (dimensions 8-10); bit selects keep them in registers
    auto addr_word = [&](const uint32_t dm, const uint32_t (&w)[4]) -> uint32_t {
        const uint32_t m1 = 0u - (dm & 1u), m2 = 0u - ((dm >> 1) & 1u);
        const uint32_t m8 = 0u - ((dm >> 3) & 1u);
        const uint32_t aw = vsel(m2, vsel(m1, w[3], w[2]), vsel(m1, w[1], w[0]));
        return vsel(m8, vsel(m2, pr, vsel(m1, dp, sp)), aw);
    };
    // one walk step (two levels, Args::tree comment): the next node, or the leaf (live = false)
    auto step = [](const uint4 q, uint32_t& idx, uint32_t& leaf, bool& live, auto key) {
        const bool c1 = key(q.x & 15u) >= q.y;
        const uint32_t lleaf = (q.x >> 13) & 1u;
        const bool cl = c1 ? ((q.x >> 14) & 1u) != 0u : lleaf != 0u;
        const uint32_t ct = c1 ? q.w : q.z;
        const uint32_t c2 = key(c1 ? (q.x >> 8) & 15u : (q.x >> 4) & 15u) >= ct ? 1u : 0u;
        if (live) {
            if (q.x & 0x1000u) {
                leaf = q.y;
                live = false;
            } else if (cl) {
                leaf = ct;
                live = false;
            } else {
                idx = (q.x >> 15) + ((c1 && !lleaf) ? 2u : 0u) + c2;
            }
        }
    };
    const uint4* S = reinterpret_cast<const uint4*>(N);
    {
        // the deep trees together (source and destination address, destination port), then the
        // shallow ones (source port, protocol: few distinct values); node loads in flight together
        const uint32_t sw6 = is6 ? dir.y >> 16 : 0u;
        uint32_t ws[4], wd[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ws[q] = (sw6 >> q & 1u) ? bswap32(s[q]) : (is6 || q == 0) ? s[q] : 0u;
            wd[q] = (sw6 >> (4 + q) & 1u) ? bswap32(d[q]) : (is6 || q == 0) ? d[q] : 0u;
        }
        uint32_t ia = first, ib = first + 1u, ic = first + 3u, la = 0, lb = 0, lc = 0;
        bool va = nt != 0u, vb = va, vc = va;
        while (__any(va || vb || vc)) {
            const uint4 qa = S[ia], qb = S[ib], qc = S[ic];
            step(qa, ia, la, va, [&](uint32_t dm) { return addr_word(dm, ws); });
            step(qb, ib, lb, vb, [&](uint32_t dm) { return addr_word(dm, wd); });
            step(qc, ic, lc, vc, [&](uint32_t) { return dp; });
        }
        leaf_tests(la);
        leaf_tests(lb);
        leaf_tests(lc);
    }
    {
        uint32_t ia = first + 2u, ib = first + 4u, la = 0, lb = 0;
        bool va = nt != 0u, vb = va;
        while (__any(va || vb)) {
            const uint4 qa = S[ia], qb = S[ib];
            step(qa, ia, la, va, [&](uint32_t) { return sp; });
            step(qb, ib, lb, vb, [&](uint32_t) { return pr; });
        }
        leaf_tests(la);
        leaf_tests(lb);
    }
    if (__any(active && best == kNone)) {
        // no tree's rule: the family's rule that matches every key, if it has one
        const uint2 dflt = N[1];
        const uint32_t dv = is6 ? dflt.y : dflt.x;
        if (active && best == kNone && dv != kNone) {
            best = dv;
            bact = (is6 ? g6[(size_t)kFamV6Stride * dv] : a.fam[2 * (size_t)dv]).z;
        }
    }
    act = bact;
    return best == kNone ? kNone : (is6 ? a.fam4 : 0u) + best;
}

// First match through the tuple-space index.  Groups are visited in order of their smallest
// sorted index, so once a lane's best index is below the next group's smallest, nothing later
// can precede it: the result is exactly the first match of the linear scan (reference
// src/rule_table.c:163-176).  Both families share one probe loop: each lane takes its own
// family's group descriptor, fingerprint array and slot table, so a wave that mixes IPv4 and
// IPv6 packets waits for one fingerprint and one slot round trip per group index, not one per
// family (one loop per family measured 1024 vs 940 us per config-D batch).  At most one
// slot per lane and group is read — the first whose fingerprint matches; a lane whose two
// fingerprints both match and whose first slot holds another key reads the second one in a
// (rare) extra step.
__device__ __forceinline__ uint32_t tss_fmix(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
template <class Tab>
__device__ __forceinline__ uint32_t tss_match_both(const Tab& a, bool active, bool is6,
                                                   uint32_t k0, uint32_t k1, const uint32_t s[4],
                                                   const uint32_t d[4], uint32_t& act,
                                                   const uint16_t* sfp) {
    uint32_t best = kNone;
    const uint32_t ng = a.ng4 > a.ng6 ? a.ng4 : a.ng6;
    const uint32_t ngf = is6 ? a.ng6 : a.ng4;
    const auto* G4 = as_const<u32x16>(a.tg4);
    const auto* G6 = as_const<u32x16>(a.tg6);
    const uint4* T = is6 ? a.tt6 : a.tt4;
    const uint32_t st = is6 ? (uint32_t)kTssSlot6 : (uint32_t)kTssSlot4;   // slot stride in uint4
    for (uint32_t g = 0; g < ng; ++g) {
        const uint32_t gu = __builtin_amdgcn_readfirstlane(g);
        u32x16 q4 = {}, q6 = {};
        if (gu < a.ng4) q4 = G4[gu];
        if (gu < a.ng6) q6 = G6[gu];
        // groups ascend by smallest sorted index within each family: once no lane wants group
        // g, no lane wants a later one
        const bool want = active && g < ngf && best > (is6 ? q6[10] : q4[10]);
        if (!__any(want)) break;
        const uint32_t cw = is6 ? q6[14] : q4[14];
        if (want && (cw & 1u)) {
            // catch-all group: the key matches (every mask is zero), its index is the group's
            if ((is6 ? q6[10] : q4[10]) < best) {
                best = is6 ? q6[10] : q4[10];
                act = (cw >> 8) << 16;
            }
        } else if (want) {
            uint32_t q[14];
#pragma unroll
            for (int j = 0; j < 14; ++j) q[j] = is6 ? q6[j] : q4[j];
            uint32_t kw[10];
            kw[0] = k0 & q[0];
            kw[1] = k1 & q[1];
            kw[2] = s[0] & q[2];
            kw[3] = is6 ? (s[1] & q[4]) : (d[0] & q[3]);
            kw[4] = s[2] & q[5]; kw[5] = s[3] & q[6]; kw[6] = d[0] & q[3];
            kw[7] = d[1] & q[7]; kw[8] = d[2] & q[8]; kw[9] = d[3] & q[9];
            // tss_hash over 4 words (IPv4) or 10 (IPv6), bit for bit
            uint32_t h = q[12] ^ 0x9E3779B9u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h = (h ^ kw[j]) * 0x01000193u;
                h ^= h >> 15;
            }
            uint32_t h6 = h;
#pragma unroll
            for (int j = 4; j < 10; ++j) {
                h6 = (h6 ^ kw[j]) * 0x01000193u;
                h6 ^= h6 >> 15;
            }
            h = tss_fmix(is6 ? h6 : h);
            const uint32_t t1 = q[13] + slot1(h, q[12], q[11]);
            const uint32_t t2 = q[13] + slot2(h, q[12], q[11]);
            const uint32_t tag = tss_tag(h);
            // fingerprints from LDS when the group's are staged; otherwise none: slot t1, then t2
            const uint32_t so = sfp ? (is6 ? q6[15] : q4[15]) : 0u;
            uint32_t f1 = tag, f2 = tag;
            if (so) {
                const uint32_t b = so - 1u - q[13];
                f1 = sfp[b + t1];
                f2 = sfp[b + t2];
            }
            const bool m1 = f1 == tag, m2 = f2 == tag;
            uint32_t idx = kNone, ac = 0;
            auto probe = [&](uint32_t t) {
                const uint4 A = T[st * t];
                uint4 B = make_uint4(0, 0, 0, 0), C = B;
                if (is6) {
                    B = T[st * t + 1];
                    C = T[st * t + 2];
                }
                const bool k4 = A.x == kw[0] && A.y == kw[1] && A.z == kw[2] && A.w == kw[3];
                // the compact IPv4 slot: v = (index + 1) | action << 22 in the key's free bits
                const uint32_t v = (A.x & 0xFFu) | ((A.y >> 16) << 8);
                const bool k4c = (A.x & ~0xFFu) == kw[0] && (A.y & 0xFFFFu) == kw[1] &&
                                 A.z == kw[2] && A.w == kw[3];
                const bool hit = is6 ? ((C.w & 1u) && k4 && B.x == kw[4] && B.y == kw[5] &&
                                        B.z == kw[6] && B.w == kw[7] && C.x == kw[8] &&
                                        C.y == kw[9])
                                     : (v != 0u && k4c);
                if (hit) {
                    idx = is6 ? C.z : (v & (kTssMaxRules - 1u)) - 1u;
                    ac = is6 ? (C.w >> 8) : v >> 22;
                }
                return hit;
            };
            if (m1 || m2) {
                const bool hit = probe(m1 ? t1 : t2);
                if (!hit && m1 && m2) probe(t2);
            }
            if (idx < best) {
                best = idx;
                act = ac << 16;
            }
        }
    }
    return best;
}

}  // namespace

#endif  // UPE_MATCH_H
