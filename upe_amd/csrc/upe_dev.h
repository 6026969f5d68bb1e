// upe_dev.h — what the rule compiler (upe_rules.cpp, plain C++) and the device code of
// upe_gpu.hip must agree on: the layouts of the compiled rule table and its indexes, their
// constants, and the hashes both sides compute.  It compiles without the HIP runtime: the vector
// types come from hip_vector_types.h.
#ifndef UPE_DEV_H
#define UPE_DEV_H

#include <stddef.h>
#include <stdint.h>

#include <string>

#include <hip/hip_vector_types.h>

// Functions both sides compute.
#ifdef __HIPCC__
#define UPE_HD __host__ __device__
#else
#define UPE_HD
#endif
#define UPE_INLINE static inline __attribute__((always_inline))
// Functions one unit of the library defines for another: not exported.
#define UPE_INTERNAL __attribute__((visibility("hidden")))

// The library's one error slot (upe_gpu.hip; every unit and upe_worker.c use it): sets the calling
// thread's upe_gpu_last_error() message and returns -1.
extern "C" UPE_INTERNAL int upe_gpu_set_last_error(const char* msg);

namespace upe {

static inline int fail(const std::string& msg) { return upe_gpu_set_last_error(msg.c_str()); }

constexpr int kUnroll = 4;             // rules per early-exit check (rule table padding unit)
constexpr uint32_t kNone = 0xFFFFFFFFu;
// kernels for linear tables past kSmallRules (family lists, whole-table scan, decision tree) keep
// no small-table copy in static LDS (~1 KB static): 158 KB for their dynamic LDS
constexpr size_t kLdsDynMaxLarge = 158 * 1024;
constexpr int kSmallRules = 64;        // up to here rule_stats go through replicated accumulators

// ---- compiled rule table (built by upe_gpu_load_rules) --------------------------------------
// rv4[i]: header + first address word, used for every packet:
//   x0 = ip_ver | proto << 8 | src_port << 16 and its wildcard mask m0
//   x1 = dst_port and mask m1; m1 bit 31 (x1 bit 31 clear, so it never decides a match) marks a
//   rule with IPv6 address words, the only rules an IPv6 key must test against rv6; x1 bits
//   16-17 (m1 bits 16-30 clear) carry the action code (0 drop, 1 forward, 2 any other type),
//   so the scan hands the matched rule's action over with its index
//   s0/sm0, d0/dm0: union bytes 0-3 of src/dst as LE u32 (the v4 view, rule_t.src_ip.v4),
//   pre-masked so a match is ((key ^ x) & m) == 0 for every pair.
// rv6[i]: union words 1-3 of src/dst (pre-masked) and masks, used only by IPv6 packets.
// rinfo[i]: (action.type, rule_id).
struct __attribute__((aligned(16))) RuleV4 {
    uint32_t x0, m0, x1, m1, s0, sm0, d0, dm0;
};
constexpr uint32_t kRuleV6Words = 0x80000000u;
struct __attribute__((aligned(16))) RuleV6 {
    uint32_t s[3], sm[3], d[3], dm[3], pad[4];
};
// FamTable (linear-scan tables past the LDS size): the rules an IPv4 key can match (ip_ver 4 or
// 0) and those an IPv6 key can match (6 or 0), each list in priority order, so that a lane walks
// only its own family's list — a wave's scan lasts as long as its deepest lane's position in its
// family's list, not in the whole table.  Image: fam4 RuleV4, then fam6 (RuleV4, RuleV6) pairs,
// then the lists' sorted indexes (u32, fam4 then fam6); padding entries never match.  An IPv6
// entry is 80 bytes: the RuleV4 words, then RuleV6's s[3] sm[3] d[3] dm[3].  When the IPv6 list
// fits beside the launch's other LDS data it is staged there (Args::fam6_lds): an IPv6 lane's
// scan, the deep one in mixed tables, then reads LDS instead of the scalar cache.
constexpr uint32_t kFamV6Stride = 5;   // uint4 per IPv6 entry

// Tuple-space index of a large rule table (built by upe_gpu_load_rules when it pays): the rules
// a packet family can match are grouped by mask signature; a group's cuckoo table maps the
// masked key to the smallest sorted index with that key.  Group descriptor words:
//   [0] m0 (proto, src_port masks)  [1] m1 (dst_port mask)  [2] src word-0 mask
//   [3] dst word-0 mask  [4..6] src words 1-3 masks  [7..9] dst words 1-3 masks (family 6)
//   [10] smallest sorted index in the group  [11] log2(slots)  [12] seed  [13] first slot
//   [14] 1 | action << 8 when every mask word is zero (a catch-all group: every packet of the
//        family matches its one key, so the probe needs no memory access), else 0
//   [15] 1 + offset of the group's fingerprints in the staged image (tfs), 0 = not staged
// Slots: family 4 = 2 x uint4 {k0, k1, s0, d0}, {index, used, -, -};
//        family 6 = 3 x uint4 {k0, k1, s0, s1}, {s2, s3, d0, d1}, {d2, d3, index, used}.
struct __attribute__((aligned(16))) TssGroup {
    uint32_t w[16];
};
// An IPv4 slot is one uint4: the masked key's free bits carry the rest — k0's low byte (the IP
// version, never part of a group's mask) and k1's high half (above the 16-bit destination port)
// hold v = (index + 1) | action << 22 (0 = empty slot), so a probe is one 16-byte load, one
// memory request (two loads into one line were two requests: tools/fetch_calib), and the IPv4
// slot array takes half the L2 (config D 755 -> 716 us per 16M against 32-byte slots).
constexpr int kTssSlot4 = 1, kTssSlot6 = 3;   // uint4 per slot
constexpr uint32_t kTssMaxRules = 1u << 22;   // index + 1 in 22 bits, the action above it
// Fingerprints of small groups staged in LDS (word [15] of such a group: 1 + its offset in the
// staged image): their probes then wait for no fingerprint round trip.
constexpr uint32_t kFpStageMax = 8192;     // staged fingerprints (2 bytes each)
constexpr uint32_t kFpStageGroup = 4096;   // largest group (slots) staged
// Groups whose fingerprints are not staged are probed without them: slot t1 (where cuckoo
// placement leaves ~80 % of the keys at this load), then t2 if t1 holds another key.  One round
// trip for most hits instead of a fingerprint trip followed by a slot trip (config D 808 -> 775
// us); a miss takes two slot reads.
constexpr uint32_t kTssRatioX2 = 5;   // tuple-space slots >= ratio / 2 x keys

// Decision-tree index of a linear-scan table past kSmallRules (round 5; built by
// upe_gpu_load_rules when the tuple-space index does not apply).  The family lists (FamTable)
// stay the rules; each list gets a binary tree over the key's words, HyperSplit-style: an inner
// node compares one key word with a threshold, a leaf lists the positions of the rules whose
// conservative range meets the leaf's box (lo = x & m, hi = x | ~m per word), in list order, cut
// after the first one that matches every key of the box (flagged: it needs no test).  A key's
// first match in (priority, rule_id) order is therefore the first of its leaf's rules that
// matches it (reference src/rule_table.c:163-176): a rule that can match the key meets the box,
// so it is listed, or the flagged rule precedes it and matches the key too.  A lane walks its
// family's tree (one node load per level) and tests a handful of rules, however deep its first
// match lies in the table — the wave-uniform scan lasted as long as the wave's deepest lane.
// Key words: 0-3 source address, 4-7 destination address (IPv6: the wire bytes as big-endian
// words, so that a prefix is a range; IPv4: word 0 host order as parse_flow_key stores it, the
// other words 0), 8 source port, 9 destination port, 10 protocol.
// The binary tree is built (build_tree_family), then packed two levels to a node, so that a walk
// step resolves two levels with one 16-byte load (the walk is a chain of dependent LDS loads):
//   node (uint4): {x, y, z, w}: x = dim P | dim L << 4 | dim R << 8 | P leaf << 12 | L leaf << 13 |
//                 R leaf << 14 | base << 15; y = P's threshold (P leaf: its leaf word); z / w =
//                 the threshold of P's left / right child L / R, or its leaf word.  A key word <
//                 threshold goes left.  L's children are nodes base, base + 1; R's follow them
//                 (base, base + 1 when L is a leaf).
//   leaf word: count << 21 | first entry
//   leaf entry (u32): list position | 0x80000000 when the rule matches every key of the leaf
// Each family's rules are split into groups by the key field on which each is narrowest, one
// tree per group (a rule narrow only in a port is then not copied into every leaf of a tree cut on
// addresses); a key's first match is the smallest of its first matches over its family's trees,
// else the family's rule that matches every key (build_forest_family).
// Image: a directory (node 0 = {IPv4 trees, IPv6 trees | byte orders << 16, IPv4 default answer,
// IPv6 default answer}), each tree's root node (IPv4 first), the other nodes, then the leaf
// entries; staged in LDS when it fits beside the launch's other LDS data.
constexpr int kTreeDims = 11;
constexpr int kTreeFields = 5;   // field trees per family (build_forest_family)
constexpr uint32_t kTreeBinth = 4;   // a node with more rules than this is split (if it can be)
constexpr size_t kTreeMinReach = 64;   // (load_rules_impl: tree or scan)

UPE_HD UPE_INLINE uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }
UPE_HD UPE_INLINE uint32_t slot1(uint32_t k, uint32_t seed, uint32_t bits) {
    return ((k ^ seed) * 0x9E3779B1u) >> (32 - bits);
}
UPE_HD UPE_INLINE uint32_t slot2(uint32_t k, uint32_t seed, uint32_t bits) {
    const uint32_t x = (k ^ seed) * 0x85EBCA77u;
    return ((x ^ (x >> 16)) * 0xC2B2AE3Du) >> (32 - bits);
}
// The neighbour indexes' third choice (round 5: three-choice cuckoo placement fills the slots to
// ~0.6-0.8 instead of two-choice's < 0.5, so an index takes half the LDS: config C's ARP and NDP
// indexes 96 -> 48 KB, config B's ARP index 16 -> 8 KB)
UPE_HD UPE_INLINE uint32_t slot3(uint32_t k, uint32_t seed, uint32_t bits) {
    const uint32_t x = (k ^ (seed * 0x9E3779B9u)) * 0x27D4EB2Fu;
    return ((x ^ (x >> 15)) * 0x165667B1u) >> (32 - bits);
}
// The NDP index's 32-bit key: the fold of an address's four LE words (different addresses may
// share it; a slot hits on the full address).
UPE_HD UPE_INLINE uint32_t fold_v6(const uint32_t ip[4]) {
    return (ip[0] * 0x9E3779B1u) ^ (ip[1] * 0x85EBCA77u) ^ (ip[2] * 0xC2B2AE3Du) ^
           (ip[3] * 0x27D4EB2Fu);
}
// Key hash of the tuple-space index (host and device agree bit for bit).
UPE_HD UPE_INLINE uint32_t tss_hash(const uint32_t* k, int nw, uint32_t seed) {
    uint32_t h = seed ^ 0x9E3779B9u;
    for (int j = 0; j < nw; ++j) {
        h = (h ^ k[j]) * 0x01000193u;
        h ^= h >> 15;
    }
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
// A slot's 16-bit fingerprint (never 0, which marks an empty slot).  The slot positions come
// from the high bits of products of the hash, the tag from its low bits.
UPE_HD UPE_INLINE uint16_t tss_tag(uint32_t h) {
    return (uint16_t)((h & 0xFFFFu) | 1u);
}

// The word forms of a MAC and of four address bytes (DevL1, the neighbour slots, RuleV4 / RuleV6).
static inline uint32_t mac_lo(const uint8_t* m) {
    return (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
}
static inline uint32_t mac_hi(const uint8_t* m) { return (uint32_t)m[4] | ((uint32_t)m[5] << 8); }
static inline uint32_t le32(const uint8_t* p) { return mac_lo(p); }

// May handle_control_packet (reference src/worker.c:23-104) call arp_update or ndp_update for
// this frame?  ARP with the Ethernet/IPv4 header (the learn does not look at len), or an IPv6
// NS/NA of at least 78 bytes (whether an option carries the address is decided on the host).
// at(k) is frame byte k, zero at or past len (a zero-filled pktbuf); only k in 12..20 and 54 is
// asked for.  The same rule as is_table_write in upe_worker.c.
template <class At>
UPE_HD UPE_INLINE bool ctrl_table_write(uint32_t len, At at) {
    const uint32_t et = at(12u) << 8 | at(13u);
    if (et == 0x0806u)
        return at(14u) == 0u && at(15u) == 1u && at(16u) == 8u && at(17u) == 0u && at(18u) == 6u &&
               at(19u) == 4u;
    return et == 0x86DDu && len >= 78u && at(20u) == 58u && (at(54u) == 135u || at(54u) == 136u);
}

}  // namespace upe

#endif  // UPE_DEV_H
