// upe_neigh_lookup.h — arp_get_mac / ndp_get_mac on the device (reference src/arp_table.c:55-80,
// src/ndp_table.c:67-86): the lookups in the neighbour snapshot's three-choice cuckoo index
// (NeighImage, upe_rules.h; built by build_neigh_image from the entries a reference probe reaches),
// for the units whose kernels resolve next hops: upe_gpu.hip (upe_classify per forwarded packet,
// upe_refresh for the L1 entries) and upe_neigh.hip (upe_resolve_keys, per flow key).  Device code
// only; internal linkage (an unnamed namespace, as upe_match.h), so each unit compiles its own
// copies into its own kernels.  slot1 / slot2 / slot3 and fold_v6 are upe_dev.h's, shared with the
// builder.
#ifndef UPE_NEIGH_LOOKUP_H
#define UPE_NEIGH_LOOKUP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "upe_dev.h"

namespace {

using namespace upe;

// Neighbour index (built by upe_gpu_load_neigh): the entries a reference probe reaches, placed
// by three-choice cuckoo hashing, so that every key sits in one of its three candidate slots.
//   ARP slot: uint4 {ip, mac0..3, mac4..5 | used << 16, 0}
//   NDP slot: 2 x uint4 {ip words 0..3}, {mac0..3, mac4..5 | used << 16, 0, 0}
struct NeighIndex {
    const uint4* t;
    uint32_t bits;   // log2(slots); 0 = empty
    uint32_t seed;
};

// ---- neighbour lookups (fold_v6: upe_dev.h) -------------------------------------------------
__device__ __forceinline__ bool arp_slot_hit(const uint4& e, uint32_t ip) {
    return ((e.z >> 16) & 1u) && e.x == ip;
}
__device__ __forceinline__ bool arp_lookup(const NeighIndex& x, uint32_t ip, uint32_t& lo,
                                           uint32_t& hi) {
    if (x.bits == 0) return false;
    const uint4 e1 = x.t[slot1(ip, x.seed, x.bits)];
    const uint4 e2 = x.t[slot2(ip, x.seed, x.bits)];
    const uint4 e3 = x.t[slot3(ip, x.seed, x.bits)];
    const bool h1 = arp_slot_hit(e1, ip), h2 = arp_slot_hit(e2, ip), h3 = arp_slot_hit(e3, ip);
    const uint4 e = h1 ? e1 : h2 ? e2 : e3;
    lo = e.y;
    hi = e.z & 0xFFFFu;
    return h1 || h2 || h3;
}
// The same lookup against an LDS copy of the slot array.
__device__ __forceinline__ bool arp_lookup_lds(const uint4* t, uint32_t bits, uint32_t seed,
                                               uint32_t ip, uint32_t& lo, uint32_t& hi) {
    const uint4 e1 = t[slot1(ip, seed, bits)];
    const uint4 e2 = t[slot2(ip, seed, bits)];
    const uint4 e3 = t[slot3(ip, seed, bits)];
    const bool h1 = arp_slot_hit(e1, ip), h2 = arp_slot_hit(e2, ip), h3 = arp_slot_hit(e3, ip);
    const uint4 e = h1 ? e1 : h2 ? e2 : e3;
    lo = e.y;
    hi = e.z & 0xFFFFu;
    return h1 || h2 || h3;
}
__device__ __forceinline__ bool ndp_slot_hit(const uint4& a, const uint4& m, const uint32_t ip[4]) {
    return ((m.y >> 16) & 1u) && a.x == ip[0] && a.y == ip[1] && a.z == ip[2] && a.w == ip[3];
}
__device__ __forceinline__ bool ndp_lookup_lds(const uint4* t, uint32_t bits, uint32_t seed,
                                               const uint32_t ip[4], uint32_t& lo, uint32_t& hi) {
    const uint32_t k = fold_v6(ip);
    const uint32_t t1 = slot1(k, seed, bits), t2 = slot2(k, seed, bits), t3 = slot3(k, seed, bits);
    const uint4 a1 = t[2 * t1], m1 = t[2 * t1 + 1];
    const uint4 a2 = t[2 * t2], m2 = t[2 * t2 + 1];
    const uint4 a3 = t[2 * t3], m3 = t[2 * t3 + 1];
    const bool h1 = ndp_slot_hit(a1, m1, ip), h2 = ndp_slot_hit(a2, m2, ip),
               h3 = ndp_slot_hit(a3, m3, ip);
    const uint4 m = h1 ? m1 : h2 ? m2 : m3;
    lo = m.x;
    hi = m.y & 0xFFFFu;
    return h1 || h2 || h3;
}
__device__ __forceinline__ bool ndp_lookup(const NeighIndex& x, const uint32_t ip[4], uint32_t& lo,
                                           uint32_t& hi) {
    if (x.bits == 0) return false;
    return ndp_lookup_lds(x.t, x.bits, x.seed, ip, lo, hi);
}

// Where a lookup's answer lies: the slot (of the index's 2^bits) that arp_lookup / ndp_lookup
// answer from, the first of the address's three candidates that hits, or kNone where they miss
// (upe_neigh_patch.hip rewrites that slot's MAC; the lookups themselves decide "held" there).
__device__ __forceinline__ uint32_t arp_slot_of(const NeighIndex& x, uint32_t ip) {
    if (x.bits == 0) return kNone;
    const uint32_t t1 = slot1(ip, x.seed, x.bits), t2 = slot2(ip, x.seed, x.bits),
                   t3 = slot3(ip, x.seed, x.bits);
    return arp_slot_hit(x.t[t1], ip) ? t1 : arp_slot_hit(x.t[t2], ip) ? t2
         : arp_slot_hit(x.t[t3], ip) ? t3 : kNone;
}
__device__ __forceinline__ uint32_t ndp_slot_of(const NeighIndex& x, const uint32_t ip[4]) {
    if (x.bits == 0) return kNone;
    const uint32_t k = fold_v6(ip);
    const uint32_t t1 = slot1(k, x.seed, x.bits), t2 = slot2(k, x.seed, x.bits),
                   t3 = slot3(k, x.seed, x.bits);
    return ndp_slot_hit(x.t[2 * t1], x.t[2 * t1 + 1], ip)   ? t1
           : ndp_slot_hit(x.t[2 * t2], x.t[2 * t2 + 1], ip) ? t2
           : ndp_slot_hit(x.t[2 * t3], x.t[2 * t3 + 1], ip) ? t3
                                                            : kNone;
}

// Both families in one lookup: the IPv4 (ARP) and IPv6 (NDP) lanes of a wave issue their slot
// loads together, so a mixed wave waits for one memory round trip, not one per family.
__device__ __forceinline__ bool neigh_lookup(const NeighIndex& arp, const NeighIndex& ndp,
                                             bool v6, const uint32_t d[4], uint32_t& lo,
                                             uint32_t& hi) {
    const uint4* t = v6 ? ndp.t : arp.t;
    const uint32_t bits = v6 ? ndp.bits : arp.bits;
    const uint32_t seed = v6 ? ndp.seed : arp.seed;
    if (bits == 0) return false;
    const uint32_t k = v6 ? fold_v6(d) : d[0];
    const uint32_t t1 = slot1(k, seed, bits), t2 = slot2(k, seed, bits), t3 = slot3(k, seed, bits);
    const uint32_t sh = v6 ? 1u : 0u;   // an NDP slot is two uint4: address, then MAC
    const uint4 a1 = t[t1 << sh], a2 = t[t2 << sh], a3 = t[t3 << sh];
    uint4 m1 = a1, m2 = a2, m3 = a3;
    if (v6) {
        m1 = t[2 * t1 + 1];
        m2 = t[2 * t2 + 1];
        m3 = t[2 * t3 + 1];
    }
    const bool h1 = v6 ? ndp_slot_hit(a1, m1, d) : arp_slot_hit(a1, d[0]);
    const bool h2 = v6 ? ndp_slot_hit(a2, m2, d) : arp_slot_hit(a2, d[0]);
    const bool h3 = v6 ? ndp_slot_hit(a3, m3, d) : arp_slot_hit(a3, d[0]);
    const uint4 e = h1 ? (v6 ? m1 : a1) : h2 ? (v6 ? m2 : a2) : (v6 ? m3 : a3);
    lo = v6 ? e.x : e.y;
    hi = (v6 ? e.y : e.z) & 0xFFFFu;
    return h1 || h2 || h3;
}

}  // namespace

#endif  // UPE_NEIGH_LOOKUP_H
