// upe_neigh_learn.hip — new neighbours learnt on the device (upe_gpu_neigh_learn,
// include/upe_gpu.h): the records of upe_gpu_ctrl_writes applied to the loaded snapshot, the ones
// for an address it does not hold included.  arp_update (reference src/arp_table.c:26-53) and
// ndp_update (src/ndp_table.c:39-65) of a held address rewrite the MAC of the slot the lookup
// answers from, as upe_neigh_patch.hip does; of a new address they take the first invalid slot of
// the probe, which succeeds exactly when the table has an invalid slot, provided every valid
// entry is one a probe reaches (`insertable`; DESIGN.md §3 has the argument).  The index then
// takes the address in the first of its three candidate slots that is free: a lookup reads all
// three, so which one holds it decides nothing.
//
// The contract is a loop over the records in rank order.  One launch of ONE workgroup runs it,
// kChunk records per step, a lane per record; the steps follow one another in the workgroup, each
// seeing the slots the one before wrote, so no result depends on how workgroups or waves are
// scheduled.  A step, between barriers:
//   lookup   the three candidate slots of the record's address: held (some used candidate holds
//            it) -> atomicMax(lane + 1) on the slot's owner word, as upe_patch_resolve; else, in
//            an insertable family, the record is new.
//   groups   the new records, compacted in rank order into LDS; each compares itself with all of
//            them: the lowest rank of an address leads its group, the highest supplies the MAC.
//            A follower of an inserted leader is a refresh of what the leader wrote (patched);
//            of a dropped leader it meets the same full table (dropped); of a deferred leader the
//            same three used candidates (deferred), unless the table has filled since (dropped).
//   bids     each leader claims, with atomicMax(kChunk - lane) on the owner word, its first
//            candidate that is unused and not claimed by a lower rank; whoever is displaced moves
//            on; repeated until a round changes nothing.  A claim only ever passes to a lower
//            rank, so a leader only moves forward, and the fixed point is the sequential greedy
//            placement: by induction over the ranks, each leader sits in its first candidate that
//            no lower rank sits in.
//   free     per family, a leader with `free` or more placed leaders below it is dropped (the
//            full table), whether it was placed or not; the others are inserted where placed and
//            deferred where all three candidates were used.  free -= the inserted.
//   stores   the held record that owns its slot stores the slot with its MAC; an inserted leader
//            stores its slot with the MAC of its group's last record; every owner word used goes
//            back to zero.  Whole 16-byte slots are loaded and stored.  The deferred ranks behind
//            a workgroup scan (upe_scan.h).
// Owner words: the context's (np_owner, shared with upe_gpu_neigh_patch), one per index slot, ARP
// then NDP, zero between calls.  In a step a used slot's word holds lane + 1 of a held record, an
// unused slot's kChunk - lane of a bidding leader: the two sets of slots are disjoint.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "upe_ctx.h"
#include "upe_neigh_lookup.h"
#include "upe_scan.h"

using namespace upe;

namespace {

constexpr uint32_t kChunk = UPE_LEARN_CHUNK;   // records per step, one per thread
constexpr uint32_t kWaves = kChunk / 64;
static_assert(kChunk == 1024, "one workgroup of 16 waves; a lane and a family fit in a word");

enum : uint32_t { kPatched = 0, kInserted = 1, kDropped = 2, kDeferred = 3 };

// The snapshot as the kernel takes it: the lookups' view, the slot arrays to write, where the NDP
// index's owner words begin, and which families take new addresses.
struct LearnTables {
    NeighIndex arp, ndp;
    uint4 *arp_w, *ndp_w;
    uint32_t arp_slots;   // 2^arp.bits, or 0
    uint32_t arp_ins, ndp_ins;
};

__device__ __forceinline__ uint32_t sel3(uint32_t q, uint32_t a, uint32_t b, uint32_t c) {
    return q == 0 ? a : q == 1 ? b : c;
}
// An owner word as the last atomic on it left it (the word changes under atomics of other waves).
__device__ __forceinline__ uint32_t owner_now(uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kChunk) upe_learn(
    const uint4* writes, uint32_t count, LearnTables t, uint32_t* owner, uint32_t* free_words,
    uint32_t from_image, uint32_t image_free_a, uint32_t image_free_n, uint32_t* defer_out,
    upe_neigh_learn_info_t* info) {
    __shared__ uint4 s_key[kChunk];      // the step's new records' addresses, in rank order
    __shared__ uint32_t s_who[kChunk];   // their lane | family << 16
    __shared__ uint32_t s_out[kChunk];   // a leader's outcome, by lane
    __shared__ uint32_t s_w[kWaves], s_wa[kWaves], s_wn[kWaves];
    __shared__ uint32_t s_cnt[3];        // patched, inserted, dropped so far
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    if (tid < 3) s_cnt[tid] = 0u;
    // every thread keeps the same running copies; the first learn after a load starts from the
    // loaded image's counts, a later one from what the learn before it left in free_words
    uint32_t free_a = from_image ? image_free_a : free_words[0];
    uint32_t free_n = from_image ? image_free_n : free_words[1];
    uint32_t ndefer = 0;   // deferred so far
    for (uint32_t c0 = 0; c0 < count; c0 += kChunk) {   // count + kChunk < 2^32: no wrap
        const uint32_t i = c0 + tid;
        const bool live = i < count;
        // ---- lookup ----
        uint32_t fam = 2u, g1 = 0, g2 = 0, g3 = 0, used = 7u, held_w = kNone;
        uint4 key = make_uint4(0, 0, 0, 0);
        bool fresh = false;   // a new address in an insertable family
        if (live) {
            const uint4 a = writes[2 * (size_t)i], b = writes[2 * (size_t)i + 1];
            const uint32_t kind = a.y & 0xFFu;
            fam = kind == UPE_CW_ARP ? 0u : kind == UPE_CW_NDP ? 1u : 2u;
            if (fam == 0u) key.x = b.x;
            if (fam == 1u) key = b;
            const NeighIndex& x = fam == 1u ? t.ndp : t.arp;
            if (fam != 2u && x.bits != 0u) {
                const uint32_t ip[4] = {key.x, key.y, key.z, key.w};
                const uint32_t k = fam == 1u ? fold_v6(ip) : key.x;
                const uint32_t t1 = slot1(k, x.seed, x.bits), t2 = slot2(k, x.seed, x.bits),
                               t3 = slot3(k, x.seed, x.bits);
                bool h1, h2, h3;
                if (fam == 0u) {
                    const uint4 e1 = x.t[t1], e2 = x.t[t2], e3 = x.t[t3];
                    used = ((e1.z >> 16) & 1u) | ((e2.z >> 16) & 1u) << 1 | ((e3.z >> 16) & 1u) << 2;
                    h1 = arp_slot_hit(e1, key.x), h2 = arp_slot_hit(e2, key.x),
                    h3 = arp_slot_hit(e3, key.x);
                } else {
                    const uint4 a1 = x.t[2 * (size_t)t1], m1 = x.t[2 * (size_t)t1 + 1];
                    const uint4 a2 = x.t[2 * (size_t)t2], m2 = x.t[2 * (size_t)t2 + 1];
                    const uint4 a3 = x.t[2 * (size_t)t3], m3 = x.t[2 * (size_t)t3 + 1];
                    used = ((m1.y >> 16) & 1u) | ((m2.y >> 16) & 1u) << 1 | ((m3.y >> 16) & 1u) << 2;
                    h1 = ndp_slot_hit(a1, m1, ip), h2 = ndp_slot_hit(a2, m2, ip),
                    h3 = ndp_slot_hit(a3, m3, ip);
                }
                const uint32_t base = fam == 1u ? t.arp_slots : 0u;
                g1 = base + t1, g2 = base + t2, g3 = base + t3;   // < the owner words' count
                if (h1 || h2 || h3) {
                    held_w = h1 ? g1 : h2 ? g2 : g3;
                    atomicMax(&owner[held_w], tid + 1u);
                } else {
                    fresh = (fam == 1u ? t.ndp_ins : t.arp_ins) != 0u;
                }
            }
        }
        __threadfence();   // the owner words' atomics have landed before the barriers below
        // ---- groups ----
        uint32_t m;   // the step's new records
        const uint32_t at = block_excl(fresh ? 1u : 0u, lane, wave, s_w, m);
        if (fresh) {
            s_key[at] = key;
            s_who[at] = tid | fam << 16;
        }
        __syncthreads();
        uint32_t lead = tid, last = tid;
        if (fresh) {
            lead = kNone;
            for (uint32_t j = 0; j < m; ++j) {
                const uint32_t who = s_who[j];
                const uint4 kj = s_key[j];
                if ((who >> 16) == fam && kj.x == key.x && kj.y == key.y && kj.z == key.z &&
                    kj.w == key.w) {
                    if (lead == kNone) lead = who & 0xFFFFu;
                    last = who & 0xFFFFu;
                }
            }
        }
        const bool leader = fresh && lead == tid;
        // ---- bids ----
        const uint32_t mine = kChunk - tid;   // 1 .. kChunk: the lower rank has the larger word
        uint32_t pos = leader ? 0u : 3u;
        for (;;) {
            bool changed = false;
            if (pos < 3u) {
                while (pos < 3u) {
                    if (!((used >> pos) & 1u) && owner_now(&owner[sel3(pos, g1, g2, g3)]) <= mine)
                        break;
                    ++pos;
                }
                if (pos < 3u)
                    changed = atomicMax(&owner[sel3(pos, g1, g2, g3)], mine) != mine;
            }
            if (!__syncthreads_or(changed ? 1 : 0)) break;
        }
        // ---- free ----
        const bool placed = leader && pos < 3u;
        uint32_t pa = placed && fam == 0u ? 1u : 0u, pn = placed && fam == 1u ? 1u : 0u;
        uint32_t all_a, all_n;
        block_excl(pa, pn, lane, wave, s_wa, s_wn, all_a, all_n);   // placed leaders below this lane
        // a new record whose turn comes with `free` or more placed leaders below it meets a full
        // table; below that, every placed leader before it was inserted
        const bool full = (fam == 0u ? pa : pn) >= (fam == 0u ? free_a : free_n);
        uint32_t out = kDeferred;
        if (leader) {
            out = full ? kDropped : placed ? kInserted : kDeferred;
            s_out[tid] = out;
        }
        __syncthreads();
        if (fresh && !leader) {
            // after an inserted leader: a refresh of its slot.  After a dropped one the table is
            // still full; after a deferred one the three candidates are still used, and the
            // table may have filled since.
            const uint32_t lo = s_out[lead];
            out = lo == kInserted ? kPatched : full ? kDropped : kDeferred;
        }
        if (held_w != kNone) out = kPatched;
        free_a -= all_a < free_a ? all_a : free_a;
        free_n -= all_n < free_n ? all_n : free_n;
        // ---- stores ----
        if (held_w != kNone && owner_now(&owner[held_w]) == tid + 1u) {
            const uint4 a = writes[2 * (size_t)i];
            const uint32_t lo = a.z, hi = a.w & 0xFFFFu;   // mac[0..3], mac[4..5]
            if (fam == 0u) {
                uint4* e = t.arp_w + held_w;
                uint4 v = *e;
                v.y = lo;
                v.z = (v.z & 0xFFFF0000u) | hi;
                *e = v;
            } else {
                uint4* e = t.ndp_w + 2 * (size_t)(held_w - t.arp_slots) + 1;
                uint4 v = *e;
                v.x = lo;
                v.y = (v.y & 0xFFFF0000u) | hi;
                *e = v;
            }
            owner[held_w] = 0u;   // the only lane whose test of this word can succeed
        }
        if (placed) {
            const uint32_t g = sel3(pos, g1, g2, g3);   // this lane's claim stands: the fixed point
            if (out == kInserted) {
                const uint4 a = writes[2 * (size_t)(c0 + last)];
                const uint32_t lo = a.z, hi = (a.w & 0xFFFFu) | (1u << 16);
                if (fam == 0u) {
                    t.arp_w[g] = make_uint4(key.x, lo, hi, 0u);
                } else {
                    uint4* e = t.ndp_w + 2 * (size_t)(g - t.arp_slots);
                    e[0] = key;
                    e[1] = make_uint4(lo, hi, 0u, 0u);
                }
            }
            owner[g] = 0u;
        }
        // ---- the step's counts and its deferred ranks ----
        const bool def = live && out == kDeferred;
#pragma unroll
        for (uint32_t o = 0; o < 3u; ++o) {
            const unsigned long long bal = __ballot(live && out == o);
            if (lane == 0 && bal) atomicAdd(&s_cnt[o], (uint32_t)__popcll(bal));
        }
        uint32_t nd;
        const uint32_t dpos = ndefer + block_excl(def ? 1u : 0u, lane, wave, s_w, nd);
        if (def) {
            if (defer_out) defer_out[dpos] = i;   // dpos < the call's deferred
            if (dpos == 0u) info->first_defer = i;
        }
        ndefer += nd;
        // the next step's lookups read this step's slots and owner words
        __threadfence();
        __syncthreads();
    }
    if (tid == 0) {
        info->records = count;
        info->patched = s_cnt[kPatched];
        info->inserted = s_cnt[kInserted];
        info->dropped = s_cnt[kDropped];
        info->deferred = ndefer;
        if (ndefer == 0u) info->first_defer = ~0ull;
        info->arp_free = free_a;
        info->ndp_free = free_n;
        free_words[0] = free_a;
        free_words[1] = free_n;
    }
}

}  // namespace

extern "C" int upe_gpu_neigh_learn(upe_gpu_ctx_t* c, const upe_ctrl_write_t* d_writes, size_t count,
                                   uint32_t* d_defer, upe_neigh_learn_info_t* d_info, void* stream) {
    if (!c) return fail("null context");
    if (!d_info || (count && !d_writes)) return fail("null buffer");
    if ((reinterpret_cast<uintptr_t>(d_writes) & 15u) != 0)
        return fail("d_writes must be 16-byte aligned");
    if (count > 0xFFFFFFFFull - UPE_LEARN_CHUNK) return fail("count must fit in 32 bits");
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    if (count == 0) return empty_info(d_info, &upe_neigh_learn_info_t::first_defer, s);
    const NeighTable& n = c->neigh;
    upe_gpu_ctx::Learn& l = c->learn;
    const uint64_t arp_slots = n.arp_bits ? 1ull << n.arp_bits : 0ull;
    const uint64_t slots = arp_slots + (n.ndp_bits ? 1ull << n.ndp_bits : 0ull);
    if (slots >= kNone) return fail("neighbour index too large to patch");
    if (!l.free.p && l.free.zeros(4) != 0) return -1;   // the context's first learn
    if (slots > c->np_owner.cap) {   // a larger index since the last call: fresh zero words
        if (c->np_owner.reserve(slots, slots) != 0) return -1;
        HIP_TRY(hipMemsetAsync(c->np_owner.p, 0, slots * sizeof(uint32_t), s));
    }
    LearnTables lt;
    lt.arp = NeighIndex{n.arp, n.arp_bits, n.arp_seed};
    lt.ndp = NeighIndex{n.ndp, n.ndp_bits, n.ndp_seed};
    lt.arp_w = n.arp;
    lt.ndp_w = n.ndp;
    lt.arp_slots = (uint32_t)arp_slots;
    lt.arp_ins = l.insertable[0] ? 1u : 0u;   // (no snapshot loaded yet: neither, nothing free)
    lt.ndp_ins = l.insertable[1] ? 1u : 0u;
    int rc = neigh_patching(c, s);
    if (rc == 0) {
        hipLaunchKernelGGL(upe_learn, dim3(1), dim3(kChunk), 0, s,
                           reinterpret_cast<const uint4*>(d_writes), (uint32_t)count, lt,
                           c->np_owner.p, l.free.p, l.on_device ? 0u : 1u, l.image_free[0],
                           l.image_free[1], d_defer, d_info);
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) l.on_device = true;
        rc = e == hipSuccess ? neigh_patched(c, s)
                             : fail(std::string("upe_learn: ") + hipGetErrorString(e));
    }
    // a call cut short may leave owner words behind: the next one starts from fresh ones
    if (rc != 0) c->np_owner.reset();
    return rc;
}
