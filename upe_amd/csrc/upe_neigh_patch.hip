// upe_neigh_patch.hip — known neighbours refreshed on the device (upe_gpu_neigh_patch,
// include/upe_gpu.h): the records of upe_gpu_ctrl_writes applied to the loaded snapshot where that
// moves nothing.  arp_update (reference src/arp_table.c:26-53) and ndp_update (src/ndp_table.c:
// 39-65) of an address that arp_get_mac / ndp_get_mac (:55-80, :67-86) finds walk the lookup's own
// probe path and rewrite the MAC of the slot it answers from; the snapshot's index holds exactly
// the entries a probe reaches, so such a record changes the six MAC bytes of one index slot.  A
// record whose address the snapshot does not hold is listed as missed and left to the host
// (DESIGN.md §3 has the argument that the two halves may be applied apart).
//
// Three launches on one stream; the kernel boundaries are the only ordering between workgroups,
// and no result depends on the order in which workgroups run:
//   upe_patch_resolve  one lane per record: the lookup (arp_lookup / ndp_lookup decide "held",
//                      arp_slot_of / ndp_slot_of say where: upe_neigh_lookup.h), the slot into a
//                      word per record, atomicMax(rank + 1) on the slot's owner word; the
//                      workgroup's misses and its first miss.
//   upe_patch_scan     one workgroup: the exclusive prefix of the misses over the workgroups, and
//                      *info.
//   upe_patch_commit   the record that owns its slot — the held record of highest rank aimed at it
//                      — stores the MAC's six bytes and puts the owner word back to zero; no two
//                      lanes write one slot.  The misses' ranks by ballot within a wave, the
//                      waves' counts through LDS, behind the workgroup's prefix.
// The lookups read the tables in the first launch only and the last one writes them: a record
// never sees another record's MAC, and "held" is held before the call.
//
// Scratch: uint32 nmiss[Tp], fmiss[Tp], mex[Tp] (misses, the first miss, misses before each
// workgroup) and where[count]; T workgroups, Tp = T rounded up to 4.  Owner words: one per index
// slot, the ARP index's 2^bits and then the NDP index's, zero between calls.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "upe_ctx.h"
#include "upe_neigh_lookup.h"
#include "upe_scan.h"

using namespace upe;

namespace {

constexpr uint32_t kBlock = UPE_PATCH_BLOCK;   // records per workgroup, one per thread
constexpr uint32_t kWaves = kBlock / 64;
constexpr uint32_t kScanThreads = 1024;        // workgroups per step of the scan
constexpr uint32_t kScanWaves = kScanThreads / 64;
static_assert(kBlock % 64 == 0 && kBlock <= 1024, "a workgroup of whole waves");

// The snapshot as the kernels take it: the lookups' view, the slot arrays to write, and where the
// NDP index's owner words begin.
struct PatchTables {
    NeighIndex arp, ndp;
    uint4 *arp_w, *ndp_w;
    uint32_t arp_slots;   // 2^arp.bits, or 0
};

__global__ void __launch_bounds__(kBlock) upe_patch_resolve(
    const uint4* writes, uint32_t count, PatchTables t, uint32_t* owner, uint32_t* where,
    uint32_t* nmiss, uint32_t* fmiss) {
    __shared__ uint32_t s_n[kWaves], s_f[kWaves];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    const uint32_t i = blockIdx.x * kBlock + tid;   // < count + kBlock: no wrap
    uint32_t w = kNone;
    if (i < count) {
        const uint4 a = writes[2 * (size_t)i], b = writes[2 * (size_t)i + 1];
        const uint32_t kind = a.y & 0xFFu;
        uint32_t lo, hi;
        if (kind == UPE_CW_ARP) {
            if (arp_lookup(t.arp, b.x, lo, hi)) w = arp_slot_of(t.arp, b.x);
        } else if (kind == UPE_CW_NDP) {
            const uint32_t ip[4] = {b.x, b.y, b.z, b.w};
            if (ndp_lookup(t.ndp, ip, lo, hi)) {
                const uint32_t s = ndp_slot_of(t.ndp, ip);
                w = s == kNone ? kNone : t.arp_slots + s;
            }
        }
        if (w != kNone) atomicMax(&owner[w], i + 1u);   // rank + 1 <= 2^32 - kBlock
        where[i] = w;
    }
    const bool miss = i < count && w == kNone;
    const unsigned long long bal = __ballot(miss);
    const uint32_t f = wave_min(miss ? i : kNone);
    if (lane == 0) {
        s_n[wave] = (uint32_t)__popcll(bal);
        s_f[wave] = f;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t n = 0, first = kNone;
#pragma unroll
        for (uint32_t j = 0; j < kWaves; ++j) {
            n += s_n[j];
            first = s_f[j] < first ? s_f[j] : first;
        }
        nmiss[blockIdx.x] = n;
        fmiss[blockIdx.x] = first;
    }
}

// One workgroup; a step covers kScanThreads workgroups of the other two launches, one per thread.
// The sums stay below count < 2^32.
__global__ void __launch_bounds__(kScanThreads) upe_patch_scan(
    uint32_t T, uint32_t count, const uint32_t* nmiss, const uint32_t* fmiss, uint32_t* mex,
    upe_neigh_patch_info_t* info) {
    __shared__ uint32_t s_ww[kScanWaves];
    __shared__ uint32_t s_fm;
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    if (tid == 0) s_fm = kNone;
    uint32_t carry = 0, fm = kNone;
    for (uint32_t c0 = 0; c0 < T; c0 += kScanThreads) {
        const uint32_t b = c0 + tid;
        const uint32_t w = b < T ? nmiss[b] : 0u;
        if (b < T) {
            const uint32_t x = fmiss[b];
            fm = x < fm ? x : fm;
        }
        uint32_t all;   // (the first step's barriers also order s_fm, set above)
        const uint32_t ex = block_excl(w, lane, wave, s_ww, all);
        if (b < T) mex[b] = carry + ex;
        carry += all;
    }
    fm = wave_min(fm);
    if (lane == 0) atomicMin(&s_fm, fm);
    __syncthreads();
    if (tid == 0) {
        const uint32_t first = s_fm;
        info->records = count;
        info->patched = count - carry;
        info->missed = carry;
        info->first_miss = first == kNone ? ~0ull : (uint64_t)first;
    }
}

__global__ void __launch_bounds__(kBlock) upe_patch_commit(
    const uint4* writes, uint32_t count, PatchTables t, uint32_t* owner, const uint32_t* where,
    const uint32_t* nmiss, const uint32_t* mex, uint32_t* miss_out) {
    __shared__ uint32_t s_n[kWaves];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    const uint32_t i = blockIdx.x * kBlock + tid;
    const bool live = i < count;
    const uint32_t w = live ? where[i] : 0u;
    // w < arp_slots + 2^ndp.bits, the owner words' count: it is a slot the first launch found
    if (live && w != kNone && owner[w] == i + 1u) {
        const uint4 a = writes[2 * (size_t)i];
        const uint32_t lo = a.z, hi = a.w & 0xFFFFu;   // mac[0..3], mac[4..5]
        if (w < t.arp_slots) {
            uint4* e = t.arp_w + w;
            e->y = lo;
            e->z = (e->z & 0xFFFF0000u) | hi;
        } else {
            uint4* m = t.ndp_w + 2 * (size_t)(w - t.arp_slots) + 1;
            m->x = lo;
            m->y = (m->y & 0xFFFF0000u) | hi;
        }
        owner[w] = 0u;   // the only lane whose test of this word can succeed
    }
    if (!miss_out || nmiss[blockIdx.x] == 0u) return;   // the whole workgroup
    const bool miss = live && w == kNone;
    const unsigned long long bal = __ballot(miss);
    if (lane == 0) s_n[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (!miss) return;
    uint32_t pos = mex[blockIdx.x] + (uint32_t)__popcll(bal & lanes_below(lane));
    for (uint32_t j = 0; j < wave; ++j) pos += s_n[j];
    miss_out[pos] = i;   // pos < the call's misses
}

struct Tab {
    uint32_t *nmiss, *fmiss, *mex, *where;
};

// The scratch of one call over `count` records in T workgroups (count > 0).
Tab layout(Carver& c, uint32_t T, uint32_t count) {
    const size_t tp = ((size_t)T + 3u) & ~(size_t)3u;
    Tab t;
    t.nmiss = c.take<uint32_t>(tp);
    t.fmiss = c.take<uint32_t>(tp);
    t.mex = c.take<uint32_t>(tp);
    t.where = c.take<uint32_t>(count);
    return t;
}

// The call's launches, with what the context does around a change of its tables.
int patch_launch(upe_gpu_ctx_t* c, const PatchTables& pt, const uint4* writes, uint32_t count,
                 uint32_t* d_miss, upe_neigh_patch_info_t* d_info, hipStream_t s) {
    const uint32_t T = tiles_of(count, kBlock);
    Carver mem(c->np_scratch.p);
    const Tab t = layout(mem, T, count);
    if (neigh_patching(c, s) != 0) return -1;
    hipLaunchKernelGGL(upe_patch_resolve, dim3(T), dim3(kBlock), 0, s, writes, count, pt,
                       c->np_owner.p, t.where, t.nmiss, t.fmiss);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(upe_patch_scan, dim3(1), dim3(kScanThreads), 0, s, T, count, t.nmiss,
                       t.fmiss, t.mex, d_info);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(upe_patch_commit, dim3(T), dim3(kBlock), 0, s, writes, count, pt,
                       c->np_owner.p, t.where, t.nmiss, t.mex, d_miss);
    HIP_TRY(hipGetLastError());
    return neigh_patched(c, s);
}

}  // namespace

extern "C" int upe_gpu_neigh_patch(upe_gpu_ctx_t* c, const upe_ctrl_write_t* d_writes, size_t count,
                                   uint32_t* d_miss, upe_neigh_patch_info_t* d_info, void* stream) {
    if (!c) return fail("null context");
    if (!d_info || (count && !d_writes)) return fail("null buffer");
    if ((reinterpret_cast<uintptr_t>(d_writes) & 15u) != 0)
        return fail("d_writes must be 16-byte aligned");
    if (count > 0xFFFFFFFFull - UPE_PATCH_BLOCK) return fail("count must fit in 32 bits");
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    if (count == 0) return empty_info(d_info, &upe_neigh_patch_info_t::first_miss, s);
    const NeighTable& n = c->neigh;
    const uint64_t arp_slots = n.arp_bits ? 1ull << n.arp_bits : 0ull;
    const uint64_t slots = arp_slots + (n.ndp_bits ? 1ull << n.ndp_bits : 0ull);
    if (slots >= kNone) return fail("neighbour index too large to patch");
    const size_t need = layout_bytes(layout, tiles_of((uint32_t)count, kBlock), (uint32_t)count);
    if (c->np_scratch.reserve(need, need + need / 4) != 0) return -1;
    if (slots > c->np_owner.cap) {   // a larger index since the last call: fresh zero words
        if (c->np_owner.reserve(slots, slots) != 0) return -1;
        HIP_TRY(hipMemsetAsync(c->np_owner.p, 0, slots * sizeof(uint32_t), s));
    }
    PatchTables pt;
    pt.arp = NeighIndex{n.arp, n.arp_bits, n.arp_seed};
    pt.ndp = NeighIndex{n.ndp, n.ndp_bits, n.ndp_seed};
    pt.arp_w = n.arp;
    pt.ndp_w = n.ndp;
    pt.arp_slots = (uint32_t)arp_slots;
    const int rc = patch_launch(c, pt, reinterpret_cast<const uint4*>(d_writes), (uint32_t)count,
                                d_miss, d_info, s);
    // a call cut short may leave owner words behind: the next one starts from fresh ones
    if (rc != 0) c->np_owner.reset();
    return rc;
}
