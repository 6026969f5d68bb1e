// upe_gpu.hip — MI355X (gfx950 / CDNA4) batch dataplane for UPE's per-packet worker hot path:
// the classify kernels and the host side that launches them (context create and destroy, the rule
// and neighbour loads, process_impl, the device-buffer upe_gpu_process* calls, statistics, timing)
// of the extern "C" ABI declared in include/upe_gpu.h.  The context itself is upe_ctx.h's; the
// other stages (upe_rx.hip, upe_egress.hip, upe_ingress.hip, upe_latency.hip), the host paths
// (upe_hostpath.hip) and the segmented path (upe_segment.hip) are units of their own.
//
// One lane owns one packet.  Per packet the kernel does what reference process_packet() does
// (src/worker.c:106-253): control-packet classification (src/worker.c:23-104), the fixed-format
// parse (src/parser.c:6-111), first-match over the priority-sorted rule table
// (src/rule_table.c:76-91,163-176), counters and rule_stats (src/worker.c:119-153), and the
// L3-forward rewrite: TTL / hop-limit decrement, RFC 1071 checksum (src/parser.c:137-169), and the
// next-hop MAC that arp_get_mac / ndp_get_mac would return (src/arp_table.c:55-80,
// src/ndp_table.c:6-17,67-86).  The rewritten header bytes go either to a 16-byte record per
// packet (emit mode, frames only read) or into the frames in place.
//
// Data layout: frames packed back to back at 16-byte aligned starts, one uint64
// descriptor per packet (offset << 16 | len), one uint32 verdict per packet, and in emit mode one
// upe_hdr_rec_t per packet.  A lane loads the first 80 bytes of its frame as 16-byte vector
// loads issued together (chunks past len are not loaded; the batch buffer carries a 96-byte
// tail, so the last frame's window is readable).
//
// Fast path: option-less IPv4 (first byte 0x45, len >= 34) and IPv6 (len >= 54), which covers
// every well-formed packet of the benchmark configurations, is parsed branch-free from those
// registers; everything else (ARP, IPv4 options, truncated or foreign frames) takes the general
// path, entered only by waves that hold such a packet.
//
// The rule table is compiled into structure-of-arrays streams that a wave scans with
// wave-uniform loads (LDS for small tables, the scalar unit otherwise), so rule operands arrive
// in SGPRs; the per-rule work is a few VALU xor / and-or against them, with an early exit as soon
// as every lane of the wave has its first match (ballot).  Large tables go through a tuple-space
// index instead.
//
// One launch per batch, one persistent 1024-thread workgroup per CU (the grid is what a
// residency census finds the chip holds at once).  Workgroup b owns 1024-packet tiles b,
// b + grid, ...; its 16 waves claim the tiles' 64-packet chunks from an LDS counter, so they
// finish together.  A wave loads its next chunk's descriptors as it starts a chunk and (emit
// mode) issues that chunk's window loads halfway through, after the rule match.  Counters, the rule_stats histogram and the L1 bookkeeping accumulate in LDS
// (ballots per chunk) and leave once per workgroup, as one device-atomic instruction per kind,
// into replicated per-batch accumulators.  Nothing waits for anything at the end of a launch:
// the next launch folds this batch's accumulators (lazy fold), the host reads them after a
// synchronisation (upe_l1_sync folds the last one).
//
// Neighbour lookups answer arp_get_mac / ndp_get_mac exactly without walking the reference's
// linear-probe chains: at upload the host keeps only the entries a reference probe can reach
// (probe from the home slot, first valid match before the first invalid slot) and places them
// by three-choice cuckoo hashing; every answer equals the reference's for the snapshot and a
// lookup is three independent LDS reads (indexes of up to 2048 slots are staged) or one memory
// round trip.
//
// The worker's one-entry L1 neighbour caches are sequential state (src/worker.c:186-195,
// 218-225), emulated exactly.  If the starting L1 entry agrees with the
// table (the steady state), every packet's answer is the table's and the only sequential output
// is the final L1 entry: the last table hit, if any packet missed the starting entry and hit the
// table.  If it disagrees (after a table change, or the calloc'd NDP entry for ::), a packet
// whose destination equals the starting entry takes the entry's MAC iff no earlier packet missed
// the entry and hit the table: each 64-packet chunk publishes whether it holds such a packet,
// and a chunk with candidates looks back over the chunks before it (decoupled look-back).
#include <hip/hip_runtime.h>
#include <ctype.h>
#include <pthread.h>
#include <sched.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <atomic>
#include <new>
#include <string>
#include <memory>
#include <vector>

#include "upe_ctx.h"
#include "upe_match.h"
#include "upe_neigh_lookup.h"
#include "upe_parse.h"
#include "upe_plan.h"

using namespace upe;

namespace {

#ifndef UPE_WAVES_PER_SIMD
#define UPE_WAVES_PER_SIMD 4
#endif
constexpr int kWavesPerSimd = UPE_WAVES_PER_SIMD;   // 4 -> VGPR budget 128, 8 -> 64
constexpr int kStatReps = 8;   // replicas of the per-sorted-index rule_stats (summed on the host)
// Claim the next chunk after finishing the current one once this few chunks are unclaimed.
#ifndef UPE_LATE_CLAIM
#define UPE_LATE_CLAIM 16
#endif
constexpr uint32_t kLateClaim = UPE_LATE_CLAIM;
// Issue the next chunk's window loads in the middle of the current chunk (after its rule
// match), so that they fly during the rest of it: bit 0 emit-mode linear-scan kernel, bit 1 also
// the in-place one, bit 2 also the tuple-space ones (config B emit 26.2 -> 25.4 us per 1M batch;
// C unchanged; in place +0.3 % with a VGPR spilled, so off; tuple space: D unchanged, with twice
// the SGPR spills, so off; issued right after the parse instead: B no gain, C 39.0 -> 40.5).
#ifndef UPE_MID_PREFETCH
#define UPE_MID_PREFETCH 1
#endif
constexpr int kReps = 32;              // replicas of the per-batch accumulators
// Cache policy of the emit-mode record store: sc1 (buffer aux 16) writes the records through
// and drops their lines from the XCD's L2, so the end of a launch has ~16 MB less dirty data to
// write back at the kernel boundary (config B 24.5 -> 24.1 us per 1M batch; nt 24.5, sc0 sc1
// 24.2).  The verdict words are written through too (B 24.25 -> 24.1 us); the in-place 16-byte
// header stores are not (written through they were slower: 33.7 -> 35.4 us, partial lines).
constexpr int kRecAux = 16;

// L1 state in word form + whether each entry agrees with the current neighbour snapshot.
// DevState keeps two, by batch parity (see "Sequential state between batches").
struct DevL1 {
    uint32_t arp_ip, arp_mac_lo, arp_mac_hi;
    uint32_t ndp_ip[4];
    uint32_t ndp_mac_lo, ndp_mac_hi;
    uint32_t arp_ok, ndp_ok;
    uint32_t pad[5];
};

// ---- Sequential state between batches ------------------------------------------------------
// Nothing is folded at the end of a launch (no last-workgroup fold, no grid-wide wait): every
// workgroup adds what it saw into replicated accumulators (replica = workgroup % kReps) and the
// NEXT launch, in its first instructions, folds the previous batch's L1 outcome into the state
// it starts from.  Batch k (the context's k-th launch) uses
//   l1[k % 2]       the L1 state after batch k - 2 (read)
//   acc[(k - 1) % 3] batch k - 1's minima / maxima and pay[(k - 1) % 2] its last-hit payloads
//                    (read: every workgroup folds them into its own starting L1 entry)
//   l1[(k + 1) % 2] the state after batch k - 1 (written by workgroup 0, for batch k + 1)
//   acc[k % 3]      this batch's accumulators, pay[k % 2] its payloads (written)
//   acc[(k + 1) % 3] re-armed by workgroup 0 for batch k + 1
// Host calls that read or replace the L1 state first fold the pending batch the same way
// (upe_l1_sync).  Batch k's counters are folded into the cumulative totals by batch k + 1
// (workgroups 0..7, one counter each); rule_stats go straight into replicated per-sorted-index
// totals, which the host sums when it reads them.  No workgroup ever waits for another.
enum { C_PARSED, C_MATCHED, C_FWD, C_DROPPED, C_CONSUMED, C_ARP_LEARN, C_ARP_REPLY, C_CTRL, C_N };
// l1r words, all combined with atomicMax (minima stored as kNone - x, so "none" is 0)
enum { R_F4, R_F6, R_M4, R_M6, R_N };
struct __attribute__((aligned(128))) BatchAcc {
    uint32_t cnt[kReps][C_N];              // this batch's counters
    unsigned long long l1r[kReps][R_N];    // R_F4 / R_F6: kNone - first miss-then-hit index
                                           // v4 / v6; R_M4 / R_M6: last table hit v4 / v6 as
                                           // (index + 1) << 32 | the workgroup holding its payload
    uint32_t ctrl[kReps];                  // kNone - first control packet (max)
    uint32_t grid;                         // the batch's grid
    uint32_t n;                            // the batch's size
    uint32_t pad0[30];
    // look-back give-ups (a launch that started from a disagreeing L1 entry): workgroups that have
    // finished, deferred (chunk, family) entries, and "some wave gave up" (later waves then wait
    // only briefly for an unpublished flag).  A line of their own: the launch polls them.
    uint32_t done, ndefer, giveup;
    uint32_t pad[29];
};
// Payload of a workgroup's last table hit per family; the next batch reads the one the batch
// maximum points at.
struct __attribute__((aligned(64))) TilePay {
    uint32_t m4_dst, m4_mac_lo, m4_mac_hi;
    uint32_t m6_dst[4], m6_mac_lo, m6_mac_hi;
    uint32_t pad[7];
};
constexpr int kPayWords = 9;
// Look-back flags (one word per 64-packet chunk: a wave's share of a tile), written only while
// a starting L1 entry disagrees with the table: launch tag << 6 | bits.  A packet the starting
// entry may answer needs to know whether any earlier packet of its family missed the entry and
// hit the table; its wave looks back over the earlier chunks' flags (decoupled look-back).
enum { LB_FP4 = 1, LB_FP6 = 2, LB_KNOWN4 = 4, LB_INCL4 = 8, LB_KNOWN6 = 16, LB_INCL6 = 32 };
constexpr uint32_t kLbTagMod = 0x3FFFFFFu;   // tags 1 .. kLbTagMod

// Everything a batch reads or writes besides the packets and the tables, in one device
// allocation.  One L1 state slot per 128-byte line.
struct __attribute__((aligned(128))) L1Slot {
    DevL1 s;
};
struct DevState {
    L1Slot l1[2];
    BatchAcc acc[3];
    unsigned long long totals[8];                           // cumulative, upe_counters_t order
    unsigned long long acc_stats[kReps][2 * kSmallRules];   // small tables, per sorted index
    uint32_t census[32];                                     // residency census (census_probe)
    TilePay* pay;                    // [grid]
    uint32_t* lb;                    // look-back flags, one per 64-packet chunk
    unsigned long long* stats;       // [cap][2] worker rule_stats (mid-size and large tables)
    unsigned long long* stats_idx;   // [kStatReps][nrules_pad][2] totals per sorted index
};

// (NeighIndex, the neighbour index a launch looks up in: upe_neigh_lookup.h)
struct Args {
    uint8_t* frames;
    const uint64_t* desc;
    uint32_t* verdict;
    uint32_t n;
    const RuleV4* rv4;
    const RuleV6* rv6;
    const int2* rinfo;
    uint32_t nrules_pad;           // multiple of kUnroll, padding rules never match
    // per-family rule lists of a linear-scan table past the LDS size (FamTable comment)
    const uint4* fam;
    uint32_t fam4, fam6;           // entries per list, multiples of kUnroll
    uint32_t fam6_lds;             // the IPv6 list is staged in LDS (after the neighbour indexes)
    uint32_t fam4_lds;             // (tree kernels) the IPv4 list too, after the IPv6 one
    uint32_t fam_x1idx;            // tables below 8192 rules: each entry's x1 bits 18-30 carry its
                                   // sorted index (no index-array load after a match)
    // decision-tree index over the family lists (kTreeDims comment)
    const uint2* tree;             // nodes, then the leaf entries (u32) from word tree_loff
    uint32_t tree_loff;            // leaf entries' offset in u32 words
    uint32_t tree_lds;             // the image is staged in LDS (uint4 count), 0 = read from memory
    uint32_t port_mac_lo, port_mac_hi, port_ip4;
    NeighIndex arp, ndp;
    DevState* st;
    // tuple-space index (tss != 0): replaces the linear scan for large tables
    const TssGroup* tg4;
    const TssGroup* tg6;
    const uint4* tt4;
    const uint4* tt6;
    const uint4* tfs;              // staged fingerprint image (Args::fp_lds uint4 go to LDS)
    uint32_t ng4, ng6, tss;
    // the context's arrays, passed by value so that no kernel waits on a pointer load
    TilePay* pay;                    // [grid]
    unsigned long long* stats;       // [cap][2]
    unsigned long long* stats_idx;   // [kStatReps][nrules_pad][2]
    uint32_t arp_lds;                // ARP index staged in LDS (slots), 0 = read from memory
    uint32_t ndp_lds;                // NDP index staged in LDS (slots, 2 x uint4 each), 0 = not
    uint32_t fp_lds;                 // staged fingerprints in LDS (uint4 of tfs), 0 = none
    uint32_t* flow_hash;             // optional [n]: flow_hash of each parsed packet (RSS)
    void* gb;                        // optional [n]: what the rule_stats group-by reads beside
                                     // the verdicts (gb_packed: u32 keys, else u16 lengths)
    uint32_t gb_packed;              // 1: gb[i] = matched ? sorted rule index << 16 | len : 0
    uint4* hdr;                      // emit mode: [n] rewritten-header records (upe_hdr_rec_t)
    uint32_t* tx;                    // the egress-list kernels (kTx): group g's forwarded
    uint32_t* tx_cnt;                // packets tx[64g .. 64g + tx_cnt[g])
    uint32_t tx_base;                // the launch's first packet in the caller's batch (a batch
                                     // past kMaxLaunch runs as several launches)
    // this batch's slots of the between-batch state (DevState comment) follow from k6 = k % 6
    // (pointers computed where they are used: the kernel's scalar registers are scarce)
    uint32_t k6;
    uint32_t paycap;                 // a.pay[(k % 2) * paycap + workgroup]
    uint32_t census;                 // non-zero: a residency census launch (census_probe) only
    uint32_t* lb;                    // look-back flags, one per 64-packet chunk
    uint32_t lb_tag;                 // this launch's flag tag
    uint32_t tw;                     // chunks per tile (kWaves; fewer for small batches)
    uint32_t ntiles;                 // tiles of tw chunks
    unsigned long long* agree_out;   // host-mapped: (launch + 1) << 2 | start-state agreement bits
    unsigned long long launch_tag;   // this launch's index + 1
    uint32_t* defer;                 // deferred look-back candidates: (index | family << 31,
                                     // record slot) pairs
    uint32_t lb_spin;                // longest look-back wait, 100 MHz ticks (then defer)
    // ring launch (upe_gpu_process_ring_emit): batches of ring_cpb chunks each; per batch the
    // workgroups that have finished it, and the clock (10 ns) at which the last one did,
    // relative to the first workgroup's start (ring_t0)
    uint32_t ring_cpb, ring_mine;    // chunks per batch, and per batch and workgroup
    uint32_t* ring_wg;
    unsigned long long* ring_done;
    unsigned long long* ring_t0;
};

// (the classify kernel variants, Path / Variant / variant_word: upe_plan.h)

// Batch k's state slots, from Args (DevState comment).
__device__ __forceinline__ const DevL1* l1_in(const Args& a) { return &a.st->l1[a.k6 % 2].s; }
__device__ __forceinline__ DevL1* l1_out(const Args& a) { return &a.st->l1[(a.k6 + 1) % 2].s; }
__device__ __forceinline__ BatchAcc* acc_cur(const Args& a) { return &a.st->acc[a.k6 % 3]; }
__device__ __forceinline__ const BatchAcc* acc_prev(const Args& a) { return &a.st->acc[(a.k6 + 2) % 3]; }
__device__ __forceinline__ BatchAcc* acc_next(const Args& a) { return &a.st->acc[(a.k6 + 1) % 3]; }
__device__ __forceinline__ TilePay* pay_cur(const Args& a) {
    return a.pay + (size_t)(a.k6 % 2) * a.paycap;
}
__device__ __forceinline__ const TilePay* pay_prev(const Args& a) {
    return a.pay + (size_t)((a.k6 + 1) % 2) * a.paycap;
}

// ---- diagnostic timestamps (UPE_STAMPS builds only; never in the product build) ------------
#ifndef UPE_STAMPS
#define UPE_STAMPS 0
#endif
#if UPE_STAMPS
__device__ unsigned long long g_stamps[8192 * 16];
#define STAMP(k)                                                                              \
    do {                                                                                      \
        if (threadIdx.x == 0) {                                                               \
            unsigned long long t_;                                                            \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");  \
            g_stamps[(blockIdx.x + ((a.lb_tag - 1u) % 4u) * 2048u) * 16 + (k)] = t_;                                             \
        }                                                                                     \
    } while (0)
#define STAMP_VM(k)                                                                           \
    do {                                                                                      \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                      \
        STAMP(k);                                                                             \
    } while (0)
// where the workgroup runs: slot 11 = XCC id, slot 12 = HW_ID (CU, SE, ...)
#define STAMP_WHERE()                                                                         \
    do {                                                                                      \
        if (threadIdx.x == 0) {                                                               \
            uint32_t x_, h_;                                                                  \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x_));                 \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(h_));                  \
            g_stamps[(blockIdx.x + ((a.lb_tag - 1u) % 4u) * 2048u) * 16 + 11] = x_;                                              \
            g_stamps[(blockIdx.x + ((a.lb_tag - 1u) % 4u) * 2048u) * 16 + 12] = h_;                                              \
        }                                                                                     \
    } while (0)
#else
#define STAMP_WHERE() do {} while (0)
#define STAMP(k) do {} while (0)
#define STAMP_VM(k) do {} while (0)
#endif

// ---- small helpers ------------------------------------------------------------------------
// Wave-wide reduction (K = 0 sum, 1 min, 2 max): DPP rotations inside each 16-lane row, then the
// four row results through scalar registers (no LDS, no shuffle round trips).
template <int K>
__device__ __forceinline__ uint32_t dpp_op(uint32_t x, uint32_t y) {
    return K == 0 ? x + y : K == 1 ? min(x, y) : max(x, y);
}
template <int K>
__device__ __forceinline__ uint32_t wave_reduce(uint32_t x) {
    x = dpp_op<K>(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xF, 0xF, false));
    x = dpp_op<K>(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x124, 0xF, 0xF, false));
    x = dpp_op<K>(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x122, 0xF, 0xF, false));
    x = dpp_op<K>(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x121, 0xF, 0xF, false));
    const uint32_t r0 = __builtin_amdgcn_readlane(x, 0), r1 = __builtin_amdgcn_readlane(x, 16);
    const uint32_t r2 = __builtin_amdgcn_readlane(x, 32), r3 = __builtin_amdgcn_readlane(x, 48);
    return dpp_op<K>(dpp_op<K>(r0, r1), dpp_op<K>(r2, r3));
}

// (byte_of, at2, be16_lo and len_mask: upe_parse.h)
// RFC 1071 fold of a sum of native-LE u16 words held as a sum of u32 (u32 = lo + hi * 2^16,
// and 2^16 == 1 in one's-complement arithmetic), complemented: src/parser.c:137-169.
__device__ __forceinline__ uint32_t csum_fold(unsigned long long sum) {
    uint32_t f = (uint32_t)(sum & 0xFFFFFFFFull) + (uint32_t)(sum >> 32);
    f += (uint32_t)(sum & 0xFFFFFFFFull) > f ? 1u : 0u;            // end-around carry
    f = (f & 0xFFFFu) + (f >> 16);
    f = (f & 0xFFFFu) + (f >> 16);
    f = (f & 0xFFFFu) + (f >> 16);
    return (~f) & 0xFFFFu;
}
__device__ __forceinline__ void store16(uint4* p, uint4 v) { *p = v; }
// Frame windows and descriptors are plain (cached) loads: non-temporal ones measured slower for
// device batches (C +12 us, B +6.5 us per 1M) and for host-memory batches (config B mapped 537
// vs 666-680 Mpps in place, C 214 vs 319; profiles/r03/v5_host_nt_ab.txt).

// (the neighbour lookups, arp_lookup ... neigh_lookup: upe_neigh_lookup.h, shared with
// upe_neigh.hip)

// Does each L1 entry agree with the table?  (ARP: an entry for 0.0.0.0 is never consulted,
// src/worker.c:186, so it always "agrees".)
__device__ void refresh_ok(DevL1* l1, const NeighIndex& arp, const NeighIndex& ndp) {
    uint32_t lo = 0, hi = 0;
    bool arp_ok = true;
    if (l1->arp_ip != 0)
        arp_ok = arp_lookup(arp, l1->arp_ip, lo, hi) && lo == l1->arp_mac_lo &&
                 hi == l1->arp_mac_hi;
    const uint32_t ip6[4] = {l1->ndp_ip[0], l1->ndp_ip[1], l1->ndp_ip[2], l1->ndp_ip[3]};
    const bool ndp_ok = ndp_lookup(ndp, ip6, lo, hi) && lo == l1->ndp_mac_lo &&
                        hi == l1->ndp_mac_hi;
    l1->arp_ok = arp_ok;
    l1->ndp_ok = ndp_ok;
}

__global__ void upe_refresh(DevL1* l1, NeighIndex arp, NeighIndex ndp) {
    if (threadIdx.x == 0 && blockIdx.x == 0) refresh_ok(l1, arp, ndp);
}

// A write-through (sc1) store: the line leaves this XCD's L2, so a reader on another XCD that
// has not cached it sees the value once the storing wave's stores have drained.
template <typename T>
__device__ __forceinline__ void st_wt(T* p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The L1 state after a batch (src/worker.c:186-195, 218-225): the state
// before it, unless some forwarded packet missed the starting entry and hit the table — then
// the batch's last table hit, whose MAC is the table's (so the entry agrees with the table).
// in: DevL1 words before the batch; f4 / f6: first miss-then-hit (kNone = none); m4 / m6: last
// table hit + 1 (0 = none); wg4 / wg6: the workgroups holding those hits' payloads in pay.
// All arguments wave-uniform.  L: DevL1 words 0..10 after the batch.
__device__ __forceinline__ void fold_l1(const u32x16& in, uint32_t f4, uint32_t f6, uint32_t m4,
                                        uint32_t m6, uint32_t wg4, uint32_t wg6,
                                        const TilePay* pay, uint32_t (&L)[11]) {
#pragma unroll
    for (int j = 0; j < 11; ++j) L[j] = in[j];
    if (f4 != kNone && m4 != 0) {
        const u32x16 P = *as_const<u32x16>(pay + wg4);
        L[0] = P[0]; L[1] = P[1]; L[2] = P[2];
        L[9] = 1;
    }
    if (f6 != kNone && m6 != 0) {
        const u32x16 P = *as_const<u32x16>(pay + wg6);
        L[3] = P[3]; L[4] = P[4]; L[5] = P[5]; L[6] = P[6]; L[7] = P[7]; L[8] = P[8];
        L[10] = 1;
    }
}

// The batch's L1 outcome from its replicated l1r words: lane r < kReps holds replica r (lo/hi
// 32-bit halves of the 64-bit words), the rest zero.  Results wave-uniform.
struct L1Out {
    uint32_t f4, f6, m4, m6, wg4, wg6;
};
__device__ __forceinline__ L1Out reduce_l1r(const unsigned long long (&w)[R_N]) {
    L1Out o;
    o.f4 = kNone - wave_reduce<2>((uint32_t)w[R_F4]);
    o.f6 = kNone - wave_reduce<2>((uint32_t)w[R_F6]);
    const uint32_t h4 = (uint32_t)(w[R_M4] >> 32), h6 = (uint32_t)(w[R_M6] >> 32);
    o.m4 = wave_reduce<2>(h4);
    o.m6 = wave_reduce<2>(h6);
    // one packet index, one workgroup: the lanes holding the maximum agree on it
    o.wg4 = wave_reduce<2>(h4 == o.m4 && o.m4 ? (uint32_t)w[R_M4] : 0u);
    o.wg6 = wave_reduce<2>(h6 == o.m6 && o.m6 ? (uint32_t)w[R_M6] : 0u);
    return o;
}

// Fold a finished batch into the state the next one starts from, on the host's request (before
// the L1 state is read or replaced, or a neighbour table changes): l1 = fold(l1, acc, pay), and
// acc's L1 fields back to "nothing happened", so the next launch's own fold is the identity.
__global__ void upe_l1_sync(DevL1* l1, BatchAcc* acc, const TilePay* pay) {
    const int lane = threadIdx.x;
    unsigned long long w[R_N] = {0, 0, 0, 0};
    if (lane < kReps)
        for (int j = 0; j < R_N; ++j) w[j] = acc->l1r[lane][j];
    const L1Out o = reduce_l1r(w);
    const u32x16 in = *as_const<u32x16>(l1);
    uint32_t L[11];
    fold_l1(in, o.f4, o.f6, o.m4, o.m6, o.wg4, o.wg6, pay, L);
    __syncthreads();
    if (lane < kReps)
        for (int j = 0; j < R_N; ++j) acc->l1r[lane][j] = 0ull;
    if (lane == 0) {
        uint32_t* w = reinterpret_cast<uint32_t*>(l1);
#pragma unroll
        for (int j = 0; j < 11; ++j) w[j] = L[j];
    }
}

// (the rule matchers scan_rules, scan_fam, tree_match and tss_match_both, with vsel, as_const and
// the u32x8 / u32x16 words: upe_match.h, shared with upe_keys.hip)

// ------------------------------------------------------------------------------------------
// General path: every live packet the fast path does not cover (ARP and NDP control frames,
// IPv4 with options, truncated, foreign or malformed frames).  Same outputs as the fast path.
// ------------------------------------------------------------------------------------------
struct Parsed {
    bool ok, consumed, v6;
    uint32_t flags;                // UPE_VF_ARP_LEARN / UPE_VF_ARP_REPLY
    uint32_t proto, sport, dport;
    uint32_t s[4], d[4];
    uint32_t ttl, c1w1, c1w2;      // TTL / hop, and bytes 20..27 as they are forwarded
};

// Inlined (only waves holding such a packet run it).  An out-of-line call (measured in round 2)
// saved the caller's live registers to scratch, ~100 bytes of private-memory traffic per slow
// packet (config D: 1.7 GB written per 16M batch); inlined, the classify kernels run without
// scratch at the 128-VGPR budget.  The path reuses the fast path's window (bytes 0..79, chunks
// at or past len zero) and loads bytes 80..95 only for frames that have them: it reads no byte
// at or past len except the ARP header, which masks them (len_mask), and its ARP reply stores
// bytes 0..47, which the window always holds as loaded.
struct Port {
    uint32_t mac_lo, mac_hi, ip4;
};
template <bool kBarrel>
__device__ __forceinline__ void general_path(Port a, uint8_t* p, uint32_t len, Parsed& r,
                                             const uint32_t (&win)[24]) {
    r.ok = false; r.consumed = false; r.v6 = false; r.flags = 0;
    r.proto = r.sport = r.dport = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) r.s[j] = r.d[j] = 0;
    r.ttl = 0;
    // bytes 0..95 (IPv4 options reach 94): the window, and bytes 80..95 when the frame has them
    uint32_t w[24];
#pragma unroll
    for (int j = 0; j < 24; ++j) w[j] = win[j];
    // Bytes 80..95 matter only to an IPv4 TCP header behind 52 or more bytes of IPv4 header (its
    // data-offset byte is byte 14 + 4 * IHL + 12): loaded here, for such frames only (loading
    // them with every window instead measured no faster for config D, 713 vs 715 us per 16M,
    // and slower for C in place, 57.3 vs 59.0 us: profiles/r04/v3_win6_ab.txt).
    if (len > 80u && (w[3] & 0xFFFFu) == 0x0008u && (byte_of(w[3], 2) & 0xFu) >= 14u &&
        byte_of(w[5], 3) == 6u) {
        const uint4 v = reinterpret_cast<const uint4*>(p)[5];
        w[20] = v.x; w[21] = v.y; w[22] = v.z; w[23] = v.w;
    }
    r.c1w1 = w[5];
    r.c1w2 = w[6];
    // Bytes 12/13 as a zero-filled pktbuf would hold them (the ethertype is read before any
    // length gate, src/worker.c:24-25).
    const uint32_t b12 = len > 12 ? byte_of(w[3], 0) : 0u;
    const uint32_t b13 = len > 13 ? byte_of(w[3], 1) : 0u;
    const uint32_t et = (b12 << 8) | b13;
    const bool is_v4 = et == 0x0800u;
    const bool is_v6 = et == 0x86DDu;
    const uint32_t ihl = byte_of(w[3], 2) & 0xFu;
    r.v6 = is_v6;

    // ---- handle_control_packet, reference src/worker.c:23-104 ----
    if (et == 0x0806u) {
        // The ARP header (bytes 14..41) is read without a length check: bytes at or past len
        // read as zero, as in a zero-filled pktbuf.
        uint32_t z[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) z[j] = w[j] & len_mask(len, j);
        const bool wellformed = (z[3] >> 16) == 0x0100u && z[4] == 0x04060008u;
        if (wellformed) {
            r.flags |= UPE_VF_ARP_LEARN;
            const bool request = (z[5] & 0xFFFFu) == 0x0100u;
            const uint32_t tpa = bswap32(at2(z[10], z[9]));
            if (request && a.ip4 != 0 && tpa == a.ip4) {
                // In-place reply, src/worker.c:42-51, assembled a dword at a time.
                uint32_t nw[12];
                nw[0] = at2(z[2], z[1]);                                  // eth.dst = eth.src
                nw[1] = (z[2] >> 16) | (a.mac_lo << 16);                  // eth.src = port MAC
                nw[2] = (a.mac_lo >> 16) | (a.mac_hi << 16);
                nw[3] = z[3];
                nw[4] = z[4];
                nw[5] = 0x0200u | (a.mac_lo << 16);                       // op = REPLY, sha
                nw[6] = (a.mac_lo >> 16) | (a.mac_hi << 16);
                nw[7] = bswap32(a.ip4);                                   // spa = port IPv4
                nw[8] = at2(z[6], z[5]);                                  // tha = old sha
                nw[9] = (z[6] >> 16) | (z[7] << 16);                      // tpa = old spa
                nw[10] = (z[7] >> 16) | (z[10] & 0xFFFF0000u);
                nw[11] = z[11];
                // bytes at or past len keep the buffer's own (never transmitted) bytes
#pragma unroll
                for (int j = 0; j < 12; ++j) {
                    const uint32_t m = len_mask(len, j);
                    w[j] = (nw[j] & m) | (w[j] & ~m);
                }
                {
                    uint4* q = reinterpret_cast<uint4*>(p);
                    store16(&q[0], make_uint4(w[0], w[1], w[2], w[3]));
                    store16(&q[1], make_uint4(w[4], w[5], w[6], w[7]));
                    store16(&q[2], make_uint4(w[8], w[9], w[10], w[11]));
                }
                r.flags |= UPE_VF_ARP_REPLY;
            }
        }
    }
    if (is_v6 && len >= 78u && byte_of(w[5], 0) == 58u) {               // src/worker.c:58-100
        const uint32_t type = byte_of(w[13], 2);                        // byte 54
        if (type == 135u || type == 136u) r.consumed = true;
    }

    // ---- parse_flow_key, reference src/parser.c:6-111 ----
    if (!r.consumed && len >= 14u) {
        if (is_v4) {
            const uint32_t ver = byte_of(w[3], 2) >> 4;
            const uint32_t hl = ihl * 4;
            if (len - 14 >= 20u && ver == 4 && hl >= 20 && len - 14 >= hl) {
                r.proto = byte_of(w[5], 3);                                  // byte 23
                r.s[0] = bswap32(at2(w[7], w[6]));                           // bytes 26..29
                r.d[0] = bswap32(at2(w[8], w[7]));                           // bytes 30..33
                const uint32_t l4len = len - 14 - hl;
                // the L4 words and x0 = w[ihl + 3] (the checksum's last half word), selected by
                // IHL (l4_select, upe_parse.h; kBarrel picks the selector)
                const L4Words l = l4_select<kBarrel>(w, ihl);
                const uint32_t l4w0 = l.w0, l4w1 = l.w1, l4w3 = l.w3, x0 = l.x0;
                // the L4 gate, a second statement of l4_gate (upe_parse.h), here and for IPv6
                // below: calling l4_gate, in every shape of parameters and result tried, changed
                // the assembly of all upe_classify instantiations (profiles/parse_share_ab.txt)
                if (r.proto == 17u) {
                    r.ok = l4len >= 8u;
                    r.sport = be16_lo(l4w0);
                    r.dport = be16_lo(l4w0 >> 16);
                } else if (r.proto == 6u) {
                    const uint32_t thl = (byte_of(l4w3, 0) >> 4) * 4;
                    r.ok = l4len >= 20u && thl >= 20u && l4len >= thl;
                    r.sport = be16_lo(l4w0);
                    r.dport = be16_lo(l4w0 >> 16);
                } else if (r.proto == 1u) {
                    r.ok = l4len >= 8u;
                    r.sport = be16_lo(l4w1);                                 // icmp id
                    r.dport = be16_lo(l4w0);                                 // type << 8 | code
                }
                // checksum over IHL*4 bytes with the TTL decremented and the field zeroed:
                // sum of u16 words = (w3 >> 16) + w4 + ... + w[2 + ihl] + (w[3 + ihl] & 0xFFFF);
                // words 7..2+ihl as the sum of their 16-bit halves (v_dot2_u32_u16 with a 0/1
                // pair: congruent mod 0xFFFF, which is all the fold needs), w[3 + ihl] = x0
                r.ttl = byte_of(w[5], 2);
                const uint32_t w5n = (w[5] & 0xFF00FFFFu) | (((r.ttl - 1) & 0xFFu) << 16);
                const uint32_t w6z = w[6] & 0xFFFF0000u;
                typedef unsigned short ushort2_t __attribute__((ext_vector_type(2)));
                uint32_t hs = x0 & 0xFFFFu;
#pragma unroll
                for (int k = 7; k <= 17; ++k) {
                    const ushort2_t one = {1, 1}, none = {0, 0};
                    hs = __builtin_amdgcn_udot2(__builtin_bit_cast(ushort2_t, w[k]),
                                                (uint32_t)k <= 2 + ihl ? one : none, hs, false);
                }
                const unsigned long long sum = (w[3] >> 16) + (unsigned long long)w[4] + w5n + w6z + hs;
                r.c1w1 = w5n;
                r.c1w2 = w6z | csum_fold(sum);
            }
        } else if (is_v6 && len - 14 >= 40u) {
            // as the fast path: next header byte 20, addresses 22..53, L4 at byte 54
            // (the L4 gate written out, as for IPv4 above)
            r.proto = byte_of(w[5], 0);
            r.s[0] = at2(w[6], w[5]);   r.s[1] = at2(w[7], w[6]);
            r.s[2] = at2(w[8], w[7]);   r.s[3] = at2(w[9], w[8]);
            r.d[0] = at2(w[10], w[9]);  r.d[1] = at2(w[11], w[10]);
            r.d[2] = at2(w[12], w[11]); r.d[3] = at2(w[13], w[12]);
            const uint32_t l4a = at2(w[14], w[13]), l4b = at2(w[15], w[14]);
            const uint32_t l4c = at2(w[17], w[16]);
            const uint32_t l4len = len - 54u;
            const uint32_t thl = (byte_of(l4c, 0) >> 4) * 4;
            const bool udp = r.proto == 17u, tcp = r.proto == 6u, icmp = r.proto == 1u;
            r.ok = (udp || icmp) ? l4len >= 8u : tcp && l4len >= 20u && thl >= 20u && l4len >= thl;
            r.sport = icmp ? be16_lo(l4b) : be16_lo(l4a);
            r.dport = icmp ? be16_lo(l4a) : be16_lo(l4a >> 16);
            r.ttl = byte_of(w[5], 1);
            r.c1w1 = (w[5] & 0xFFFF00FFu) | (((r.ttl - 1) & 0xFFu) << 8);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Decoupled look-back (only while a starting L1 entry disagrees with the table).  A packet whose
// destination is the starting entry took the entry's MAC in the reference (src/worker.c:186-188,
// 218-220) iff no earlier packet of its family missed the entry and hit the table.  Every chunk
// (a wave's 64 packets of a tile) publishes whether it holds such a packet; a wave holding
// candidates reads the flags of the chunks before it, nearest first, until one holds such a
// packet or one already knows the answer for everything up to it (LB_KNOWN*), waiting for any
// chunk that has not published yet — but only for `spin` ticks of the 100 MHz clock.  The wait
// must be bounded: a chunk it waits for may belong to a workgroup that is not resident (another
// kernel holds CUs, or another context's grid on the same GPU) and can only start once a
// resident one exits.  A wave that gives up defers its candidates (upe_classify: they keep the
// table's answer for now, and the launch's last workgroup repairs them once every chunk has
// published), so no workgroup ever waits on one that has not started.  Returns the families of
// `need` (bit 0 v4, bit 1 v6) still unresolved (0 = all resolved); `got` = for the resolved
// ones, whether an earlier chunk holds a miss-then-hit packet.
// ------------------------------------------------------------------------------------------
__device__ uint32_t lookback(const uint32_t* lb, uint32_t chunk, uint32_t tag, uint32_t need,
                             int lane, uint32_t spin, uint32_t& got) {
    got = 0;
    int64_t base = chunk;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
    while (need && base > 0) {
        const int64_t j = base - 64 + lane;
        uint32_t f = 0;
        bool ready = j < 0;
        for (;;) {
            if (!ready) {
                f = __hip_atomic_load(&lb[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ready = (f >> 6) == tag;
            }
            if (__all(ready)) break;
            if (__builtin_amdgcn_s_memrealtime() - t0 >= spin) return need;   // defer
            __builtin_amdgcn_s_sleep(2);
        }
#pragma unroll
        for (int F = 0; F < 2; ++F) {
            const uint32_t fb = F ? LB_FP6 : LB_FP4;
            const uint32_t kb = F ? LB_KNOWN6 : LB_KNOWN4, ib = F ? LB_INCL6 : LB_INCL4;
            if (!(need & fb)) continue;
            const unsigned long long info = __ballot(j >= 0 && (f & (fb | kb)));
            if (info) {
                const int hl = 63 - __builtin_clzll(info);   // the nearest chunk that knows
                const uint32_t fh = (uint32_t)__shfl((int)f, hl, 64);
                if (fh & (fb | ib)) got |= fb;
                need &= ~fb;
            }
        }
        base -= 64;
    }
    return 0;   // walked to chunk 0: what is still needed has no earlier miss-then-hit packet
}

// The launch's last workgroup (wave 0) answers the candidates that waves deferred: every chunk
// has been processed by now, so every flag word of this launch is written or about to land.  F4 /
// F6 = the first chunk holding a miss-then-hit packet of each family; a deferred candidate of
// chunk c takes the starting entry's MAC iff F >= c (the earlier lanes of its own chunk were
// checked when it deferred).  entries[e] = packet index | family << 31 (1 = IPv6).  Plain
// stores suffice: launches on a context are ordered (no launch of the context starts before this
// one's end-of-kernel writeback), and nothing else in this launch writes these words after the
// deferring wave did.
constexpr int kRepairUnroll = 4;
struct Repair {
    uint32_t mac4_lo, mac4_hi, mac6_lo, mac6_hi;   // the batch's starting L1 entries' MACs
};
template <bool kEmit>
__device__ void repair_deferred(const Args& a, uint32_t nd, int lane, Repair m) {
    const uint32_t nchunks = (a.n + 63u) / 64u;
    uint32_t last = 0;   // the highest chunk with a deferred candidate: F beyond it does not matter
    for (uint32_t e = lane; e < nd; e += 64) last = max(last, (a.defer[2 * e] & 0x7FFFFFFFu) / 64u);
    last = wave_reduce<2>(last);
    uint32_t F4 = kNone, F6 = kNone;
    for (uint32_t b = 0; b <= last && b < nchunks && (F4 == kNone || F6 == kNone); b += 64) {
        const uint32_t j = b + (uint32_t)lane;
        uint32_t f = 0;
        if (j < nchunks && j <= last) {
            do {
                f = __hip_atomic_load(&a.lb[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } while ((f >> 6) != a.lb_tag);
        }
        const unsigned long long b4 = __ballot(f & LB_FP4), b6 = __ballot(f & LB_FP6);
        if (F4 == kNone && b4) F4 = b + (uint32_t)__builtin_ctzll(b4);
        if (F6 == kNone && b6) F6 = b + (uint32_t)__builtin_ctzll(b6);
    }
    const uint32_t w1_4 = m.mac4_hi | (a.port_mac_lo << 16), w1_6 = m.mac6_hi | (a.port_mac_lo << 16);
    const uint32_t w2 = (a.port_mac_lo >> 16) | (a.port_mac_hi << 16);
    // kRepairUnroll entries per lane at a time, their loads issued together (one wave does this)
    constexpr int U = kRepairUnroll;
    for (uint32_t e0 = 0; e0 < nd; e0 += U * 64) {
        uint32_t x[U], v[U], rs[U];
        uint4 q[U];
        bool p[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const uint32_t e = e0 + 64u * k + (uint32_t)lane;
            x[k] = e < nd ? a.defer[2 * e] : kNone;
            rs[k] = e < nd ? a.defer[2 * e + 1] : 0u;   // the record slot (emit mode)
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const uint32_t i = x[k] & 0x7FFFFFFFu;
            const bool v6 = (x[k] >> 31) != 0;
            // an earlier chunk's packet took the table: the provisional answer stands
            p[k] = x[k] != kNone && (v6 ? F6 : F4) >= i / 64u;
            if (p[k]) {
                v[k] = a.verdict[i];
                q[k] = kEmit ? a.hdr[rs[k]]
                             : *reinterpret_cast<const uint4*>(a.frames + ((size_t)(a.desc[i] >> 20) << 4));
            }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (!p[k]) continue;
            const uint32_t i = x[k] & 0x7FFFFFFFu;
            const bool v6 = (x[k] >> 31) != 0;
            a.verdict[i] = v[k] | UPE_VF_NEIGH_HIT;
            const uint4 o = make_uint4(v6 ? m.mac6_lo : m.mac4_lo, v6 ? w1_6 : w1_4, w2, q[k].w);
            if (kEmit)
                a.hdr[rs[k]] = o;
            else
                *reinterpret_cast<uint4*>(a.frames + ((size_t)(a.desc[i] >> 20) << 4)) = o;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Residency census (one launch per kernel configuration, before its first batch): how many
// workgroups of this kernel, with this much dynamic LDS, the chip really holds at once.  The
// occupancy API can answer one workgroup per CU too many (MI355X_MICROARCH.md, "Residency and
// cooperative launch"), and a persistent grid larger than what is resident runs its surplus
// workgroups after the others, doubling the tail.  Each workgroup arrives on w[0] and waits (at
// most ~60 us) for the whole grid; a workgroup that gives up records how many had arrived
// when it gave up (w[1], min).  Resident workgroups all arrive within a few microseconds of
// the first one and give up together, seeing every resident arrival and no other (the rest
// can only start once a resident one has exited); nobody gives up when the whole grid is
// resident.
// ------------------------------------------------------------------------------------------
__device__ void census_probe(uint32_t* w, uint32_t grid) {
    uint32_t v = __hip_atomic_fetch_add(&w[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
    while (v < grid) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > 6000) {
            v = __hip_atomic_load(&w[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(&w[1], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        __builtin_amdgcn_s_sleep(8);
        v = __hip_atomic_load(&w[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------------------------------
// classify: persistent workgroups over 256-packet tiles
// ------------------------------------------------------------------------------------------
// kEmit: the rewritten header bytes of forwarded packets go to a record per packet (a.hdr,
// upe_hdr_rec_t, one coalesced 16-byte store per lane) and the frames are only read; otherwise
// frames are rewritten in place (bytes 0..31 of each forwarded frame).
// kLean: the launch has no flow_hash output, every non-empty neighbour index staged in LDS and
// (linear scan) no length side array, so those paths are not compiled in (fewer live kernel
// arguments: config B/C emit kernels spill 70 SGPRs instead of 96, ~1 % faster).
// kNoLB (lean only): chosen once the host has seen a launch start from L1 entries that agree with
// the tables (agreement then holds until the host changes the tables or the L1 state) or whose
// family's index is empty; the look-back is not compiled in, and an entry that disagrees with an
// empty index answers its candidates itself (no packet can hit that table first).
// kPath (Path above): Tx (emit only) the egress-list kernels (kTx, upe_gpu_process_emit_tx); Ring
// (lean emit only) a ring launch — a batch of a.ring_cpb chunks completes when every workgroup
// owning part of it has finished its chunks of it; the last one stamps the time; Host the same
// code as Device under a name of its own.
template <bool kTssMode, bool kEmit, bool kLean, bool kNoLB, Path kPath, int kScan>
__global__ void __launch_bounds__(kBlock, kWavesPerSimd) upe_classify(Args a) {
    // rule match of a linear-scan table (kScan; the host picks the instantiation, so no kernel
    // carries another flavour's code): 0 small table from its LDS copy, 1 family lists, 2 whole
    // table through the scalar unit, 3 decision tree over the family lists
    constexpr bool kFam = kScan == 1, kGlb = kScan == 2, kTree = kScan == 3;
    constexpr bool kTx = kPath == Path::Tx;       // the egress list (see above)
    constexpr bool kRingL = kPath == Path::Ring;  // a ring launch
    constexpr bool kFamIdx = kFam || kTree;   // the match is a FamTable index-array entry
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_hist[]; // [nrules_pad][2]
    // per wave: 8 counters, first f4 / f6 / ctrl, last m4 / m6
    __shared__ uint32_t s_tot[C_N + 3];   // the workgroup's counters; first f4 / f6 / ctrl (min)
    __shared__ uint32_t s_wm[kWaves][2];  // per wave: its last table hit per family (index + 1)
    __shared__ uint32_t s_pay[kWaves][kPayWords];   // ... and that hit's (ip, MAC)
    __shared__ u32x8 s_rv4[kTssMode || kScan ? 1 : kSmallRules];   // small tables: RuleV4 / RuleV6
    __shared__ u32x16 s_rv6[kTssMode || kScan ? 1 : kSmallRules];  // words (only kScan 0 has them)
    __shared__ uint32_t s_claim;   // the workgroup's next unclaimed chunk (workgroup-local index)
    __shared__ uint32_t s_bdone[kRingL ? kRingMax : 1];   // ring: the workgroup's chunks done per batch

    if (a.census) {
        if (threadIdx.x == 0) census_probe(a.st->census, gridDim.x);
        return;
    }
    STAMP(0);
    STAMP_WHERE();
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const bool lds_stats = a.nrules_pad <= (uint32_t)kLdsStatsMax;
    // (kGlb is chosen when a family's list is a single catch-all: there the family split
    // measured slower, config C 39.8 vs 41.9 us)
    const bool small_stats = kScan == 0 && a.nrules_pad <= (uint32_t)kSmallRules;

    if (lds_stats)
        for (uint32_t r = tid; r < 2 * a.nrules_pad; r += kBlock) lds_hist[r] = 0;

    // The next chunk's window issued in the middle of the current chunk (after its rule match),
    // so that its loads fly during the rest of it: into named registers carried into the next
    // iteration (not an array the compiler might place in scratch).  Only the linear-scan
    // kernels: the tuple-space ones have no registers to spare.
    constexpr bool kMid = (UPE_MID_PREFETCH & 1) && (!kTssMode || (UPE_MID_PREFETCH & 4)) &&
                          (kEmit || (UPE_MID_PREFETCH & 2));
    // ---- header window: bytes 0..79 as 16-byte loads issued together.  Chunks at or past len
    // are not loaded (they read as zero, as in a zero-filled pktbuf): a 64-byte frame costs
    // four loads, not five.  Frames shorter than 49 bytes never take the fast path.
    auto load_window = [&](uint64_t dsc, bool live, uint32_t (&w)[24]) {
#pragma unroll
        for (int j = 0; j < 24; ++j) w[j] = 0;
        if (live) {
            const uint32_t len = (uint32_t)(dsc & 0xFFFFu);
            const uint4* q = reinterpret_cast<const uint4*>(a.frames + ((size_t)(dsc >> 20) << 4));
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                if (c < 3 || len > 16u * c) {
                    const uint4 v = q[c];
                    w[4 * c + 0] = v.x; w[4 * c + 1] = v.y; w[4 * c + 2] = v.z; w[4 * c + 3] = v.w;
                }
            }
        }
    };
    struct Win { uint4 c0, c1, c2, c3, c4; };
    auto fetch_window = [&](uint64_t dsc, bool live) -> Win {
        const uint4 z = make_uint4(0, 0, 0, 0);
        Win v{z, z, z, z, z};
        if (live) {
            const uint32_t len = (uint32_t)(dsc & 0xFFFFu);
            const uint4* q = reinterpret_cast<const uint4*>(a.frames + ((size_t)(dsc >> 20) << 4));
            v.c0 = q[0]; v.c1 = q[1]; v.c2 = q[2];
            if (len > 48u) v.c3 = q[3];
            if (len > 64u) v.c4 = q[4];
        }
        return v;
    };
    Win nw;
    bool have_nw = false;   // nw holds the window of the wave's next chunk
    // Work: the workgroup owns tiles blockIdx, blockIdx + grid, ... (one per CU at a time, so a
    // CU's tiles are one workgroup's), and each wave takes 64-packet chunks of them in order:
    // workgroup-local chunk k is chunk k % kWaves of the workgroup's tile k / kWaves.  Waves
    // claim k from an LDS counter, so the workgroup's waves finish together however unevenly
    // the CU schedules them (with several workgroups per CU and static tiles, the last one to
    // finish ran alone for ~4 us after the first: the CU favours older waves).  Global chunk
    // numbers ascend with k, and a wave's claims ascend.
    auto chunk_of = [&](uint32_t k) -> uint32_t {
        const uint32_t t = blockIdx.x + (k / a.tw) * gridDim.x;
        const uint32_t c = t * a.tw + k % a.tw;
        return t < a.ntiles && c * 64u < a.n ? c : kNone;
    };
    if (tid == 0) s_claim = kWaves;
    if (kRingL)
        for (uint32_t k = tid; k < (uint32_t)kRingMax; k += kBlock) s_bdone[k] = 0u;
    if (kRingL && tid == 0)   // the ring's time origin: the first workgroup to start
        __hip_atomic_fetch_min(a.ring_t0, (unsigned long long)__builtin_amdgcn_s_memrealtime(),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < C_N + 3) s_tot[tid] = tid < C_N ? 0u : kNone;
    if (tid < 2 * kWaves) s_wm[tid / 2][tid % 2] = 0u;
    uint32_t ch = chunk_of((uint32_t)wave);   // this wave's chunk
    // The first descriptor (its round trip runs under the table staging below), then small
    // rule tables into LDS, before the entry barrier.  (Issuing the first chunk's window loads
    // here too queues the staging loads behind them: B 26.3 -> 27.6 us, C 40.1 -> 43.8 us.)
    uint64_t dsc_next = 0;
    if (ch != kNone && ch * 64u + (uint32_t)lane < a.n) dsc_next = a.desc[ch * 64u + lane];
    if (!kTssMode && small_stats) {
        // small tables: the whole table
        const uint32_t nst = a.nrules_pad;
        const uint4* g4 = reinterpret_cast<const uint4*>(a.rv4);
        const uint4* g6 = reinterpret_cast<const uint4*>(a.rv6);
        uint4* d4 = reinterpret_cast<uint4*>(s_rv4);
        uint4* d6 = reinterpret_cast<uint4*>(s_rv6);
        for (uint32_t k = tid; k < 2 * nst; k += kBlock) d4[k] = g4[k];
        for (uint32_t k = tid; k < 4 * nst; k += kBlock) d6[k] = g6[k];
    }
    // The starting L1 entries: the state after batch k - 2 (one scalar load) with batch k - 1's
    // outcome folded in (its replicated minima / maxima, then at most two payload loads).
    // DevL1 words: arp_ip, arp_mac_lo/hi, ndp_ip[4], ndp_mac_lo/hi, arp_ok, ndp_ok.
    static_assert(sizeof(DevL1) == 64, "DevL1 is one scalar load");
    const u32x16 lin = *as_const<u32x16>(l1_in(a));
    unsigned long long pr[R_N] = {0, 0, 0, 0};
    if (lane < kReps)
        for (int j = 0; j < R_N; ++j) pr[j] = acc_prev(a)->l1r[lane][j];
    // small neighbour indexes into LDS after the rule-stats bins: a lookup is then an LDS read,
    // not a memory round trip queued behind the batch's frame traffic
    uint4* s_arp = reinterpret_cast<uint4*>(lds_hist + (lds_stats ? 2 * a.nrules_pad : 0u));
    uint4* s_ndp = s_arp + a.arp_lds;
    for (uint32_t k = tid; k < a.arp_lds; k += kBlock) s_arp[k] = a.arp.t[k];
    for (uint32_t k = tid; k < 2 * a.ndp_lds; k += kBlock) s_ndp[k] = a.ndp.t[k];
    uint4* s_fp4 = s_ndp + 2 * a.ndp_lds;
    if (kTssMode)
        for (uint32_t k = tid; k < a.fp_lds; k += kBlock) s_fp4[k] = a.tfs[k];
    // the decision tree's image, when the host found room for it
    uint4* s_tree = s_fp4;
    if (kTree) {
        const uint4* g = reinterpret_cast<const uint4*>(a.tree);
        for (uint32_t k = tid; k < a.tree_lds; k += kBlock) s_tree[k] = g[k];
    }
    // linear-scan tables past kSmallRules: the IPv6 family list, when the host found room
    // (staging the lists' sorted indexes as well measured slower: config C 41.6 -> 42.7 us)
    uint4* s_fam6 = s_fp4 + (kTree ? a.tree_lds : 0u);
    if (kFamIdx && a.fam6_lds) {
        const uint4* g = a.fam + 2 * (size_t)a.fam4;
        for (uint32_t k = tid; k < kFamV6Stride * a.fam6; k += kBlock) s_fam6[k] = g[k];
    }
    // (tree kernels) the IPv4 list as well, for the leaves' rule tests
    uint4* s_fam4 = s_fam6 + (a.fam6_lds ? kFamV6Stride * a.fam6 : 0u);
    if (kTree && a.fam4_lds)
        for (uint32_t k = tid; k < 2 * a.fam4; k += kBlock) s_fam4[k] = a.fam[k];
    const uint16_t* s_fps = kTssMode && a.fp_lds ? reinterpret_cast<const uint16_t*>(s_fp4) : nullptr;
    __syncthreads();
    STAMP(1);
    // The fold itself waits on those loads (and then on at most two payload loads), so it runs
    // after the first tile's frame loads are issued (or after the loop if there is no tile),
    // off the path to the first frames.
    uint32_t L1[11];
    bool look4 = false, look6 = false, folded = false;
    // Bookkeeping between batches, done by wave 0 of workgroups 0..7 before its first chunk (so
    // that it is off the end of the launch: their other waves take more chunks meanwhile).
    // Nothing else in this launch touches what it writes.
    auto books = [&]() {
        // batch k - 1's counters into the cumulative totals (upe_counters_t order): total j by
        // workgroup j % grid (j = 0 the batch size, pkts_in; j >= 1 counter j - 1)
        if (blockIdx.x < 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if ((uint32_t)j % gridDim.x != blockIdx.x) continue;
                const uint32_t v =
                    j == 0 ? __builtin_amdgcn_readfirstlane(__hip_atomic_load(
                                 &acc_prev(a)->n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                           : wave_reduce<0>(lane < kReps ? __hip_atomic_load(&acc_prev(a)->cnt[lane][j - 1],
                                                                             __ATOMIC_RELAXED,
                                                                             __HIP_MEMORY_SCOPE_AGENT)
                                                         : 0u);
                if (lane == 0 && v) atomicAdd(&a.st->totals[j], (unsigned long long)v);
            }
        }
        if (blockIdx.x == 0) {
            // workgroup 0: this batch's grid and size, batch k + 1's accumulators re-armed
            // (batch k - 2's, folded by batch k - 1)
            if (lane == 0) {
                st_wt(&acc_cur(a)->grid, gridDim.x);
                st_wt(&acc_cur(a)->n, a.n);
            }
            uint32_t* nc = &acc_next(a)->cnt[0][0];
            unsigned long long* nr = &acc_next(a)->l1r[0][0];
            for (uint32_t k = lane; k < (uint32_t)(kReps * C_N); k += 64) st_wt(&nc[k], 0u);
            for (uint32_t k = lane; k < (uint32_t)(kReps * R_N); k += 64) st_wt(&nr[k], 0ull);
            if (lane < kReps) st_wt(&acc_next(a)->ctrl[lane], 0u);
            if (lane < 3) st_wt(&(&acc_next(a)->done)[lane], 0u);   // done, ndefer, giveup
        }
    };
    auto fold_start = [&]() {
        const L1Out o = reduce_l1r(pr);
        fold_l1(lin, o.f4, o.f6, o.m4, o.m6, o.wg4, o.wg6, pay_prev(a), L1);
        look4 = L1[9] == 0u;    // the ARP entry disagrees with the table
        look6 = L1[10] == 0u;   // the NDP entry disagrees with the table
        folded = true;
    };
    if (wave == 0 && blockIdx.x < 8) books();

    // Persistent workgroups: the grid is what the chip holds at once, so the per-workgroup
    // flush happens once per workgroup, at the very end of its life.  (Per-wave claims from
    // device-scope counters shared by many workgroups cost 2.5 us per 1M batch: every claim
    // serialised on a few hot lines; the LDS counter is private to the workgroup.)
    // Descriptors run one chunk ahead of the frames they point at.
    // The workgroup's number of chunks: a wave claims its next chunk one ahead (so that its
    // descriptors arrive while it works) only while more than kLateClaim chunks are unclaimed;
    // after that it claims when it has finished its chunk, so that near the end no wave holds
    // an unstarted chunk while another waits with nothing.
    uint32_t nloc = 0;
    if (blockIdx.x < a.ntiles) {
        const uint32_t own = (a.ntiles - 1u - blockIdx.x) / gridDim.x + 1u;
        const uint32_t tl = blockIdx.x + (own - 1u) * gridDim.x;
        const uint32_t lc = min(a.tw, (a.n - tl * a.tw * 64u + 63u) / 64u);
        nloc = (own - 1u) * a.tw + lc;
    }
    auto claim = [&]() {
        uint32_t kn = 0;
        if (lane == 0) kn = atomicAdd(&s_claim, 1u);
        return chunk_of(__builtin_amdgcn_readfirstlane(kn));
    };
    uint32_t chn = kNone;   // this wave's next chunk
    // The descriptors a wave loads are consumed where they were loaded (this one, and the late
    // claim's at the end of the loop body), so that no descriptor is still pending at the loop
    // header: the wait for it would be a vmcnt(0) every iteration shares, which also waits for
    // the previous chunk's stores.
    asm volatile("" : "+v"(dsc_next));
    for (bool first = true; ch != kNone; first = false, ch = chn) {
        bool late;
        {
            uint32_t cur = 0;
            if (lane == 0)
                cur = __hip_atomic_load(&s_claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            late = __builtin_amdgcn_readfirstlane(cur) + kLateClaim >= nloc;
            chn = late ? kNone : claim();
        }
        const uint32_t i = ch * 64u + (uint32_t)lane;
        const bool live = i < a.n;
        const uint64_t dsc = dsc_next;
        const uint32_t len = (uint32_t)(dsc & 0xFFFFu);
        // frames are 16-byte aligned: the offset in 16-byte units fits one register
        const uint32_t off16 = (uint32_t)(dsc >> 20);
        uint8_t* p = a.frames + ((size_t)off16 << 4);
        uint32_t w[24];
        if (kMid && have_nw) {
            const uint4 c[5] = {nw.c0, nw.c1, nw.c2, nw.c3, nw.c4};
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                w[4 * j + 0] = c[j].x; w[4 * j + 1] = c[j].y; w[4 * j + 2] = c[j].z; w[4 * j + 3] = c[j].w;
            }
            w[20] = w[21] = w[22] = w[23] = 0;
        } else {
            load_window(dsc, live, w);
        }
        have_nw = false;
        dsc_next = 0;
        if (chn != kNone && chn * 64u + (uint32_t)lane < a.n) dsc_next = a.desc[chn * 64u + lane];
        if (!folded) fold_start();

        if (first) STAMP_VM(2);
        // ---- fast path (option-less IPv4 / IPv6) or general path, chosen per wave ----
        // (the fast path specialises parse_key, upe_parse.h, for the two shapes it takes)
        const uint32_t e12 = w[3] & 0xFFFFu;          // bytes 12,13 (ethertype, byte-swapped)
        const bool fast4 = live && len >= 34u && e12 == 0x0008u && byte_of(w[3], 2) == 0x45u;
        const bool fast6 = live && len >= 54u && e12 == 0xDD86u;
        const bool slow = live && !fast4 && !fast6;
        Parsed r;
        // Tuple-space kernels (large tables): a wave holding any other frame parses all 64 on
        // the general path, which gives the fast path's results for the fast path's frames — one
        // parse per wave instead of both (config D: IPv4 options, VLAN tags and malformed headers
        // put such a frame in nearly every wave; classify 651 -> 641 us per 16M).  The scan
        // kernels keep the fast path for every wave and the general path for the lanes that need
        // it: there the merged form costs registers (C's emit kernel spilled 12 VGPRs to scratch,
        // 39.9 -> 44.3 us; B 24.7 -> 25.1; profiles/r04/v4_wave_general_ab.txt).
        constexpr bool kWaveGeneral = kTssMode;
        const bool wave_general = kWaveGeneral && __any(slow);
        if (wave_general) {
            general_path<kTssMode>(Port{a.port_mac_lo, a.port_mac_hi, a.port_ip4}, p, len, r, w);
        } else {
            r.ok = false; r.consumed = false; r.v6 = fast6; r.flags = 0;
            r.proto = fast6 ? byte_of(w[5], 0) : byte_of(w[5], 3);              // byte 20 / 23
            // addresses: v4 host order in word 0 (src/parser.c:40-41); v6 wire bytes
            r.s[0] = fast6 ? at2(w[6], w[5]) : bswap32(at2(w[7], w[6]));
            r.d[0] = fast6 ? at2(w[10], w[9]) : bswap32(at2(w[8], w[7]));
            r.s[1] = at2(w[7], w[6]);  r.s[2] = at2(w[8], w[7]);  r.s[3] = at2(w[9], w[8]);
            r.d[1] = at2(w[11], w[10]); r.d[2] = at2(w[12], w[11]); r.d[3] = at2(w[13], w[12]);
            {
                // L4 at byte 34 (v4) or 54 (v6), both 2 mod 4
                const uint32_t l4a = fast6 ? at2(w[14], w[13]) : at2(w[9], w[8]);     // L4 0..3
                const uint32_t l4b = fast6 ? at2(w[15], w[14]) : at2(w[10], w[9]);    // L4 4..7
                const uint32_t l4c = fast6 ? at2(w[17], w[16]) : at2(w[12], w[11]);   // L4 12..15
                const uint32_t l4len = len - (fast6 ? 54u : 34u);
                const uint32_t thl = (byte_of(l4c, 0) >> 4) * 4;
                const bool udp = r.proto == 17u, tcp = r.proto == 6u, icmp = r.proto == 1u;
                r.ok = (fast4 || fast6) &&
                       ((udp || icmp) ? l4len >= 8u
                                      : tcp && l4len >= 20u && thl >= 20u && l4len >= thl);
                r.sport = icmp ? be16_lo(l4b) : be16_lo(l4a);                  // icmp: id
                r.dport = icmp ? be16_lo(l4a) : be16_lo(l4a >> 16);            // type << 8 | code
                // NDP NS / NA, consumed by handle_control_packet (src/worker.c:57-100)
                r.consumed = fast6 && len >= 78u && r.proto == 58u &&
                             ((l4a & 0xFFu) == 135u || (l4a & 0xFFu) == 136u);
            }
            // forward rewrite of bytes 20..27: v4 ttl-- and checksum over the 20-byte header
            // (src/worker.c:174-176, src/parser.c:137-169, stored LE), v6 hop-- (src/worker.c:213)
            r.ttl = fast6 ? byte_of(w[5], 1) : byte_of(w[5], 2);               // byte 21 / 22
            if (fast6) {
                r.c1w1 = (w[5] & 0xFFFF00FFu) | (((r.ttl - 1) & 0xFFu) << 8);
                r.c1w2 = w[6];
            } else {
                const uint32_t w5n = (w[5] & 0xFF00FFFFu) | (((r.ttl - 1) & 0xFFu) << 16);
                const uint32_t w6z = w[6] & 0xFFFF0000u;
                const unsigned long long sum = (unsigned long long)(w[3] >> 16) + w[4] + w5n + w6z +
                                               w[7] + (w[8] & 0xFFFFu);
                r.c1w1 = w5n;
                r.c1w2 = w6z | csum_fold(sum);
            }

        }
        if (!kWaveGeneral && __any(slow) && slow) {
            Parsed g;
            general_path<kTssMode>(Port{a.port_mac_lo, a.port_mac_hi, a.port_ip4}, p, len, g, w);
            r = g;
        }

        const bool ctrl = live && (r.consumed || (r.flags & UPE_VF_ARP_LEARN));
        const bool ok = live && r.ok && !r.consumed;

        // ---- next hop, looked up before the rule scan: it needs only the destination, so its
        // latency hides behind the scan (the answer is unused unless the packet is forwarded) ----
        uint32_t mlo = 0, mhi = 0;
        bool nhit = false;
        if (ok && r.ttl > 1u) {
            if (!r.v6 && a.arp_lds)
                nhit = arp_lookup_lds(s_arp, a.arp.bits, a.arp.seed, r.d[0], mlo, mhi);
            else if (r.v6 && a.ndp_lds)
                nhit = ndp_lookup_lds(s_ndp, a.ndp.bits, a.ndp.seed, r.d, mlo, mhi);
            else if (!kLean)
                nhit = neigh_lookup(a.arp, a.ndp, r.v6, r.d, mlo, mhi);
        }

        // ---- rule_table_match ----
        const uint32_t k0 = key_k0(r.v6, r.proto, r.sport);   // (upe_match.h)
        const uint32_t k1 = key_k1(r.dport);
        const bool need_v6 = __any(ok && r.v6);
        uint32_t ri, act = 0;   // act: the matched rule's x1 word (action code in bits 16-17)
        if (kTssMode) {
            ri = tss_match_both(a, ok, r.v6, k0, k1, r.s, r.d, act, s_fps);
        } else {
            // small tables from their LDS copy, larger ones through the scalar unit
            const uint32_t nr = a.nrules_pad;
            if (kTree)
                ri = a.tree_lds ? tree_match<true>(a, ok, r.v6, k0, k1, r.s, r.d, act,
                                                   reinterpret_cast<const uint2*>(s_tree), s_fam6,
                                                   s_fam4)
                                : tree_match<false>(a, ok, r.v6, k0, k1, r.s, r.d, act, nullptr,
                                                    s_fam6, s_fam4);
            else if (kFam)
                ri = need_v6 ? scan_fam<true>(a, !ok, r.v6, k0, k1, r.s, r.d, act, s_fam6)
                             : scan_fam<false>(a, !ok, r.v6, k0, k1, r.s, r.d, act, s_fam6);
            else if (kGlb)
                ri = need_v6 ? scan_rules<true, false>(a, !ok, r.v6, k0, k1, r.s, r.d, act, s_rv4, s_rv6, 0u, nr)
                             : scan_rules<false, false>(a, !ok, r.v6, k0, k1, r.s, r.d, act, s_rv4, s_rv6, 0u, nr);
            else
                ri = need_v6 ? scan_rules<true, true>(a, !ok, r.v6, k0, k1, r.s, r.d, act, s_rv4, s_rv6, 0u, nr)
                             : scan_rules<false, true>(a, !ok, r.v6, k0, k1, r.s, r.d, act, s_rv4, s_rv6, 0u, nr);
        }
        // kFam: ri is the lane's entry in the FamTable index array; the sorted index it holds is
        // loaded now and first used at the verdict store
        uint32_t rsi = ri;
        if (kFamIdx && ri != kNone) rsi = fam_sorted_index(a, ri, act);   // (upe_match.h)

        // ---- verdict, counters, rule_stats (src/worker.c:117-153) ----
        uint32_t code = 0, rbits = 0;
        if (r.consumed) {
            code = UPE_V_CONSUMED;
        } else if (!ok) {
            code = UPE_V_DROP_PARSE;
        } else if (ri == kNone) {
            code = UPE_V_DROP_NOMATCH;
        } else {
            const uint32_t ac = (act >> 16) & 3u;
            if (!kFamIdx) rbits = (ri + 1) << 8;
            // rule_stats[rule_id] += {1, len}, src/worker.c:141-144: an LDS histogram below for
            // LDS-resident tables; for larger ones upe_rule_hist folds the verdict words after
            // the launch (one scattered device atomic per packet would cost more than the
            // whole classification)
            code = ac == 0u ? UPE_V_DROP_RULE : ac == 1u ? UPE_V_FWD : UPE_V_DROP_ACTION;
        }
        uint32_t flags = r.flags;
        if (first) STAMP_VM(3);
        // the next chunk's window (its descriptor has been back since early in this chunk):
        // issued here, it arrives while this chunk finishes
        if (kMid && chn != kNone) {
            nw = fetch_window(dsc_next, chn * 64u + (uint32_t)lane < a.n);
            have_nw = true;
        }

        // ---- L3 forward (src/worker.c:155-244) ----
        bool fp4 = false, fp6 = false;       // this packet misses the start entry, hits table
        bool thit4 = false, thit6 = false;   // the table answered this packet
        bool hit = false;      // the packet gets a MAC: the table's (or the starting entry's)
        bool cand = false;     // destination == starting L1 entry (ARP: and != 0)
        bool wrote1 = false;
        bool deferred = false;   // this wave deferred candidates (wave-uniform)
        if (code == UPE_V_FWD) {
            if (r.ttl <= 1u) {                         // src/worker.c:165-172, 204-211
                code = UPE_V_DROP_TTL;
            } else if (!r.v6) {
                wrote1 = true;
                hit = nhit;
                cand = L1[0] != 0 && r.d[0] == L1[0];
                fp4 = !cand && hit;
                thit4 = hit;
            } else {
                wrote1 = true;
                hit = nhit;
                cand = r.d[0] == L1[3] && r.d[1] == L1[4] && r.d[2] == L1[5] &&
                       r.d[3] == L1[6];
                fp6 = !cand && hit;
                thit6 = hit;
            }
            if (cand) flags |= UPE_VF_L1_INIT;
        }
        // emit mode: a record for each forwarded packet only, compacted per 64-packet group in
        // packet order (the wave's chunk is one group): a ballot and a lane count give its slot,
        // 64 * (i / 64) + the forwarded packets before it in the group.  No record is written for
        // the other packets (config B: 7.5 MB of zero records per 1M batch before round 5).
        uint32_t rslot = 0;
        if (kEmit) {
            const unsigned long long fm = __ballot(live && code == UPE_V_FWD);
            rslot = ch * 64u + __builtin_amdgcn_mbcnt_hi((uint32_t)(fm >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)fm, 0u));
        }
        if (kNoLB) {
            // a disagreeing entry here belongs to a family whose index is empty
            if (cand && (r.v6 ? look6 : look4)) {
                hit = true;
                mlo = r.v6 ? L1[7] : L1[1];
                mhi = r.v6 ? L1[8] : L1[2];
            }
        } else if (look4 || look6) {
            // The starting entry disagrees with the table: publish this chunk's miss-then-hit
            // packets, and give the packets aimed at the entry the entry's MAC unless an earlier
            // packet of their family missed it and hit the table (lookback).
            const uint32_t chunk = ch;
            const unsigned long long b4 = __ballot(fp4), b6 = __ballot(fp6);
            const uint32_t fpb = (b4 ? (uint32_t)LB_FP4 : 0u) | (b6 ? (uint32_t)LB_FP6 : 0u);
            const uint32_t tag = a.lb_tag << 6;
            if (lane == 0)
                __hip_atomic_store(&a.lb[chunk], tag | fpb, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            const bool c4 = cand && !r.v6 && look4, c6 = cand && r.v6 && look6;
            const uint32_t need = (__ballot(c4) ? (uint32_t)LB_FP4 : 0u) |
                                  (__ballot(c6) ? (uint32_t)LB_FP6 : 0u);
            if (need) {
                // once any wave of the launch has given up, wait only briefly (1/16 of the bound)
                // for an unpublished flag: the workgroup it belongs to is likely not resident,
                // but a short wait still resolves the flags that are merely in flight, so that
                // the give-up does not cascade into a long serial repair
                const uint32_t spin = __hip_atomic_load(&acc_cur(a)->giveup, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT) ? a.lb_spin / 16u : a.lb_spin;
                uint32_t before = 0;
                const uint32_t left = lookback(a.lb, chunk, a.lb_tag, need, lane, spin, before);
                const unsigned long long lt = (1ull << lane) - 1ull;
                const bool prior4 = (before & LB_FP4) || (b4 & lt);
                const bool prior6 = (before & LB_FP6) || (b6 & lt);
                const bool r4 = c4 && !(left & LB_FP4), r6 = c6 && !(left & LB_FP6);
                if ((r4 && !prior4) || (r6 && !prior6)) {
                    hit = true;
                    mlo = r.v6 ? L1[7] : L1[1];
                    mhi = r.v6 ? L1[8] : L1[2];
                }
                // what this chunk now knows about everything up to it (resolved families only)
                const uint32_t res = need & ~left;
                uint32_t kn = 0;
                if (res & LB_FP4)
                    kn |= LB_KNOWN4 | (((before & LB_FP4) || b4) ? (uint32_t)LB_INCL4 : 0u);
                if (res & LB_FP6)
                    kn |= LB_KNOWN6 | (((before & LB_FP6) || b6) ? (uint32_t)LB_INCL6 : 0u);
                if (lane == 0 && kn)
                    __hip_atomic_store(&a.lb[chunk], tag | fpb | kn, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                if (left) {
                    // Gave up: the candidates an earlier packet of this chunk does not answer keep
                    // the table's answer for now and list themselves (index | family << 31); the
                    // launch's last workgroup repairs them (repair_deferred) once every chunk has
                    // published.
                    const bool dl = (c4 && (left & LB_FP4) && !(b4 & lt)) ||
                                    (c6 && (left & LB_FP6) && !(b6 & lt));
                    const unsigned long long dm = __ballot(dl);
                    uint32_t base = 0;
                    if (lane == 0) {
                        __hip_atomic_store(&acc_cur(a)->giveup, 1u, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                        if (dm) base = atomicAdd(&acc_cur(a)->ndefer, (uint32_t)__popcll(dm));
                    }
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (dl) {   // (index | family, and the packet's record slot in emit mode)
                        const uint32_t e = base + (uint32_t)__popcll(dm & lt);
                        a.defer[2 * e] = i | (r.v6 ? 0x80000000u : 0u);
                        a.defer[2 * e + 1] = rslot;
                    }
                    deferred = dm != 0;
                }
            }
        }
        if (hit) flags |= UPE_VF_NEIGH_HIT;

        // ---- write back ----
        if (kEmit && live && code == UPE_V_FWD) {
            // record: bytes 0..11 as forwarded (neighbour + port MAC on a hit, else unchanged),
            // the new TTL / hop limit, the new IPv4 checksum, the family
            uint4 rec;
            rec.x = hit ? mlo : w[0];
            rec.y = hit ? (mhi | (a.port_mac_lo << 16)) : w[1];
            rec.z = hit ? ((a.port_mac_lo >> 16) | (a.port_mac_hi << 16)) : w[2];
            rec.w = r.v6 ? (((r.c1w1 >> 8) & 0xFFu) | (6u << 24))
                         : (((r.c1w1 >> 16) & 0xFFu) | ((r.c1w2 & 0xFFFFu) << 8) | (4u << 24));
            {   // a buffer store with the write-through cache policy (kRecAux)
                typedef uint32_t v4u __attribute__((ext_vector_type(4)));
                const auto rs = __builtin_amdgcn_make_buffer_rsrc(a.hdr, 0, 0x7FFFFFF0, 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b128(v4u{rec.x, rec.y, rec.z, rec.w}, rs,
                                                       rslot * 16u, 0, kRecAux);
            }
        } else if (!kEmit && live) {
            uint4* q = reinterpret_cast<uint4*>(a.frames + ((size_t)off16 << 4));
            if (hit)
                store16(&q[0], make_uint4(mlo, mhi | (a.port_mac_lo << 16),
                                                (a.port_mac_lo >> 16) | (a.port_mac_hi << 16), w[3]));
            if (wrote1) store16(&q[1], make_uint4(w[4], r.c1w1, r.c1w2, w[7]));
        }
        if (kFamIdx && ok && !r.consumed && ri != kNone) rbits = (rsi + 1) << 8;
        if (live)   // written through (sc1): no dirty lines left for the boundary
            __hip_atomic_store(&a.verdict[i], code | flags | rbits, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        // the egress list in the same pass (upe_gpu_process_emit_tx): each forwarded packet's
        // index in its record's slot, and the group's count (src/worker.c:240-243 queues the
        // forwarded frames in packet order).  Its own kernel instantiations (kTx), so that no
        // other launch carries the code or its registers.
        if (kTx) {
            const unsigned long long fm = __ballot(live && code == UPE_V_FWD);
            if (live && code == UPE_V_FWD)
                a.tx[ch * 64u + __builtin_amdgcn_mbcnt_hi((uint32_t)(fm >> 32),
                                                          __builtin_amdgcn_mbcnt_lo((uint32_t)fm, 0u))] =
                    a.tx_base + i;
            if (lane == 0) a.tx_cnt[ch] = (uint32_t)__popcll(fm);
        }
        // the side array upe_rule_hist reads (lean linear-scan launches never have it; the
        // tuple-space tables it serves always do)
        if ((kTssMode || !kLean) && a.gb && live) {
            // tables of up to 64k rules: the rule and the length in one 4-byte key, so that the
            // group-by reads 4 bytes per packet per rule range instead of verdict + length (6)
            if (a.gb_packed)
                static_cast<uint32_t*>(a.gb)[i] = rbits ? ((rbits << 8) - 0x10000u) | len : 0u;
            else
                static_cast<uint16_t*>(a.gb)[i] = (uint16_t)len;
        }
        if (!kLean && a.flow_hash && live) {
            // software RSS in the same pass: flow_hash (reference src/parser.c:113-135) of the
            // key parse_flow_key gives the RX thread (src/rx_pcap.c:71-72), 0 if it fails
            uint32_t h = r.sport ^ r.dport ^ r.proto;
            h ^= r.v6 ? (r.s[0] ^ r.s[1] ^ r.s[2] ^ r.s[3] ^ r.d[0] ^ r.d[1] ^ r.d[2] ^ r.d[3])
                      : (r.s[0] ^ r.d[0]);
            a.flow_hash[i] = ok ? h : 0u;
        }
        // a deferring wave's outputs and entries are complete before its workgroup counts itself
        // done (the repair reads and patches them)
        if (!kNoLB && deferred) __threadfence();

        // ---- rule_stats: LDS histogram (same-address lanes serialise in the LDS atomic unit,
        // cheaper than a cross-lane reduction per distinct rule).  One 64-bit atomic per packet:
        // the bin's low word counts packets, the high word bytes; neither carries into the other:
        // the host gives no workgroup more than kWgPackets packets (launch_limit and plan_tiling,
        // upe_plan.h; a batch past that runs as several launches), so a workgroup's packets and
        // bytes each fit 32 bits, as the u32 views of the flushes below assume ----
        if (lds_stats && ok && ri != kNone)
            atomicAdd(reinterpret_cast<unsigned long long*>(&lds_hist[2 * rsi]),
                      ((unsigned long long)len << 32) | 1ull);

        // ---- counters and L1 bookkeeping: ballots, added by one lane into the workgroup's LDS
        // totals (no per-lane accumulators to reduce at the end).  A wave's chunks ascend, so its
        // latest table hit per family is the highest such lane of its latest chunk with one, and
        // that lane leaves the hit's payload in the wave's slot. ----
        {
            const bool nc = live && !r.consumed;
            const unsigned long long bm[C_N] = {
                __ballot(ok), __ballot(ok && ri != kNone), __ballot(live && code == UPE_V_FWD),
                __ballot(live && code != UPE_V_FWD && code != UPE_V_CONSUMED),
                __ballot(live && r.consumed), __ballot(nc && (r.flags & UPE_VF_ARP_LEARN)),
                __ballot(nc && (r.flags & UPE_VF_ARP_REPLY)), __ballot(ctrl)};
            const unsigned long long q4 = __ballot(fp4), q6 = __ballot(fp6);
            const unsigned long long h4 = __ballot(thit4), h6 = __ballot(thit6);
            const uint32_t base = ch * 64u;
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < C_N; ++c)
                    if (bm[c]) atomicAdd(&s_tot[c], (uint32_t)__popcll(bm[c]));
                if (q4) atomicMin(&s_tot[C_N + 0], base + (uint32_t)__builtin_ctzll(q4));
                if (q6) atomicMin(&s_tot[C_N + 1], base + (uint32_t)__builtin_ctzll(q6));
                if (bm[C_CTRL])
                    atomicMin(&s_tot[C_N + 2], base + (uint32_t)__builtin_ctzll(bm[C_CTRL]));
                if (h4) s_wm[wave][0] = base + 64u - (uint32_t)__builtin_clzll(h4);   // index + 1
                if (h6) s_wm[wave][1] = base + 64u - (uint32_t)__builtin_clzll(h6);
            }
            if (h4 && lane == 63 - __builtin_clzll(h4)) {
                s_pay[wave][0] = r.d[0]; s_pay[wave][1] = mlo; s_pay[wave][2] = mhi;
            }
            if (h6 && lane == 63 - __builtin_clzll(h6)) {
                s_pay[wave][3] = r.d[0]; s_pay[wave][4] = r.d[1]; s_pay[wave][5] = r.d[2];
                s_pay[wave][6] = r.d[3]; s_pay[wave][7] = mlo; s_pay[wave][8] = mhi;
            }
        }
        if (kRingL) {
            // every workgroup owns ring_mine chunks of each batch (the host launches the ring
            // kernel only when a batch's tiles divide evenly over the grid, and for at most
            // kRingMax batches: one LDS counter per batch, however far apart the workgroup's
            // waves are)
            const uint32_t j = ch / a.ring_cpb, mine = a.ring_mine;
            uint32_t d = 0;
            if (lane == 0) d = atomicAdd(&s_bdone[j], 1u) + 1u;
            d = __builtin_amdgcn_readfirstlane(d);
            if (d == mine) {   // the workgroup is done with batch j
                uint32_t t = 0;
                if (lane == 0) t = atomicAdd(&a.ring_wg[j], 1u) + 1u;
                t = __builtin_amdgcn_readfirstlane(t);
                if (lane == 0 && t == gridDim.x) {
                    const unsigned long long t0 = __hip_atomic_load(a.ring_t0, __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&a.ring_done[j],
                                       ((unsigned long long)__builtin_amdgcn_s_memrealtime() - t0) * 10ull,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
        if (late) {
            chn = claim();
            dsc_next = 0;
            if (chn != kNone && chn * 64u + (uint32_t)lane < a.n) dsc_next = a.desc[chn * 64u + lane];
            asm volatile("" : "+v"(dsc_next));   // consumed here (see before the loop)
        }
    }
    STAMP(4);
    if (!folded) fold_start();
    STAMP(9);
    // A bare barrier: LDS drained (lgkmcnt), global stores left in flight (nothing in this launch
    // reads what this workgroup wrote; __syncthreads() would make every wave wait for its write
    // acknowledgements).
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    STAMP(10);

    // A look-back-live launch counts its finished workgroups; the last one answers whatever the
    // waves deferred (nobody waits for that: a workgroup that is not resident yet delays only the
    // count).  Wave 1 counts, with one atomic whose return it waits for, issued before anything
    // else it has to send, while wave 0 flushes the accumulators and the other waves the
    // mid-size rule_stats, so the round trip overlaps those.
    constexpr int kCounter = kWaves > 1 ? 1 : 0;
    const bool counting = !kNoLB && (look4 || look6);
    if (counting && wave == kCounter) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(&acc_cur(a)->done, 1u);
        t = __builtin_amdgcn_readfirstlane(t);
        if (t + 1u == gridDim.x) {
            const uint32_t nd = __hip_atomic_load(&acc_cur(a)->ndefer, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
            if (nd) {
                __threadfence();   // acquire: the deferring waves' entries and outputs
                repair_deferred<kEmit>(a, nd, lane, Repair{L1[1], L1[2], L1[7], L1[8]});
            }
        }
    }

    // ---- rule_stats of mid-size tables: into one of kStatReps replicas of the per-sorted-index
    // totals (the host sums them and credits rule_id; nothing in this launch reads them), so
    // that the hot rules' counters take 1/kStatReps of the workgroups' atomics each (by every
    // wave but the counting one) ----
    if (lds_stats && !small_stats && !(counting && kWaves > 1 && wave == kCounter)) {
        unsigned long long* rep = a.stats_idx + (size_t)(blockIdx.x % kStatReps) * 2 * a.nrules_pad;
        const uint32_t skip = counting && kWaves > 1 ? 64u : 0u;
        const uint32_t t0 = (uint32_t)tid - (counting && kWaves > 1 && wave > kCounter ? 64u : 0u);
        for (uint32_t k = t0; k < 2 * a.nrules_pad; k += kBlock - skip) {
            const uint32_t v = lds_hist[k];
            if (v) atomicAdd(&rep[k], (unsigned long long)v);
        }
    }
    if (wave != 0) return;
    // ---- wave 0: flush the workgroup into the replicated accumulators ----
    // Device atomics are priced per wave-instruction (~50 ns per CU, whatever the lane count),
    // so every accumulator kind goes out as ONE instruction, lane k carrying field k.  Nothing
    // waits for them: the next launch reads them (kernel boundary), the host after a
    // synchronisation.
    const uint32_t rep = blockIdx.x % kReps;
    const uint32_t f4 = s_tot[C_N + 0], f6 = s_tot[C_N + 1], fc = s_tot[C_N + 2];
    // the workgroup's last table hit per family and the wave holding its payload: lane v reads
    // wave v's (index + 1) << 4 | v, and the maximum names both (index + 1 < 2^25)
    static_assert(kWaves <= 16, "the wave index is packed in 4 bits");
    const uint32_t m4 = wave_reduce<2>(lane < kWaves ? s_wm[lane][0] << 4 | (uint32_t)lane : 0u);
    const uint32_t m6 = wave_reduce<2>(lane < kWaves ? s_wm[lane][1] << 4 | (uint32_t)lane : 0u);
    const uint32_t x4 = m4 >> 4, x6 = m6 >> 4;
    const int w4 = (int)(m4 & 15u), w6 = (int)(m6 & 15u);
    {
        const uint32_t cv = lane < C_N ? s_tot[lane] : 0u;   // lane c < C_N: counter c
        if (lane < C_N && cv) atomicAdd(&acc_cur(a)->cnt[rep][lane], cv);
        // the L1 outcome, one atomicMax instruction: minima as kNone - x, the last table hits
        // with the workgroup whose payload describes them
        const unsigned long long rv =
            lane == R_F4 ? (unsigned long long)(kNone - f4)
          : lane == R_F6 ? (unsigned long long)(kNone - f6)
          : lane == R_M4 ? (x4 ? (unsigned long long)x4 << 32 | blockIdx.x : 0ull)
                         : (x6 ? (unsigned long long)x6 << 32 | blockIdx.x : 0ull);
        if (lane < R_N && rv) atomicMax(&acc_cur(a)->l1r[rep][lane], rv);
        if (lane == 0 && fc != kNone) atomicMax(&acc_cur(a)->ctrl[rep], kNone - fc);
        if (lds_stats && small_stats) {
            for (uint32_t k = lane; k < 2 * a.nrules_pad; k += 64) {
                const uint32_t v = lds_hist[k];
                if (v) atomicAdd(&a.st->acc_stats[rep][k], (unsigned long long)v);
            }
        }
    }
    // the workgroup's last table hit per family (the next launch reads the one the batch
    // maximum points at)
    if ((lane < 3 && x4) || (lane >= 3 && lane < kPayWords && x6))
        st_wt(&reinterpret_cast<uint32_t*>(&pay_cur(a)[blockIdx.x])[lane], s_pay[lane < 3 ? w4 : w6][lane]);
    // workgroup 0: the folded starting state for batch k + 1 (which folds this batch's outcome
    // into it)
    if (blockIdx.x == 0 && lane < 16) {
        // lane j: word j (written through, as the payloads)
        uint32_t v = 0u;
#pragma unroll
        for (int j = 0; j < 11; ++j) v = lane == j ? L1[j] : v;
        st_wt(&reinterpret_cast<uint32_t*>(l1_out(a))[lane], v);
    }
    if (blockIdx.x == 0 && lane == 0) {
        // tell the host whether this batch started from agreeing entries (upe_gpu_process picks
        // the kernel without look-back once one has)
        if (!kNoLB && a.agree_out)
            __hip_atomic_store(a.agree_out,
                               a.launch_tag << 2 | (L1[9] ? 1ull : 0ull) | (L1[10] ? 2ull : 0ull),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    STAMP(5);
}


// ------------------------------------------------------------------------------------------
// rule_stats of large tables (more rules than an LDS histogram holds): a group-by of the
// batch's verdict words by matched rule.  Workgroup (x, y) counts the packets of chunk x whose
// rule falls in range y in LDS bins (packets << 40 | bytes, which cannot overflow: a chunk holds
// at most kHistChunk = 2^23 packets, under the 2^24 the packets field counts to, of at most 65535
// bytes, under 2^40 in all), then writes the bins densely into per-chunk
// partials that upe_hist_reduce sums (device atomics per nonzero bin, measured in round 2, were
// no faster and needed a packed staging array).  Every range re-reads its chunk (for tables of up
// to 64k rules the 4-byte key the classify pass left — rule << 16 | length, round 4: 6 -> 4 bytes
// per packet per range; larger ones the verdict word + a 2-byte length), so ranges are as wide
// as LDS allows; 1024-thread workgroups with sixteen packets
// per thread per round keep enough loads in flight (config D: 256-thread workgroups with four
// packets a round spent ~300 us per 16M batch waiting on them; eight a round 69.5 us, sixteen
// 62.6 us, thirty-two slower again).
// ------------------------------------------------------------------------------------------
// (kHistRange, kHistChunk, kHistChunkMin, kHistTarget: upe_plan.h)
constexpr int kHistBlock = 1024;
#ifndef UPE_HIST_PER
#define UPE_HIST_PER 16
#endif
constexpr int kHistPer = UPE_HIST_PER;   // packets per thread per round (a multiple of 8)
static_assert(kHistPer % 8 == 0 && 8192 % (kHistPer * 1) == 0, "group-by rounds stay 16-byte aligned");

template <bool kPacked>
__global__ void __launch_bounds__(kHistBlock) upe_rule_hist(const uint32_t* verdict,
                                                            const void* gb, uint32_t n,
                                                            uint32_t nrules,
                                                            unsigned long long* part,
                                                            uint32_t chunk, uint32_t range) {
    extern __shared__ unsigned long long h[];   // [range]: packets << 40 | bytes
    const uint32_t r0 = blockIdx.y * range;
    const uint32_t p0 = blockIdx.x * chunk;
    for (uint32_t k = threadIdx.x; k < range; k += kHistBlock) h[k] = 0;
    __syncthreads();
    const uint32_t pend = n - p0 < chunk ? n : p0 + chunk;
    // kHistPer packets per thread per round, all loads issued before the first bin update
    // (chunks start at multiples of 8192, so full groups are 16-byte aligned).  Packed keys:
    // kHistPer / 4 16-byte key loads (rule index << 16 | len, 0 = not counted); otherwise
    // kHistPer / 4 verdict loads and kHistPer / 8 length loads.
    const uint32_t* keys = static_cast<const uint32_t*>(gb);
    const uint16_t* lens = static_cast<const uint16_t*>(gb);
    for (uint32_t i = p0 + kHistPer * threadIdx.x; i < pend; i += kHistPer * kHistBlock) {
        uint32_t rb[kHistPer], len[kHistPer];   // rule index + 1 (0 = none), length
        if (i + kHistPer <= pend) {
#pragma unroll
            for (int q = 0; q < kHistPer / 4; ++q) {
                const uint4 a0 = *reinterpret_cast<const uint4*>((kPacked ? keys : verdict) + i + 4 * q);
                rb[4 * q + 0] = a0.x; rb[4 * q + 1] = a0.y; rb[4 * q + 2] = a0.z; rb[4 * q + 3] = a0.w;
            }
            if (!kPacked) {
#pragma unroll
                for (int q = 0; q < kHistPer / 8; ++q) {
                    const uint4 l = *reinterpret_cast<const uint4*>(lens + i + 8 * q);
                    len[8 * q + 0] = l.x & 0xFFFFu; len[8 * q + 1] = l.x >> 16;
                    len[8 * q + 2] = l.y & 0xFFFFu; len[8 * q + 3] = l.y >> 16;
                    len[8 * q + 4] = l.z & 0xFFFFu; len[8 * q + 5] = l.z >> 16;
                    len[8 * q + 6] = l.w & 0xFFFFu; len[8 * q + 7] = l.w >> 16;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < kHistPer; ++j) {
                rb[j] = i + j < pend ? (kPacked ? keys : verdict)[i + j] : 0u;
                if (!kPacked) len[j] = i + j < pend ? (uint32_t)lens[i + j] : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < kHistPer; ++j) {
            if (kPacked) {
                len[j] = rb[j] & 0xFFFFu;
                rb[j] = len[j] ? (rb[j] >> 16) + 1u : 0u;
            } else {
                rb[j] >>= 8;   // matched rule's sorted index + 1, 0 = none
            }
            if (rb[j] != 0 && rb[j] - 1u - r0 < range) atomicAdd(&h[rb[j] - 1u - r0], (1ull << 40) | len[j]);
        }
    }
    __syncthreads();
    // this chunk's bins, zeros included, as plain coalesced stores (upe_hist_reduce sums them
    // over the chunks; no device atomics)
    const uint32_t rend = nrules - r0 < range ? nrules : r0 + range;
    unsigned long long* o = part + (size_t)blockIdx.x * nrules + r0;
    for (uint32_t k = threadIdx.x; k < rend - r0; k += kHistBlock) o[k] = h[k];
}

// The dense group-by partials ([nchunks][nrules], packets << 40 | bytes) summed over the chunks:
// slice y of the grid sums chunks y, y + S, ... for rule r = blockIdx.x * 256 + thread and adds
// the unpacked totals to replica y % kStatReps of stats_idx; with S = kStatReps every replica
// word has exactly one writer in the launch, so the adds are plain.
__global__ void __launch_bounds__(256) upe_hist_reduce(const unsigned long long* part,
                                                       uint32_t nchunks, uint32_t nrules,
                                                       uint32_t nrules_pad,
                                                       unsigned long long* stats_idx) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nrules) return;
    unsigned long long pk = 0, by = 0;
    uint32_t c = blockIdx.y;
    for (; c + 7 * gridDim.y < nchunks; c += 8 * gridDim.y) {
        unsigned long long b[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = part[(size_t)(c + j * gridDim.y) * nrules + r];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            pk += b[j] >> 40;
            by += b[j] & ((1ull << 40) - 1);
        }
    }
    for (; c < nchunks; c += gridDim.y) {
        const unsigned long long b = part[(size_t)c * nrules + r];
        pk += b >> 40;
        by += b & ((1ull << 40) - 1);
    }
    if (pk) {
        unsigned long long* o = stats_idx + (size_t)(blockIdx.y % kStatReps) * 2 * nrules_pad + 2 * (size_t)r;
        o[0] += pk;
        o[1] += by;
    }
}

// ------------------------------------------------------------------------------------------
// Egress list: the indexes of the packets with a given verdict code, in packet order (the order
// process_packet queues frames for tx_send_batch, reference src/worker.c:240-243).  Pass 1
// counts per block; pass 2 gives each block its offset (sum of the counts before it) and writes
// its indexes with wave ballots.  (kCompactBlock packets per workgroup: upe_ctx.h.)
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) upe_compact_count(const uint32_t* verdict, uint32_t n,
                                                         uint32_t code, uint32_t* counts) {
    __shared__ uint32_t s_c;
    if (threadIdx.x == 0) s_c = 0;
    __syncthreads();
    const uint32_t p0 = blockIdx.x * kCompactBlock;
    uint32_t c = 0;
    for (uint32_t k = threadIdx.x; k < kCompactBlock; k += 256) {
        const uint32_t i = p0 + k;
        c += (i < n && (verdict[i] & 0xFu) == code) ? 1u : 0u;
    }
    c = wave_reduce<0>(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_c, c);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_c;
}

__global__ void __launch_bounds__(256) upe_compact_write(const uint32_t* verdict, uint32_t n,
                                                         uint32_t code, const uint32_t* counts,
                                                         uint32_t nblocks, uint32_t* index,
                                                         unsigned long long* total) {
    __shared__ uint32_t s_base;
    __shared__ uint32_t s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t pre = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += 256) pre += counts[b];
    pre = wave_reduce<0>(pre);
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    if (lane == 0 && pre) atomicAdd(&s_base, pre);
    __syncthreads();
    uint32_t base = s_base;
    const uint32_t p0 = blockIdx.x * kCompactBlock;
    for (uint32_t k = 0; k < kCompactBlock; k += 256) {
        const uint32_t i = p0 + k + threadIdx.x;
        const bool m = i < n && (verdict[i] & 0xFu) == code;
        const unsigned long long bal = __ballot(m);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = base;
        for (int v = 0; v < wave; ++v) off += s_wave[v];
        const uint32_t rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (m) index[off + rank] = i;
        const uint32_t tot = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
        base += tot;
    }
    if (blockIdx.x == nblocks - 1 && threadIdx.x == 0) *total = base;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
thread_local std::string g_err;   // upe_gpu_last_error(); fail() sets it (upe_gpu_set_last_error)

NeighIndex arp_index(const upe_gpu_ctx* c) {
    return NeighIndex{c->neigh.arp, c->neigh.arp_bits, c->neigh.arp_seed};
}
NeighIndex ndp_index(const upe_gpu_ctx* c) {
    return NeighIndex{c->neigh.ndp, c->neigh.ndp_bits, c->neigh.ndp_seed};
}

// Point the DevState at the separately allocated arrays (after any of them is reallocated).
int publish(upe_gpu_ctx* c) {
    struct {
        TilePay* pay;
        uint32_t* lb;
        unsigned long long* stats;
        unsigned long long* stats_idx;
    } p = {c->pay, c->lb.flags, c->stats.rule, c->stats.idx};
    static_assert(offsetof(DevState, stats_idx) - offsetof(DevState, pay) == 3 * sizeof(void*),
                  "DevState pointer block");
    HIP_TRY(hipMemcpy(reinterpret_cast<char*>(c->st.p) + offsetof(DevState, pay), &p, sizeof p,
                      hipMemcpyHostToDevice));
    return 0;
}

int ensure_scratch(upe_gpu_ctx* c, size_t ntiles) {
    if (2 * 64 * ntiles * kWaves > c->lb.defer.cap) {   // (the last one made)
        c->lb.flags.reset();   // both go before either comes back
        c->lb.defer.reset();
        const size_t chunks = (ntiles + ntiles / 4 + 16) * kWaves;
        if (c->lb.flags.zeros(chunks) != 0 ||
            c->lb.defer.reserve(2 * 64 * chunks, 2 * 64 * chunks) != 0 || publish(c) != 0)
            return -1;
    }
    return 0;
}

// The state slots of batch k (DevState comment).
DevL1* l1_slot(upe_gpu_ctx* c, uint64_t k) { return &c->st->l1[k % 2].s; }
BatchAcc* acc_slot(upe_gpu_ctx* c, uint64_t k) { return &c->st->acc[k % 3]; }
TilePay* pay_slot(upe_gpu_ctx* c, uint64_t k) { return c->pay + (size_t)(k % 2) * c->paycap; }

// Does the L1 state the next batch starts from agree with the tables?  (After l1_sync.)  On the
// context's stream, or on `s` (upe::neigh_patched).
int refresh(upe_gpu_ctx* c, hipStream_t s = nullptr) {
    if (!s) s = c->stream;
    if (order_on(c, s) != 0) return -1;
    c->lb.no_lb = false;   // the entries may disagree with the new tables until a launch says not
    c->lb.reset_k = c->k;
    hipLaunchKernelGGL(upe_refresh, dim3(1), dim3(64), 0, s, l1_slot(c, c->k), arp_index(c),
                       ndp_index(c));
    HIP_TRY(hipGetLastError());
    return 0;
}

// Fold the last batch's L1 outcome into l1[k % 2], the state the next batch starts from (and
// clear it from that batch's accumulators, so the next launch does not fold it again).
int l1_sync(upe_gpu_ctx* c, hipStream_t s = nullptr) {
    if (c->k == 0) return 0;
    if (!s) s = c->stream;
    if (order_on(c, s) != 0) return -1;
    hipLaunchKernelGGL(upe_l1_sync, dim3(1), dim3(64), 0, s, l1_slot(c, c->k),
                       acc_slot(c, c->k + 2), pay_slot(c, c->k + 1));
    HIP_TRY(hipGetLastError());
    return 0;
}

// The between-batch state of a fresh context (a calloc'd worker_t): L1 all zero, accumulators
// armed (nothing happened), totals zero.
int arm_state(upe_gpu_ctx* c) {
    if (order_on(c, c->stream) != 0) return -1;
    static DevState init;   // zero, then the armed accumulator fields
    for (auto& acc : init.acc) acc.grid = 1;   // every other word zero: nothing happened
    HIP_TRY(hipMemcpyAsync(c->st, &init, offsetof(DevState, pay), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->k = 0;
    c->last_n = 0;
    c->lb.no_lb = false;
    c->lb.reset_k = 0;
    return 0;
}

// The built variants (variant_built), listed once; kernel i of the table is kBuilt.v[i]'s.
struct BuiltList {
    Variant v[256];
    int n;
};
constexpr BuiltList list_built() {
    BuiltList l{};
    for (int scan = 0; scan < 4; ++scan)
        for (Path path : {Path::Device, Path::Ring, Path::Host, Path::Tx})
            for (int tss = 0; tss < 2; ++tss)
                for (int emit = 0; emit < 2; ++emit)
                    for (int lean = 0; lean < 2; ++lean)
                        for (int nolb = 0; nolb < 2; ++nolb) {
                            const Variant v{tss != 0, emit != 0, lean != 0, nolb != 0, path, scan};
                            if (variant_built(v)) l.v[l.n++] = v;
                        }
    return l;
}
constexpr BuiltList kBuilt = list_built();
static_assert(kBuilt.n == 83, "the classify instantiations (each costs about a second of build)");

template <int I>
const void* classify_fn_at() {
    constexpr Variant v = kBuilt.v[I];
    return reinterpret_cast<const void*>(
        &upe_classify<v.tss, v.emit, v.lean, v.nolb, v.path, v.scan>);
}
template <int... I>
std::array<const void*, sizeof...(I)> classify_table(std::integer_sequence<int, I...>) {
    return {{classify_fn_at<I>()...}};
}
const std::array<const void*, kBuilt.n>& classify_fns() {
    static const auto fns = classify_table(std::make_integer_sequence<int, kBuilt.n>{});
    return fns;
}
// The kernel of a variant, nullptr when it is not built: one load from an array keyed by the
// variant's word (the word's range, 8 bits), filled from the list at the first call.
const void* classify_fn(Variant v) {
    static const std::array<const void*, 256> by_word = [] {
        std::array<const void*, 256> t{};
        for (int i = 0; i < kBuilt.n; ++i) t[variant_word(kBuilt.v[i])] = classify_fns()[i];
        return t;
    }();
    return by_word[variant_word(v) & 255u];
}

void launch_classify(Variant v, uint32_t grid, size_t lds, hipStream_t s, const Args& a) {
    // dynamic LDS beyond 64 KB must be allowed per kernel and device (once per device)
    static std::atomic<uint64_t> lds_attr{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = 1ull << (dev & 63);
    if (!(lds_attr.fetch_or(bit) & bit))
        for (int i = 0; i < kBuilt.n; ++i)
            (void)hipFuncSetAttribute(classify_fns()[i], hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(kBuilt.v[i].scan ? kLdsDynMaxLarge : kLdsDynMax));
    Args arg = a;
    void* args[] = {&arg};
    (void)hipLaunchKernel(classify_fn(v), dim3(grid), dim3(kBlock), args, lds, s);
}

// The persistent grid of a kernel configuration: the occupancy API's answer, checked by a census
// launch the first time the configuration is used (census_probe).  0 on error.
uint32_t resident_grid(upe_gpu_ctx* c, Variant var, size_t lds, hipStream_t s) {
    const uint64_t key = (uint64_t)lds << 8 | variant_word(var);   // the word takes 8 bits
    auto it = c->resident.find(key);
    if (it != c->resident.end()) return it->second;
    // (every launch asks here first: a variant that is not built never reaches hipLaunchKernel)
    if (!classify_fn(var)) {
        fail("no classify kernel is built for variant " + std::to_string(variant_word(var)));
        return 0;
    }
    int per_cu = 0;
    hipError_t e;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, classify_fn(var), kBlock, lds);
    if (e != hipSuccess) {
        fail(std::string("hipOccupancyMaxActiveBlocksPerMultiprocessor: ") + hipGetErrorString(e));
        return 0;
    }
    if (per_cu < 1) per_cu = 1;
    uint32_t grid = (uint32_t)per_cu * (uint32_t)c->cus;
    if (c->blocks_per_cu_override > 0) {
        grid = (uint32_t)c->blocks_per_cu_override * (uint32_t)c->cus;   // diagnostic
    } else {
        if (grid > c->paycap) grid = c->paycap;
        Args a;
        memset(&a, 0, sizeof a);
        a.census = 1;
        a.st = c->st;
        uint32_t* w = &c->st->census[0];
        const uint32_t init[2] = {0u, kNone};
        if (hipMemcpyAsync(w, init, sizeof init, hipMemcpyHostToDevice, s) != hipSuccess) {
            fail("census upload failed");
            return 0;
        }
        launch_classify(var, grid, lds, s, a);
        uint32_t out[2] = {0u, 0u};
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(out, w, sizeof out, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {
            fail("census launch failed");
            return 0;
        }
        if (out[1] != kNone && out[1] < grid) {
            // round down to whole workgroups per CU
            const uint32_t per = out[1] / (uint32_t)c->cus;
            grid = (per ? per : 1u) * (uint32_t)c->cus;
        }
    }
    if (grid > c->paycap) grid = c->paycap;
    if (c->grid_cap && grid > c->grid_cap) grid = c->grid_cap;   // diagnostic: only ever lowers
    c->resident[key] = grid;
    if (getenv("UPE_GPU_VERBOSE"))
        fprintf(stderr, "upe_gpu: persistent grid %u (occupancy API %d per CU, lds %zu, kernel "
                "variant %u)\n", grid, per_cu, lds, variant_word(var));
    return grid;
}

}  // namespace

extern "C" {

const char* upe_gpu_last_error(void) { return g_err.c_str(); }

// For the library's other units (fail(), upe_dev.h) and its C parts (upe_worker.c): set the
// calling thread's message, return -1.  Not declared in include/upe_gpu.h and not exported.
UPE_INTERNAL int upe_gpu_set_last_error(const char* msg) {
    g_err = msg ? msg : "";
    return -1;
}

int upe_gpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

// The process's allowed CPUs as they were when the library was loaded (before any thread of it
// was pinned: a pinned thread's own mask is one CPU).
static cpu_set_t g_process_cpus;
__attribute__((constructor)) static void upe_capture_cpus() {
    CPU_ZERO(&g_process_cpus);
    if (sched_getaffinity(0, sizeof g_process_cpus, &g_process_cpus) != 0)
        for (int c = 0; c < CPU_SETSIZE; ++c) CPU_SET(c, &g_process_cpus);
}

// The host CPUs local to a GPU: the device's PCI function in sysfs names its NUMA node and the
// CPUs attached to it (local_cpulist), kept in the process's allowed set.
int upe_gpu_local_cpus(int device, int* cpus, size_t cap, int* numa_node) {
    char bus[64] = {0};
    HIP_TRY(hipDeviceGetPCIBusId(bus, (int)sizeof bus, device));
    for (char* p = bus; *p; ++p) *p = (char)tolower((unsigned char)*p);
    const std::string dir = std::string("/sys/bus/pci/devices/") + bus;
    int node = -1;
    if (FILE* f = fopen((dir + "/numa_node").c_str(), "r")) {
        if (fscanf(f, "%d", &node) != 1) node = -1;
        fclose(f);
    }
    if (numa_node) *numa_node = node;
    std::string list;
    if (FILE* f = fopen((dir + "/local_cpulist").c_str(), "r")) {
        char buf[4096];
        if (fgets(buf, sizeof buf, f)) list = buf;
        fclose(f);
    }
    if (list.empty()) return fail("no local_cpulist for PCI device " + std::string(bus));
    const cpu_set_t& allowed = g_process_cpus;
    size_t n = 0;
    const char* p = list.c_str();
    while (*p) {   // "0-63,128-191"
        char* e = nullptr;
        const long lo = strtol(p, &e, 10);
        if (e == p) break;
        long hi = lo;
        p = e;
        if (*p == '-') {
            hi = strtol(p + 1, &e, 10);
            p = e;
        }
        for (long c = lo; c <= hi; ++c)
            if (c >= 0 && c < CPU_SETSIZE && CPU_ISSET(c, &allowed)) {
                if (cpus && n < cap) cpus[n] = (int)c;
                ++n;
            }
        while (*p == ',' || *p == '\n' || *p == ' ') ++p;
    }
    return (int)n;
}

// Pin the calling thread to one CPU local to `device` (the slot-th of them, modulo their
// number) — the reference pins each worker thread with affinity_pin_self (src/affinity.c:48,
// cores from assign_cores, src/main.c:143-175); a GPU worker's host thread belongs on the GPU's
// NUMA node, where its pinned buffers are then allocated.  Returns the CPU.
int upe_gpu_pin_self(int device, int slot) {
    std::vector<int> cpus(CPU_SETSIZE);
    const int n = upe_gpu_local_cpus(device, cpus.data(), cpus.size(), nullptr);
    if (n <= 0) return n == 0 ? fail("no allowed CPU is local to the device") : -1;
    const int cpu = cpus[(size_t)(slot < 0 ? 0 : slot) % (size_t)n];
    cpu_set_t one;
    CPU_ZERO(&one);
    CPU_SET(cpu, &one);
    if (pthread_setaffinity_np(pthread_self(), sizeof one, &one) != 0)
        return fail("pthread_setaffinity_np failed");
    return cpu;
}

upe_gpu_ctx_t* upe_gpu_open(int device, size_t rule_capacity) {
    if (rule_capacity == 0 || rule_capacity > (1u << 24)) {
        fail("rule_capacity must be in [1, 2^24]");
        return nullptr;
    }
    upe_gpu_ctx* c = new (std::nothrow) upe_gpu_ctx();
    if (!c) {
        fail("out of memory");
        return nullptr;
    }
    c->device = device;
    c->stats.cap = rule_capacity;
    auto failed = [&]() {   // the message is the failed step's
        const std::string m = g_err;
        upe_gpu_close(c);
        g_err = m;
        return nullptr;
    };
    auto bad = [&](hipError_t e, const char* what) {
        fail(std::string(what) + ": " + hipGetErrorString(e));
        return failed();
    };
    DevScope dg(device);
    hipError_t e;
    if ((e = dg.e) != hipSuccess) return bad(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess)
        return bad(e, "hipStreamCreate");
    if ((e = hipEventCreateWithFlags(&c->order_ev, hipEventDisableTiming)) != hipSuccess)
        return bad(e, "hipEventCreate");
    if (c->st.zeros(1) != 0 || c->stats.rule.reserve(rule_capacity * 2, rule_capacity * 2) != 0)
        return failed();
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) ==
                hipSuccess && cus > 0)
            c->cus = cus;
        if (const char* v = getenv("UPE_GPU_BLOCKS_PER_CU")) c->blocks_per_cu_override = atoi(v);
        // diagnostic: at most this many workgroups in a persistent grid (a small partition's grid
        // on a whole device); 0 or unset: no cap
        if (const char* v = getenv("UPE_GPU_GRID_CAP")) c->grid_cap = (uint32_t)strtoul(v, nullptr, 10);
        // diagnostics: the look-back wait before deferring (0 = defer whenever a flag is not yet
        // published), a synchronous agreement report per launch (the switch to the kernel without
        // look-back then happens at a deterministic launch), no kernel without look-back
        if (const char* v = getenv("UPE_GPU_LB_SPIN")) c->lb.spin = (uint32_t)strtoul(v, nullptr, 10);
        if (const char* v = getenv("UPE_GPU_LB_SYNC")) c->lb.sync = v[0] == '1';
        if (const char* v = getenv("UPE_GPU_NOLB")) c->lb.allow_nolb = v[0] != '0';
        if (const char* v = getenv("UPE_GPU_HOST_SLOTS"))
            c->host.nslots = std::min(8u, std::max(2u, (uint32_t)strtoul(v, nullptr, 10)));
    }
    // payload slots for the largest grid a launch uses (at most 8 workgroups per CU)
    c->paycap = 8u * (uint32_t)c->cus;
    if (c->pay.zeros(2 * (size_t)c->paycap) != 0) return failed();
    // host-mapped report of each launch's start-state agreement (the kernel without look-back
    // is used once one arrives; without it, every launch keeps the look-back)
    if (hipHostMalloc(reinterpret_cast<void**>(&c->lb.agree_h), sizeof(unsigned long long),
                      hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
        *c->lb.agree_h = 0;
        if (hipHostGetDevicePointer(reinterpret_cast<void**>(&c->lb.agree_d), c->lb.agree_h, 0) !=
            hipSuccess) {
            (void)hipHostFree(c->lb.agree_h);
            c->lb.agree_h = nullptr;
            c->lb.agree_d = nullptr;
        }
    } else {
        c->lb.agree_h = nullptr;
    }
    if (arm_state(c) != 0) return failed();
    {
        std::vector<unsigned long long> img;
        if (latency_init_image(img) != 0 || c->lat_hist.put(img.data(), img.size()) != 0)
            return failed();
    }
    if ((e = hipMemsetAsync(c->stats.rule, 0, rule_capacity * 2 * sizeof(unsigned long long),
                            c->stream)) != hipSuccess)
        return bad(e, "hipMemsetAsync");
    // An empty rule table: one padding block of never-matching rules.
    if (upe_gpu_load_rules(c, nullptr, 0) != 0) return failed();
    if (upe_gpu_load_neigh(c, nullptr, 0, nullptr, 0) != 0 || refresh(c) != 0) return failed();
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return bad(e, "sync");
    return c;
}

void upe_gpu_close(upe_gpu_ctx_t* c) {
    if (!c) return;
    DevScope dg(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : c->timing.ev) (void)hipEventDestroy(e);
    if (c->order_ev) (void)hipEventDestroy(c->order_ev);
    for (hipEvent_t e : c->marks)
        if (e) (void)hipEventDestroy(e);
    for (auto& sl : c->host.slots)
        for (hipEvent_t e : {sl.in_done, sl.k_done, sl.out_done})
            if (e) (void)hipEventDestroy(e);
    if (c->host.s_in) (void)hipStreamSynchronize(c->host.s_in), (void)hipStreamDestroy(c->host.s_in);
    if (c->host.s_out) (void)hipStreamSynchronize(c->host.s_out), (void)hipStreamDestroy(c->host.s_out);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->lb.agree_h) (void)hipHostFree(c->lb.agree_h);
    delete c;   // the device buffers go with it (DevBuf), on the context's device
}

}  // extern "C"

namespace {
// Credit the sorted-index totals of the current table to rule_stats[rule_id] (device) and clear
// them: called before upe_gpu_load_rules changes the table, so the counts carry over by rule_id
// (upe_gpu_reload_rules instead starts a fresh rule_stats, as the reference's SIGHUP reload does).
// Every table size keeps its counts per sorted index: small tables in the per-batch replicated
// accumulators (acc_stats, added here), mid-size ones in kStatReps replicas (each workgroup's LDS
// bins) and large ones too (upe_rule_hist).  The host sums the replicas and credits rule_id.
int read_stats_idx(upe_gpu_ctx* c, std::vector<unsigned long long>& idx) {
    const size_t E = 2 * (size_t)c->table.nrules_pad;
    std::vector<unsigned long long> all(E * kStatReps);
    HIP_TRY(hipMemcpy(all.data(), c->stats.idx, all.size() * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost));
    idx.assign(E, 0);
    for (size_t r = 0; r < (size_t)kStatReps; ++r)
        for (size_t e = 0; e < E; ++e) idx[e] += all[r * E + e];
    if (E <= 2 * (size_t)kSmallRules) {
        // small tables: the classify kernel's replicated per-sorted-index totals
        std::vector<unsigned long long> sm((size_t)kReps * 2 * kSmallRules);
        HIP_TRY(hipMemcpy(sm.data(), &c->st->acc_stats[0][0], sm.size() * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost));
        for (size_t r = 0; r < (size_t)kReps; ++r)
            for (size_t e = 0; e < E; ++e) idx[e] += sm[r * 2 * kSmallRules + e];
    }
    return 0;
}

int fold_stats_idx(upe_gpu_ctx* c) {
    if (!c->stats.idx || c->table.rinfo_host.empty()) return 0;
    const size_t E = 2 * (size_t)c->table.nrules_pad;
    std::vector<unsigned long long> idx, st(2 * c->stats.cap);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (read_stats_idx(c, idx) != 0) return -1;
    bool any = false;
    for (unsigned long long v : idx) any |= v != 0;
    if (!any) return 0;
    HIP_TRY(hipMemcpy(st.data(), c->stats.rule, st.size() * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost));
    for (size_t e = 0; e < E; ++e)
        if (idx[e]) st[2 * (size_t)(uint32_t)c->table.rinfo_host[e >> 1].y + (e & 1)] += idx[e];
    HIP_TRY(hipMemcpy(c->stats.rule, st.data(), st.size() * sizeof(unsigned long long),
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(c->stats.idx, 0, E * kStatReps * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(&c->st->acc_stats[0][0], 0, sizeof(c->st->acc_stats)));
    return 0;
}

// rule_stats[0..capacity) as the worker holds them: the per-rule_id array plus the current
// table's per-sorted-index totals credited to their rule_id (after a device synchronisation).
int read_rule_stats(upe_gpu_ctx* c, upe_rule_stat_t* rule_stats, size_t capacity) {
    const size_t k = capacity < c->stats.cap ? capacity : c->stats.cap;
    memset(rule_stats, 0, capacity * sizeof(upe_rule_stat_t));
    HIP_TRY(hipMemcpy(rule_stats, c->stats.rule, k * sizeof(upe_rule_stat_t), hipMemcpyDeviceToHost));
    if (c->stats.idx && !c->table.rinfo_host.empty()) {
        const size_t E = 2 * (size_t)c->table.nrules_pad;
        std::vector<unsigned long long> idx;
        if (read_stats_idx(c, idx) != 0) return -1;
        for (size_t e = 0; e < E; ++e) {
            const uint32_t rid = (uint32_t)c->table.rinfo_host[e >> 1].y;
            if (!idx[e] || rid >= k) continue;
            if (e & 1) rule_stats[rid].bytes += idx[e];
            else rule_stats[rid].packets += idx[e];
        }
    }
    return 0;
}

using StatsBuf = DevBuf<unsigned long long>;
// upe_gpu_load_rules / upe_gpu_reload_rules[_image] with a compiled image: `fresh` (a zeroed
// rule_stats of fresh_cap entries) replaces the context's statistics on a reload, the old
// per-index totals dropped instead of credited.  Everything the new table needs is uploaded
// before the context changes: on an error the context keeps classifying with the old table and
// its statistics.
int install_image(upe_gpu_ctx_t* c, const upe_rule_image& im, StatsBuf* fresh, size_t fresh_cap) {
    DeviceTable next;   // dropped on an error return
    if (next.upload(im) != 0) return -1;
    // the per-index totals are kept while they hold the new table
    StatsBuf idx;
    const size_t idx_words = im.pad * 2 * kStatReps;
    const bool grow = idx_words > c->stats.idx.cap;
    if (grow && idx.zeros(idx_words) != 0) return -1;
    // previous batches may still read the table, on whichever stream they went
    if (c->last_stream) HIP_TRY(hipStreamSynchronize(c->last_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (fresh) {
        // the reload's fresh statistics: the old table's per-index totals are dropped
        if (c->stats.idx)
            HIP_TRY(hipMemset(c->stats.idx, 0, c->stats.idx.cap * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(&c->st->acc_stats[0][0], 0, sizeof(c->st->acc_stats)));
        c->stats.rule = std::move(*fresh);
        c->stats.cap = fresh_cap;
    } else if (fold_stats_idx(c) != 0) {   // the old table's counts credited to their rule_ids
        return -1;
    }
    // the swap (the moves free what the context held)
    c->table = std::move(next);
    if (grow) c->stats.idx = std::move(idx);
    const char* tl = getenv("UPE_GPU_TREE_LDS");   // diagnostic: 0 = the image stays in memory
    c->tree_stage = !(tl && tl[0] == '0');
    // the kernel without look-back may have been chosen because a family could not forward
    // under the old table: back to the full kernel until a launch under this one reports
    c->lb.no_lb = false;
    c->lb.reset_k = c->k;
    return publish(c);   // the DevState's pointers (stats.rule, stats.idx)
}

int load_rules_impl(upe_gpu_ctx_t* c, const upe_rule_t* rules, size_t count,
                    StatsBuf* fresh, size_t fresh_cap) {
    upe_rule_image im;
    if (build_image(rules, count, fresh ? fresh_cap : c->stats.cap, im) != 0) return -1;
    return install_image(c, im, fresh, fresh_cap);
}
}  // namespace

extern "C" {

extern "C" int upe_gpu_load_rules(upe_gpu_ctx_t* c, const upe_rule_t* rules, size_t count) {
    if (!c) return fail("null context");
    if (count > c->stats.cap) return fail("rule count exceeds the capacity given at open");
    if (count && !rules) return fail("null rules");
    DEV_SCOPE(c->device);
    return load_rules_impl(c, rules, count, nullptr, 0);
}

// The reference's SIGHUP reload (src/main.c:216-282): the stats thread builds a new table
// (rule_table_init(1024) + rule_config_load), gives every worker a fresh calloc'd rule_stats of
// the new table's capacity, swaps w->rt and w->rule_stats between two of the worker's bursts and
// frees the old ones after a grace period.  The worker's pkts_* counters and its one-entry L1
// neighbour caches are untouched.  Here: the batches queued so far finish with the old table,
// their rule_stats (credited to the old rule_ids) are handed back in old_stats if asked for,
// and the next batch runs with the new table and an all-zero rule_stats[rule_capacity].  All or
// nothing: on an error the old table and its statistics stay (as the reference keeps both when
// rule_config_load fails, src/main.c:229-255).
extern "C" int upe_gpu_reload_rules(upe_gpu_ctx_t* c, const upe_rule_t* rules, size_t count,
                                    size_t rule_capacity, upe_rule_stat_t* old_stats,
                                    size_t old_capacity) {
    if (!c) return fail("null context");
    if (rule_capacity == 0 || rule_capacity > (1u << 24)) return fail("rule_capacity must be in [1, 2^24]");
    if (count > rule_capacity) return fail("rule count exceeds the new capacity");
    if (count && !rules) return fail("null rules");
    if (old_capacity && !old_stats) return fail("null old_stats");
    for (size_t i = 0; i < count; ++i)
        if (rules[i].rule_id >= rule_capacity) return fail("rule_id >= capacity (rule_stats index)");
    DEV_SCOPE(c->device);
    // the batches queued with the old table finish first (on whichever stream they went)
    if (c->last_stream) HIP_TRY(hipStreamSynchronize(c->last_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (old_capacity && read_rule_stats(c, old_stats, old_capacity) != 0) return -1;
    StatsBuf fresh;   // a zeroed rule_stats of the new capacity (freed unless the reload succeeds)
    if (fresh.zeros(rule_capacity * 2) != 0) return -1;
    return load_rules_impl(c, rules, count, &fresh, rule_capacity);
}

extern "C" int upe_gpu_reload_image(upe_gpu_ctx_t* c, const upe_rule_image_t* im,
                                    upe_rule_stat_t* old_stats, size_t old_capacity) {
    if (!c || !im) return fail("null context or image");
    if (old_capacity && !old_stats) return fail("null old_stats");
    DEV_SCOPE(c->device);
    if (c->last_stream) HIP_TRY(hipStreamSynchronize(c->last_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (old_capacity && read_rule_stats(c, old_stats, old_capacity) != 0) return -1;
    StatsBuf fresh;
    if (fresh.zeros(im->cap * 2) != 0) return -1;
    return install_image(c, *im, &fresh, im->cap);
}

// (not part of the ABI; upe_worker.c) tag this context's launches as a host-side loop's: they
// run the host-path kernel instantiation (the same code), so that a profile of a process that
// also classifies device-resident batches keeps the two kinds of launch apart
extern "C" int upe_gpu_tag_host(upe_gpu_ctx_t* c, int on) {
    if (!c) return fail("null context");
    c->host_tag = on != 0;
    return 0;
}

extern "C" int upe_gpu_rule_index_kind(upe_gpu_ctx_t* c) {
    if (!c) return fail("null context");
    return c->table.tss ? 1 : c->table.tree_ok ? 2 : 0;
}

extern "C" int upe_gpu_rule_index_info(upe_gpu_ctx_t* c, upe_rule_index_info_t* info) {
    if (!c || !info) return fail("null argument");
    *info = c->table.tree_ok ? c->table.tree_info : upe_rule_index_info_t{};
    return 0;
}

// All or nothing, as a rule reload is: the new snapshot is built (build_neigh_image, upe_rules.cpp)
// and uploaded beside the old one, and only then moved into the context; on an error the context
// keeps looking up in the old snapshot.
int upe_gpu_load_neigh(upe_gpu_ctx_t* c, const upe_arp_entry_t* arp, size_t arp_capacity,
                       const upe_ndp_entry_t* ndp, size_t ndp_capacity) {
    if (!c) return fail("null context");
    upe_neigh_image image;
    if (compile_neigh(arp, arp_capacity, ndp, ndp_capacity, image.im) != 0) return -1;
    return upe_gpu_load_neigh_image(c, &image);
}

// The second half of the same load, for a snapshot compiled beforehand (upe_neigh_compile, any
// thread): the upload, the swap, and the L1 entries' agreement with the new tables.
int upe_gpu_load_neigh_image(upe_gpu_ctx_t* c, const upe_neigh_image_t* image) {
    if (!c) return fail("null context");
    if (!image) return fail("null neighbour image");
    DEV_SCOPE(c->device);
    NeighTable next;   // dropped on an error return
    if (next.upload(image->im) != 0) return -1;
    // the last batch's L1 outcome into the starting state before the tables change
    if (c->st && l1_sync(c) != 0) return -1;
    if (c->last_stream) HIP_TRY(hipStreamSynchronize(c->last_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->neigh = std::move(next);   // frees the old snapshot: nothing queued reads it any more
    c->learn.loaded(image->im);   // (host state only: upe_gpu_neigh_learn's free counts start here)
    if (c->st && refresh(c) != 0) return -1;   // does the L1 state agree with the new tables?
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"

// (upe_ctx.h) The two halves of what a load does around its swap, for a snapshot whose MACs change
// in place (upe_gpu_neigh_patch, upe_neigh_patch.hip), queued on the patch's stream: before, the
// last batch's L1 outcome into the starting state, after everything the context has queued;
// after, the L1 entries' agreement with the changed tables.
int upe::neigh_patching(upe_gpu_ctx_t* c, hipStream_t s) {
    if (order_on(c, s) != 0) return -1;
    return c->st ? l1_sync(c, s) : 0;
}
int upe::neigh_patched(upe_gpu_ctx_t* c, hipStream_t s) { return c->st ? refresh(c, s) : 0; }

extern "C" {

int upe_gpu_set_port(upe_gpu_ctx_t* c, const uint8_t eth_addr[6], uint32_t ip4_addr) {
    if (!c || !eth_addr) return fail("null argument");
    c->port_mac_lo = mac_lo(eth_addr);
    c->port_mac_hi = mac_hi(eth_addr);
    c->port_ip4 = ip4_addr;
    return 0;
}

int upe_gpu_set_l1(upe_gpu_ctx_t* c, const upe_l1_state_t* l1) {
    if (!c || !l1) return fail("null argument");
    DEV_SCOPE(c->device);
    DevL1 d;
    memset(&d, 0, sizeof d);
    d.arp_ip = l1->last_arp_ip;
    d.arp_mac_lo = mac_lo(l1->last_arp_mac);
    d.arp_mac_hi = mac_hi(l1->last_arp_mac);
    for (int j = 0; j < 4; ++j) d.ndp_ip[j] = le32(l1->last_ndp_ip + 4 * j);
    d.ndp_mac_lo = mac_lo(l1->last_ndp_mac);
    d.ndp_mac_hi = mac_hi(l1->last_ndp_mac);
    // the pending batch's outcome is replaced, not folded in later: fold (clears it), overwrite
    if (l1_sync(c) != 0) return -1;
    HIP_TRY(hipMemcpyAsync(l1_slot(c, c->k), &d, sizeof d, hipMemcpyHostToDevice, c->stream));
    if (refresh(c) != 0) return -1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int upe_gpu_get_l1(upe_gpu_ctx_t* c, upe_l1_state_t* l1) {
    if (!c || !l1) return fail("null argument");
    DEV_SCOPE(c->device);
    if (l1_sync(c) != 0) return -1;
    HIP_TRY(hipDeviceSynchronize());
    DevL1 d;
    HIP_TRY(hipMemcpy(&d, l1_slot(c, c->k), sizeof d, hipMemcpyDeviceToHost));
    memset(l1, 0, sizeof *l1);
    l1->last_arp_ip = d.arp_ip;
    memcpy(l1->last_arp_mac, &d.arp_mac_lo, 4);
    memcpy(l1->last_arp_mac + 4, &d.arp_mac_hi, 2);
    memcpy(l1->last_ndp_ip, d.ndp_ip, 16);
    memcpy(l1->last_ndp_mac, &d.ndp_mac_lo, 4);
    memcpy(l1->last_ndp_mac + 4, &d.ndp_mac_hi, 2);
    return 0;
}

}  // extern "C"

namespace {
// One batch: the classify launch (in place, or emit mode when d_hdr is given), plus the
// rule_stats group-by for tables over kLdsStatsMax rules.  A launch takes at most
// launch_limit() packets (upe_plan.h: kMaxLaunch, and fewer where a small grid's workgroups would
// otherwise outgrow their 32-bit rule_stats bins).
// The smallest persistent grid resident_grid can answer with: whole workgroups per CU, at least
// one, unless the diagnostic cap is lower.
uint32_t min_grid(const upe_gpu_ctx* c) {
    const uint32_t cus = (uint32_t)c->cus;
    return c->grid_cap && c->grid_cap < cus ? c->grid_cap : cus;
}

// Timing sample: an event pair around `span` consecutive calls, opened on every
// every-th call (samples never overlap).
int open_sample(upe_gpu_ctx* c, hipStream_t s) {
    upe_gpu_ctx::Timing& t = c->timing;
    const bool open = t.on && t.left == 0 &&
                      (t.calls % t.every) == t.phase;
    if (t.on) ++t.calls;
    if (!open) return 0;
    while (t.ev.size() < t.ev_used + 3) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        t.ev.push_back(e);
    }
    HIP_TRY(hipEventRecord(t.ev[t.ev_used], s));
    t.left = t.span;
    return 0;
}
// mid: the sample's middle event was recorded (mid_sample)
int close_sample(upe_gpu_ctx* c, hipStream_t s, bool mid) {
    upe_gpu_ctx::Timing& t = c->timing;
    if (t.left && --t.left == 0) {
        HIP_TRY(hipEventRecord(t.ev[t.ev_used + 2], s));
        t.ev_mid.push_back(mid);
        t.ev_used += 3;
        t.launches += t.span;
    }
    return 0;
}

// Once a launch has been seen starting from agreeing L1 entries (or from an entry whose
// family's index is empty), every later one does until the host changes tables or entries:
// c->lb.no_lb.
int settle_no_lb(upe_gpu_ctx* c) {
    if (c->lb.no_lb || !c->lb.agree_h || !c->lb.allow_nolb) return 0;
    if (c->lb.sync && c->k > c->lb.reset_k && c->last_stream)
        HIP_TRY(hipStreamSynchronize(c->last_stream));   // the previous launch's report
    const unsigned long long v = __atomic_load_n(c->lb.agree_h, __ATOMIC_ACQUIRE);
    const unsigned long long tag = v >> 2;
    if (tag != 0 && tag - 1 >= c->lb.reset_k &&
        ((v & 1) || c->neigh.arp_bits == 0 || !c->table.fwd4) &&
        ((v & 2) || c->neigh.ndp_bits == 0 || !c->table.fwd6))
        c->lb.no_lb = true;
    return 0;
}

// The plan's view of the loaded tables (upe_plan.h): the rule table's, the neighbour indexes'
// sizes and whether a tree may be staged in LDS (a context option).
TableShape table_shape(const upe_gpu_ctx* c) {
    const DeviceTable& t = c->table;
    return TableShape{t.tss, t.nrules, t.nrules_pad, c->neigh.arp_bits, c->neigh.ndp_bits, t.nfs,
                      t.tree_ok, c->tree_stage, t.tree_words, t.fam4, t.fam6, t.fam_all != 0};
}

// The kernel's arguments but for the tiling and the ring's (process_impl sets those).
Args fill_args(const upe_gpu_ctx* c, const ProcessReq& q, const LdsPlan& p) {
    const DeviceTable& t = c->table;
    Args a;
    memset(&a, 0, sizeof a);   // every field a launch does not set stays null / zero
    a.frames = q.frames;
    a.desc = q.desc;
    a.verdict = q.verdict;
    a.n = (uint32_t)q.n;
    a.tx = q.tx;
    a.tx_cnt = q.tx_cnt;
    a.tx_base = (uint32_t)q.tx_base;
    a.flow_hash = q.flow_hash;
    a.hdr = reinterpret_cast<uint4*>(q.hdr);
    a.rv4 = t.rv4;
    a.rv6 = t.rv6;
    a.rinfo = t.rinfo;
    a.nrules_pad = t.nrules_pad;
    a.fam = t.fam;
    a.fam4 = t.fam4;
    a.fam6 = t.fam6;
    a.fam_x1idx = t.fam_x1idx;
    a.tree = reinterpret_cast<const uint2*>(t.tree.p);
    a.tree_loff = t.tree_loff;
    a.arp = arp_index(c);
    a.ndp = ndp_index(c);
    a.st = c->st;
    a.port_mac_lo = c->port_mac_lo;
    a.port_mac_hi = c->port_mac_hi;
    a.port_ip4 = c->port_ip4;
    a.tg4 = t.tg4;
    a.tg6 = t.tg6;
    a.tt4 = t.tt4;
    a.tt6 = t.tt6;
    a.tfs = reinterpret_cast<const uint4*>(t.tfs.p);
    a.ng4 = t.ng4;
    a.ng6 = t.ng6;
    a.tss = t.tss ? 1u : 0u;
    a.pay = c->pay;
    a.paycap = c->paycap;
    a.stats = c->stats.rule;
    a.stats_idx = c->stats.idx;
    a.k6 = (uint32_t)(c->k % 6);
    a.lb = c->lb.flags;
    a.defer = c->lb.defer;
    a.lb_spin = c->lb.spin;
    a.lb_tag = (uint32_t)(c->k % kLbTagMod) + 1u;
    a.agree_out = c->lb.no_lb ? nullptr : c->lb.agree_d;
    a.launch_tag = c->k + 1;
    // the plan's share (upe_plan.h)
    a.gb = p.gb ? c->stats.gb.p : nullptr;
    a.gb_packed = p.gb_packed;
    a.arp_lds = p.arp_lds;
    a.ndp_lds = p.ndp_lds;
    a.fp_lds = p.fp_lds;
    a.tree_lds = p.tree_lds;
    a.fam6_lds = p.fam6_lds;
    a.fam4_lds = p.fam4_lds;
    return a;
}

// The rule_stats group-by of a batch the classify launch left keys for (tables over
// kLdsStatsMax rules): dense partials, one 8-byte bin per chunk and rule, summed by
// upe_hist_reduce.
int launch_group_by(upe_gpu_ctx* c, const uint32_t* d_verdict, size_t n, bool packed,
                    hipStream_t s) {
    const GroupByPlan g = plan_group_by(c->table.nrules, n);
    const size_t part_words = (size_t)g.grid_x * g.nrules;
    if (c->stats.hist_part.reserve(part_words, part_words) != 0) return -1;
    static std::atomic<uint64_t> hist_attr{0};   // 128 KB of dynamic LDS, once per device
    if (!(hist_attr.fetch_or(1ull << (c->device & 63)) & (1ull << (c->device & 63)))) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&upe_rule_hist<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(kHistRange * sizeof(unsigned long long)));
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&upe_rule_hist<false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(kHistRange * sizeof(unsigned long long)));
    }
    const dim3 hg(g.grid_x, g.nr);
    const size_t lds = g.range * sizeof(unsigned long long);
    if (packed)
        hipLaunchKernelGGL(upe_rule_hist<true>, hg, dim3(kHistBlock), lds, s, d_verdict,
                           c->stats.gb.p, (uint32_t)n, g.nrules, c->stats.hist_part.p, g.chunk,
                           g.range);
    else
        hipLaunchKernelGGL(upe_rule_hist<false>, hg, dim3(kHistBlock), lds, s, d_verdict,
                           c->stats.gb.p, (uint32_t)n, g.nrules, c->stats.hist_part.p, g.chunk,
                           g.range);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(upe_hist_reduce, dim3((g.nrules + 255) / 256, kStatReps), dim3(256), 0, s,
                       c->stats.hist_part.p, g.grid_x, g.nrules, c->table.nrules_pad,
                       c->stats.idx.p);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

int upe::process_impl(upe_gpu_ctx_t* c, const ProcessReq& q) {
    // 1. validate
    if (!c) return fail("null context");
    const size_t n = q.n;
    const bool host = q.host || c->host_tag;
    if (n > 0xFFFFFFFFull - kTile) return fail("batch too large (n must fit in 32 bits)");
    if (n && (!q.frames || !q.desc || !q.verdict)) return fail("null batch buffer");
    if (((uintptr_t)q.frames & 15u) != 0) return fail("frames buffer must be 16-byte aligned");
    if (((uintptr_t)q.hdr & 15u) != 0) return fail("header records must be 16-byte aligned");
    // 2. consecutive launches of at most `limit` packets: the worker's stream semantics are
    // those of one batch (batch_info describes the last launch)
    const size_t limit = launch_limit(c->table.nrules_pad <= (uint32_t)kLdsStatsMax, min_grid(c));
    if (q.ring && n > limit)
        return fail("a ring holds at most " + std::to_string(limit) + " packets");
    if (n > limit) {
        for (size_t s0 = 0; s0 < n; s0 += limit) {
            ProcessReq part = q;
            part.desc += s0;
            part.verdict += s0;
            part.n = n - s0 < limit ? n - s0 : limit;
            if (q.hdr) part.hdr += s0;
            if (q.flow_hash) part.flow_hash += s0;
            part.host = host;
            if (q.tx) part.tx += s0;
            if (q.tx_cnt) part.tx_cnt += s0 / 64;
            part.tx_base = q.tx_base + s0;
            if (process_impl(c, part) != 0) return -1;
        }
        return 0;
    }
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, q.stream);
    if (ensure_scratch(c, n ? (n + kTile - 1) / kTile : 1) != 0) return -1;
    // 3. after the context's previous launch and its own uploads (tables, L1), on whichever stream
    // they went: a batch starts from the state the one before it left
    if (order_on(c, s) != 0 || open_sample(c, s) != 0) return -1;
    if (c->k > 0 && c->k % kLbTagMod == 0)   // tags wrap: no flag may carry this launch's tag
        HIP_TRY(hipMemsetAsync(c->lb.flags, 0, c->lb.flags.cap * sizeof(uint32_t), s));
    // 4. plan (upe_plan.h)
    if (settle_no_lb(c) != 0) return -1;
    const bool emit = q.hdr != nullptr && n > 0;
    const PlanReq pq{n, emit, q.flow_hash != nullptr, q.tx != nullptr, host,
                     q.ring ? q.ring->per : 0, q.ring && q.ring->done};
    const LdsPlan p = plan_lds(table_shape(c), pq, c->lb.no_lb);
    if (p.gb && c->stats.gb.reserve(n, (n + n / 4 + 64) & ~(size_t)3) != 0) return -1;   // either form
    // 5. the arguments
    Args a = fill_args(c, q, p);
    // persistent grid: the workgroups the chip holds at once
    Variant var = p.var;
    const uint32_t grid_cap = resident_grid(c, var, p.lds, s);
    if (grid_cap == 0) return -1;
    // the census of the no-look-back counterpart now as well, so that the switch to it (a few
    // launches later) does not put a synchronous census launch in the middle of a batch stream
    if (p.lean && !c->lb.no_lb) {
        Variant nolb = var;
        nolb.nolb = true;
        if (resident_grid(c, nolb, p.lds, s) == 0) return -1;
    }
    const Tiling t = plan_tiling(n, grid_cap);
    a.tw = t.tw;
    a.ntiles = t.ntiles;
    // 6. a ring's stamps
    if (pq.ring_done) {
        const size_t nb = n / q.ring->per;
        HIP_TRY(hipMemsetAsync(q.ring->done, 0, nb * sizeof(unsigned long long), s));
        const RingPlan r = plan_ring(p, pq, t);
        var = r.var;
        if (!r.stamp) {
            if (resident_grid(c, var, p.lds, s) == 0) return -1;
        } else {
            // the batches' counters, then the time origin
            if (c->ring_wg.reserve(nb + 2, nb + 2) != 0) return -1;
            HIP_TRY(hipMemsetAsync(c->ring_wg, 0, nb * sizeof(unsigned long long), s));
            HIP_TRY(hipMemsetAsync(c->ring_wg + nb, 0xFF, sizeof(unsigned long long), s));
            a.ring_cpb = r.ring_cpb;
            a.ring_mine = r.ring_mine;
            a.ring_wg = reinterpret_cast<uint32_t*>(c->ring_wg.p);
            a.ring_done = q.ring->done;
            a.ring_t0 = c->ring_wg + nb;
        }
    }
    // 7. launch
    launch_classify(var, t.grid, p.lds, s, a);
    HIP_TRY(hipGetLastError());
    c->last_var = (int)variant_word(var);
    c->last_grid = t.grid;
    // 8. the group-by; before it the sample's middle event, between the classify launch and the
    // group-by (last call of the sample only; launches without a group-by have none)
    const bool mid = c->timing.left == 1 && p.gb;
    if (mid) HIP_TRY(hipEventRecord(c->timing.ev[c->timing.ev_used + 1], s));
    if (p.gb && launch_group_by(c, q.verdict, n, p.gb_packed != 0, s) != 0) return -1;
    // 9., 10.
    if (close_sample(c, s, mid) != 0) return -1;
    ++c->k;
    c->last_n = (uint32_t)n;
    c->have_batch = true;
    return 0;
}

extern "C" {

int upe_gpu_process(upe_gpu_ctx_t* c, uint8_t* d_frames, const uint64_t* d_desc,
                    uint32_t* d_verdict, size_t n, void* stream) {
    return process_impl(c, ProcessReq{d_frames, d_desc, d_verdict, n, stream});
}

int upe_gpu_process_rss(upe_gpu_ctx_t* c, uint8_t* d_frames, const uint64_t* d_desc,
                        uint32_t* d_verdict, uint32_t* d_flow_hash, size_t n, void* stream) {
    ProcessReq q{d_frames, d_desc, d_verdict, n, stream};
    q.flow_hash = d_flow_hash;
    return process_impl(c, q);
}

int upe_gpu_process_emit(upe_gpu_ctx_t* c, uint8_t* d_frames, const uint64_t* d_desc,
                         uint32_t* d_verdict, upe_hdr_rec_t* d_hdr, size_t n, void* stream) {
    if (n && !d_hdr) return fail("null header records");
    ProcessReq q{d_frames, d_desc, d_verdict, n, stream};
    q.hdr = d_hdr;
    return process_impl(c, q);
}

int upe_gpu_process_emit_tx(upe_gpu_ctx_t* c, uint8_t* d_frames, const uint64_t* d_desc,
                            uint32_t* d_verdict, upe_hdr_rec_t* d_hdr, uint32_t* d_tx,
                            uint32_t* d_tx_count, size_t n, void* stream) {
    if (n && (!d_hdr || !d_tx || !d_tx_count)) return fail("null header records or egress list");
    ProcessReq q{d_frames, d_desc, d_verdict, n, stream};
    q.hdr = d_hdr;
    q.tx = d_tx;
    q.tx_cnt = d_tx_count;
    return process_impl(c, q);
}

int upe_gpu_process_ring_emit(upe_gpu_ctx_t* c, uint8_t* d_frames, const uint64_t* d_desc,
                              uint32_t* d_verdict, upe_hdr_rec_t* d_hdr, size_t n, size_t count,
                              uint64_t* d_done_ns, void* stream) {
    if (!c) return fail("null context");
    if (count == 0 || n == 0) return 0;
    if (!d_hdr) return fail("null header records");
    if (n % 1024 != 0) return fail("a ring batch must hold a multiple of 1024 packets");
    if (n * count > kMaxLaunch) return fail("a ring holds at most 2^24 packets");
    // (process_impl refuses a ring past launch_limit(): a ring is one launch)
    const RingReq r{n, reinterpret_cast<unsigned long long*>(d_done_ns)};
    ProcessReq q{d_frames, d_desc, d_verdict, n * count, stream};
    q.hdr = d_hdr;
    q.ring = &r;
    return process_impl(c, q);
}

int upe_gpu_process_batches(upe_gpu_ctx_t* c, uint8_t* const* d_frames_list, const uint64_t* d_desc,
                            uint32_t* d_verdict, size_t n, size_t count, void* stream) {
    if (!c) return fail("null context");
    if (count && !d_frames_list) return fail("null frames list");
    for (size_t k = 0; k < count; ++k)
        if (upe_gpu_process(c, d_frames_list[k], d_desc, d_verdict, n, stream) != 0) return -1;
    return 0;
}

int upe_gpu_process_queue_emit(upe_gpu_ctx_t* c, const upe_gpu_batch_t* batches, size_t count,
                               void* stream) {
    if (!c) return fail("null context");
    if (count && !batches) return fail("null batch list");
    // one launch after another (overlapping consecutive launches on two streams measured slower
    // on MI355X: DESIGN.md §8, round 3); every batch is checked before any is queued
    for (size_t k = 0; k < count; ++k)
        if (batches[k].n && !batches[k].hdr) return fail("null header records in a queued batch");
    for (size_t k = 0; k < count; ++k) {
        ProcessReq q{batches[k].frames, batches[k].desc, batches[k].verdict, batches[k].n, stream};
        q.hdr = batches[k].hdr;
        if (process_impl(c, q) != 0) return -1;
    }
    return 0;
}

int upe_gpu_process_batches_emit(upe_gpu_ctx_t* c, uint8_t* const* d_frames_list,
                                 const uint64_t* d_desc, uint32_t* d_verdict, upe_hdr_rec_t* d_hdr,
                                 size_t n, size_t count, void* stream) {
    if (!c) return fail("null context");
    if (count && !d_frames_list) return fail("null frames list");
    std::vector<upe_gpu_batch_t> q(count);
    for (size_t k = 0; k < count; ++k) q[k] = upe_gpu_batch_t{d_frames_list[k], d_desc, d_verdict, d_hdr, n};
    return upe_gpu_process_queue_emit(c, q.data(), count, stream);
}

#if UPE_STAMPS
int upe_gpu_diag_stamps(void* host, size_t bytes) {
    HIP_TRY(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), bytes, 0, hipMemcpyDeviceToHost));
    return 0;
}
#endif

int upe_gpu_compact(upe_gpu_ctx_t* c, const uint32_t* d_verdict, size_t n, uint32_t code,
                    uint32_t* d_index, uint64_t* d_count, void* stream) {
    if (!c) return fail("null context");
    if (!d_count || (n && (!d_verdict || !d_index))) return fail("null buffer");
    if (n > 0xFFFFFFFFull - kCompactBlock) return fail("n must fit in 32 bits");
    if (code > 15) return fail("verdict code out of range");
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint64_t), s));
        return 0;
    }
    const uint32_t nb = (uint32_t)((n + kCompactBlock - 1) / kCompactBlock);
    if (c->compact_counts.reserve(nb, nb) != 0) return -1;
    hipLaunchKernelGGL(upe_compact_count, dim3(nb), dim3(256), 0, s, d_verdict, (uint32_t)n, code,
                       c->compact_counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(upe_compact_write, dim3(nb), dim3(256), 0, s, d_verdict, (uint32_t)n, code,
                       c->compact_counts, nb, d_index,
                       reinterpret_cast<unsigned long long*>(d_count));
    HIP_TRY(hipGetLastError());
    return 0;
}

// For the worker loop (upe_worker.c), not part of the ABI: a completion mark after everything
// queued so far on the context's stream, and a wait for it, so that the loop walks batch k - 1
// while batch k is on the GPU.
__attribute__((visibility("hidden"))) int upe_gpu_mark(upe_gpu_ctx_t* c, int slot) {
    if (!c || slot < 0 || slot >= 4) return fail("bad mark");
    DEV_SCOPE(c->device);
    if (!c->marks[slot]) HIP_TRY(hipEventCreateWithFlags(&c->marks[slot], hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->marks[slot], c->stream));
    return 0;
}
__attribute__((visibility("hidden"))) int upe_gpu_mark_wait(upe_gpu_ctx_t* c, int slot) {
    if (!c || slot < 0 || slot >= 4 || !c->marks[slot]) return fail("bad mark");
    DEV_SCOPE(c->device);
    HIP_TRY(hipEventSynchronize(c->marks[slot]));
    return 0;
}

int upe_gpu_sync(upe_gpu_ctx_t* c, void* stream) {
    if (!c) return fail("null context");
    DEV_SCOPE(c->device);
    HIP_TRY(hipStreamSynchronize(pick(c, stream)));
    return 0;
}

int upe_gpu_batch_info(upe_gpu_ctx_t* c, upe_batch_info_t* info) {
    if (!c || !info) return fail("null argument");
    DEV_SCOPE(c->device);
    HIP_TRY(hipDeviceSynchronize());
    memset(info, 0, sizeof *info);
    info->first_ctrl = ~0ull;
    if (!c->have_batch || c->k == 0) return 0;
    BatchAcc b;   // the last batch's accumulators
    HIP_TRY(hipMemcpy(&b, acc_slot(c, c->k + 2), sizeof b, hipMemcpyDeviceToHost));
    uint64_t* dst = &info->counters.pkts_in;
    dst[0] = b.n;
    uint32_t cm = 0;
    for (int r = 0; r < kReps; ++r) {
        for (int j = 0; j < 7; ++j) dst[1 + j] += b.cnt[r][j];
        info->n_ctrl += b.cnt[r][C_CTRL];
        cm = std::max(cm, b.ctrl[r]);
    }
    if (cm) info->first_ctrl = kNone - cm;
    return 0;
}

int upe_gpu_launch_info(upe_gpu_ctx_t* c, upe_launch_info_t* info) {
    if (!c || !info) return fail("null argument");
    DEV_SCOPE(c->device);
    HIP_TRY(hipDeviceSynchronize());
    memset(info, 0, sizeof *info);
    info->launches = c->k;
    if (c->k == 0 || c->last_var < 0) return 0;
    info->variant = (uint32_t)c->last_var;
    info->grid = c->last_grid;
    HIP_TRY(hipMemcpy(&info->deferred, &acc_slot(c, c->k + 2)->ndefer, sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
    return 0;
}

int upe_gpu_get_stats(upe_gpu_ctx_t* c, upe_counters_t* counters, upe_rule_stat_t* rule_stats,
                      size_t capacity) {
    if (!c) return fail("null context");
    DEV_SCOPE(c->device);
    HIP_TRY(hipDeviceSynchronize());
    if (counters) {
        // the totals up to batch k - 2, plus batch k - 1 (folded in by the next launch)
        unsigned long long t[8];
        HIP_TRY(hipMemcpy(t, &c->st->totals[0], sizeof t, hipMemcpyDeviceToHost));
        uint64_t* dst = &counters->pkts_in;
        for (int j = 0; j < 8; ++j) dst[j] = t[j];
        if (c->k > 0) {
            BatchAcc b;
            HIP_TRY(hipMemcpy(&b, acc_slot(c, c->k + 2), sizeof b, hipMemcpyDeviceToHost));
            dst[0] += b.n;
            for (int r = 0; r < kReps; ++r)
                for (int j = 0; j < 7; ++j) dst[1 + j] += b.cnt[r][j];
        }
    }
    if (rule_stats && read_rule_stats(c, rule_stats, capacity) != 0) return -1;
    return 0;
}

int upe_gpu_reset_stats(upe_gpu_ctx_t* c) {
    if (!c) return fail("null context");
    DEV_SCOPE(c->device);
    if (order_on(c, c->stream) != 0) return -1;
    HIP_TRY(hipMemsetAsync(&c->st->totals[0], 0, sizeof(c->st->totals), c->stream));
    if (c->k > 0) {   // the last batch's counters, not yet folded into the totals
        BatchAcc* b = acc_slot(c, c->k + 2);
        HIP_TRY(hipMemsetAsync(&b->cnt[0][0], 0, sizeof(b->cnt), c->stream));
        HIP_TRY(hipMemsetAsync(&b->n, 0, sizeof(b->n), c->stream));
    }
    HIP_TRY(hipMemsetAsync(&c->st->acc_stats[0][0], 0, sizeof(c->st->acc_stats), c->stream));
    HIP_TRY(hipMemsetAsync(c->stats.rule, 0, c->stats.cap * 2 * sizeof(unsigned long long), c->stream));
    if (c->stats.idx)
        HIP_TRY(hipMemsetAsync(c->stats.idx, 0, c->stats.idx.cap * sizeof(unsigned long long),
                               c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_batch = false;
    return 0;
}

int upe_gpu_timing_span(upe_gpu_ctx_t* c, int every, int span) {
    if (!c) return fail("null context");
    if (span < 1) return fail("span must be at least 1");
    DEV_SCOPE(c->device);
    HIP_TRY(hipDeviceSynchronize());
    c->timing.ev_used = 0;   // the pool is kept for reuse
    c->timing.ev_mid.clear();
    c->timing.on = every > 0;
    c->timing.every = every > 0 ? (uint32_t)every : 1u;
    c->timing.phase = c->timing.every / 2;   // not the first call: it starts from an idle queue
    c->timing.span = (uint32_t)span;
    c->timing.calls = 0;
    c->timing.left = 0;
    c->timing.launches = 0;
    return 0;
}

int upe_gpu_timing_enable(upe_gpu_ctx_t* c, int enable) {
    return upe_gpu_timing_span(c, enable, 1);
}

int upe_gpu_timing_read(upe_gpu_ctx_t* c, double* classify_ms, double* finalize_ms,
                        uint64_t* launches) {
    if (!c) return fail("null context");
    DEV_SCOPE(c->device);
    double a = 0, b = 0;
    for (size_t j = 0, k = 0; j + 3 <= c->timing.ev_used; j += 3, ++k) {
        HIP_TRY(hipEventSynchronize(c->timing.ev[j + 2]));
        float x = 0, y = 0;
        if (c->timing.ev_mid[k]) {
            HIP_TRY(hipEventElapsedTime(&x, c->timing.ev[j], c->timing.ev[j + 1]));
            HIP_TRY(hipEventElapsedTime(&y, c->timing.ev[j + 1], c->timing.ev[j + 2]));
        } else {
            HIP_TRY(hipEventElapsedTime(&x, c->timing.ev[j], c->timing.ev[j + 2]));
        }
        a += x;
        b += y;
    }
    if (classify_ms) *classify_ms = a;
    if (finalize_ms) *finalize_ms = b;
    if (launches) *launches = c->timing.launches;
    return 0;
}

void* upe_gpu_malloc(upe_gpu_ctx_t* c, size_t bytes) {
    if (!c) {
        fail("null context");
        return nullptr;
    }
    void* p = nullptr;
    DevScope dg(c->device);
    if (dg.e != hipSuccess || hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) {
        fail("hipMalloc failed");
        return nullptr;
    }
    return p;
}

int upe_gpu_free(upe_gpu_ctx_t* c, void* p) {
    if (!c) return fail("null context");
    DEV_SCOPE(c->device);
    if (p) HIP_TRY(hipFree(p));
    return 0;
}

int upe_gpu_memcpy_h2d(upe_gpu_ctx_t* c, void* dst, const void* src, size_t bytes, void* stream) {
    if (!c) return fail("null context");
    DEV_SCOPE(c->device);
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, pick(c, stream)));
    return 0;
}

int upe_gpu_memcpy_d2h(upe_gpu_ctx_t* c, void* dst, const void* src, size_t bytes, void* stream) {
    if (!c) return fail("null context");
    DEV_SCOPE(c->device);
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, pick(c, stream)));
    return 0;
}

}  // extern "C"
