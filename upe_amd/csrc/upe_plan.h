// upe_plan.h — what a classify launch decides before it runs, as plain functions over plain
// structs: which upe_classify variant, how much dynamic LDS and for what, the tiling and grid, the
// ring stamps, and the rule_stats group-by's shape.  Plain C++17, no HIP runtime: upe_gpu.hip
// (process_impl) executes the plan, tools/plan_check.cpp (`make plan-check`) checks it on the CPU.
//
// Everything here has internal linkage (an unnamed namespace, as in upe_gpu.hip before the split):
// upe_classify is instantiated on Path, so Path's scope is part of every kernel's symbol.
#ifndef UPE_PLAN_H
#define UPE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "upe_dev.h"

namespace {

using namespace upe;

#ifndef UPE_BLOCK
#define UPE_BLOCK 1024
#endif
constexpr int kBlock = UPE_BLOCK;      // threads per workgroup = packets per tile
constexpr int kWaves = kBlock / 64;    // 64-packet chunks per tile
constexpr int kTile = kBlock;

#ifndef UPE_LDS_STATS_MAX
#define UPE_LDS_STATS_MAX 4096
#endif
constexpr int kLdsStatsMax = UPE_LDS_STATS_MAX;   // rule_stats in the classify kernel's LDS up to here
// Neighbour indexes staged in LDS (one workgroup per CU, so a CU reads them once per launch):
// ARP up to 2048 slots (32 KB), NDP up to 2048 slots (64 KB), within kLdsDynMax of dynamic LDS.
#ifndef UPE_ARP_LDS_SLOTS
#define UPE_ARP_LDS_SLOTS 2048
#endif
#ifndef UPE_NDP_LDS_SLOTS
#define UPE_NDP_LDS_SLOTS 2048
#endif
constexpr uint32_t kArpLdsSlots = UPE_ARP_LDS_SLOTS;
constexpr uint32_t kNdpLdsSlots = UPE_NDP_LDS_SLOTS;
constexpr size_t kLdsDynMax = 152 * 1024;   // 160 KB per CU less the static LDS (7 KB at most)
constexpr int kRingMax = 64;           // batches of a ring launch whose completion is stamped

#ifndef UPE_FAM_LDS
#define UPE_FAM_LDS 1
#endif
constexpr bool kFamLds = UPE_FAM_LDS;

// The rule_stats group-by (upe_rule_hist): see its comment in upe_gpu.hip.
#ifndef UPE_HIST_RANGE
#define UPE_HIST_RANGE 16384
#endif
constexpr uint32_t kHistRange = UPE_HIST_RANGE;   // most rules per workgroup: 128 KB of LDS
// most packets per workgroup: below 2^24, so that a chunk's packets on one rule fit the 24-bit
// field of a bin (packets << 40 | bytes) and their bytes (65535 each at most) its 40-bit field
constexpr uint32_t kHistChunk = 1u << 23;
constexpr uint32_t kHistChunkMin = 8192;
static_assert(kHistChunk < (1u << 24) && (uint64_t)kHistChunk * 65535u < (1ull << 40),
              "a group-by bin holds a whole chunk on one rule");
static_assert(kHistChunk % kHistChunkMin == 0 && kHistChunkMin % 8192 == 0,
              "chunks start at multiples of 8192");
#ifndef UPE_HIST_TARGET
#define UPE_HIST_TARGET 256
#endif
constexpr uint32_t kHistTarget = UPE_HIST_TARGET;   // workgroups per group-by launch

// ---- classify kernel variants ----------------------------------------------------------------
// What a launch is for.  Host runs the same code as Device: it is a name, so that a profile of a
// process that also classifies device-resident batches keeps the host paths' launches
// (upe_gpu_process_mapped / upe_gpu_process_host) apart.  Ring: a ring launch that stamps its
// batches' completion (upe_gpu_process_ring_emit).  Tx: the egress-list kernels
// (upe_gpu_process_emit_tx).
enum class Path { Device, Ring, Host, Tx };
// One upe_classify instantiation.  nolb: no look-back (lean only).  scan: how a linear-scan table
// is matched (never with tuple space): 0 small table (LDS copy), 1 its family lists (FamTable),
// 2 the whole table through the scalar unit, 3 the decision tree over the family lists.
struct Variant {
    bool tss, emit, lean, nolb;
    Path path;
    int scan;
};
// The instantiated variants: every combination a launch can ask for.
constexpr bool variant_built(Variant v) {
    if (v.nolb && !v.lean) return false;
    if (v.scan && v.tss) return false;
    if (v.path == Path::Tx) return v.emit;
    if (v.path == Path::Ring) return v.emit && v.lean && !v.tss;
    return true;
}
// upe_launch_info_t.variant (include/upe_gpu.h): bit 0 emit, 1 tuple space, 2 lean, 3 no
// look-back, 4 ring, 5 host path (4 and 5 together: the egress-list kernels), 6-7 scan.
constexpr uint32_t variant_word(Variant v) {
    const bool ring = v.path == Path::Ring || v.path == Path::Tx;
    const bool host = v.path == Path::Host || v.path == Path::Tx;
    return (v.emit ? 1u : 0u) | (v.tss ? 2u : 0u) | (v.lean ? 4u : 0u) | (v.nolb ? 8u : 0u) |
           (ring ? 16u : 0u) | (host ? 32u : 0u) | (uint32_t)v.scan << 6;
}

// ---- the plan's inputs ------------------------------------------------------------------------
// The loaded tables, as far as a launch's shape depends on them.
struct TableShape {
    bool tss;                      // tuple-space index (else a linear-scan table)
    uint32_t nrules, nrules_pad;
    uint32_t arp_bits, ndp_bits;   // log2(slots) of the neighbour indexes, 0 = empty
    uint32_t nfs;                  // staged fingerprint image, uint4
    bool tree_ok, tree_stage;      // a decision tree is built / may be staged in LDS
    uint32_t tree_words;           // its image, uint4
    uint32_t fam4, fam6;           // family list entries
    bool fam_all;                  // a family's list is a single catch-all
};
// One batch.  ring_per: packets per batch of a ring launch, 0 = not a ring.
struct PlanReq {
    size_t n;
    bool emit, flow_hash, tx, host;
    size_t ring_per;
    bool ring_done;                // the ring's caller wants completion stamps
};

// ---- LDS and variant --------------------------------------------------------------------------
struct LdsPlan {
    size_t hist;                   // bytes of rule_stats bins
    uint32_t arp_lds, ndp_lds, fp_lds, tree_lds, fam6_lds, fam4_lds;   // as Args carries them
    size_t lds;                    // total dynamic LDS, bytes
    int scan;
    bool lds_stats;                // rule_stats in the kernel's LDS bins (else the group-by)
    bool gb;                       // the launch writes the group-by's side array
    uint32_t gb_packed;
    bool lean;
    Variant var;
};
// Dynamic LDS is handed out greedily, in this order: rule_stats bins, ARP index, NDP index,
// tuple-space fingerprints, decision tree, IPv6 family list, IPv4 family list.  A region that does
// not fit the remaining budget is skipped (its *_lds stays 0, the kernel reads it from memory) and
// later, smaller ones may still fit.  upe_classify's carve-up at the top of the kernel walks the
// same order over the same Args fields: the two must change together.
inline LdsPlan plan_lds(const TableShape& t, const PlanReq& q, bool no_lb) {
    LdsPlan p{};
    p.lds_stats = t.nrules_pad <= (uint32_t)kLdsStatsMax;
    p.gb = !p.lds_stats && q.n > 0;
    p.gb_packed = t.nrules <= 65536u ? 1u : 0u;   // sorted indexes of matches < nrules
    p.hist = p.lds_stats ? 2 * (size_t)t.nrules_pad * sizeof(uint32_t) : 0;
    // large linear tables: the decision tree (when built), else family lists, unless a family's
    // list is a single catch-all (then the split gains that family nothing and measured slower
    // for the other)
    p.scan = t.tss || t.nrules_pad <= (uint32_t)kSmallRules ? 0
           : t.tree_ok ? 3 : t.fam_all ? 2 : 1;
    const size_t lds_max = p.scan ? kLdsDynMaxLarge : kLdsDynMax;
    size_t lds = p.hist;
    auto fits = [&](size_t bytes) {
        if (lds + bytes > lds_max) return false;
        lds += bytes;
        return true;
    };
    // stage the ARP index in LDS when it is small (the nrules_pad multiple of 4 keeps the slot
    // array 16-byte aligned after the bins)
    const uint32_t arp_slots = t.arp_bits ? (1u << t.arp_bits) : 0u;
    const uint32_t ndp_slots = t.ndp_bits ? (1u << t.ndp_bits) : 0u;
    if (arp_slots && arp_slots <= kArpLdsSlots && fits(arp_slots * sizeof(uint4)))
        p.arp_lds = arp_slots;
    if (ndp_slots && ndp_slots <= kNdpLdsSlots && fits(2 * ndp_slots * sizeof(uint4)))
        p.ndp_lds = ndp_slots;
    if (t.tss && t.nfs && fits(t.nfs * sizeof(uint4))) p.fp_lds = t.nfs;
    // the tree's image in LDS first (every lane reads a node per level), then the IPv6 list
    if (p.scan == 3 && t.tree_stage && fits(t.tree_words * sizeof(uint4))) p.tree_lds = t.tree_words;
    if (kFamLds && !t.tss && (p.scan == 3 || !t.fam_all) && t.fam6 &&
        fits(kFamV6Stride * t.fam6 * sizeof(uint4)))
        p.fam6_lds = 1u;
    // the tree kernels' leaf tests read the IPv4 list's rule words too: from LDS when it fits
    if (p.scan == 3 && t.tree_stage && t.fam4 && fits(2 * t.fam4 * sizeof(uint4))) p.fam4_lds = 1u;
    p.lds = lds;
    // the lean emit kernel when nothing it leaves out is needed (non-empty neighbour indexes
    // all in LDS, no flow_hash, no length side array)
    p.lean = !q.flow_hash && (t.tss || !p.gb) && (arp_slots == 0 || p.arp_lds != 0) &&
             (ndp_slots == 0 || p.ndp_lds != 0);
    // a ring launch stamps its batches' completion with the ring kernels (lean emit linear scan)
    // (at most kRingMax batches: one LDS counter each); plan_ring has the last word
    const bool stamp = q.ring_per && q.ring_done && q.emit && p.lean && !t.tss &&
                       q.n / q.ring_per <= (size_t)kRingMax;
    // (the egress list: emit, device batches, never a ring: upe_gpu_process_emit_tx)
    p.var = Variant{t.tss, q.emit, p.lean, p.lean && no_lb,
                    q.tx ? Path::Tx : stamp ? Path::Ring : q.host ? Path::Host : Path::Device,
                    p.scan};
    return p;
}

// ---- tiling -----------------------------------------------------------------------------------
struct Tiling {
    uint32_t tw, ntiles, grid;
};
// Tiles of kWaves chunks (one per wave of a workgroup); a batch too small to give every
// resident workgroup a tile gets narrower tiles, down to one chunk, so that it spreads over
// more CUs (a 10k-packet batch on ten CUs, four waves per SIMD, took 9.2 us; spread, 7.9).
// grid_cap: the workgroups the chip holds at once; the grid is that, or one per tile if fewer
// (an empty batch still launches one workgroup).
inline Tiling plan_tiling(size_t n, uint32_t grid_cap) {
    const uint32_t nchunks = (uint32_t)((n + 63) / 64);
    Tiling t{(uint32_t)kWaves, 0, 0};
    while (t.tw > 1 && (nchunks + t.tw - 1) / t.tw < grid_cap) t.tw >>= 1;
    t.ntiles = (nchunks + t.tw - 1) / t.tw;
    t.grid = t.ntiles == 0 ? 1u : t.ntiles < grid_cap ? t.ntiles : grid_cap;
    return t;
}

// ---- launch size ------------------------------------------------------------------------------
// A launch takes at most kMaxLaunch packets; a larger batch runs as consecutive launches.  The
// bound dates from per-lane counters kept as 16-bit halves (a lane sees at most one packet per
// tile).  upe_classify has no per-lane counters any more: a wave's ballots go into the workgroup's
// 32-bit LDS totals (s_tot), which hold any launch's packets, so that reason no longer applies to
// tables without LDS rule_stats bins (launch_limit below answers kMaxLaunch for them on any grid).
// The bound stays because the group-by is planned and checked for at most that many packets
// (plan_group_by, tools/plan_check.cpp), the deferred look-back list packs a packet index into 31
// bits, and no test runs a longer launch.
constexpr size_t kMaxLaunch = (size_t)1 << 24;
static_assert(kMaxLaunch % 64 == 0, "a split launch starts on a 64-packet group (egress list)");
static_assert(kMaxLaunch <= (size_t)1 << 24, "the group-by is planned for at most 2^24 packets");
// Tables whose rule_stats the classify kernel bins in LDS (LdsPlan::lds_stats) count a workgroup's
// packets and bytes per rule in the two 32-bit halves of one bin.  A workgroup owns the tiles
// blockIdx, blockIdx + grid, ... (plan_tiling), whatever order its waves claim their chunks in, so
// it sees at most ceil(ntiles / grid) * tw * 64 packets: with at most kWgPackets of them, of at
// most 65535 bytes each, neither half can wrap.
constexpr size_t kWgPackets = 65536;
static_assert((uint64_t)kWgPackets * 65535u < (1ull << 32), "a workgroup's bytes on one rule fit 32 bits");
static_assert(kWgPackets % kTile == 0, "whole tiles");
// The most packets of one launch: min_grid = the smallest persistent grid the context can come to
// (a launch's grid_cap is never below it), so that plan_tiling gives no workgroup more than
// kWgPackets packets.  With 256 workgroups or more this is kMaxLaunch.
inline size_t launch_limit(bool lds_stats, uint32_t min_grid) {
    if (!lds_stats) return kMaxLaunch;
    const size_t lim = (size_t)(min_grid ? min_grid : 1u) * kWgPackets;
    return lim < kMaxLaunch ? lim : kMaxLaunch;
}
// The most packets plan_tiling hands one workgroup of the grid.
inline size_t wg_packets(const Tiling& t) {
    return (size_t)((t.ntiles + t.grid - 1) / t.grid) * t.tw * 64u;
}

// ---- ring stamps ------------------------------------------------------------------------------
struct RingPlan {
    bool stamp;
    Variant var;                   // the variant to launch
    uint32_t ring_cpb, ring_mine;  // chunks per batch, and per batch and workgroup
};
// A ring whose caller wants stamps (q.ring_per, q.ring_done): they are written only when every
// workgroup owns the same number of tiles of every batch (at least one).  Otherwise the launch
// runs the plain device-path variant, also on a host-tagged context.
inline RingPlan plan_ring(const LdsPlan& p, const PlanReq& q, const Tiling& t) {
    RingPlan r{p.var.path == Path::Ring, p.var, 0, 0};
    const size_t tpb = (q.ring_per / 64) / t.tw;
    if (r.stamp && (tpb < t.grid || tpb % t.grid != 0)) r.stamp = false;
    if (!r.stamp) {
        r.var.path = Path::Device;
    } else {
        r.ring_cpb = (uint32_t)(q.ring_per / 64);
        r.ring_mine = (uint32_t)(tpb / t.grid * t.tw);
    }
    return r;
}

// ---- rule_stats group-by ------------------------------------------------------------------------
struct GroupByPlan {
    uint32_t nrules, range, nr, chunk, grid_x;   // grid (grid_x, nr)
};
// bins for up to kHistRange rules per workgroup; packet chunks halved (down to kHistChunkMin)
// while the grid has fewer than about kHistTarget workgroups
// (over the rules that can match, sorted indexes 0..nrules-1: the padding block never
// does, and counting it cost config D a fifth range pass over the batch)
inline GroupByPlan plan_group_by(uint32_t nrules, size_t n) {
    GroupByPlan g{};
    g.nrules = nrules ? nrules : 1u;
    g.range = g.nrules < kHistRange ? g.nrules : kHistRange;
    g.nr = (g.nrules + g.range - 1) / g.range;
    g.chunk = kHistChunk;
    while (g.chunk > kHistChunkMin &&
           ((n + g.chunk / 2 - 1) / (g.chunk / 2)) * g.nr <= kHistTarget)
        g.chunk >>= 1;
    g.grid_x = (uint32_t)((n + g.chunk - 1) / g.chunk);
    return g;
}

}  // namespace

#endif  // UPE_PLAN_H
