// The launch plan (upe_amd/csrc/upe_plan.h) on the CPU, stand-alone: `make -C upe_amd/csrc
// plan-check` builds this file under the host sanitizers (-fsanitize=address,undefined) and runs
// it.  The expected values are worked out by hand from the planning rules at the default UPE_*
// settings: which upe_classify variant a launch asks for, its dynamic LDS region by region, the
// tiling and grid, the ring stamps, the rule_stats group-by's shape, and the widths the accounting
// relies on (a group-by chunk's 24-bit packet count, a workgroup's 32-bit byte bins).
#include <stdio.h>

#include <set>

#include "../upe_amd/csrc/upe_plan.h"

static int g_bad = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "plan_check:%d: %s\n", __LINE__, #cond);         \
            ++g_bad;                                                         \
        }                                                                    \
    } while (0)

// a linear-scan table with empty neighbour indexes, and a device-path emit batch
static TableShape linear(uint32_t nrules, uint32_t pad) {
    TableShape t{};
    t.nrules = nrules;
    t.nrules_pad = pad;
    t.tree_stage = true;
    return t;
}
static PlanReq emit_batch(size_t n) {
    PlanReq q{};
    q.n = n;
    q.emit = true;
    return q;
}

static void small_table() {
    TableShape t = linear(8, 8);
    t.arp_bits = 9;
    PlanReq q = emit_batch(1000);
    const LdsPlan p = plan_lds(t, q, false);
    CHECK(p.lds_stats && p.scan == 0 && p.hist == 64 && p.arp_lds == 512 && p.ndp_lds == 0);
    CHECK(p.lds == 8256 && !p.gb && p.lean);
    CHECK(variant_word(p.var) == 5);
    CHECK(variant_word(plan_lds(t, q, true).var) == 13);
    q.flow_hash = true;
    CHECK(!plan_lds(t, q, false).lean && variant_word(plan_lds(t, q, false).var) == 1);
    q.flow_hash = false;
    q.tx = true;
    CHECK(variant_word(plan_lds(t, q, false).var) == 53);
}

static void tiling() {
    const struct {
        size_t n;
        uint32_t tw, ntiles, grid;
    } cases[] = {{1048576, 16, 1024, 256}, {10000, 1, 157, 157}, {64, 1, 1, 1}, {0, 1, 0, 1}};
    for (const auto& c : cases) {
        const Tiling t = plan_tiling(c.n, 256);
        CHECK(t.tw == c.tw && t.ntiles == c.ntiles && t.grid == c.grid);
    }
}

static void greedy_order() {
    TableShape t = linear(4096, 4096);
    t.tree_ok = true;
    t.tree_words = 1500;
    t.fam4 = 32;
    t.fam6 = 100;
    t.arp_bits = t.ndp_bits = 11;
    LdsPlan p = plan_lds(t, emit_batch(1000), false);
    CHECK(p.scan == 3 && p.hist == 32768 && p.arp_lds == 2048 && p.ndp_lds == 2048);
    // the IPv6 list would make 163072 bytes, over the 158 KB: skipped, the IPv4 list still fits
    CHECK(p.tree_lds == 1500 && p.fam6_lds == 0 && p.fam4_lds == 1 && p.lds == 156096 && p.lean);
    t.tree_stage = false;
    p = plan_lds(t, emit_batch(1000), false);
    CHECK(p.tree_lds == 0 && p.fam4_lds == 0 && p.fam6_lds == 1 && p.lds == 139072);
    // fam6_lds needs a list, and under scan 1 or 2 no catch-all family
    t.fam6 = 0;
    CHECK(plan_lds(t, emit_batch(1000), false).fam6_lds == 0);
    t.fam6 = 100;
    t.tree_ok = false;
    CHECK(plan_lds(t, emit_batch(1000), false).scan == 1);
    CHECK(plan_lds(t, emit_batch(1000), false).fam6_lds == 1);
    t.fam_all = true;
    CHECK(plan_lds(t, emit_batch(1000), false).scan == 2);
    CHECK(plan_lds(t, emit_batch(1000), false).fam6_lds == 0);
}

static void past_the_bins() {
    TableShape t = linear(4100, 4100);
    LdsPlan p = plan_lds(t, emit_batch(1000), false);
    CHECK(!p.lds_stats && p.hist == 0 && p.gb && !p.lean && p.gb_packed == 1);
    CHECK(!plan_lds(t, emit_batch(0), false).gb);
    t.nrules = 65536;
    CHECK(plan_lds(t, emit_batch(1000), false).gb_packed == 1);
    t.nrules = 65537;
    CHECK(plan_lds(t, emit_batch(1000), false).gb_packed == 0);
}

static void tuple_space() {
    TableShape t = linear(65536, 65536);
    t.tss = true;
    t.nfs = 1024;
    t.arp_bits = t.ndp_bits = 11;
    LdsPlan p = plan_lds(t, emit_batch(1000), false);
    CHECK(p.scan == 0 && p.hist == 0 && p.fp_lds == 1024 && p.lds == 114688);
    CHECK(p.gb && p.lean && variant_word(p.var) == 7);
    t.arp_bits = 12;
    p = plan_lds(t, emit_batch(1000), false);
    CHECK(p.arp_lds == 0 && !p.lean);
}

static RingPlan ring(const TableShape& t, size_t per, size_t count, Path* first) {
    PlanReq q = emit_batch(per * count);
    q.ring_per = per;
    q.ring_done = true;
    const LdsPlan p = plan_lds(t, q, false);
    *first = p.var.path;
    return plan_ring(p, q, plan_tiling(q.n, 256));
}

static void ring_stamps() {
    TableShape t = linear(8, 8);
    Path first;
    RingPlan r = ring(t, 262144, 4, &first);
    CHECK(first == Path::Ring && r.stamp && r.ring_cpb == 4096 && r.ring_mine == 16);
    CHECK(r.var.path == Path::Ring && variant_built(r.var));
    // 100 tiles per batch for 256 workgroups
    r = ring(t, 102400, 4, &first);
    CHECK(first == Path::Ring && !r.stamp && r.var.path == Path::Device);
    r = ring(t, 1024, 65, &first);
    CHECK(first == Path::Device && !r.stamp && r.var.path == Path::Device);
    r = ring(t, 1024, 64, &first);
    CHECK(first == Path::Ring);
    t.tss = true;
    r = ring(t, 262144, 4, &first);
    CHECK(first == Path::Device && !r.stamp && r.var.path == Path::Device);
    // an unstamped ring runs the device-path variant on a host-tagged context too
    t.tss = false;
    PlanReq q = emit_batch(4 * 102400);
    q.ring_per = 102400;
    q.ring_done = true;
    q.host = true;
    const LdsPlan p = plan_lds(t, q, false);
    CHECK(plan_ring(p, q, plan_tiling(q.n, 256)).var.path == Path::Device);
    q.ring_done = false;   // no stamps asked for: the host path's name stays
    CHECK(plan_lds(t, q, false).var.path == Path::Host);
}

static void group_by() {
    GroupByPlan g = plan_group_by(65536, (size_t)1 << 24);
    CHECK(g.range == 16384 && g.nr == 4 && g.chunk == 262144 && g.grid_x == 64);
    g = plan_group_by(4100, 5000);
    CHECK(g.nrules == 4100 && g.range == 4100 && g.nr == 1 && g.chunk == 8192 && g.grid_x == 1);
    CHECK(plan_group_by(0, 5000).nrules == 1);
}

// The widths the accounting relies on, over the table and batch sizes the accounting tests run
// (tests/accounting_cases.py) and the largest an API call can bring.
static void group_by_widths() {
    const uint32_t small_last = (uint32_t)kSmallRules - (uint32_t)kUnroll;        // pad = kSmallRules
    const uint32_t lds_last = (uint32_t)kLdsStatsMax - (uint32_t)kUnroll;         // pad = kLdsStatsMax
    const uint32_t tables[] = {8, small_last, small_last + 1, 1000, lds_last, lds_last + 1,
                               kHistRange, kHistRange + 1, 65536, 65537, kTssMaxRules};
    const size_t sizes[] = {1, 63, 64, 65, kHistChunkMin - 1, kHistChunkMin, kHistChunkMin + 1,
                            kHistChunkMin + 15, 2 * kHistChunkMin + 1, 40005, (size_t)1 << 24,
                            (size_t)1 << 31, ((size_t)1 << 32) - kTile - 1};
    for (uint32_t nrules : tables)
        for (size_t n : sizes) {
            const GroupByPlan g = plan_group_by(nrules, n);
            CHECK((size_t)g.grid_x * g.chunk >= n);
            CHECK((size_t)g.nr * g.range >= nrules && g.range <= kHistRange);
            CHECK(g.chunk % 8192 == 0);
            CHECK(g.chunk < (1u << 24));   // a chunk's packets on one rule fit the 24-bit field
        }
    // the group-by never sees more than one launch, and a launch is at most 2^24 packets
    CHECK(kMaxLaunch <= (size_t)1 << 24 && launch_limit(false, 1) == kMaxLaunch);
    CHECK(kHistChunk < kMaxLaunch);
    // the classify kernel's LDS bins: no workgroup of any grid gets more than kWgPackets packets
    // of a launch within its limit, so its bytes on one rule stay below 2^32
    CHECK(launch_limit(true, 256) == kMaxLaunch && launch_limit(true, 8) == 8 * kWgPackets);
    CHECK(launch_limit(true, 0) == kWgPackets);
    for (uint32_t floor : {1u, 2u, 8u, 60u, 255u, 256u, 304u}) {
        const size_t lim = launch_limit(true, floor);
        for (uint32_t cap : {floor, 2 * floor, 8 * floor})   // the launch's grid_cap is never below
            for (size_t n : {(size_t)1, (size_t)65, (size_t)kTile + 1, lim / 2 + 1, lim - 1, lim}) {
                const Tiling t = plan_tiling(n, cap);
                CHECK(t.grid <= cap && (size_t)t.ntiles * t.tw * 64 >= n);
                CHECK(wg_packets(t) <= kWgPackets);
                CHECK((uint64_t)wg_packets(t) * 65535u < (1ull << 32));
            }
    }
    // one packet more on the smallest grid would not fit
    CHECK(wg_packets(plan_tiling(launch_limit(true, 8) + 1, 8)) > kWgPackets);
}

static void variants() {
    int built = 0;
    std::set<uint32_t> words;
    for (int scan = 0; scan < 4; ++scan)
        for (Path path : {Path::Device, Path::Ring, Path::Host, Path::Tx})
            for (int bits = 0; bits < 16; ++bits) {
                const Variant v{(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0,
                                path, scan};
                CHECK(variant_word(v) < 256);
                if (!variant_built(v)) continue;
                ++built;
                words.insert(variant_word(v));
            }
    CHECK(built == 83 && words.size() == 83);
}

int main() {
    small_table();
    tiling();
    greedy_order();
    past_the_bins();
    tuple_space();
    ring_stamps();
    group_by();
    group_by_widths();
    variants();
    if (g_bad) return fprintf(stderr, "plan_check: %d checks failed\n", g_bad), 1;
    printf("plan_check: the launch plan agrees with the hand-derived cases\n");
    return 0;
}
