// upe_ctx.h — the context (struct upe_gpu_ctx) and the few helpers every entry point of the
// library uses (owned device buffers, the carving of a stage's scratch, an empty batch's info,
// timing events, stream order), for the units that hold the host side of the extern "C" ABI: upe_gpu.hip (the
// classify path, create / destroy, the loads), upe_rx.hip, upe_egress.hip, upe_ingress.hip,
// upe_latency.hip, upe_ctrl.hip, upe_neigh_patch.hip, upe_neigh_learn.hip, upe_release.hip,
// upe_hostpath.hip and
// upe_segment.hip.  Internal: not part of
// the ABI, and nothing declared here is exported.
#ifndef UPE_CTX_H
#define UPE_CTX_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/upe_gpu.h"
#include "upe_dev.h"
#include "upe_rules.h"

/* The latency histogram on the device (upe_latency.hip; made at context creation):
 * UPE_LATENCY_REPLICAS copies of a upe_latency_hist_t, UPE_LATENCY_REPLICA_WORDS 64-bit words (one
 * 128-byte line) apart, each in the upe_latency_init state when empty; their upe_latency_merge is
 * the histogram.  A workgroup adds to the copy blockIdx % UPE_LATENCY_REPLICAS, which keeps a
 * launch's atomics from queueing on one line. */
#define UPE_LATENCY_REPLICAS 64
#define UPE_LATENCY_REPLICA_WORDS 16

// What the context holds only through a pointer.  DevState and TilePay are upe_gpu.hip's, in its
// unnamed namespace (TilePay's scope is part of a kernel's symbol); ApplyPool is
// upe_hostpath.hip's, where its holder (HostPath) is therefore made and destroyed.
namespace {
struct DevState;
struct TilePay;
}  // namespace
struct ApplyPool;

#pragma GCC visibility push(hidden)
namespace upe {

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return upe::fail(std::string(#expr) + ": " + hipGetErrorString(e_));             \
    } while (0)

// Makes the context's device current for the duration of an ABI call and restores the caller's
// current device on return (the ABI must not move the calling thread to another device).
struct DevScope {
    int prev = -1;
    hipError_t e;
    explicit DevScope(int d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        e = prev == d ? hipSuccess : hipSetDevice(d);
    }
    ~DevScope() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DevScope(const DevScope&) = delete;
    DevScope& operator=(const DevScope&) = delete;
};
#define DEV_SCOPE(dev)                                                                       \
    upe::DevScope dev_scope_(dev);                                                           \
    HIP_TRY(dev_scope_.e)

// A device allocation of `cap` elements that its holder owns: freed with it, movable, not
// copyable.  It converts to the raw pointer, which is what kernels, Args and DevState take.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // Room for `count` elements: when there is not, the old allocation is freed first and one of
    // `want` elements (>= count: each caller's growth formula) made.  Nothing is kept across a
    // growth, and after a failed one the buffer holds nothing.
    int reserve(size_t count, size_t want) {
        if (count <= cap) return 0;
        reset();
        HIP_TRY(hipMalloc(&p, want * sizeof(T)));
        cap = want;
        return 0;
    }
    // (an empty buffer) `count` elements uploaded from the host; none: stays empty
    int put(const T* src, size_t count) {
        if (reserve(count, count) != 0) return -1;
        if (count) HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
    // (an empty buffer) `count` zeroed elements
    int zeros(size_t count) {
        if (reserve(count, count) != 0) return -1;
        HIP_TRY(hipMemset(p, 0, count * sizeof(T)));
        return 0;
    }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};

// One allocation carved into arrays: take<T>(count) is the next address aligned for T (or to
// `align` bytes, a power of two, where a kernel loads wider than T) and moves past count elements;
// bytes() is what the takes so far need.  Over a null base nothing is dereferenced, so a stage's
// one layout function gives both its scratch size and, over the allocation, its pointers.  The
// base is a hipMalloc'ed address: aligned for every type taken.
struct Carver {
    uintptr_t base;
    size_t used = 0;
    explicit Carver(void* p) : base(reinterpret_cast<uintptr_t>(p)) {}
    template <class T>
    T* take(size_t count, size_t align = alignof(T)) {
        used = (used + align - 1) & ~(align - 1);
        T* p = reinterpret_cast<T*>(base + used);
        used += count * sizeof(T);
        return p;
    }
    size_t bytes() const { return used; }
};
// The bytes a stage's `layout(Carver&, args...)` takes: the layout over no memory.
template <class Layout, class... Args>
size_t layout_bytes(Layout layout, Args... args) {
    Carver none(nullptr);
    layout(none, args...);
    return none.bytes();
}

// Workgroups ("tiles") of `block` items that cover n of them.
inline uint32_t tiles_of(uint32_t n, uint32_t block) {
    return (uint32_t)(((uint64_t)n + block - 1) / block);
}

// What an empty batch leaves in a stage's info, queued on `s`: zero, but for the word that names
// the first packet of a kind, which says "none" (UINT64_MAX).
template <class Info>
int empty_info(Info* d_info, uint64_t Info::*first, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(d_info, 0, sizeof(Info), s));
    HIP_TRY(hipMemsetAsync(&(d_info->*first), 0xFF, sizeof(uint64_t), s));
    return 0;
}

// The timing events of one diagnostic call (the _timed entry points), destroyed with it: N - 2
// around the call's N - 3 passes, then a pair around a yardstick copy.
template <int N>
struct Events {
    hipEvent_t e[N] = {};
    Events() = default;
    Events(const Events&) = delete;
    Events& operator=(const Events&) = delete;
    ~Events() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int create() {
        for (hipEvent_t& x : e) HIP_TRY(hipEventCreate(&x));
        return 0;
    }
    int elapsed(float* ms, int from, int to) {
        HIP_TRY(hipEventElapsedTime(ms, e[from], e[to]));
        return 0;
    }
    // The end of such a call, once the passes' events are recorded: a plain copy on `s` between
    // the last two events, waited for (`what` names it in the error); then ms[k] = pass k's time
    // and ms[N - 3] = the copy's.
    int yardstick(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s,
                  const char* what, float* ms) {
        if (hipEventRecord(e[N - 2], s) != hipSuccess ||
            hipMemcpyAsync(dst, src, bytes, kind, s) != hipSuccess ||
            hipEventRecord(e[N - 1], s) != hipSuccess || hipEventSynchronize(e[N - 1]) != hipSuccess)
            return fail(what);
        for (int k = 0; k < N - 3; ++k)
            if (elapsed(&ms[k], k, k + 1) != 0) return -1;
        return elapsed(&ms[N - 3], N - 2, N - 1);
    }
};

// The neighbour snapshot on the device (NeighIndex): one value, uploaded whole and then swapped
// into the context (upe_gpu_load_neigh_image), or looked up in for one call and dropped
// (upe_gpu_resolve_keys' dry run, upe_neigh.hip).
struct NeighTable {
    DevBuf<uint4> arp, ndp;
    uint32_t arp_bits = 0, arp_seed = 0, ndp_bits = 0, ndp_seed = 0;
    // (an empty table)
    int upload(const NeighImage& im) {
        if (arp.put(im.arp.data(), im.arp.size()) || ndp.put(im.ndp.data(), im.ndp.size()))
            return -1;
        arp_bits = im.arp_bits, arp_seed = im.arp_seed;
        ndp_bits = im.ndp_bits, ndp_seed = im.ndp_seed;
        return 0;
    }
};

// The compiled rule table on the device (upe_rule_image, upe_rules.h): one value, uploaded whole
// and then swapped into the context (install_image).
struct DeviceTable {
    DevBuf<RuleV4> rv4;
    DevBuf<RuleV6> rv6;
    DevBuf<int2> rinfo;
    DevBuf<uint4> fam;                // FamTable image (linear-scan tables > kSmallRules)
    uint32_t fam4 = 0, fam6 = 0, fam_all = 0, fam_x1idx = 0;
    // whether a packet of each family can be forwarded at all under the table: some rule it can
    // reach first (up to its family's first catch-all) forwards
    bool fwd4 = true, fwd6 = true;
    uint32_t nrules = 0, nrules_pad = 0;
    std::vector<int2> rinfo_host;     // (action, rule_id) per sorted index
    // tuple-space index of large tables (null when the linear scan is used)
    DevBuf<TssGroup> tg4, tg6;
    DevBuf<uint4> tt4, tt6;
    DevBuf<uint16_t> tfs;             // staged fingerprint image
    uint32_t nfs = 0;                 // its length in uint4
    uint32_t ng4 = 0, ng6 = 0;
    bool tss = false;
    // decision-tree index over the family lists (null / tree_ok false when not used)
    DevBuf<uint4> tree;
    bool tree_ok = false;
    uint32_t tree_words = 0, tree_loff = 0;
    upe_rule_index_info_t tree_info = {};

    // (an empty table) every image of `im` on the device
    int upload(const upe_rule_image& im) {
        const TreeImage& t = im.t;
        if (rv4.put(im.v4.data(), im.pad) || rv6.put(im.v6.data(), im.pad) ||
            rinfo.put(im.info.data(), im.pad) || fam.put(im.fimg.data(), im.fimg.size()) ||
            (im.tss && (tfs.put(im.fps.data(), im.fps.size()) ||
                        tg4.put(im.f4.groups.data(), im.f4.groups.size()) ||
                        tg6.put(im.f6.groups.data(), im.f6.groups.size()) ||
                        tt4.put(im.f4.slots.data(), im.f4.slots.size()) ||
                        tt6.put(im.f6.slots.data(), im.f6.slots.size()))) ||
            (im.tree_ok && tree.put(im.timg.data(), im.timg.size())))
            return -1;
        fam4 = im.fam4, fam6 = im.fam6, fam_all = im.fam_all, fam_x1idx = im.fam_x1idx;
        fwd4 = im.fwd4, fwd6 = im.fwd6;
        nrules = (uint32_t)im.count;
        nrules_pad = (uint32_t)im.pad;
        rinfo_host = im.info;
        tss = im.tss;
        nfs = tss ? (uint32_t)(im.fps.size() / 8) : 0u;
        ng4 = tss ? (uint32_t)im.f4.groups.size() : 0u;
        ng6 = tss ? (uint32_t)im.f6.groups.size() : 0u;
        tree_ok = im.tree_ok;
        tree_words = tree_ok ? (uint32_t)im.timg.size() : 0u;
        tree_loff = tree_ok ? (uint32_t)(2 * t.nodes.size()) : 0u;
        if (tree_ok)
            tree_info = upe_rule_index_info_t{(uint64_t)t.nodes.size(), (uint64_t)t.leaves.size(),
                                              t.depth[0], t.depth[1], t.max_leaf,
                                              t.trees[0] | t.trees[1] << 16};
        return 0;
    }
};

}  // namespace upe

struct upe_gpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int cus = 256;
    int blocks_per_cu_override = 0;   // UPE_GPU_BLOCKS_PER_CU (diagnostic)
    uint32_t grid_cap = 0;            // UPE_GPU_GRID_CAP (diagnostic): 0 = none
    bool host_tag = false;   // launches on behalf of a host-side loop (upe_gpu_tag_host)
    bool tree_stage = true;  // stage a decision tree's image in LDS when it fits (UPE_GPU_TREE_LDS)
    uint32_t port_mac_lo = 0, port_mac_hi = 0, port_ip4 = 0;
    // what the launches classify with: each a value that a load uploads whole and then swaps in
    upe::DeviceTable table;        // the compiled rule table (install_image)
    upe::NeighTable neigh;         // the neighbour snapshot (upe_gpu_load_neigh)
    template <class T> using DevBuf = upe::DevBuf<T>;
    // rule_stats: they outlive a table (upe_gpu_load_rules credits them by rule_id)
    struct Stats {
        size_t cap = 0;                       // rule_stats capacity
        DevBuf<unsigned long long> rule;      // [cap][2] rule_stats by rule_id
        DevBuf<unsigned long long> idx;       // [kStatReps][pad][2] totals per sorted index, pad
                                              // the largest table so far
        DevBuf<unsigned long long> hist_part; // [chunks][nrules] dense group-by partials
        DevBuf<uint32_t> gb;                  // group-by keys (u32), or u16 lengths
    } stats;
    // state: one DevState allocation (see "Sequential state between batches", upe_gpu.hip)
    DevBuf<DevState> st;
    DevBuf<TilePay> pay;           // [2][paycap] per-workgroup last-hit payloads, by batch parity
    uint32_t paycap = 0;           // largest grid
    // launch bookkeeping
    uint64_t k = 0;                // launches so far: the next batch is batch k
    uint32_t last_n = 0;           // the last batch's size (batch_info)
    int last_var = -1;             // kernel variant of the last classify launch
    uint32_t last_grid = 0;
    bool have_batch = false;
    // every launch and state upload is ordered after the previous one, whatever its stream
    hipStream_t last_stream = nullptr;
    hipEvent_t order_ev = nullptr;
    std::map<uint64_t, uint32_t> resident;   // persistent grid per (lds, variant word) (census)
    hipEvent_t marks[4] = {};      // worker loop completion marks (upe_gpu_mark)
    // the look-back between a batch's chunks, and the switch to the kernel without it (kNoLB): the
    // launches' start-state agreement, written by the device into host-mapped memory, and the
    // first launch whose report counts
    struct LookBack {
        // per-batch scratch, for tiles of kWaves chunks
        DevBuf<uint32_t> flags;    // a look-back flag per chunk (zeroed at allocation)
        DevBuf<uint32_t> defer;    // 64 deferred look-back candidates (two words each) per chunk
        uint32_t spin = 5000;      // look-back wait before deferring (UPE_GPU_LB_SPIN, 100 MHz ticks)
        bool sync = false;         // UPE_GPU_LB_SYNC=1: wait for each launch's agreement report
        bool allow_nolb = true;    // UPE_GPU_NOLB=0: never use the kernels without look-back
        bool no_lb = false;
        uint64_t reset_k = 0;
        unsigned long long* agree_h = nullptr;
        unsigned long long* agree_d = nullptr;
    } lb;
    // kernel timing (upe_gpu_timing_*)
    struct Timing {
        bool on = false;
        uint32_t every = 1, calls = 0;   // sample every n-th process() call
        uint32_t phase = 0;        // samples open at calls c with c % every == phase
        uint32_t span = 1;         // calls one sample's event pair brackets
        uint32_t left = 0;         // calls left in the open sample (0: none open)
        uint64_t launches = 0;     // calls covered by closed samples
        std::vector<hipEvent_t> ev;    // event pool, 3 per sample
        size_t ev_used = 0;        // 3 per closed sample: start, after the classify, end
        std::vector<bool> ev_mid;  // per closed sample: the middle event was recorded
    } timing;
    // host round trip (upe_gpu_process_host, upe_hostpath.hip): copy streams and the device slots
    struct HostSlot {
        DevBuf<uint8_t> frames;
        DevBuf<uint64_t> desc;          // desc, verdict (and hdr, once used) hold as many packets
        DevBuf<uint32_t> verdict;
        DevBuf<upe_hdr_rec_t> hdr;      // emit-mode records (upe_gpu_process_host_emit)
        hipEvent_t in_done = nullptr, k_done = nullptr, out_done = nullptr;
        bool busy = false;
        uint64_t lo = 0, wb = 0;   // host byte range the slot's copy-back writes
    };
    struct HostPath {
        hipStream_t s_in = nullptr, s_out = nullptr;
        HostSlot slots[8];
        uint32_t nslots = 4;       // slots in use (UPE_GPU_HOST_SLOTS, 2..8)
        // host threads applying emit-mode records to the caller's frames
        // (upe_gpu_process_host_emit)
        std::unique_ptr<ApplyPool> pool;
        HostPath();    // both in upe_hostpath.hip, where ApplyPool is complete
        ~HostPath();
    } host;
    // upe_gpu_process_segmented scratch (upe_segment.hip): marks / index per packet, gathered
    // windows per mark
    struct SegScratch {
        DevBuf<uint32_t> marks, index;
        DevBuf<uint64_t> count;
        DevBuf<uint8_t> win;
        DevBuf<uint32_t> lens;
        // upe_gpu_process_segmented_resident: the batch's records behind their upe_ctrl_info_t
        DevBuf<uint4> rec;
        DevBuf<upe_neigh_patch_info_t> pinfo;   // its patches' info (nobody reads it)
    } seg;
    // single-use scratch
    DevBuf<uint32_t> compact_counts;      // upe_gpu_compact: per-block counts
    DevBuf<uint8_t> rx_scratch;           // upe_gpu_rx_dispatch: the passes' tile table (upe_rx.hip)
    DevBuf<uint8_t> eg_scratch;           // upe_gpu_egress_pack: the tile table (upe_egress.hip)
    DevBuf<uint8_t> in_scratch;           // upe_gpu_ingress_gather: tile table + meta (upe_ingress.hip)
    DevBuf<uint8_t> cw_scratch;           // upe_gpu_ctrl_writes: tile table + words (upe_ctrl.hip)
    DevBuf<uint8_t> np_scratch;           // upe_gpu_neigh_patch: tile table + words (upe_neigh_patch.hip)
    DevBuf<uint8_t> rl_scratch;           // upe_gpu_release_order: tile table + bitmaps (upe_release.hip)
    DevBuf<uint32_t> np_owner;            // its owner word per index slot, ARP then NDP: zero between calls
    DevBuf<unsigned long long> ring_wg;   // ring launches: per-batch counters + time origin
    // the latency histogram (upe_gpu_latency_record, upe_latency.hip): replicas of the 12 words
    // of a upe_latency_hist_t, touched by nothing but the four latency calls
    DevBuf<unsigned long long> lat_hist;
    double cycles_per_ns = 0.0;           // upe_gpu_set_tsc: 0 until it succeeds once
    // upe_gpu_neigh_learn's state beside the loaded snapshot (upe_neigh_learn.hip): what the
    // loaded image says of each family {ARP, NDP} — its free count and whether it takes new
    // addresses — set by a load; the free counts as the learns since that load left them live on
    // the device (made by the first learn; a load needs no device work for them: the first learn
    // after it takes the image's counts as arguments).
    struct Learn {
        uint32_t image_free[2] = {0, 0};
        bool insertable[2] = {false, false};
        bool on_device = false;           // `free` holds the counts (a learn ran since the load)
        DevBuf<uint32_t> free;            // {ARP, NDP, 0, 0}
        void loaded(const upe::NeighImage& im) {
            image_free[0] = im.arp_free, image_free[1] = im.ndp_free;
            insertable[0] = im.arp_insertable, insertable[1] = im.ndp_insertable;
            on_device = false;
        }
    } learn;
};

namespace upe {

inline hipStream_t pick(upe_gpu_ctx* c, void* s) { return s ? (hipStream_t)s : c->stream; }

// The device address of page-locked, mapped host memory; nullptr (and an error) for anything
// else, so that a kernel never dereferences an unmapped host address.
template <typename T>
T* mapped(T* h, const char* what) {
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<void*>(static_cast<const void*>(h)), 0) != hipSuccess ||
        !d) {
        (void)hipGetLastError();
        fail(std::string(what) + " is not pinned, mapped host memory (upe_gpu_host_alloc / "
             "upe_gpu_host_register)");
        return nullptr;
    }
    return static_cast<T*>(d);
}

// Order work about to be queued on `s` after everything queued so far on the context's state
// (the last launch, or a state upload), whatever stream that went to.
inline int order_on(upe_gpu_ctx* c, hipStream_t s) {
    if (c->last_stream && c->last_stream != s) {
        HIP_TRY(hipEventRecord(c->order_ev, c->last_stream));
        HIP_TRY(hipStreamWaitEvent(s, c->order_ev, 0));
    }
    c->last_stream = s;
    return 0;
}

// Where the device allocation that holds `p` ends; `otherwise` when p is not a device
// allocation's pointer (mapped host memory).  A caller's buffer counts up to there when an output
// is kept apart from it: where the buffer itself ends is not known.
inline uintptr_t alloc_end(const void* p, uintptr_t otherwise) {
    hipDeviceptr_t abase = nullptr;
    size_t asize = 0;
    if (hipMemGetAddressRange(&abase, &asize, const_cast<void*>(p)) == hipSuccess)
        return reinterpret_cast<uintptr_t>(abase) + asize;
    (void)hipGetLastError();
    return otherwise;
}

// packets per workgroup of upe_gpu_compact's kernels (upe_gpu.hip); upe_gpu_process_segmented
// bounds its batch by it too
constexpr uint32_t kCompactBlock = 4096;   // 256 threads x 16

// A ring launch's completion stamps (upe_gpu_process_ring_emit): batches of `per` packets.
struct RingReq {
    size_t per;
    unsigned long long* done;   // [count] ns after the first workgroup's start, 0 = not stamped
};
// One request to process_impl: a batch in device-visible memory, and what is wanted beside the
// verdicts.
struct ProcessReq {
    uint8_t* frames;
    const uint64_t* desc;
    uint32_t* verdict;
    size_t n;
    void* stream;
    upe_hdr_rec_t* hdr = nullptr;    // emit mode: [n] rewritten-header records, frames only read
    uint32_t* flow_hash = nullptr;   // [n] flow hashes (RSS)
    const RingReq* ring = nullptr;   // the batch is a ring of batches
    bool host = false;               // launched for a host path (Path::Host)
    uint32_t* tx = nullptr;          // the egress list (Path::Tx) and its per-group counts
    uint32_t* tx_cnt = nullptr;
    size_t tx_base = 0;              // the launch's first packet in the caller's batch
};
// One batch through the classify launch (upe_gpu.hip); the host paths (upe_hostpath.hip) call it
// with requests of their own.
UPE_INTERNAL int process_impl(upe_gpu_ctx_t* c, const ProcessReq& q);

// Around a change of the loaded neighbour snapshot's MACs in place (upe_gpu_neigh_patch,
// upe_neigh_patch.hip), both queued on `s` (upe_gpu.hip, beside the load they mirror).
// neigh_patching: `s` ordered after everything the context has queued, and the last batch's L1
// outcome folded into the state the next batch starts from, before the tables change.
// neigh_patched: do the L1 entries agree with the tables now?  (The entries themselves stay.)
UPE_INTERNAL int neigh_patching(upe_gpu_ctx_t* c, hipStream_t s);
UPE_INTERNAL int neigh_patched(upe_gpu_ctx_t* c, hipStream_t s);

// The empty latency histogram's device image (upe_latency.hip): every replica in the
// upe_latency_init state.  Context creation uploads it.
UPE_INTERNAL int latency_init_image(std::vector<unsigned long long>& img);

}  // namespace upe
#pragma GCC visibility pop

#endif  // UPE_CTX_H
