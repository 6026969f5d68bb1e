// upe_segment.hip — upe_gpu_process_segmented (include/upe_gpu.h): a batch whose control packets
// write a neighbour table, run as segments between those packets, each table write applied on
// the host and uploaded before the next segment.  The segments go through the public entry
// points (upe_gpu_process, upe_gpu_compact, upe_gpu_load_neigh); of the context this unit uses
// its scratch (c->seg) alone.  upe_gpu_process_segmented_resident is the same run from the
// records of upe_gpu_ctrl_writes, a refresh queued as a upe_gpu_neigh_patch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "upe_ctx.h"

using namespace upe;

namespace {

// ------------------------------------------------------------------------------------------
// Control packets that write a neighbour table (upe_gpu_process_segmented).  A packet is
// marked when handle_control_packet (reference src/worker.c:23-104) may call arp_update or
// ndp_update for it: ARP with the Ethernet/IPv4 header (the learn does not look at len), or an
// IPv6 NS/NA of at least 78 bytes (whether an option carries the address is decided on the
// host, from the gathered bytes).  Bytes at or past len read as zero (zero-filled pktbuf).
// Marks are verdict-shaped words (code 1 = marked) so upe_gpu_compact lists them in order.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kCtrlWin = 256;   // bytes of each marked frame gathered for the host

__global__ void __launch_bounds__(256) upe_ctrl_mark(const uint8_t* frames, const uint64_t* desc,
                                                     uint32_t n, uint32_t* marks) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t d = desc[i];
    const uint32_t len = (uint32_t)(d & 0xFFFFu);
    const uint8_t* p = frames + (d >> 16);
    auto at = [&](uint32_t k) -> uint32_t { return k < len ? (uint32_t)p[k] : 0u; };
    marks[i] = ctrl_table_write(len, at) ? 1u : 0u;
}

// One workgroup per marked packet: its first kCtrlWin bytes (zero past len) and its length.
__global__ void __launch_bounds__(256) upe_ctrl_gather(const uint8_t* frames, const uint64_t* desc,
                                                       const uint32_t* index, uint8_t* win,
                                                       uint32_t* lens) {
    const uint32_t i = index[blockIdx.x];
    const uint64_t d = desc[i];
    const uint32_t len = (uint32_t)(d & 0xFFFFu);
    const uint32_t k = threadIdx.x;
    win[(size_t)blockIdx.x * kCtrlWin + k] = k < len ? frames[(d >> 16) + k] : (uint8_t)0;
    if (k == 0) lens[blockIdx.x] = len;
}

// The table writes of handle_control_packet, restated on the caller's host slot arrays.
// arp_update, reference src/arp_table.c:26-53: home slot ip & (cap-1), linear probe, insert at
// the first free slot or update the slot holding ip, at most cap probes.
void host_arp_update(upe_arp_entry_t* t, size_t cap, uint32_t ip, const uint8_t* mac,
                     int64_t now) {
    const size_t idx = ip & (cap - 1);
    for (size_t k = 0; k < cap; ++k) {
        upe_arp_entry_t& e = t[(idx + k) & (cap - 1)];
        if (!e.valid || e.ip == ip) {
            if (!e.valid) {
                e.valid = true;
                e.ip = ip;
            }
            memcpy(e.mac, mac, 6);
            e.update_at = now;
            return;
        }
    }
}

// ndp_update, reference src/ndp_table.c:39-65 (hash_ipv6 :6-17: XOR of the address's four
// native-endian words, & (cap-1)).
void host_ndp_update(upe_ndp_entry_t* t, size_t cap, const uint8_t* ip, const uint8_t* mac,
                     int64_t now) {
    const uint32_t h = le32(ip) ^ le32(ip + 4) ^ le32(ip + 8) ^ le32(ip + 12);
    const size_t idx = h & (cap - 1);
    for (size_t k = 0; k < cap; ++k) {
        upe_ndp_entry_t& e = t[(idx + k) & (cap - 1)];
        if (!e.valid || memcmp(e.ip, ip, 16) == 0) {
            if (!e.valid) {
                e.valid = true;
                memcpy(e.ip, ip, 16);
            }
            memcpy(e.mac, mac, 6);
            e.update_at = now;
            return;
        }
    }
}

}  // namespace

extern "C" int upe_gpu_process_segmented(upe_gpu_ctx_t* c, uint8_t* d_frames,
                                         const uint64_t* d_desc, uint32_t* d_verdict, size_t n,
                                         upe_arp_entry_t* arp, size_t arp_capacity,
                                         upe_ndp_entry_t* ndp, size_t ndp_capacity, int64_t now,
                                         size_t* n_writes, void* stream) {
    if (!c) return fail("null context");
    if (n_writes) *n_writes = 0;
    if (n > 0xFFFFFFFFull - kCompactBlock) return fail("batch too large (n must fit in 32 bits)");
    if (n && (!d_frames || !d_desc || !d_verdict)) return fail("null batch buffer");
    if ((arp_capacity && !arp) || (ndp_capacity && !ndp)) return fail("null neighbour table");
    if ((arp_capacity & (arp_capacity - 1)) || (ndp_capacity & (ndp_capacity - 1)))
        return fail("neighbour table capacities must be powers of two");
    if (n == 0) return upe_gpu_process(c, d_frames, d_desc, d_verdict, 0, stream);
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    // 1. mark and list the table-writing control packets, in packet order
    if (n > c->seg.index.cap) {   // (the last one made: all are there when it is)
        c->seg.marks.reset();
        c->seg.index.reset();
        if (c->seg.count.reserve(1, 1) != 0 ||   // once
            c->seg.marks.reserve(n, n) != 0 || c->seg.index.reserve(n, n) != 0)
            return -1;
    }
    hipLaunchKernelGGL(upe_ctrl_mark, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s,
                       d_frames, d_desc, (uint32_t)n, c->seg.marks);
    HIP_TRY(hipGetLastError());
    if (upe_gpu_compact(c, c->seg.marks, n, 1u, c->seg.index, c->seg.count, s) != 0) return -1;
    uint64_t cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, c->seg.count, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (cnt == 0) return upe_gpu_process(c, d_frames, d_desc, d_verdict, n, stream);
    // 2. their bytes, gathered before any segment runs (the ARP reply is built in place)
    if (cnt > c->seg.lens.cap) {   // (the last one made)
        c->seg.win.reset();
        c->seg.lens.reset();
        if (c->seg.win.reserve(cnt * kCtrlWin, cnt * kCtrlWin) != 0 ||
            c->seg.lens.reserve(cnt, cnt) != 0)
            return -1;
    }
    hipLaunchKernelGGL(upe_ctrl_gather, dim3((uint32_t)cnt), dim3(kCtrlWin), 0, s, d_frames,
                       d_desc, c->seg.index, c->seg.win, c->seg.lens);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> idx(cnt), lens(cnt);
    std::vector<uint8_t> win(cnt * kCtrlWin);
    HIP_TRY(hipMemcpyAsync(idx.data(), c->seg.index, cnt * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(lens.data(), c->seg.lens, cnt * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(win.data(), c->seg.win, win.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // 3. segments: up to and including each control packet, then its table write
    size_t start = 0, writes = 0;
    std::vector<uint8_t> full;
    for (uint64_t j = 0; j < cnt; ++j) {
        const size_t k = idx[j];
        if (upe_gpu_process(c, d_frames, d_desc + start, d_verdict + start, k + 1 - start,
                            stream) != 0)
            return -1;
        start = k + 1;
        const uint8_t* b = win.data() + j * kCtrlWin;
        const uint32_t len = lens[j];
        bool wrote = false;
        if (b[12] == 0x08 && b[13] == 0x06) {
            // ARP learn, src/worker.c:30-39: spa (network order) -> host order, sha
            if (arp_capacity) {
                const uint32_t spa = (uint32_t)b[28] << 24 | (uint32_t)b[29] << 16 |
                                     (uint32_t)b[30] << 8 | (uint32_t)b[31];
                host_arp_update(arp, arp_capacity, spa, b + 22, now);
                wrote = true;
            }
        } else {
            // NS / NA option walk, src/worker.c:64-95, over the whole frame when it is long.
            // This reads len bytes at the frame start: the call takes full frames only
            // (include/upe_gpu.h), never the UPE_FRAME_TAIL-byte header windows of the host path.
            const uint8_t* f = b;
            if (len > kCtrlWin) {
                uint64_t d = 0;
                HIP_TRY(hipMemcpy(&d, d_desc + k, sizeof d, hipMemcpyDeviceToHost));
                full.assign(len, 0);
                HIP_TRY(hipMemcpy(full.data(), d_frames + (d >> 16), len, hipMemcpyDeviceToHost));
                f = full.data();
            }
            const bool ns = f[54] == 135;
            for (size_t off = 78; off + 2 <= len;) {
                // uint8_t opt_len, as the reference's (src/worker.c:73): 32 wraps to 0, 33 to 8
                const uint32_t ot = f[off], ol = (uint8_t)(f[off + 1] * 8u);
                if (ol == 0 || off + ol > len) break;
                if (ol >= 8 && ((ns && ot == 1) || (!ns && ot == 2))) {
                    if (ndp_capacity) {
                        host_ndp_update(ndp, ndp_capacity, ns ? f + 22 : f + 62, f + off + 2, now);
                        wrote = true;
                    }
                    break;
                }
                off += ol;
            }
        }
        if (wrote) {
            ++writes;
            // the next segment reads the new snapshot (load_neigh waits for the context's
            // stream; a caller stream is drained first)
            if (s != c->stream) HIP_TRY(hipStreamSynchronize(s));
            if (upe_gpu_load_neigh(c, arp, arp_capacity, ndp, ndp_capacity) != 0) return -1;
        }
    }
    if (start < n &&
        upe_gpu_process(c, d_frames, d_desc + start, d_verdict + start, n - start, stream) != 0)
        return -1;
    HIP_TRY(hipStreamSynchronize(s));
    if (n_writes) *n_writes = writes;
    return 0;
}

// The same run from the batch's records (upe_gpu_ctrl_writes): the host sees 32 bytes per table
// write and no frame byte, and a write to an address the tables hold — a refresh — is queued as a
// patch of the loaded snapshot (upe_gpu_neigh_patch) behind its segment, with no synchronisation
// and no rebuild.  Only a write that teaches a new address takes upe_gpu_load_neigh.
extern "C" int upe_gpu_process_segmented_resident(upe_gpu_ctx_t* c, uint8_t* d_frames,
                                                  const uint64_t* d_desc, uint32_t* d_verdict,
                                                  size_t n, upe_arp_entry_t* arp,
                                                  size_t arp_capacity, upe_ndp_entry_t* ndp,
                                                  size_t ndp_capacity, int64_t now,
                                                  upe_segment_info_t* info, void* stream) {
    if (!c) return fail("null context");
    if (info) *info = upe_segment_info_t{0, 0, 0, 0};
    if (n > 0xFFFFFFFFull - kCompactBlock) return fail("batch too large (n must fit in 32 bits)");
    if (n && (!d_frames || !d_desc || !d_verdict)) return fail("null batch buffer");
    if ((arp_capacity && !arp) || (ndp_capacity && !ndp)) return fail("null neighbour table");
    if ((arp_capacity & (arp_capacity - 1)) || (ndp_capacity & (ndp_capacity - 1)))
        return fail("neighbour table capacities must be powers of two");
    if (n == 0) return upe_gpu_process(c, d_frames, d_desc, d_verdict, 0, stream);
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    // 1. the batch's records, in packet order, behind their info: one copy to the host covers
    // both (the first kEager records; a batch with more takes a second copy)
    constexpr size_t kEager = 1024;
    static_assert(sizeof(upe_ctrl_info_t) == 2 * sizeof(uint4) &&
                      sizeof(upe_ctrl_write_t) == 2 * sizeof(uint4), "record buffer layout");
    if (c->seg.pinfo.reserve(1, 1) != 0) return -1;
    std::vector<upe_ctrl_write_t> rec;
    upe_ctrl_info_t ci;
    size_t cap = c->seg.rec.cap ? c->seg.rec.cap / 2 - 1 : 64;
    upe_ctrl_write_t* d_rec = nullptr;
    for (;;) {
        if (c->seg.rec.reserve(2 * (cap + 1), 2 * (cap + 1)) != 0) return -1;
        d_rec = reinterpret_cast<upe_ctrl_write_t*>(c->seg.rec.p + 2);
        if (upe_gpu_ctrl_writes(c, d_frames, d_desc, n, d_rec, cap,
                                reinterpret_cast<upe_ctrl_info_t*>(c->seg.rec.p), s) != 0)
            return -1;
        const size_t eager = cap < kEager ? cap : kEager;
        rec.resize(eager + 1);   // slot 0: the info
        HIP_TRY(hipMemcpyAsync(rec.data(), c->seg.rec.p, (eager + 1) * sizeof(upe_ctrl_write_t),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        memcpy(&ci, rec.data(), sizeof ci);
        if (ci.writes <= cap) break;
        cap = (size_t)ci.writes + (size_t)ci.writes / 4;   // a batch with more records: again
    }
    rec.erase(rec.begin());
    if (ci.writes > rec.size()) {
        const size_t have = rec.size();
        rec.resize((size_t)ci.writes);
        HIP_TRY(hipMemcpyAsync(rec.data() + have, d_rec + have,
                               (rec.size() - have) * sizeof(upe_ctrl_write_t),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    rec.resize((size_t)ci.writes);
    // 2. where the batch is cut: after every marked packet, as upe_gpu_process_segmented cuts it
    // (a verdict's UPE_VF_L1_INIT is defined against the entry its segment starts from).  Every
    // record's packet is marked; when some marked packet has no record (an NS / NA without the
    // option) the marked packets are listed on the device as that call lists them — positions,
    // not bytes.
    std::vector<uint32_t> cut(rec.size());
    for (size_t j = 0; j < rec.size(); ++j) cut[j] = rec[j].index;
    if (ci.ctrl > ci.writes) {
        if (n > c->seg.index.cap) {   // (the last one made: all are there when it is)
            c->seg.marks.reset();
            c->seg.index.reset();
            if (c->seg.count.reserve(1, 1) != 0 || c->seg.marks.reserve(n, n) != 0 ||
                c->seg.index.reserve(n, n) != 0)
                return -1;
        }
        hipLaunchKernelGGL(upe_ctrl_mark, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s,
                           d_frames, d_desc, (uint32_t)n, c->seg.marks);
        HIP_TRY(hipGetLastError());
        if (upe_gpu_compact(c, c->seg.marks, n, 1u, c->seg.index, c->seg.count, s) != 0) return -1;
        cut.resize((size_t)ci.ctrl);
        HIP_TRY(hipMemcpyAsync(cut.data(), c->seg.index, cut.size() * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    // 3. segments: up to and including each marked packet, then its table write, if it has one
    upe_segment_info_t out = {0, 0, 0, ci.ctrl};
    size_t start = 0, j = 0;
    for (const uint32_t k : cut) {
        if (upe_gpu_process(c, d_frames, d_desc + start, d_verdict + start, k + 1 - start,
                            stream) != 0)
            return -1;
        start = (size_t)k + 1;
        if (j == rec.size() || rec[j].index != k) continue;   // a marked packet without a record
        const upe_ctrl_write_t& w = rec[j];
        const upe_ctrl_write_t* d_w = d_rec + j;
        ++j;
        const bool v6 = w.kind == UPE_CW_NDP;
        if (!(v6 ? ndp_capacity : arp_capacity)) continue;   // no table of its family: no write
        // does a probe of the tables reach the address (before the write)?  Then the write is a
        // refresh: it rewrites that slot's MAC, and the snapshot's index keeps its shape
        upe_flow_key_t key;
        memset(&key, 0, sizeof key);
        key.ip_ver = v6 ? 6 : 4;
        memcpy(key.dst_ip.v6, w.ip, 16);
        uint64_t mac = 0;
        if (upe_neigh_lookup_host(arp, arp_capacity, ndp, ndp_capacity, &key, 1, &mac) != 0 ||
            upe_neigh_apply_writes(arp, arp_capacity, ndp, ndp_capacity, &w, 1, now, nullptr) != 0)
            return fail(upe_host_last_error());
        ++out.writes;
        if (mac & UPE_MAC_FOUND) {
            if (upe_gpu_neigh_patch(c, d_w, 1, nullptr, c->seg.pinfo, stream) != 0) return -1;
            ++out.patched;
        } else {
            // the next segment reads the new snapshot (load_neigh waits for the context's
            // stream; a caller stream is drained first)
            if (s != c->stream) HIP_TRY(hipStreamSynchronize(s));
            if (upe_gpu_load_neigh(c, arp, arp_capacity, ndp, ndp_capacity) != 0) return -1;
            ++out.rebuilds;
        }
    }
    if (start < n &&
        upe_gpu_process(c, d_frames, d_desc + start, d_verdict + start, n - start, stream) != 0)
        return -1;
    HIP_TRY(hipStreamSynchronize(s));
    if (info) *info = out;
    return 0;
}
