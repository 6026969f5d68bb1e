// upe_ctrl.hip — a batch's neighbour-table writes on the device (upe_gpu_ctrl_writes,
// include/upe_gpu.h): what handle_control_packet (reference src/worker.c:23-104) would teach the
// ARP and NDP tables from a batch resident in GPU memory, as an ordered list of 32-byte records —
// the marking rule of upe_gpu_ingress_gather's d_ctrl, the ARP learn (src/worker.c:28-39) and the
// NS / NA option walk (src/worker.c:57-95) that upe_segment.hip runs on the host.
//
// Up to three launches on one stream, the ordered-output shape of upe_ingress.hip; the kernel
// boundaries are the only ordering between workgroups, and no result depends on the order in
// which workgroups run:
//   upe_ctrl_mark   per workgroup (kBlock packets, a "tile"), one lane per packet: the descriptor,
//                   frame bytes 12..23 (inside the UPE_FRAME_TAIL bytes that are always readable:
//                   loaded without a branch on len, masked with it), byte 54 of an IPv6 / ICMPv6
//                   frame of 78 bytes or more, and for a marked NS / NA the option walk, which
//                   reads bytes below len only.  A word per packet into scratch — 0, or kind |
//                   mac_off << 8 | NA << 24 — and the tile's marks, records and first record.
//   upe_ctrl_scan   one workgroup: the exclusive prefix of the records over the tiles, the totals
//                   and *info.
//   upe_ctrl_write  per tile that has records below cap: ranks by ballot, the 16 groups' counts
//                   through LDS; each record built from its word and the frame and stored as two
//                   16-byte quads.  Not launched when cap is 0.
// A batch without control packets costs the first pass and the scan: the write pass's workgroups
// leave on their tile's count.
//
// Scratch: uint32 nctrl[Tp], nwr[Tp], fwr[Tp], wex[Tp] (marks, records, the first record's
// packet, records before each tile) and word[n]; T tiles, Tp = T rounded up to 4.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "upe_ctx.h"
#include "upe_scan.h"

using namespace upe;

namespace {

constexpr uint32_t kBlock = UPE_CTRL_BLOCK;   // packets per workgroup of the mark and write pass
constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kPer = kBlock / kThreads;   // packets per thread
constexpr uint32_t kGroups = kBlock / 64;      // (round, wave) pairs of a tile: 64-packet groups
constexpr uint32_t kScanThreads = 1024;        // tiles per step of the scan
constexpr uint32_t kScanWaves = kScanThreads / 64;
constexpr uint32_t kNaBit = 1u << 24;          // word: the record's address is the NA's target
// The walk's proof bound: every iteration advances off by at least 8 and off + 2 <= len <= 65535.
constexpr uint32_t kWalkMax = 8190;
static_assert(kBlock % kThreads == 0 && kGroups == kPer * kWaves, "tile shape");
static_assert(78u + 8u * kWalkMax + 2u > 65535u, "the bound covers every frame length");

// Frame i: its first byte (a 64-bit offset: byte_offset goes up to 2^36) and its length.
__device__ __forceinline__ const uint8_t* frame_of(const uint8_t* frames, uint64_t d, uint32_t& len) {
    len = (uint32_t)(d & 0xFFFFu);
    return frames + (d >> 16);
}

__global__ void __launch_bounds__(kThreads) upe_ctrl_mark(
    const uint8_t* frames, const uint64_t* desc, uint32_t n, uint32_t* word, uint32_t* nctrl,
    uint32_t* nwr, uint32_t* fwr) {
    __shared__ uint32_t s_nc, s_nw, s_fw;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        s_nc = 0;
        s_nw = 0;
        s_fw = kNone;
    }
    __syncthreads();
    const uint32_t p0 = blockIdx.x * kBlock;
    uint32_t nc = 0, nw = 0, fw = kNone;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t i = p0 + k * kThreads + tid;   // < n + kBlock: no wrap
        if (i >= n) continue;
        uint32_t len;
        const uint8_t* f = frame_of(frames, desc[i], len);
        // bytes 12..23: a frame starts on a 16-byte boundary with UPE_FRAME_TAIL readable bytes
        const uint32_t b12 = *reinterpret_cast<const uint32_t*>(f + 12);
        const uint2 b16 = *reinterpret_cast<const uint2*>(f + 16);
        auto at = [&](uint32_t j) -> uint32_t {   // asked for 12..20 and 54
            if (j >= len) return 0u;
            if (j < 16u) return (b12 >> (8u * (j - 12u))) & 0xFFu;
            if (j < 20u) return (b16.x >> (8u * (j - 16u))) & 0xFFu;
            if (j < 24u) return (b16.y >> (8u * (j - 20u))) & 0xFFu;
            return (uint32_t)f[j];
        };
        uint32_t w = 0;
        if (upe::ctrl_table_write(len, at)) {
            nc += 1u;
            if (at(12u) == 0x08u) {
                // ARP: arp_update(spa, sha) whatever len is (src/worker.c:31-35)
                w = UPE_CW_ARP | 22u << 8;
            } else {
                // NS / NA, len >= 78: the option walk of src/worker.c:68-95
                const bool na = f[54] == 136u;
                const uint32_t want = na ? 2u : 1u;
                uint32_t off = 78u;
                for (uint32_t it = 0; it < kWalkMax && off + 2u <= len; ++it) {
                    const uint32_t ot = f[off];
                    const uint32_t ol = ((uint32_t)f[off + 1u] * 8u) & 0xFFu;   // uint8_t opt_len
                    if (ol == 0u || off + ol > len) break;
                    if (ot == want) {   // ol >= 8: the MAC's six bytes lie below len
                        w = UPE_CW_NDP | (off + 2u) << 8 | (na ? kNaBit : 0u);
                        break;
                    }
                    off += ol;
                }
            }
        }
        word[i] = w;
        if (w) {
            nw += 1u;
            fw = i < fw ? i : fw;
        }
    }
    nc = wave_sum(nc);
    nw = wave_sum(nw);
    fw = wave_min(fw);
    if ((tid & 63u) == 0) {
        atomicAdd(&s_nc, nc);
        atomicAdd(&s_nw, nw);
        atomicMin(&s_fw, fw);
    }
    __syncthreads();
    if (tid == 0) {
        nctrl[blockIdx.x] = s_nc;
        nwr[blockIdx.x] = s_nw;
        fwr[blockIdx.x] = s_fw;
    }
}

// One workgroup; a step covers kScanThreads tiles, one per thread.  The sums stay below n < 2^32.
__global__ void __launch_bounds__(kScanThreads) upe_ctrl_scan(
    uint32_t T, uint64_t cap, const uint32_t* nctrl, const uint32_t* nwr, const uint32_t* fwr,
    uint32_t* wex, upe_ctrl_info_t* info) {
    __shared__ uint32_t s_ww[kScanWaves];
    __shared__ uint32_t s_nc, s_fw;
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    if (tid == 0) {
        s_nc = 0;
        s_fw = kNone;
    }
    uint32_t carry = 0, nc = 0, fw = kNone;
    for (uint32_t c0 = 0; c0 < T; c0 += kScanThreads) {
        const uint32_t t = c0 + tid;
        const uint32_t w = t < T ? nwr[t] : 0u;
        if (t < T) {
            nc += nctrl[t];
            const uint32_t x = fwr[t];
            fw = x < fw ? x : fw;
        }
        uint32_t all;   // (the first step's barriers also order the shared words set above)
        const uint32_t ex = block_excl(w, lane, wave, s_ww, all);
        if (t < T) wex[t] = carry + ex;
        carry += all;
    }
    nc = wave_sum(nc);
    fw = wave_min(fw);
    if (lane == 0) {
        atomicAdd(&s_nc, nc);
        atomicMin(&s_fw, fw);
    }
    __syncthreads();
    if (tid == 0) {
        const uint32_t first = s_fw;
        info->ctrl = s_nc;
        info->writes = carry;
        info->stored = (uint64_t)carry < cap ? (uint64_t)carry : cap;
        info->first_write = first == kNone ? ~0ull : (uint64_t)first;
    }
}

__global__ void __launch_bounds__(kThreads) upe_ctrl_write(
    const uint8_t* frames, const uint64_t* desc, const uint32_t* word, uint32_t n,
    const uint32_t* nwr, const uint32_t* wex, uint4* out, uint64_t cap) {
    __shared__ uint32_t s_gc[kGroups];   // records per 64-packet group
    const uint32_t tile = blockIdx.x;
    const uint32_t tile_w = wex[tile];
    if (nwr[tile] == 0u || (uint64_t)tile_w >= cap) return;   // the whole workgroup
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    const uint32_t p0 = tile * kBlock;
    uint32_t w[kPer], rank[kPer];
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t i = p0 + k * kThreads + tid;
        w[k] = i < n ? word[i] : 0u;
        const unsigned long long bal = __ballot(w[k] != 0u);
        rank[k] = (uint32_t)__popcll(bal & lanes_below(lane));
        if (lane == 0) s_gc[k * kWaves + wave] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        if (w[k] == 0u) continue;
        const uint32_t grp = k * kWaves + wave;
        uint32_t pos = tile_w + rank[k];   // <= the batch's records: below 2^32
        for (uint32_t j = 0; j < grp; ++j) pos += s_gc[j];
        if ((uint64_t)pos >= cap) continue;
        const uint32_t i = p0 + k * kThreads + tid;
        uint32_t len;
        const uint8_t* f = frame_of(frames, desc[i], len);
        const uint32_t kind = w[k] & 0xFFu, mac_off = (w[k] >> 8) & 0xFFFFu;
        uint4 a, b;
        a.x = i;
        a.y = kind | mac_off << 16;
        if (kind == UPE_CW_ARP) {
            // sha 22..27 and spa 28..31 from the words at 20, 24 and 28 (always readable), zero
            // at or past len
            const uint32_t* q = reinterpret_cast<const uint32_t*>(f + 20);
            const uint32_t d0 = keep(q[0], len, 20u), d1 = keep(q[1], len, 24u),
                           d2 = keep(q[2], len, 28u);
            a.z = d0 >> 16 | d1 << 16;
            a.w = d1 >> 16;
            b = make_uint4(__builtin_bswap32(d2), 0u, 0u, 0u);   // ntohl(spa), upe_ip_addr_t.v4
        } else {
            // len >= 78: the address (NS: 22..37, NA: 62..77) lies below len, in the words from
            // 20 or 60; the MAC at any offset, its six bytes below len
            const uint32_t* q =
                reinterpret_cast<const uint32_t*>(f + ((w[k] & kNaBit) ? 60 : 20));
            const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
            b = make_uint4(d0 >> 16 | d1 << 16, d1 >> 16 | d2 << 16, d2 >> 16 | d3 << 16,
                           d3 >> 16 | d4 << 16);
            const uint8_t* m = f + mac_off;
            a.z = (uint32_t)m[0] | (uint32_t)m[1] << 8 | (uint32_t)m[2] << 16 | (uint32_t)m[3] << 24;
            a.w = (uint32_t)m[4] | (uint32_t)m[5] << 8;
        }
        out[2u * (size_t)pos] = a;
        out[2u * (size_t)pos + 1u] = b;
    }
}

struct Tab {
    uint32_t *nctrl, *nwr, *fwr, *wex, *word;
};

// The scratch of one call over n packets in T tiles (n > 0).
Tab layout(Carver& c, uint32_t T, uint32_t n) {
    const size_t tp = ((size_t)T + 3u) & ~(size_t)3u;
    Tab t;
    t.nctrl = c.take<uint32_t>(tp);
    t.nwr = c.take<uint32_t>(tp);
    t.fwr = c.take<uint32_t>(tp);
    t.wex = c.take<uint32_t>(tp);
    t.word = c.take<uint32_t>(n);
    return t;
}

}  // namespace

extern "C" int upe_gpu_ctrl_writes(upe_gpu_ctx_t* c, const uint8_t* d_frames,
                                   const uint64_t* d_desc, size_t n, upe_ctrl_write_t* d_writes,
                                   size_t cap, upe_ctrl_info_t* d_info, void* stream) {
    if (!c) return fail("null context");
    if (!d_info || (n && (!d_frames || !d_desc)) || (cap && !d_writes)) return fail("null buffer");
    if ((reinterpret_cast<uintptr_t>(d_writes) & 15u) != 0)
        return fail("d_writes must be 16-byte aligned");
    if (n > 0xFFFFFFFFull - UPE_CTRL_BLOCK) return fail("n must fit in 32 bits");
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    if (n == 0) return empty_info(d_info, &upe_ctrl_info_t::first_write, s);
    const uint32_t T = tiles_of((uint32_t)n, kBlock);
    const size_t need = layout_bytes(layout, T, (uint32_t)n);
    if (c->cw_scratch.reserve(need, need + need / 4) != 0) return -1;
    Carver mem(c->cw_scratch.p);
    const Tab t = layout(mem, T, (uint32_t)n);
    hipLaunchKernelGGL(upe_ctrl_mark, dim3(T), dim3(kThreads), 0, s, d_frames, d_desc, (uint32_t)n,
                       t.word, t.nctrl, t.nwr, t.fwr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(upe_ctrl_scan, dim3(1), dim3(kScanThreads), 0, s, T, (uint64_t)cap, t.nctrl,
                       t.nwr, t.fwr, t.wex, d_info);
    HIP_TRY(hipGetLastError());
    if (cap == 0) return 0;   // nothing may be stored
    hipLaunchKernelGGL(upe_ctrl_write, dim3(T), dim3(kThreads), 0, s, d_frames, d_desc, t.word,
                       (uint32_t)n, t.nwr, t.wex, reinterpret_cast<uint4*>(d_writes),
                       (uint64_t)cap);
    HIP_TRY(hipGetLastError());
    return 0;
}
