// upe_rx.hip — the RX thread's dispatch of a batch to the worker rings, on the device
// (upe_gpu_rx_dispatch, include/upe_gpu.h).
//
// The reference's RX thread (src/rx_pcap.c:19-25,67-80) parses each packet with parse_flow_key
// (src/parser.c:6-111); a packet that parses goes to ring flow_hash & (ring_count - 1)
// (src/parser.c:113-135), every other packet to the ring a round-robin cursor names, and the
// cursor steps.  Each ring receives its packets in arrival order.
//
// Three launches on one stream; the kernel boundaries are the only ordering between
// workgroups (no workgroup waits on another, no atomic's arrival order reaches an output):
//   upe_rx_hash    per packet: the parse gates and flow_hash; ring[i] = the ring id, or
//                  kFallback; per workgroup (kRxBlock packets, a "tile") the count of parsed
//                  packets per ring and of fallback packets.
//   upe_rx_scan    one workgroup: per tile the fallback packets before it (F), and per ring the
//                  packets of earlier tiles.  The k-th fallback packet of the batch goes to ring
//                  (rr + k) & (W - 1), so a tile with F fallbacks before it and f of its own
//                  hands them out in a run and its share per ring follows from F, f and rr.
//   upe_rx_scatter per packet: a fallback packet's ring from its rank (F + its rank in the
//                  tile), then the stable multi-way partition: rank in the wave by match masks
//                  (ballots over the ring-id bits), per-wave per-ring counts through LDS.
//
// Scratch (uint32): tab[(W + 2) * Tp], T tiles, Tp = T rounded up to 8; column c < W: tile
// counts of ring c, turned in place into the packets of ring c in earlier tiles; column W: the
// tiles' fallback counts; column W + 1: the fallback packets before each tile.  Then base[64]:
// where each ring's segment starts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "upe_ctx.h"
#include "upe_scan.h"

using namespace upe;

namespace {

constexpr uint32_t kRxBlock = UPE_RX_BLOCK;    // packets per workgroup of the hash and scatter pass
constexpr uint32_t kRxThreads = 256;
constexpr uint32_t kRxPer = kRxBlock / kRxThreads;   // packets per thread
constexpr uint32_t kRxSlots = kRxPer * (kRxThreads / 64);   // (round, wave) pairs of a tile
constexpr uint32_t kFallback = 0xFFFFFFFFu;    // ring[] between the hash and the scatter pass
constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kScanWaves = kScanThreads / 64;
constexpr uint32_t kScanPer = 8;               // tiles per lane and step of the scan
constexpr uint32_t kScanRings = UPE_RX_RINGS_MAX / kScanWaves;   // rings per wave, at most
static_assert(kRxBlock % kRxThreads == 0 && kRxSlots == 16, "tile shape");
static_assert(UPE_RX_RINGS_MAX == 64 && UPE_RX_RINGS_MAX < kRxThreads, "one thread per ring");

// The lanes of the wave whose (live) packet has this lane's ring: one ballot per ring-id bit.
// Called by every lane of the wave.
__device__ __forceinline__ unsigned long long match_ring(bool live, uint32_t ring, uint32_t lg) {
    unsigned long long m = __ballot(live);
    for (uint32_t b = 0; b < lg; ++b) {
        const bool bit = (ring >> b) & 1u;
        const unsigned long long bb = __ballot(live && bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}

// parse_flow_key's gates and flow_hash over the header window, read
// as 16-byte loads the way the classify kernel reads it: bytes 0..47 always (UPE_FRAME_TAIL
// bytes follow every frame start), 48..63 and 64..79 only when the frame reaches them.  A
// successful parse uses no byte at or past len.  Its own statement of parse_key (upe_parse.h):
// over the shared one, with the L4 words chosen by the select chain instead of the
// IHL-indexed load below, upe_rx_hash took 46 VGPRs for 38 and measured 0.1-0.4 us per 1M
// packets above this text's own range (profiles/parse_share_ab.txt).
struct RxKey {
    bool ok;
    uint32_t hash;
};

__device__ __forceinline__ uint32_t be16_at(uint32_t w, int byte) {   // BE u16 at bytes byte, byte+1
    return (((w >> (8 * byte)) & 0xFFu) << 8) | ((w >> (8 * byte + 8)) & 0xFFu);
}

__device__ __forceinline__ RxKey rx_parse(const uint8_t* p, uint32_t len) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint32_t w[20];
    const uint4 q0 = q[0], q1 = q[1], q2 = q[2];
    uint4 q3 = make_uint4(0, 0, 0, 0), q4 = q3;
    if (len > 48u) q3 = q[3];
    if (len > 64u) q4 = q[4];
    w[0] = q0.x; w[1] = q0.y; w[2] = q0.z; w[3] = q0.w;
    w[4] = q1.x; w[5] = q1.y; w[6] = q1.z; w[7] = q1.w;
    w[8] = q2.x; w[9] = q2.y; w[10] = q2.z; w[11] = q2.w;
    w[12] = q3.x; w[13] = q3.y; w[14] = q3.z; w[15] = q3.w;
    w[16] = q4.x; w[17] = q4.y; w[18] = q4.z; w[19] = q4.w;
    const uint32_t et = be16_at(w[3], 0);                 // bytes 12, 13
    const bool is4 = et == 0x0800u, is6 = et == 0x86DDu;
    bool ok = len >= 14u && (is4 || is6);
    const uint32_t ip_len = len - 14u;
    // a, b, c: the dwords at l4 - 2, l4 + 2 and l4 + 10 (L4 starts at 2 mod 4 in both families)
    uint32_t proto, l4_len, h, a, b, c;
    if (is4) {
        const uint32_t vi = (w[3] >> 16) & 0xFFu;         // byte 14
        const uint32_t ihl = vi & 0xFu;
        ok = ok && ip_len >= 20u && (vi >> 4) == 4u && ihl >= 5u && ip_len >= ihl * 4u;
        proto = w[5] >> 24;                               // byte 23
        l4_len = ip_len - ihl * 4u;
        // ntohl(src) ^ ntohl(dst): wire dwords at bytes 26 and 30
        h = __builtin_bswap32(((w[6] >> 16) | (w[7] << 16)) ^ ((w[7] >> 16) | (w[8] << 16)));
        a = w[8]; b = w[9]; c = w[11];                    // IHL 5: L4 at byte 34
        if (ok && ihl != 5u) {                            // options: L4 at 14 + 4 * IHL <= 74
            const uint32_t* g = reinterpret_cast<const uint32_t*>(p);
            a = g[3u + ihl]; b = g[4u + ihl]; c = g[6u + ihl];
        }
    } else {
        ok = ok && ip_len >= 40u;                         // no version check, no extension walk
        proto = w[5] & 0xFFu;                             // byte 20
        l4_len = ip_len - 40u;
        h = 0;                                            // the 8 address dwords at bytes 22..53
#pragma unroll
        for (int k = 5; k < 13; ++k) h ^= (w[k] >> 16) | (w[k + 1] << 16);
        a = w[13]; b = w[14]; c = w[16];                  // L4 at byte 54
    }
    const uint32_t f0 = be16_at(a, 2), f2 = be16_at(b, 0), f4 = be16_at(b, 2);
    uint32_t sport = 0, dport = 0;
    if (proto == 17u) {
        ok = ok && l4_len >= 8u;
        sport = f0; dport = f2;
    } else if (proto == 6u) {
        const uint32_t doff4 = ((c >> 20) & 0xFu) * 4u;   // byte l4 + 12, high nibble
        ok = ok && l4_len >= 20u && doff4 >= 20u && doff4 <= l4_len;
        sport = f0; dport = f2;
    } else if (proto == 1u) {                             // ICMP: sport = id, dport = type << 8 | code
        ok = ok && l4_len >= 8u;
        sport = f4; dport = f0;
    } else {
        ok = false;                                       // proto 58 included
    }
    return RxKey{ok, sport ^ dport ^ proto ^ h};
}

__global__ void __launch_bounds__(kRxThreads) upe_rx_hash(const uint8_t* frames,
                                                          const uint64_t* desc, uint32_t n,
                                                          uint32_t lg, uint32_t* ring,
                                                          uint32_t* flow_hash, uint32_t* tab,
                                                          uint32_t tp) {
    __shared__ uint32_t s_cnt[UPE_RX_RINGS_MAX + 1];
    const uint32_t W = 1u << lg, tid = threadIdx.x;
    const int lane = tid & 63;
    if (tid <= W) s_cnt[tid] = 0;
    __syncthreads();
    const uint32_t p0 = blockIdx.x * kRxBlock;
    uint64_t d[kRxPer];
#pragma unroll
    for (uint32_t k = 0; k < kRxPer; ++k) {
        const uint32_t i = p0 + k * kRxThreads + tid;
        d[k] = i < n ? desc[i] : 0;
    }
#pragma unroll
    for (uint32_t k = 0; k < kRxPer; ++k) {
        const uint32_t i = p0 + k * kRxThreads + tid;
        const bool live = i < n;
        RxKey key{false, 0};
        if (live) key = rx_parse(frames + ((size_t)(d[k] >> 20) << 4), (uint32_t)(d[k] & 0xFFFFu));
        const bool hit = live && key.ok;
        const uint32_t r = key.hash & (W - 1u);
        if (live) {
            ring[i] = hit ? r : kFallback;
            if (flow_hash) flow_hash[i] = hit ? key.hash : 0u;
        }
        const unsigned long long m = match_ring(hit, hit ? r : 0u, lg);
        if (hit && (m & lanes_below(lane)) == 0) atomicAdd(&s_cnt[r], (uint32_t)__popcll(m));
        const unsigned long long fb = __ballot(live && !key.ok);
        if (lane == 0 && fb) atomicAdd(&s_cnt[W], (uint32_t)__popcll(fb));
    }
    __syncthreads();
    if (tid <= W) tab[(size_t)tid * tp + blockIdx.x] = s_cnt[tid];
}

// kScanPer entries of a column from tile t0 (a multiple of kScanPer, so they lie inside the
// column's padded stride whenever t0 < tp); entries at or past T read as zero.
__device__ __forceinline__ void col_load(const uint32_t* col, uint32_t t0, uint32_t T, uint32_t tp,
                                         uint32_t (&v)[kScanPer]) {
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j) v[j] = 0;
    if (t0 >= tp) return;
    const uint4* q = reinterpret_cast<const uint4*>(col + t0);
#pragma unroll
    for (uint32_t j = 0; j < kScanPer / 4; ++j) {
        const uint4 x = q[j];
        v[4 * j + 0] = x.x; v[4 * j + 1] = x.y; v[4 * j + 2] = x.z; v[4 * j + 3] = x.w;
    }
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j)
        if (t0 + j >= T) v[j] = 0;
}

__device__ __forceinline__ void col_store(uint32_t* col, uint32_t t0, uint32_t tp,
                                          const uint32_t (&v)[kScanPer]) {
    if (t0 >= tp) return;
    uint4* q = reinterpret_cast<uint4*>(col + t0);
#pragma unroll
    for (uint32_t j = 0; j < kScanPer / 4; ++j)
        q[j] = make_uint4(v[4 * j + 0], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
}

// Of the batch's fallback packets of rank 0 .. x - 1, how many the cursor hands to the ring at
// distance d = (ring - rr) & (W - 1) from the starting cursor: ranks d, d + W, d + 2W, ...
__device__ __forceinline__ uint32_t rr_upto(uint32_t x, uint32_t d, uint32_t lg) {
    return (x + (1u << lg) - 1u - d) >> lg;
}

// One workgroup.  Wave v owns rings v, v + 16, ...; every wave scans the fallback column
// itself (it needs F per tile), so the waves never wait for one another until the ring totals
// are put together at the end.  A step covers 64 lanes x kScanPer tiles; the loads of a step do
// not depend on the carries of the step before.
__global__ void __launch_bounds__(kScanThreads) upe_rx_scan(uint32_t* tab, uint32_t T, uint32_t tp,
                                                            uint32_t lg, uint32_t rr,
                                                            uint32_t* base,
                                                            unsigned long long* counts) {
    __shared__ uint32_t s_tot[UPE_RX_RINGS_MAX + 1];
    const uint32_t W = 1u << lg;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t* fcol = tab + (size_t)W * tp;
    uint32_t* fex = tab + (size_t)(W + 1u) * tp;
    uint32_t carry_f = 0, carry[kScanRings];
#pragma unroll
    for (uint32_t q = 0; q < kScanRings; ++q) carry[q] = 0;
    for (uint32_t c0 = 0; c0 < T; c0 += 64u * kScanPer) {
        const uint32_t t0 = c0 + (uint32_t)lane * kScanPer;
        // every load of the step first: the columns' round trips overlap, and none waits
        // behind a store of the column before it
        uint32_t f[kScanPer], F[kScanPer], v[kScanRings][kScanPer], tot;
        col_load(fcol, t0, T, tp, f);
#pragma unroll
        for (uint32_t q = 0; q < kScanRings; ++q)
            col_load(tab + (size_t)(wave + kScanWaves * q) * tp, t0, T,
                     wave + kScanWaves * q < W ? tp : 0u, v[q]);
        uint32_t s = 0;
#pragma unroll
        for (uint32_t j = 0; j < kScanPer; ++j) {
            F[j] = s;
            s += f[j];
        }
        const uint32_t ex_f = wave_excl(s, lane, tot) + carry_f;
#pragma unroll
        for (uint32_t j = 0; j < kScanPer; ++j) F[j] += ex_f;
        carry_f += tot;
        if (wave == 0) col_store(fex, t0, tp, F);
#pragma unroll
        for (uint32_t q = 0; q < kScanRings; ++q) {
            const uint32_t r = wave + kScanWaves * q;
            if (r >= W) continue;
            uint32_t* col = tab + (size_t)r * tp;
            const uint32_t dist = (r - rr) & (W - 1u);
            s = 0;
#pragma unroll
            for (uint32_t j = 0; j < kScanPer; ++j) {
                const uint32_t x =
                    v[q][j] + rr_upto(F[j] + f[j], dist, lg) - rr_upto(F[j], dist, lg);
                v[q][j] = s;
                s += x;
            }
            const uint32_t ex = wave_excl(s, lane, tot) + carry[q];
#pragma unroll
            for (uint32_t j = 0; j < kScanPer; ++j) v[q][j] += ex;
            carry[q] += tot;
            col_store(col, t0, tp, v[q]);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t q = 0; q < kScanRings; ++q)
            if (wave + kScanWaves * q < W) s_tot[wave + kScanWaves * q] = carry[q];
        if (wave == 0) s_tot[W] = carry_f;
    }
    __syncthreads();
    if (wave == 0) {
        const uint32_t mine = (uint32_t)lane < W ? s_tot[lane] : 0u;
        uint32_t all;
        const uint32_t start = wave_excl(mine, lane, all);
        if ((uint32_t)lane < W) {
            base[lane] = start;
            counts[lane] = mine;
        }
        if (lane == 0) counts[W] = s_tot[W];
    }
}

__global__ void __launch_bounds__(kRxThreads) upe_rx_scatter(uint32_t* ring, const uint64_t* desc,
                                                             uint32_t n, uint32_t lg, uint32_t rr,
                                                             const uint32_t* tab, uint32_t tp,
                                                             const uint32_t* base, uint32_t* index,
                                                             uint64_t* desc_out) {
    __shared__ uint32_t s_fw[kRxSlots];                     // fallback packets per (round, wave)
    __shared__ uint32_t s_wc[kRxSlots][UPE_RX_RINGS_MAX];   // packets per (round, wave) and ring
    const uint32_t W = 1u << lg, tid = threadIdx.x, tile = blockIdx.x;
    const int lane = tid & 63;
    const uint32_t wave = tid >> 6;
    const uint32_t p0 = tile * kRxBlock;
    uint32_t rv[kRxPer], rk[kRxPer], fbits = 0;
#pragma unroll
    for (uint32_t k = 0; k < kRxPer; ++k) {
        const uint32_t i = p0 + k * kRxThreads + tid;
        rv[k] = i < n ? ring[i] : 0u;
        const bool fb = i < n && rv[k] == kFallback;
        const unsigned long long bal = __ballot(fb);
        if (lane == 0) s_fw[k * (kRxThreads / 64) + wave] = (uint32_t)__popcll(bal);
        rk[k] = (uint32_t)__popcll(bal & lanes_below(lane));   // rank among the wave's fallbacks
        fbits |= fb ? 1u << k : 0u;
    }
    for (uint32_t j = tid; j < kRxSlots * UPE_RX_RINGS_MAX; j += kRxThreads) (&s_wc[0][0])[j] = 0;
    __syncthreads();
    const uint32_t F = tab[(size_t)(W + 1u) * tp + tile];
#pragma unroll
    for (uint32_t k = 0; k < kRxPer; ++k) {
        const uint32_t i = p0 + k * kRxThreads + tid;
        const uint32_t slot = k * (kRxThreads / 64) + wave;
        const bool live = i < n;
        uint32_t pre = F;
        for (uint32_t j = 0; j < slot; ++j) pre += s_fw[j];
        if ((fbits >> k) & 1u) rv[k] = (rr + pre + rk[k]) & (W - 1u);
        rv[k] &= W - 1u;
        const unsigned long long m = match_ring(live, rv[k], lg);
        rk[k] = (uint32_t)__popcll(m & lanes_below(lane));     // rank among the wave's ring peers
        if (live && rk[k] == 0) s_wc[slot][rv[k]] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (tid < W) {   // per ring: where each (round, wave) starts writing
        uint32_t run = base[tid] + tab[(size_t)tid * tp + tile];
#pragma unroll
        for (uint32_t j = 0; j < kRxSlots; ++j) {
            const uint32_t c = s_wc[j][tid];
            s_wc[j][tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kRxPer; ++k) {
        const uint32_t i = p0 + k * kRxThreads + tid;
        if (i >= n) continue;
        const uint32_t pos = s_wc[k * (kRxThreads / 64) + wave][rv[k]] + rk[k];
        if (pos < n) {   // always, when ring[] is what the hash pass wrote
            index[pos] = i;
            if (desc_out) desc_out[pos] = desc[i];
        }
        if ((fbits >> k) & 1u) ring[i] = rv[k] | UPE_RX_FALLBACK;
    }
}

uint32_t stride_of(uint32_t tiles) { return (tiles + kScanPer - 1) / kScanPer * kScanPer; }

struct Tab {
    uint32_t *tab, *base;
};

// The scratch of one dispatch over T tiles and `rings` rings.
Tab layout(Carver& c, uint32_t T, uint32_t rings) {
    Tab t;
    // col_load / col_store move uint4: the table starts on 16 bytes, and every column does, a
    // stride (a multiple of kScanPer entries) after the one before
    t.tab = c.take<uint32_t>((size_t)(rings + 2u) * stride_of(T), sizeof(uint4));
    t.base = c.take<uint32_t>(UPE_RX_RINGS_MAX);
    return t;
}

// Queue the three passes on `s`, with the arguments as rx_dispatch has checked them.
hipError_t upe_rx_launch(const uint8_t* frames, const uint64_t* desc, uint32_t n, uint32_t rings,
                         uint32_t rr, uint32_t* ring, uint32_t* flow_hash, uint32_t* index,
                         uint64_t* desc_out, uint64_t* counts, void* scratch, hipStream_t s,
                         hipEvent_t* ev) {
    const uint32_t T = tiles_of(n, kRxBlock), tp = stride_of(T);
    uint32_t lg = 0;
    while ((1u << lg) < rings) ++lg;
    Carver mem(scratch);
    const Tab t = layout(mem, T, rings);
    hipError_t e;
    if (ev && (e = hipEventRecord(ev[0], s)) != hipSuccess) return e;
    hipLaunchKernelGGL(upe_rx_hash, dim3(T), dim3(kRxThreads), 0, s, frames, desc, n, lg, ring,
                       flow_hash, t.tab, tp);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[1], s)) != hipSuccess) return e;
    hipLaunchKernelGGL(upe_rx_scan, dim3(1), dim3(kScanThreads), 0, s, t.tab, T, tp, lg, rr, t.base,
                       reinterpret_cast<unsigned long long*>(counts));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[2], s)) != hipSuccess) return e;
    hipLaunchKernelGGL(upe_rx_scatter, dim3(T), dim3(kRxThreads), 0, s, ring, desc, n, lg, rr,
                       t.tab, tp, t.base, index, desc_out);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return ev ? hipEventRecord(ev[3], s) : hipSuccess;
}

// The RX thread's dispatch (reference src/rx_pcap.c:19-25,67-80).  ev: NULL, or four events
// recorded before the hash pass and after each pass (tools/rx_dispatch_time.py).
int rx_dispatch(upe_gpu_ctx_t* c, const uint8_t* d_frames, const uint64_t* d_desc, size_t n,
                uint32_t rings, uint32_t rr_start, uint32_t* d_ring, uint32_t* d_flow_hash,
                uint32_t* d_index, uint64_t* d_desc_out, uint64_t* d_counts, void* stream,
                hipEvent_t* ev) {
    if (!c) return fail("null context");
    if (rings == 0 || (rings & (rings - 1)) != 0 || rings > UPE_RX_RINGS_MAX)
        return fail("rings must be a power of two between 1 and " +
                    std::to_string(UPE_RX_RINGS_MAX));
    if (!d_counts || (n && (!d_frames || !d_desc || !d_ring || !d_index)))
        return fail("null buffer");
    if (n > 0xFFFFFFFFull - UPE_RX_BLOCK) return fail("n must fit in 32 bits");
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_counts, 0, (rings + 1) * sizeof(uint64_t), s));
        return 0;
    }
    const size_t need = layout_bytes(layout, tiles_of((uint32_t)n, kRxBlock), rings);
    if (c->rx_scratch.reserve(need, need + need / 4) != 0) return -1;
    HIP_TRY(upe_rx_launch(d_frames, d_desc, (uint32_t)n, rings, rr_start & (rings - 1), d_ring,
                          d_flow_hash, d_index, d_desc_out, d_counts, c->rx_scratch.p, s, ev));
    return 0;
}

}  // namespace

extern "C" {

int upe_gpu_rx_dispatch(upe_gpu_ctx_t* c, const uint8_t* d_frames, const uint64_t* d_desc, size_t n,
                        uint32_t rings, uint32_t rr_start, uint32_t* d_ring, uint32_t* d_flow_hash,
                        uint32_t* d_index, uint64_t* d_desc_out, uint64_t* d_counts, void* stream) {
    return rx_dispatch(c, d_frames, d_desc, n, rings, rr_start, d_ring, d_flow_hash, d_index,
                       d_desc_out, d_counts, stream, nullptr);
}

// Diagnostic (tools/rx_dispatch_time.py; not in the header): one dispatch of n > 0 packets with
// HIP events around each pass; ms[0..2] = the hash, scan and scatter pass.  Synchronous.
int upe_gpu_rx_dispatch_timed(upe_gpu_ctx_t* c, const uint8_t* d_frames, const uint64_t* d_desc,
                              size_t n, uint32_t rings, uint32_t rr_start, uint32_t* d_ring,
                              uint32_t* d_flow_hash, uint32_t* d_index, uint64_t* d_desc_out,
                              uint64_t* d_counts, void* stream, float* ms) {
    if (!c || !ms || n == 0) return fail("null context, no output or an empty batch");
    DEV_SCOPE(c->device);
    Events<4> ev;
    if (ev.create() != 0 ||
        rx_dispatch(c, d_frames, d_desc, n, rings, rr_start, d_ring, d_flow_hash, d_index,
                    d_desc_out, d_counts, stream, ev.e) != 0)
        return -1;
    HIP_TRY(hipEventSynchronize(ev.e[3]));
    for (int k = 0; k < 3; ++k)
        if (ev.elapsed(&ms[k], k, k + 1) != 0) return -1;
    return 0;
}

}  // extern "C"
