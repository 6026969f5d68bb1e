// upe_ingress.hip — the ingress batch builder on the device (upe_gpu_ingress_gather,
// include/upe_gpu.h): a burst of pktbuf handles (buffer indexes into a pool of stride-byte
// buffers: timestamp@0, len@8, data@16; reference include/pktbuf.h:8-14) turned into the "Batch
// layout" the classify, dispatch and pack stages start from — what the worker loop does per
// packet on the CPU (upe_worker.c: ops->data / ops->len, the descriptor, the 96-byte window copy,
// is_table_write).
//
// Every length is counted in 16-byte quads, as in upe_egress.hip: strides and the data offset are
// multiples of 16, so a quad never crosses a buffer, and frames start on quad boundaries on both
// sides.
//
// Up to three launches on one stream; the kernel boundaries are the only ordering between
// workgroups:
//   upe_ingress_size   per workgroup (kBlock packets, a "tile"), one lane per packet: the buffer's
//                      header quad (timestamp, len), the bad-handle test, the control mark from
//                      the first two data quads (and byte 54's quad for an IPv6 frame of 78
//                      bytes or more); a meta word per packet into scratch (len | mark << 16 |
//                      bad << 17) and the tile's sums.  REF and WINDOW mode: the descriptors and
//                      timestamps too, which do not depend on any other packet.
//   upe_ingress_scan   one workgroup: the exclusive prefix over the tiles of the marks and (FULL)
//                      the quads in 64 bits, the totals, and *info.  When the output is too
//                      small, the first tile that does not fit whole is scanned packet by packet
//                      for the exact cut.
//   upe_ingress_write  per tile: the marked positions in order (ballot ranks, the 16 groups'
//                      counts through LDS).  WINDOW: output quad g of the tile is lane g's, six
//                      lanes per packet, so a wave stores 1 KiB runs.  FULL: the in-tile scan of
//                      the quads, the descriptors and timestamps, then the bytes as the egress
//                      pack moves them: the lanes of a wave walk the quads of their 64-packet
//                      group in output order, each finding its packet by a search over the
//                      group's 64 quad prefixes.  A frame's last quad is zeroed past len.  REF:
//                      launched only when the caller wants the marked positions.
//
// Scratch: qex[Tp] uint64 (quads before each tile), then uint32 nbad[Tp], fbad[Tp], nctrl[Tp],
// fctrl[Tp], qs[Tp], cex[Tp] (bad handles and the first one's position, marks and the first
// one's position, quads, marks before each tile) and meta[n]; T tiles, Tp = T rounded up to 2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "upe_ctx.h"
#include "upe_scan.h"

using namespace upe;

namespace {

constexpr uint32_t kBlock = UPE_INGRESS_BLOCK;   // packets per workgroup of the size and write pass
constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kPer = kBlock / kThreads;     // packets per thread
constexpr uint32_t kGroups = kBlock / 64;        // (round, wave) pairs of a tile: 64-packet groups
constexpr uint32_t kScanThreads = kBlock;        // one thread per packet of the tile with the cut
constexpr uint32_t kScanWaves = kScanThreads / 64;
constexpr uint32_t kWinQuads = UPE_HDR_WINDOW / 16;
constexpr uint32_t kMark = 1u << 16, kBad = 1u << 17;   // meta word bits above the length
static_assert(kBlock % kThreads == 0 && kGroups == kPer * kWaves, "tile shape");
static_assert(kScanThreads <= 1024, "one workgroup");
static_assert(UPE_HDR_WINDOW % 16 == 0, "windows are whole quads");

__device__ __forceinline__ uint32_t quads_of(uint32_t meta) { return ((meta & 0xFFFFu) + 15u) >> 4; }

// Byte j (0..15) of a quad.
__device__ __forceinline__ uint32_t byte_of(const uint4& q, uint32_t j) {
    const uint32_t w = j < 4u ? q.x : j < 8u ? q.y : j < 12u ? q.z : q.w;
    return (w >> (8u * (j & 3u))) & 0xFFu;
}

// Zero the bytes of a quad from byte `rem` on (rem > 0).
__device__ __forceinline__ void zero_tail(uint4& x, uint32_t rem) {
    if (rem < 16u) {
        x.x = keep(x.x, rem, 0u);
        x.y = keep(x.y, rem, 4u);
        x.z = keep(x.z, rem, 8u);
        x.w = keep(x.w, rem, 12u);
    }
}

// The first quad of buffer s (s < nbuf, so s * stride < pool_bytes <= 2^36).
__device__ __forceinline__ uint64_t buffer_quad(uint32_t s, uint64_t stride) {
    return ((uint64_t)s * stride) >> 4;
}

// nbuf = pool_bytes / stride: slot s lies inside the pool exactly when s < nbuf
// ((uint64_t)s * stride + stride <= pool_bytes, without the product's overflow).
template <int kMode>
__global__ void __launch_bounds__(kThreads) upe_ingress_size(
    const uint4* pool, uint64_t nbuf, uint64_t stride, const uint32_t* slot, uint32_t n,
    uint64_t* desc, uint64_t* timestamp, uint32_t* meta, uint32_t* nbad, uint32_t* fbad,
    uint32_t* nctrl, uint32_t* fctrl, uint32_t* qs) {
    __shared__ uint32_t s_nb, s_fb, s_nc, s_fc, s_q;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        s_nb = 0;
        s_fb = kNone;
        s_nc = 0;
        s_fc = kNone;
        s_q = 0;
    }
    __syncthreads();
    const uint32_t p0 = blockIdx.x * kBlock;
    uint32_t nb = 0, fb = kNone, nc = 0, fc = kNone, q = 0;   // a tile: at most 1024 x 4096 quads
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t i = p0 + k * kThreads + tid;
        if (i >= n) continue;
        const uint32_t s = slot[i];
        bool bad = (uint64_t)s >= nbuf;
        uint32_t len = 0;
        uint64_t ts = 0, base = 0;
        bool mark = false;
        if (!bad) {
            base = (uint64_t)s * stride;
            const uint4* b = pool + (base >> 4);
            const uint4 h = b[0];
            ts = (uint64_t)h.x | ((uint64_t)h.y << 32);
            const uint64_t l64 = (uint64_t)h.z | ((uint64_t)h.w << 32);
            bad = l64 > stride - 16u || l64 > 65535u;
            if (!bad) {
                len = (uint32_t)l64;
                // bytes 12..20 lie in data quads 0 and 1; byte 54 is asked for only of an IPv6
                // frame of at least 78 bytes
                uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
                if (len > 12u) q0 = b[1];
                if (len > 16u) q1 = b[2];
                auto at = [&](uint32_t j) -> uint32_t {
                    if (j >= len) return 0u;
                    if (j < 16u) return byte_of(q0, j);
                    if (j < 32u) return byte_of(q1, j - 16u);
                    return byte_of(b[1u + (j >> 4)], j & 15u);
                };
                mark = upe::ctrl_table_write(len, at);
            }
        }
        if (kMode == UPE_INGRESS_REF)
            desc[i] = bad ? UPE_DESC(16u, 0u) : UPE_DESC(base + 16u, len);
        else if (kMode == UPE_INGRESS_WINDOW)
            desc[i] = UPE_DESC((uint64_t)i * UPE_HDR_WINDOW, len);
        if (kMode != UPE_INGRESS_FULL && timestamp) timestamp[i] = ts;
        meta[i] = len | (mark ? kMark : 0u) | (bad ? kBad : 0u);
        if (bad) {
            nb += 1u;
            fb = i < fb ? i : fb;
        }
        if (mark) {
            nc += 1u;
            fc = i < fc ? i : fc;
        }
        q += (len + 15u) >> 4;
    }
    nb = wave_sum(nb);
    nc = wave_sum(nc);
    q = wave_sum(q);
    fb = wave_min(fb);
    fc = wave_min(fc);
    if ((tid & 63u) == 0) {
        atomicAdd(&s_nb, nb);
        atomicAdd(&s_nc, nc);
        atomicAdd(&s_q, q);
        atomicMin(&s_fb, fb);
        atomicMin(&s_fc, fc);
    }
    __syncthreads();
    if (tid == 0) {
        nbad[blockIdx.x] = s_nb;
        fbad[blockIdx.x] = s_fb;
        nctrl[blockIdx.x] = s_nc;
        fctrl[blockIdx.x] = s_fc;
        qs[blockIdx.x] = s_q;
    }
}

// One workgroup; a step covers kScanThreads tiles, one per thread.  cap: the output's size in
// quads (FULL; else the largest value, and `fixed` = the mode's bytes).  A tile whose quads end at
// or below cap fits whole; the first one that does not holds the cut, and no later tile packs
// anything (offsets ascend).
__global__ void __launch_bounds__(kScanThreads) upe_ingress_scan(
    const uint32_t* meta, uint32_t n, uint32_t T, int full, uint64_t cap, uint64_t fixed,
    const uint32_t* nbad, const uint32_t* fbad, const uint32_t* nctrl, const uint32_t* fctrl,
    const uint32_t* qs, uint32_t* cex, uint64_t* qex, upe_ingress_info_t* info) {
    __shared__ uint32_t s_wc[kScanWaves];
    __shared__ uint64_t s_wq[kScanWaves];
    __shared__ uint32_t s_cut, s_nb, s_fb, s_fc;
    __shared__ uint64_t s_cut_q;
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    if (tid == 0) {
        s_cut = kNone;
        s_nb = 0;
        s_fb = kNone;
        s_fc = kNone;
    }
    uint32_t carry_c = 0, my_t = kNone, nb = 0, fb = kNone, fc = kNone;
    uint64_t carry_q = 0, my_q = 0;
    for (uint32_t c0 = 0; c0 < T; c0 += kScanThreads) {
        const uint32_t t = c0 + tid;
        const uint32_t c = t < T ? nctrl[t] : 0u;
        const uint64_t q = t < T ? (uint64_t)qs[t] : 0ull;
        if (t < T) {
            nb += nbad[t];
            const uint32_t x = fbad[t], y = fctrl[t];
            fb = x < fb ? x : fb;
            fc = y < fc ? y : fc;
        }
        // block_excl's step (upe_scan.h), written out: through the helper this kernel, the one
        // with the most live values across the step, took 7 more VGPRs and measured 0.05-0.1 us
        // slower than the form below (profiles/scan_share_ab.txt)
        uint32_t wc;
        uint64_t wq;
        uint32_t ec = wave_excl(c, lane, wc);
        uint64_t eq = wave_excl(q, lane, wq);
        __syncthreads();   // the step before has read s_wc / s_wq (and the shared words are set)
        if (lane == 0) {
            s_wc[wave] = wc;
            s_wq[wave] = wq;
        }
        __syncthreads();
        uint32_t all_c = 0;
        uint64_t all_q = 0;
#pragma unroll
        for (uint32_t j = 0; j < kScanWaves; ++j) {
            const uint32_t x = s_wc[j];
            const uint64_t y = s_wq[j];
            if (j < wave) {
                ec += x;
                eq += y;
            }
            all_c += x;
            all_q += y;
        }
        ec += carry_c;
        eq += carry_q;
        if (t < T) {
            cex[t] = ec;
            qex[t] = eq;
            if (eq + q > cap && my_t == kNone) {   // this thread's tiles ascend: keep the first
                my_t = t;
                my_q = eq;
                atomicMin(&s_cut, t);
            }
        }
        carry_c += all_c;
        carry_q += all_q;
    }
    nb = wave_sum(nb);
    fb = wave_min(fb);
    fc = wave_min(fc);
    if (lane == 0) {
        atomicAdd(&s_nb, nb);
        atomicMin(&s_fb, fb);
        atomicMin(&s_fc, fc);
    }
    __syncthreads();
    const uint32_t cut = s_cut;   // the same for every thread
    uint64_t packed = n, used = carry_q;
    if (cut != kNone) {
        if (my_t == cut) s_cut_q = my_q;
        __syncthreads();
        const uint64_t base_q = s_cut_q;
        const uint32_t i = cut * kBlock + tid;
        const uint32_t p = i < n ? quads_of(meta[i]) : 0u;
        uint32_t wp;
        uint32_t pre = wave_excl(p, lane, wp);
        if (lane == 0) s_wc[wave] = wp;
        __syncthreads();
        for (uint32_t j = 0; j < wave; ++j) pre += s_wc[j];
        const bool fit = i < n && base_q + pre + p <= cap;
        const uint32_t fcnt = (uint32_t)__popcll(__ballot(fit));
        const uint64_t fq = wave_sum((uint64_t)(fit ? p : 0u));
        __syncthreads();   // every wave has read the packet prefixes
        if (lane == 0) {
            s_wc[wave] = fcnt;
            s_wq[wave] = fq;
        }
        __syncthreads();
        packed = (uint64_t)cut * kBlock;
        used = base_q;
        for (uint32_t j = 0; j < kScanWaves; ++j) {
            packed += s_wc[j];
            used += s_wq[j];
        }
    }
    if (tid == 0) {
        const uint32_t first_bad = s_fb, first_ctrl = s_fc;
        info->packets = n;
        info->packed = packed;
        info->bytes = full ? used << 4 : fixed;
        info->need = full ? carry_q << 4 : fixed;
        info->bad = s_nb;
        info->first_bad = first_bad == kNone ? ~0ull : (uint64_t)first_bad;
        info->n_ctrl = carry_c;
        info->first_ctrl = first_ctrl == kNone ? ~0ull : (uint64_t)first_ctrl;
    }
}

template <int kMode>
__global__ void __launch_bounds__(kThreads) upe_ingress_write(
    const uint4* pool, uint64_t nbuf, uint64_t stride, const uint32_t* slot, const uint32_t* meta,
    uint32_t n, uint4* out, uint64_t cap, const uint32_t* nctrl, const uint32_t* cex,
    const uint64_t* qex, uint64_t* desc, uint64_t* timestamp, uint32_t* ctrl) {
    constexpr bool kFull = kMode == UPE_INGRESS_FULL;
    __shared__ uint32_t s_gc[kGroups], s_gq[kGroups];   // marks and quads per 64-packet group
    const uint32_t tile = blockIdx.x;
    if (kMode == UPE_INGRESS_REF && nctrl[tile] == 0) return;   // the whole workgroup
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    const uint32_t p0 = tile * kBlock;
    uint32_t m[kPer], rank[kPer], pre[kPer];
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t i = p0 + k * kThreads + tid;
        m[k] = i < n ? meta[i] : 0u;
        const unsigned long long bal = __ballot((m[k] & kMark) != 0u);
        rank[k] = (uint32_t)__popcll(bal & lanes_below(lane));
        uint32_t gq = 0;
        pre[k] = kFull ? wave_excl(quads_of(m[k]), lane, gq) : 0u;
        if (lane == 0) {
            s_gc[k * kWaves + wave] = (uint32_t)__popcll(bal);
            s_gq[k * kWaves + wave] = gq;
        }
    }
    __syncthreads();
    const uint32_t tile_c = cex[tile];
    const uint64_t tile_q = kFull ? qex[tile] : 0ull;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t grp = k * kWaves + wave;
        if (p0 + grp * 64u >= n) continue;   // the whole wave
        uint32_t cb = tile_c;
        uint64_t qb = tile_q;
        for (uint32_t j = 0; j < grp; ++j) {
            cb += s_gc[j];
            qb += s_gq[j];
        }
        const uint32_t i = p0 + k * kThreads + tid;
        const bool valid = i < n;
        const bool mark = (m[k] & kMark) != 0u;
        if (!kFull) {
            if (ctrl && mark) ctrl[cb + rank[k]] = i;
            continue;
        }
        const bool bad = (m[k] & kBad) != 0u;
        const uint32_t len = m[k] & 0xFFFFu;
        const uint32_t p = (len + 15u) >> 4;
        const uint64_t o = qb + pre[k];
        const bool fits = valid && o + p <= cap;
        uint32_t srcq = 0;   // the frame's first quad: below 2^32, the pool is at most 2^36 bytes
        if (valid) {
            const uint32_t s = slot[i];
            const bool inside = (uint64_t)s < nbuf;
            if (!bad) srcq = (uint32_t)(buffer_quad(s, stride) + 1u);
            if (fits) {
                desc[i] = bad ? UPE_DESC(16u, 0u) : ((o << 20) | len);   // UPE_DESC(16 * o, len)
                if (timestamp) {
                    uint64_t ts = 0;
                    if (inside) {
                        const uint2 h = *reinterpret_cast<const uint2*>(pool + buffer_quad(s, stride));
                        ts = (uint64_t)h.x | ((uint64_t)h.y << 32);
                    }
                    timestamp[i] = ts;
                }
                if (ctrl && mark) ctrl[cb + rank[k]] = i;
            }
        }
        // the group's quads that go out: up to the first frame that does not fit
        const unsigned long long cutm = __ballot(valid && !fits);
        const uint32_t first_out = __shfl(pre[k], cutm ? __ffsll((long long)cutm) - 1 : 0);
        const uint32_t Q = cutm ? first_out : s_gq[grp];
        uint4* dst = out + qb;
        for (uint32_t q0 = 0; q0 < Q; q0 += 64u) {
            const uint32_t q = q0 + (uint32_t)lane;
            const uint32_t qq = q < Q ? q : Q - 1u;
            // the last lane whose prefix is <= qq: its frame holds quad qq (lanes with no quads
            // share the prefix of the lane after them, so the last one of a run is the owner)
            int L = 0;
#pragma unroll
            for (int sft = 32; sft > 0; sft >>= 1) {
                const uint32_t y = __shfl(pre[k], L + sft);
                if (y <= qq) L += sft;
            }
            const uint32_t pl = __shfl(pre[k], L);
            const uint32_t sq = __shfl(srcq, L);
            const uint32_t ln = __shfl(len, L);
            if (q < Q) {
                const uint32_t j = q - pl;   // quad j of the frame
                uint4 x = pool[(size_t)sq + j];
                zero_tail(x, ln - 16u * j);   // > 0: the frame reaches quad j
                dst[q] = x;
            }
        }
    }
    if (kMode == UPE_INGRESS_WINDOW) {
        // output quad g of the tile: packet g / 6, quad g % 6 of its window
        const uint32_t left = n - p0;
        const uint32_t G = (left < kBlock ? left : kBlock) * kWinQuads;
        uint4* dst = out + (size_t)p0 * kWinQuads;
        for (uint32_t g = tid; g < G; g += kThreads) {
            const uint32_t r = g / kWinQuads, j = g - r * kWinQuads;
            const uint32_t len = meta[p0 + r] & 0xFFFFu;   // 0 for a bad handle
            uint4 x = make_uint4(0, 0, 0, 0);
            if (16u * j < len) {
                x = pool[buffer_quad(slot[p0 + r], stride) + 1u + j];
                zero_tail(x, len - 16u * j);
            }
            dst[g] = x;
        }
    }
}

struct Tab {
    uint64_t* qex;
    uint32_t *nbad, *fbad, *nctrl, *fctrl, *qs, *cex, *meta;
};

// The scratch of one gather of n packets in T tiles (n > 0).
Tab layout(Carver& c, uint32_t T, uint32_t n) {
    const size_t tp = ((size_t)T + 1u) & ~(size_t)1u;
    Tab t;
    t.qex = c.take<uint64_t>(tp);   // the 64-bit column first
    t.nbad = c.take<uint32_t>(tp);
    t.fbad = c.take<uint32_t>(tp);
    t.nctrl = c.take<uint32_t>(tp);
    t.fctrl = c.take<uint32_t>(tp);
    t.qs = c.take<uint32_t>(tp);
    t.cex = c.take<uint32_t>(tp);
    t.meta = c.take<uint32_t>(n);
    return t;
}

// Queue the passes on `s`, with the arguments as ingress_gather has checked them.  A pass that a
// mode does not launch leaves its pair of events back to back.
hipError_t upe_ingress_launch(const uint8_t* pool, uint64_t pool_bytes, uint64_t stride,
                              const uint32_t* slot, uint32_t n, int mode, uint8_t* out,
                              uint64_t out_bytes, uint64_t* desc, uint64_t* timestamp,
                              uint32_t* ctrl, upe_ingress_info_t* info, void* scratch,
                              hipStream_t s, hipEvent_t* ev) {
    const uint32_t T = tiles_of(n, kBlock);
    Carver mem(scratch);
    const Tab t = layout(mem, T, n);
    const uint64_t nbuf = pool_bytes / stride;
    const bool full = mode == UPE_INGRESS_FULL;
    const uint64_t cap = full ? out_bytes >> 4 : ~0ull;
    const uint64_t fixed = mode == UPE_INGRESS_WINDOW ? (uint64_t)n * UPE_HDR_WINDOW : 0ull;
    const uint4* p4 = reinterpret_cast<const uint4*>(pool);
    uint4* o4 = reinterpret_cast<uint4*>(out);
    hipError_t e;
    if (ev && (e = hipEventRecord(ev[0], s)) != hipSuccess) return e;
#define UPE_INGRESS_SIZE(M)                                                                    \
    hipLaunchKernelGGL(upe_ingress_size<M>, dim3(T), dim3(kThreads), 0, s, p4, nbuf, stride,  \
                       slot, n, desc, timestamp, t.meta, t.nbad, t.fbad, t.nctrl, t.fctrl, t.qs)
    if (mode == UPE_INGRESS_REF)
        UPE_INGRESS_SIZE(UPE_INGRESS_REF);
    else if (mode == UPE_INGRESS_WINDOW)
        UPE_INGRESS_SIZE(UPE_INGRESS_WINDOW);
    else
        UPE_INGRESS_SIZE(UPE_INGRESS_FULL);
#undef UPE_INGRESS_SIZE
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[1], s)) != hipSuccess) return e;
    hipLaunchKernelGGL(upe_ingress_scan, dim3(1), dim3(kScanThreads), 0, s, t.meta, n, T,
                       full ? 1 : 0, cap, fixed, t.nbad, t.fbad, t.nctrl, t.fctrl, t.qs, t.cex,
                       t.qex, info);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[2], s)) != hipSuccess) return e;
#define UPE_INGRESS_WRITE(M)                                                                   \
    hipLaunchKernelGGL(upe_ingress_write<M>, dim3(T), dim3(kThreads), 0, s, p4, nbuf, stride, \
                       slot, t.meta, n, o4, cap, t.nctrl, t.cex, t.qex, desc, timestamp, ctrl)
    if (mode == UPE_INGRESS_REF) {
        if (ctrl) UPE_INGRESS_WRITE(UPE_INGRESS_REF);   // nothing else is left to write
    } else if (mode == UPE_INGRESS_WINDOW) {
        UPE_INGRESS_WRITE(UPE_INGRESS_WINDOW);
    } else {
        UPE_INGRESS_WRITE(UPE_INGRESS_FULL);
    }
#undef UPE_INGRESS_WRITE
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return ev ? hipEventRecord(ev[3], s) : hipSuccess;
}

// The ingress batch builder (reference src/worker.c:255-307 hands the worker pktbuf handles;
// upe_worker.c gathers them per packet on the CPU).  ev: NULL, or four events recorded before the
// size pass and after each pass (tools/ingress_gather_time.py).
int ingress_gather(upe_gpu_ctx_t* c, const uint8_t* pool, size_t pool_bytes, size_t stride,
                   const uint32_t* d_slot, size_t n, int mode, uint8_t* d_out, size_t out_bytes,
                   uint64_t* d_desc, uint64_t* d_timestamp, uint32_t* d_ctrl,
                   upe_ingress_info_t* d_info, void* stream, hipEvent_t* ev) {
    if (!c) return fail("null context");
    if (!d_info || (n && (!pool || !d_slot || !d_desc))) return fail("null buffer");
    if (mode != UPE_INGRESS_REF && mode != UPE_INGRESS_WINDOW && mode != UPE_INGRESS_FULL)
        return fail("unknown ingress mode");
    if (stride % 16 != 0 || stride < 16 + UPE_FRAME_TAIL)
        return fail("stride must be a multiple of 16 and at least 16 + UPE_FRAME_TAIL");
    if (pool_bytes < stride || pool_bytes > (1ull << 36))
        return fail("pool_bytes must be at least stride and at most 2^36");
    if ((reinterpret_cast<uintptr_t>(pool) & 15u) != 0) return fail("pool must be 16-byte aligned");
    if (mode == UPE_INGRESS_REF ? (d_out != nullptr || out_bytes != 0) : (n && !d_out))
        return fail("d_out goes with WINDOW and FULL mode only");
    if ((reinterpret_cast<uintptr_t>(d_out) & 15u) != 0) return fail("d_out must be 16-byte aligned");
    if (n > 0xFFFFFFFFull - UPE_INGRESS_BLOCK) return fail("n must fit in 32 bits");
    if (mode == UPE_INGRESS_WINDOW && out_bytes / UPE_HDR_WINDOW < n)
        return fail("d_out is smaller than n header windows");
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_info, 0, sizeof(upe_ingress_info_t), s));
        HIP_TRY(hipMemsetAsync(&d_info->first_bad, 0xFF, sizeof(uint64_t), s));
        HIP_TRY(hipMemsetAsync(&d_info->first_ctrl, 0xFF, sizeof(uint64_t), s));
        return 0;
    }
    // the pool as the kernels address it: device memory, or pinned host memory through its mapping
    hipPointerAttribute_t attr = {};
    if (hipPointerGetAttributes(&attr, pool) != hipSuccess) {
        (void)hipGetLastError();
        return fail("pool is neither device memory nor pinned, mapped host memory");
    }
    const uint8_t* dpool = pool;
    uintptr_t lo = reinterpret_cast<uintptr_t>(pool), hi = lo + pool_bytes;
    if (attr.type == hipMemoryTypeHost) {
        dpool = mapped(pool, "pool");
        if (!dpool) return -1;
        lo = reinterpret_cast<uintptr_t>(dpool), hi = lo + pool_bytes;
    } else if (attr.type == hipMemoryTypeDevice) {
        // where the caller's buffers end is not checked against the allocation, but d_out is kept
        // out of all of it, as upe_gpu_egress_pack keeps it out of d_frames'
        const uintptr_t end = alloc_end(pool, hi);
        if (end > hi) hi = end;
    } else {
        return fail("pool is neither device memory nor pinned, mapped host memory");
    }
    if (d_out) {
        const uintptr_t out = reinterpret_cast<uintptr_t>(d_out);
        if (out < hi && lo < out + (out_bytes ? out_bytes : 1)) return fail("d_out overlaps the pool");
    }
    const size_t need = layout_bytes(layout, tiles_of((uint32_t)n, kBlock), (uint32_t)n);
    if (c->in_scratch.reserve(need, need + need / 4) != 0) return -1;
    HIP_TRY(upe_ingress_launch(dpool, pool_bytes, stride, d_slot, (uint32_t)n, mode, d_out,
                               out_bytes, d_desc, d_timestamp, d_ctrl, d_info, c->in_scratch.p, s,
                               ev));
    return 0;
}

}  // namespace

extern "C" {

int upe_gpu_ingress_gather(upe_gpu_ctx_t* c, const uint8_t* pool, size_t pool_bytes, size_t stride,
                           const uint32_t* d_slot, size_t n, int mode, uint8_t* d_out,
                           size_t out_bytes, uint64_t* d_desc, uint64_t* d_timestamp,
                           uint32_t* d_ctrl, upe_ingress_info_t* d_info, void* stream) {
    return ingress_gather(c, pool, pool_bytes, stride, d_slot, n, mode, d_out, out_bytes, d_desc,
                          d_timestamp, d_ctrl, d_info, stream, nullptr);
}

// Diagnostic (tools/ingress_gather_time.py; not in the header): one gather of n > 0 packets with
// HIP events around each pass, then a plain hipMemcpyAsync of copy_bytes from copy_src to copy_dst
// on the same stream (device to device, or host to device when copy_src is pinned host memory):
// the yardstick for the bytes the gather moves.  ms[0..3] = the size, scan and write pass and that
// copy.  Synchronous.
int upe_gpu_ingress_gather_timed(upe_gpu_ctx_t* c, const uint8_t* pool, size_t pool_bytes,
                                 size_t stride, const uint32_t* d_slot, size_t n, int mode,
                                 uint8_t* d_out, size_t out_bytes, uint64_t* d_desc,
                                 uint64_t* d_timestamp, uint32_t* d_ctrl,
                                 upe_ingress_info_t* d_info, const uint8_t* copy_src,
                                 uint8_t* copy_dst, size_t copy_bytes, void* stream, float* ms) {
    if (!c || !ms || !copy_src || !copy_dst || n == 0)
        return fail("null context, no output or an empty batch");
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    Events<6> ev;
    if (ev.create() != 0 ||
        ingress_gather(c, pool, pool_bytes, stride, d_slot, n, mode, d_out, out_bytes, d_desc,
                       d_timestamp, d_ctrl, d_info, stream, ev.e) != 0)
        return -1;
    if (hipStreamSynchronize(s) != hipSuccess) return fail("waiting for the gather");
    return ev.yardstick(copy_dst, copy_src, copy_bytes, hipMemcpyDefault, s, "the yardstick copy",
                        ms);
}

}  // extern "C"
