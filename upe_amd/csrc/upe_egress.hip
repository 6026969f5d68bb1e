// upe_egress.hip — the egress batch builder on the device (upe_gpu_egress_pack,
// include/upe_gpu.h): the forwarded frames of a classified batch, rewritten as process_packet
// leaves them, back to back in one buffer in the order the reference queues them for
// tx_send_batch (src/worker.c:240-243, 287-303).
//
// Every length is counted in 16-byte quads: a frame of len bytes takes (len + 15) >> 4 of them,
// frames start on quad boundaries on both sides, and the copy moves whole quads.
//
// Three launches on one stream; the kernel boundaries are the only ordering between workgroups
// (no workgroup waits on another, no atomic's arrival order reaches an output):
//   upe_egress_size  per workgroup (kBlock packets, a "tile"): the forwarded packets and the sum
//                    of their quads.
//   upe_egress_scan  one workgroup: the exclusive prefix of both over the tiles (quads in 64 bits:
//                    a tile can hold 1024 x 4096 of them and a batch far more than 2^32 bytes),
//                    and *info.  When the output is too small, the first tile that does not fit
//                    whole is scanned packet by packet (one per thread) for the exact cut.
//   upe_egress_copy  per tile: the in-tile scan again (ballot ranks, a wave prefix of the quads,
//                    the 16 groups' sums through LDS), the descriptors and indexes, then the
//                    bytes: the lanes of a wave walk the quads of their 64-packet group in output
//                    order, each finding its packet by a search over the group's 64 quad
//                    prefixes (held one per lane), so that a wave's stores are 1 KiB runs of the
//                    output whatever the frame size.  The quads holding bytes 0..31 get the
//                    record's bytes (emit mode); a frame's last quad is zeroed past len.
//
// Scratch: qex[Tp] uint64 (quads before each tile), then uint32 cnt[Tp], qs[Tp] (the tiles'
// counts and quads) and cex[Tp] (forwarded packets before each tile); T tiles, Tp = T rounded up
// to 2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "upe_ctx.h"
#include "upe_scan.h"

using namespace upe;

namespace {

constexpr uint32_t kBlock = UPE_EGRESS_BLOCK;   // packets per workgroup of the size and copy pass
constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kPer = kBlock / kThreads;    // packets per thread
constexpr uint32_t kGroups = kBlock / 64;       // (round, wave) pairs of a tile: 64-packet groups
constexpr uint32_t kScanThreads = kBlock;       // one thread per packet of the tile with the cut
constexpr uint32_t kScanWaves = kScanThreads / 64;
static_assert(kBlock % kThreads == 0 && kGroups == kPer * kWaves, "tile shape");
static_assert(kScanThreads <= 1024, "one workgroup");

__device__ __forceinline__ bool is_fwd(uint32_t v) { return (v & 0xFu) == (uint32_t)UPE_V_FWD; }
__device__ __forceinline__ uint32_t quads_of(uint64_t d) {
    return ((uint32_t)(d & 0xFFFFu) + 15u) >> 4;
}

__global__ void __launch_bounds__(kThreads) upe_egress_size(const uint64_t* desc,
                                                            const uint32_t* verdict, uint32_t n,
                                                            uint32_t* cnt, uint32_t* qs) {
    __shared__ uint32_t s_c, s_q;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        s_c = 0;
        s_q = 0;
    }
    __syncthreads();
    const uint32_t p0 = blockIdx.x * kBlock;
    uint32_t c = 0, q = 0;   // a tile holds at most 1024 x 4096 quads
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t i = p0 + k * kThreads + tid;
        if (i < n) {
            const uint32_t v = verdict[i];
            const uint64_t d = desc[i];
            if (is_fwd(v)) {
                c += 1u;
                q += quads_of(d);
            }
        }
    }
    c = wave_sum(c);
    q = wave_sum(q);
    if ((tid & 63u) == 0) {
        atomicAdd(&s_c, c);
        atomicAdd(&s_q, q);
    }
    __syncthreads();
    if (tid == 0) {
        cnt[blockIdx.x] = s_c;
        qs[blockIdx.x] = s_q;
    }
}

// One workgroup; a step covers kScanThreads tiles, one per thread.  cap: the output's size in
// quads.  A tile whose quads end at or below cap fits whole; the first one that does not holds
// the cut, and no later tile packs anything (offsets ascend).
__global__ void __launch_bounds__(kScanThreads) upe_egress_scan(
    const uint64_t* desc, const uint32_t* verdict, uint32_t n, uint32_t T, uint64_t cap,
    const uint32_t* cnt, const uint32_t* qs, uint32_t* cex, uint64_t* qex,
    upe_egress_info_t* info) {
    __shared__ uint32_t s_wc[kScanWaves];
    __shared__ uint64_t s_wq[kScanWaves];
    __shared__ uint32_t s_cut, s_cut_c;
    __shared__ uint64_t s_cut_q;
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    if (tid == 0) s_cut = kNone;
    uint32_t carry_c = 0, my_t = kNone, my_c = 0;
    uint64_t carry_q = 0, my_q = 0;
    for (uint32_t c0 = 0; c0 < T; c0 += kScanThreads) {
        const uint32_t t = c0 + tid;
        const uint32_t c = t < T ? cnt[t] : 0u;
        const uint64_t q = t < T ? (uint64_t)qs[t] : 0ull;
        uint32_t ec = c, all_c;
        uint64_t eq = q, all_q;   // (the first step's barriers also order s_cut, set above)
        block_excl(ec, eq, lane, wave, s_wc, s_wq, all_c, all_q);
        ec += carry_c;
        eq += carry_q;
        if (t < T) {
            cex[t] = ec;
            qex[t] = eq;
            if (eq + q > cap && my_t == kNone) {   // this thread's tiles ascend: keep the first
                my_t = t;
                my_c = ec;
                my_q = eq;
                atomicMin(&s_cut, t);
            }
        }
        carry_c += all_c;
        carry_q += all_q;
    }
    __syncthreads();
    const uint32_t cut = s_cut;   // the same for every thread
    uint64_t packed = carry_c, used = carry_q;
    if (cut != kNone) {
        if (my_t == cut) {
            s_cut_c = my_c;
            s_cut_q = my_q;
        }
        __syncthreads();
        const uint64_t base_q = s_cut_q;
        const uint32_t i = cut * kBlock + tid;
        uint32_t p = 0;
        bool fwd = false;
        if (i < n) {
            fwd = is_fwd(verdict[i]);
            if (fwd) p = quads_of(desc[i]);
        }
        uint32_t wp;
        uint32_t pre = wave_excl(p, lane, wp);
        if (lane == 0) s_wc[wave] = wp;
        __syncthreads();
        for (uint32_t j = 0; j < wave; ++j) pre += s_wc[j];
        const bool fit = fwd && base_q + pre + p <= cap;
        const uint32_t fc = (uint32_t)__popcll(__ballot(fit));
        const uint64_t fq = wave_sum((uint64_t)(fit ? p : 0u));
        __syncthreads();   // every wave has read the packet prefixes
        if (lane == 0) {
            s_wc[wave] = fc;
            s_wq[wave] = fq;
        }
        __syncthreads();
        packed = s_cut_c;
        used = base_q;
        for (uint32_t j = 0; j < kScanWaves; ++j) {
            packed += s_wc[j];
            used += s_wq[j];
        }
    }
    if (tid == 0) {
        info->frames = carry_c;
        info->packed = packed;
        info->bytes = used << 4;
        info->need = carry_q << 4;
    }
}

// The record's bytes in the two quads that hold frame bytes 0..31, as upe_hdr_apply places
// them: quad 0 takes b[0..11]; quad 1 the TTL (byte 22) and checksum (bytes 24, 25) of an IPv4
// packet or the hop limit (byte 21) of an IPv6 one.  A record whose b[15] is neither changes
// nothing.
__device__ __forceinline__ void patch(uint4& x, const uint4 r, uint32_t j) {
    const uint32_t fam = r.w >> 24;
    if (fam != 4u && fam != 6u) return;
    if (j == 0) {
        x.x = r.x;
        x.y = r.y;
        x.z = r.z;
    } else if (fam == 4u) {
        x.y = (x.y & 0xFF00FFFFu) | ((r.w & 0xFFu) << 16);
        x.z = (x.z & 0xFFFF0000u) | ((r.w >> 8) & 0xFFFFu);
    } else {
        x.y = (x.y & 0xFFFF00FFu) | ((r.w & 0xFFu) << 8);
    }
}

template <bool kHdr>
__global__ void __launch_bounds__(kThreads) upe_egress_copy(
    const uint4* frames, const uint64_t* desc, const uint32_t* verdict, const uint4* hdr,
    uint32_t n, uint4* out, uint64_t cap, const uint32_t* cnt, const uint32_t* cex,
    const uint64_t* qex, uint64_t* out_desc, uint32_t* out_index) {
    __shared__ uint32_t s_gc[kGroups], s_gq[kGroups];   // forwarded packets and quads per group
    const uint32_t tile = blockIdx.x;
    if (cnt[tile] == 0) return;   // the whole workgroup
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    const uint32_t p0 = tile * kBlock;
    uint64_t d[kPer];
    uint32_t rank[kPer], pre[kPer], fbits = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t i = p0 + k * kThreads + tid;
        const uint32_t v = i < n ? verdict[i] : 0u;
        d[k] = i < n ? desc[i] : 0ull;
        const bool fwd = i < n && is_fwd(v);
        const unsigned long long bal = __ballot(fwd);
        rank[k] = (uint32_t)__popcll(bal & lanes_below(lane));   // UPE_HDR_SLOT's k, too
        uint32_t gq;
        pre[k] = wave_excl(fwd ? quads_of(d[k]) : 0u, lane, gq);
        if (lane == 0) {
            s_gc[k * kWaves + wave] = (uint32_t)__popcll(bal);
            s_gq[k * kWaves + wave] = gq;
        }
        fbits |= fwd ? 1u << k : 0u;
    }
    __syncthreads();
    const uint32_t tile_c = cex[tile];
    const uint64_t tile_q = qex[tile];
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t slot = k * kWaves + wave;
        if (s_gc[slot] == 0) continue;   // the whole wave
        uint32_t cb = tile_c;
        uint64_t qb = tile_q;
        for (uint32_t j = 0; j < slot; ++j) {
            cb += s_gc[j];
            qb += s_gq[j];
        }
        const uint32_t i = p0 + k * kThreads + tid;
        const bool fwd = (fbits >> k) & 1u;
        const uint32_t len = (uint32_t)(d[k] & 0xFFFFu);
        const uint32_t p = fwd ? (len + 15u) >> 4 : 0u;
        const uint64_t o = qb + pre[k];
        const bool fits = fwd && o + p <= cap;
        if (fits) {
            const uint32_t at = cb + rank[k];
            out_desc[at] = (o << 20) | len;   // UPE_DESC(16 * o, len)
            if (out_index) out_index[at] = i;
        }
        // the group's quads that go out: up to the first frame that does not fit
        const unsigned long long cutm = __ballot(fwd && !fits);
        const uint32_t first_out = __shfl(pre[k], cutm ? __ffsll((long long)cutm) - 1 : 0);
        const uint32_t Q = cutm ? first_out : s_gq[slot];
        const uint32_t srcq = (uint32_t)(d[k] >> 20);     // the frame's first quad
        const uint32_t meta = len | (rank[k] << 16);
        const uint4* rec = hdr + (p0 + slot * 64u);       // kHdr: the group's record slots
        uint4* dst = out + qb;
        for (uint32_t q0 = 0; q0 < Q; q0 += 64u) {
            const uint32_t q = q0 + (uint32_t)lane;
            const uint32_t qq = q < Q ? q : Q - 1u;
            // the last lane whose prefix is <= qq: its frame holds quad qq (lanes with no quads
            // share the prefix of the lane after them, so the last one of a run is the owner)
            int L = 0;
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const uint32_t y = __shfl(pre[k], L + s);
                if (y <= qq) L += s;
            }
            const uint32_t pl = __shfl(pre[k], L);
            const uint32_t sq = __shfl(srcq, L);
            const uint32_t m = __shfl(meta, L);
            if (q < Q) {
                const uint32_t j = q - pl;   // quad j of the frame
                uint4 x = frames[(size_t)sq + j];
                if (kHdr && j < 2u) patch(x, rec[m >> 16], j);
                const uint32_t rem = (m & 0xFFFFu) - 16u * j;   // > 0: the frame reaches quad j
                if (rem < 16u) {   // the quad's bytes from `rem` on are zeroed
                    x.x = keep(x.x, rem, 0u);
                    x.y = keep(x.y, rem, 4u);
                    x.z = keep(x.z, rem, 8u);
                    x.w = keep(x.w, rem, 12u);
                }
                dst[q] = x;
            }
        }
    }
}

struct Tab {
    uint64_t* qex;
    uint32_t *cnt, *qs, *cex;
};

// The scratch of one pack over T tiles.
Tab layout(Carver& c, uint32_t T) {
    const size_t tp = ((size_t)T + 1u) & ~(size_t)1u;
    Tab t;
    t.qex = c.take<uint64_t>(tp);   // the 64-bit column first
    t.cnt = c.take<uint32_t>(tp);
    t.qs = c.take<uint32_t>(tp);
    t.cex = c.take<uint32_t>(tp);
    return t;
}

// Queue the three passes on `s`, with the arguments as egress_pack has checked them.  hdr NULL:
// the frames are copied; else each forwarded frame gets its record.
hipError_t upe_egress_launch(const uint8_t* frames, const uint64_t* desc, const uint32_t* verdict,
                             const upe_hdr_rec_t* hdr, uint32_t n, uint8_t* out,
                             uint64_t out_bytes, uint64_t* out_desc, uint32_t* out_index,
                             upe_egress_info_t* info, void* scratch, hipStream_t s,
                             hipEvent_t* ev) {
    const uint32_t T = tiles_of(n, kBlock);
    Carver mem(scratch);
    const Tab t = layout(mem, T);
    const uint64_t cap = out_bytes >> 4;
    const uint4* f4 = reinterpret_cast<const uint4*>(frames);
    const uint4* h4 = reinterpret_cast<const uint4*>(hdr);
    uint4* o4 = reinterpret_cast<uint4*>(out);
    hipError_t e;
    if (ev && (e = hipEventRecord(ev[0], s)) != hipSuccess) return e;
    hipLaunchKernelGGL(upe_egress_size, dim3(T), dim3(kThreads), 0, s, desc, verdict, n, t.cnt,
                       t.qs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[1], s)) != hipSuccess) return e;
    hipLaunchKernelGGL(upe_egress_scan, dim3(1), dim3(kScanThreads), 0, s, desc, verdict, n, T, cap,
                       t.cnt, t.qs, t.cex, t.qex, info);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[2], s)) != hipSuccess) return e;
    if (hdr)
        hipLaunchKernelGGL(upe_egress_copy<true>, dim3(T), dim3(kThreads), 0, s, f4, desc, verdict,
                           h4, n, o4, cap, t.cnt, t.cex, t.qex, out_desc, out_index);
    else
        hipLaunchKernelGGL(upe_egress_copy<false>, dim3(T), dim3(kThreads), 0, s, f4, desc, verdict,
                           h4, n, o4, cap, t.cnt, t.cex, t.qex, out_desc, out_index);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return ev ? hipEventRecord(ev[3], s) : hipSuccess;
}

// The egress batch builder (reference src/worker.c:240-243, 287-303: the frames queued for
// tx_send_batch, in order).  ev: NULL, or four events recorded before the size pass and after each
// pass (tools/egress_pack_time.py).
int egress_pack(upe_gpu_ctx_t* c, const uint8_t* d_frames, const uint64_t* d_desc,
                const uint32_t* d_verdict, const upe_hdr_rec_t* d_hdr, size_t n, uint8_t* d_out,
                size_t out_bytes, uint64_t* d_out_desc, uint32_t* d_out_index,
                upe_egress_info_t* d_info, void* stream, hipEvent_t* ev) {
    if (!c) return fail("null context");
    if (!d_info || (n && (!d_frames || !d_desc || !d_verdict || !d_out || !d_out_desc)))
        return fail("null buffer");
    if ((reinterpret_cast<uintptr_t>(d_out) & 15u) != 0 ||
        (reinterpret_cast<uintptr_t>(d_frames) & 15u) != 0 ||
        (reinterpret_cast<uintptr_t>(d_hdr) & 15u) != 0)
        return fail("d_out, d_frames and d_hdr must be 16-byte aligned");
    if (n > 0xFFFFFFFFull - UPE_EGRESS_BLOCK) return fail("n must fit in 32 bits");
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_info, 0, sizeof(upe_egress_info_t), s));
        return 0;
    }
    // where the frames end is not known here: they count up to the end of their allocation
    const uintptr_t fr = reinterpret_cast<uintptr_t>(d_frames);
    const uintptr_t out = reinterpret_cast<uintptr_t>(d_out);
    const uintptr_t fr_end = alloc_end(d_frames, fr + 1);
    if (out < fr_end && fr < out + (out_bytes ? out_bytes : 1))
        return fail("d_out overlaps d_frames");
    const size_t need = layout_bytes(layout, tiles_of((uint32_t)n, kBlock));
    if (c->eg_scratch.reserve(need, need + need / 4) != 0) return -1;
    HIP_TRY(upe_egress_launch(d_frames, d_desc, d_verdict, d_hdr, (uint32_t)n, d_out, out_bytes,
                              d_out_desc, d_out_index, d_info, c->eg_scratch.p, s, ev));
    return 0;
}

}  // namespace

extern "C" {

int upe_gpu_egress_pack(upe_gpu_ctx_t* c, const uint8_t* d_frames, const uint64_t* d_desc,
                        const uint32_t* d_verdict, const upe_hdr_rec_t* d_hdr, size_t n,
                        uint8_t* d_out, size_t out_bytes, uint64_t* d_out_desc,
                        uint32_t* d_out_index, upe_egress_info_t* d_info, void* stream) {
    return egress_pack(c, d_frames, d_desc, d_verdict, d_hdr, n, d_out, out_bytes, d_out_desc,
                       d_out_index, d_info, stream, nullptr);
}

// Diagnostic (tools/egress_pack_time.py; not in the header): one pack of n > 0 packets with HIP
// events around each pass, then a plain device-to-device copy of the packed bytes (info.bytes,
// d_out -> d_copy, out_bytes of room) on the same stream: the floor of the copy pass.
// ms[0..3] = the size, scan and copy pass and that copy.  Synchronous.
int upe_gpu_egress_pack_timed(upe_gpu_ctx_t* c, const uint8_t* d_frames, const uint64_t* d_desc,
                              const uint32_t* d_verdict, const upe_hdr_rec_t* d_hdr, size_t n,
                              uint8_t* d_out, size_t out_bytes, uint64_t* d_out_desc,
                              uint32_t* d_out_index, upe_egress_info_t* d_info, uint8_t* d_copy,
                              void* stream, float* ms) {
    if (!c || !ms || !d_copy || n == 0)
        return fail("null context, no output or an empty batch");
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    Events<6> ev;
    if (ev.create() != 0 ||
        egress_pack(c, d_frames, d_desc, d_verdict, d_hdr, n, d_out, out_bytes, d_out_desc,
                    d_out_index, d_info, stream, ev.e) != 0)
        return -1;
    upe_egress_info_t info = {};
    if (hipMemcpyAsync(&info, d_info, sizeof(info), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return fail("reading the pack's info");
    return ev.yardstick(d_copy, d_out, info.bytes, hipMemcpyDeviceToDevice, s,
                        "the device-to-device copy", ms);
}

}  // extern "C"
