// upe_release.hip — the order in which the reference worker releases a classified batch's buffers
// (upe_gpu_release_order, include/upe_gpu.h): per burst, the packets that are not forwarded in
// packet order — process_packet's frees at its exits (reference src/worker.c:97, 123, 135, 151,
// 170, 209, 252) — then the forwarded ones in packet order — tx_bufs[] (src/worker.c:240-243),
// the burst's tx_send_batch arguments and the frees after it (src/worker.c:287-303); beside it the
// forwarded count of every burst, the handles in that order and the list of answered ARP requests
// (tx_send, src/worker.c:51).
//
// Three launches on one stream; the kernel boundaries are the only ordering between workgroups, no
// result depends on the order in which workgroups run, and there is no atomic on global memory:
//   upe_release_count  per workgroup (kBlock packets, a "tile"), one lane per packet and one
//                      coalesced dword load of each verdict, the only one: a wave's forwarded lanes
//                      and its reply lanes become two 64-bit ballot words in scratch, and the
//                      tile's forwarded, consumed and reply counts and first reply go to the tile
//                      table.
//                      With an offset array the workgroup also checks bursts tile * kBlock ..
//                      + kBlock - 1 (nb <= n: the tiles cover them), and a valid burst that covers
//                      a tile's first packet writes its index to that tile's entry (a burst of at
//                      most 64 packets covers at most one).
//   upe_release_scan   one workgroup: the exclusive prefix of the reply counts over the tiles, the
//                      totals, *info and the word that stops the last pass when the offset array
//                      is not valid.
//   upe_release_write  per tile: the 16 forwarded words and one word of halo on each side (zero
//                      past the batch's ends) in LDS.  A burst never exceeds 64 packets, so a
//                      packet's two counts — forwarded in [s, i) and in [s, e) — are popcounts
//                      over a window of at most 64 bits cut from that bitmap, and its store of
//                      d_order lands within 64 entries of its own index.  With an offset array the
//                      tile's offsets (at most 1025 touch a tile, a few more the halo) are staged
//                      from the tile's first burst on as bits of a second bitmap: s is the highest
//                      such bit at or below i, e the lowest above it, a burst's index the bits
//                      before it.
//                      A tile without replies never enters the reply path.
//
// Scratch: uint64 fwd[16 T], rep[16 T] (the ballot words); uint32 tf[Tp], tc[Tp], tr[Tp], tfr[Tp],
// tb[Tp], rex[Tp], b0[Tp] (per tile: forwarded, consumed, replies, first reply, bad bursts, replies
// before the tile, the burst that covers its first packet) and flag[4]; T tiles, Tp = T rounded up
// to 4.  Every word a pass reads was written by an earlier pass of the same call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "upe_ctx.h"
#include "upe_scan.h"

using namespace upe;

namespace {

constexpr uint32_t kBlock = UPE_RELEASE_BLOCK;   // packets per workgroup of the count / write pass
constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kPer = kBlock / kThreads;     // packets per thread
constexpr uint32_t kGroups = kBlock / 64;        // (round, wave) pairs of a tile: 64-packet groups
constexpr uint32_t kWords = kGroups + 3;         // the tile's bitmap: halo, groups, halo, a zero
constexpr uint32_t kBits = (kGroups + 2) * 64;   // positions a bitmap holds: the last word stays 0
constexpr uint32_t kStageRounds = (kBits + kThreads - 1) / kThreads;
constexpr uint32_t kScanThreads = 1024;          // tiles per step of the scan
constexpr uint32_t kScanWaves = kScanThreads / 64;
static_assert(kBlock % kThreads == 0 && kGroups == kPer * kWaves, "tile shape");
static_assert(UPE_TX_BATCH_MAX == 64, "a burst fits one ballot word");

struct Tab {
    unsigned long long *fwd, *rep;
    uint32_t *tf, *tc, *tr, *tfr, *tb, *rex, *b0, *flag;
};

__device__ __forceinline__ unsigned long long low_bits(uint32_t k) {   // k <= 64
    return k >= 64u ? ~0ull : (1ull << k) - 1ull;
}

__global__ void __launch_bounds__(kThreads) upe_release_count(
    const uint32_t* __restrict__ verdict, uint32_t n, const uint32_t* __restrict__ first,
    uint32_t nb, uint32_t T, Tab t) {
    __shared__ uint32_t s_w[kWaves][5];   // forwarded, consumed, replies, first reply, bad bursts
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t tile = blockIdx.x, p0 = tile * kBlock;
    uint32_t v[kPer];
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t i = p0 + k * kThreads + tid;   // < n + kBlock: no wrap
        v[k] = i < n ? verdict[i] : 0u;               // past the batch: no forward, no reply
    }
    uint32_t nf = 0, nc = 0, nr = 0, fr = kNone;      // the same in every lane of a wave
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t g = k * kWaves + wave, code = UPE_VERDICT_CODE(v[k]);
        const unsigned long long bf = __ballot(code == (uint32_t)UPE_V_FWD);
        const unsigned long long bc = __ballot(code == (uint32_t)UPE_V_CONSUMED);
        const unsigned long long br = __ballot((v[k] & (uint32_t)UPE_VF_ARP_REPLY) != 0u);
        nf += (uint32_t)__popcll(bf);
        nc += (uint32_t)__popcll(bc);
        nr += (uint32_t)__popcll(br);
        if (br != 0ull && fr == kNone)   // the wave's groups ascend with k
            fr = p0 + g * 64u + (uint32_t)__builtin_ctzll(br);
        if (lane == 0) {
            t.fwd[(size_t)tile * kGroups + g] = bf;
            t.rep[(size_t)tile * kGroups + g] = br;
        }
    }
    uint32_t bad = 0;
    if (first) {
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t b = p0 + k * kThreads + tid;   // a burst's index here
            if (b >= nb) continue;
            const uint32_t f0 = first[b], f1 = first[b + 1u];
            if (f1 - f0 - 1u >= (uint32_t)UPE_TX_BATCH_MAX) {   // modulo 2^32: descending too
                bad += 1u;
                continue;
            }
            // the first tile boundary at or past f0; the burst covers it when it lies below f1
            const uint32_t tk = f0 / kBlock + (f0 % kBlock != 0u ? 1u : 0u);
            if (tk < T && tk * kBlock < f1) t.b0[tk] = b;
        }
        if (tile == 0 && tid == 0) bad += (first[0] != 0u ? 1u : 0u) + (first[nb] != n ? 1u : 0u);
        bad = wave_sum(bad);
    }
    if (lane == 0) {
        s_w[wave][0] = nf;
        s_w[wave][1] = nc;
        s_w[wave][2] = nr;
        s_w[wave][3] = fr;
        s_w[wave][4] = bad;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t a = 0, b = 0, c = 0, d = kNone, e = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            a += s_w[w][0];
            b += s_w[w][1];
            c += s_w[w][2];
            d = s_w[w][3] < d ? s_w[w][3] : d;
            e += s_w[w][4];
        }
        t.tf[tile] = a;
        t.tc[tile] = b;
        t.tr[tile] = c;
        t.tfr[tile] = d;
        t.tb[tile] = e;
    }
}

// One workgroup; a step covers kScanThreads tiles, one per thread.  The sums stay below 2^32: the
// counts over the packets are at most n, the bad bursts at most nb + 2 <= n + 2.
__global__ void __launch_bounds__(kScanThreads) upe_release_scan(
    uint32_t T, uint32_t n, uint64_t bursts, Tab t, upe_release_info_t* info) {
    __shared__ uint32_t s_rr[kScanWaves];
    __shared__ uint32_t s_q[kScanWaves][4];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    uint32_t carry = 0, nf = 0, nc = 0, bad = 0, fr = kNone;
    for (uint32_t c0 = 0; c0 < T; c0 += kScanThreads) {
        const uint32_t x = c0 + tid;
        uint32_t r = 0;
        if (x < T) {
            r = t.tr[x];
            nf += t.tf[x];
            nc += t.tc[x];
            bad += t.tb[x];
            const uint32_t y = t.tfr[x];
            fr = y < fr ? y : fr;
        }
        uint32_t all;
        const uint32_t ex = block_excl(r, lane, wave, s_rr, all);
        if (x < T) t.rex[x] = carry + ex;
        carry += all;
    }
    nf = wave_sum(nf);
    nc = wave_sum(nc);
    bad = wave_sum(bad);
    fr = wave_min(fr);
    if (lane == 0) {
        s_q[wave][0] = nf;
        s_q[wave][1] = nc;
        s_q[wave][2] = bad;
        s_q[wave][3] = fr;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t a = 0, b = 0, c = 0, d = kNone;
        for (uint32_t w = 0; w < kScanWaves; ++w) {
            a += s_q[w][0];
            b += s_q[w][1];
            c += s_q[w][2];
            d = s_q[w][3] < d ? s_q[w][3] : d;
        }
        info->packets = n;
        info->bursts = bursts;
        info->forwarded = a;
        info->consumed = b;
        info->dropped = (uint64_t)n - a - b;
        info->replies = carry;
        info->first_reply = d == kNone ? ~0ull : (uint64_t)d;
        info->bad_bursts = c;
        *t.flag = c;
    }
}

// 64 bits of a bitmap of kWords words from position q on; q / 64 + 1 < kWords
__device__ __forceinline__ unsigned long long cut(const unsigned long long* w, uint32_t q) {
    const uint32_t j = q >> 6, sh = q & 63u;
    const unsigned long long a = w[j], b = w[j + 1u];
    return sh ? (a >> sh) | (b << (64u - sh)) : a;
}

// kVar: bursts from the offset array `first` (valid: the scan's flag is zero), else of `burst`
// packets each.  A position in the tile's bitmaps is the packet's index - p0 + 64.
template <bool kVar>
__global__ void __launch_bounds__(kThreads) upe_release_write(
    uint32_t n, const uint32_t* __restrict__ first, uint32_t nb, uint32_t burst,
    const uint32_t* __restrict__ slot, uint32_t* order, uint32_t* handle, uint32_t* burst_fwd,
    uint32_t* reply, Tab t) {
    __shared__ unsigned long long s_fwd[kWords];   // forwarded packets
    __shared__ unsigned long long s_st[kWords];    // kVar: first packets of bursts
    __shared__ uint32_t s_st32[2 * kWords];        // the same while the bits are being set
    __shared__ uint32_t s_pre[kWords];             // kVar: such bits before each word
    __shared__ unsigned long long s_rep[kGroups];  // replies
    __shared__ uint32_t s_rpre[kGroups];           // replies before each group
    if (*t.flag != 0u) return;                     // a bad offset array: nothing is touched
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t tile = blockIdx.x, p0 = tile * kBlock;
    const uint32_t groups = (n + 63u) / 64u;       // n <= 2^32 - 1 - kBlock
    const uint32_t nrep = reply ? t.tr[tile] : 0u;
    const uint32_t bursts = kVar ? nb : (n + burst - 1u) / burst;
    if (tid < kWords) {
        // word w holds group tile * kGroups + w - 1, when there is one
        const uint32_t g = tile * kGroups + tid - 1u;   // tile 0, word 0: wraps past `groups`
        s_fwd[tid] = tid < kGroups + 2u && g < groups ? t.fwd[g] : 0ull;
    }
    if (nrep && tid >= 64u && tid < 64u + kGroups)
        s_rep[tid - 64u] = t.rep[(size_t)tile * kGroups + (tid - 64u)];
    uint32_t b0 = 0;
    if (kVar) {
        if (tid < 2u * kWords) s_st32[tid] = 0u;
        b0 = t.b0[tile];   // first[b0] <= p0 < first[b0 + 1]: first[b0] > p0 - 64
        __syncthreads();
        for (uint32_t r = 0; r < kStageRounds; ++r) {
            const uint32_t idx = b0 + r * kThreads + tid;   // nb + kBits < 2^32
            bool in = false;
            if (idx <= nb) {
                const uint32_t rel = first[idx] - p0 + 64u;   // the offsets ascend from rel >= 1
                in = rel < kBits;
                if (in) atomicOr(&s_st32[rel >> 5], 1u << (rel & 31u));
            }
            if (!__syncthreads_or(in)) break;   // every offset from here on is past the halo
        }
        if (tid < kWords)
            s_st[tid] = (unsigned long long)s_st32[2u * tid] |
                        (unsigned long long)s_st32[2u * tid + 1u] << 32;
    }
    __syncthreads();
    if (kVar && tid < kWords) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < tid; ++w) c += (uint32_t)__popcll(s_st[w]);
        s_pre[tid] = c;
    }
    if (nrep && tid >= 64u && tid < 64u + kGroups) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < tid - 64u; ++w) c += (uint32_t)__popcll(s_rep[w]);
        s_rpre[tid - 64u] = c;
    }
    __syncthreads();
    const uint32_t rbase = nrep ? t.rex[tile] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t i = p0 + k * kThreads + tid;
        if (i >= n) continue;
        const uint32_t rel = i - p0 + 64u;   // 64 .. kBlock + 63
        uint32_t s, e;
        if (kVar) {
            // positions rel - 63 .. rel and rel + 1 .. rel + 64: a burst holds at most 64 packets
            const unsigned long long back = cut(s_st, rel - 63u), fore = cut(s_st, rel + 1u);
            s = i - (back ? (uint32_t)__builtin_clzll(back) : 63u);
            e = i + 1u + (fore ? (uint32_t)__builtin_ctzll(fore) : 63u);
        } else {
            s = i / burst * burst;
            e = n - s < burst ? n : s + burst;
        }
        const uint32_t len = e - s < 64u ? e - s : 64u, d = i - s;   // 1 .. 64; 0 .. 63
        const uint32_t srel = s - p0 + 64u;                          // >= 1
        const unsigned long long f = cut(s_fwd, srel) & low_bits(len);
        const uint32_t before = (uint32_t)__popcll(f & low_bits(d)), total = (uint32_t)__popcll(f);
        const bool fwd = (f >> d) & 1ull;
        // not forwarded: after the burst's such packets before it; forwarded: after all of them
        const uint32_t pos = fwd ? s + (len - total) + before : s + (d - before);
        if (pos < n) {   // always
            order[pos] = i;
            if (slot) handle[pos] = slot[i];
        }
        if (d == 0u) {   // the burst's first packet stores its count
            uint32_t b;
            if (kVar)
                b = b0 + s_pre[srel >> 6] +
                    (uint32_t)__popcll(s_st[srel >> 6] & low_bits(srel & 63u));
            else
                b = i / burst;
            if (b < bursts) burst_fwd[b] = total;   // always
        }
        if (nrep) {
            const uint32_t g = k * kWaves + wave;
            const unsigned long long m = s_rep[g];
            if ((m >> lane) & 1ull) {
                const uint32_t rank = rbase + s_rpre[g] + (uint32_t)__popcll(m & low_bits(lane));
                if (rank < n) reply[rank] = i;   // always
            }
        }
    }
}

// The scratch of one call over T tiles.
Tab layout(Carver& c, uint32_t T) {
    const size_t tp = ((size_t)T + 3u) & ~(size_t)3u;
    Tab t;
    t.fwd = c.take<unsigned long long>((size_t)T * kGroups);   // the ballot words: 64-bit, first
    t.rep = c.take<unsigned long long>((size_t)T * kGroups);
    t.tf = c.take<uint32_t>(tp);
    t.tc = c.take<uint32_t>(tp);
    t.tr = c.take<uint32_t>(tp);
    t.tfr = c.take<uint32_t>(tp);
    t.tb = c.take<uint32_t>(tp);
    t.rex = c.take<uint32_t>(tp);
    t.b0 = c.take<uint32_t>(tp);
    t.flag = c.take<uint32_t>(4);
    return t;
}

}  // namespace

extern "C" int upe_gpu_release_order(upe_gpu_ctx_t* c, const uint32_t* d_verdict, size_t n,
                                     const uint32_t* d_burst_first, size_t nb, uint32_t burst,
                                     const uint32_t* d_slot, uint32_t* d_order,
                                     uint32_t* d_handle, uint32_t* d_burst_fwd, uint32_t* d_reply,
                                     upe_release_info_t* d_info, void* stream) {
    if (!c) return fail("null context");
    if (!d_info || (n && (!d_verdict || !d_order || !d_burst_fwd))) return fail("null buffer");
    if ((d_slot == nullptr) != (d_handle == nullptr))
        return fail("d_slot and d_handle are given together or not at all");
    if (!d_burst_first && (burst == 0 || burst > UPE_TX_BATCH_MAX))
        return fail("burst must be 1..UPE_TX_BATCH_MAX");
    if (d_burst_first && ((nb == 0 && n > 0) || nb > n))
        return fail("an offset array describes 1..n bursts");
    if (n > 0xFFFFFFFFull - UPE_RELEASE_BLOCK) return fail("n must fit in 32 bits");
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    if (n == 0) return empty_info(d_info, &upe_release_info_t::first_reply, s);
    const uint32_t T = tiles_of((uint32_t)n, kBlock);
    const size_t need = layout_bytes(layout, T);
    if (c->rl_scratch.reserve(need, need + need / 4) != 0) return -1;
    Carver mem(c->rl_scratch.p);
    const Tab t = layout(mem, T);
    const uint64_t bursts = d_burst_first ? (uint64_t)nb : ((uint64_t)n + burst - 1) / burst;
    hipLaunchKernelGGL(upe_release_count, dim3(T), dim3(kThreads), 0, s, d_verdict, (uint32_t)n,
                       d_burst_first, (uint32_t)nb, T, t);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(upe_release_scan, dim3(1), dim3(kScanThreads), 0, s, T, (uint32_t)n, bursts,
                       t, d_info);
    HIP_TRY(hipGetLastError());
    if (d_burst_first)
        hipLaunchKernelGGL(upe_release_write<true>, dim3(T), dim3(kThreads), 0, s, (uint32_t)n,
                           d_burst_first, (uint32_t)nb, burst, d_slot, d_order, d_handle,
                           d_burst_fwd, d_reply, t);
    else
        hipLaunchKernelGGL(upe_release_write<false>, dim3(T), dim3(kThreads), 0, s, (uint32_t)n,
                           d_burst_first, (uint32_t)nb, burst, d_slot, d_order, d_handle,
                           d_burst_fwd, d_reply, t);
    HIP_TRY(hipGetLastError());
    return 0;
}
