// upe_keys.hip — flow keys on the device, apart from the classify launch (upe_gpu_parse_keys,
// upe_gpu_match_keys, include/upe_gpu.h): the two reference entry points callers use on their own,
// parse_flow_key (src/parser.c:6-111; the RX thread, src/rx_pcap.c:71-72) over a resident batch,
// and rule_table_match (src/rule_table.c:163-176) over an array of keys, against the context's
// loaded table or against a compiled image that is not loaded (a dry run before a reload).
//
// Both kernels: one key per lane, workgroups of 256 threads walking 256-key tiles a grid apart, no
// state between keys, no atomics; neither touches anything of the context's but the rule table.
//
// Keys are 44-byte records, so a tile's 256 records move between the caller's array and LDS row
// by row, 256 contiguous words per instruction, and a lane takes its own record from LDS at an
// odd stride (upe_key_tile.h, shared with upe_neigh.hip).
//
// upe_parse_keys reads a frame's first 96 bytes as 16-byte loads, only the chunks that begin below
// len (the batch layout keeps UPE_FRAME_TAIL bytes readable behind every frame start), and clears
// every byte at or past len in the loaded words before any gate looks at them: what it computes
// is parse_flow_key (parse_key, upe_parse.h) over a zero-filled pktbuf holding the frame.
//
// upe_match_keys unpacks a record into the words upe_classify hands its matchers (upe_match.h:
// key_k0 / key_k1 and the address words) and calls the matcher of the table's index kind: the
// same source as the classify kernels', here reading the tree, the family lists and the
// tuple-space fingerprints from memory; a table of up to kSmallRules rules is staged in LDS as
// upe_classify stages it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "upe_ctx.h"
#include "upe_key_tile.h"
#include "upe_match.h"
#include "upe_parse.h"

namespace {

// A flow key (Key, upe_parse.h) as a record.  Record words: 0 ip_ver (bytes 1-3 padding), 1-4
// src_ip, 5-8 dst_ip, 9 src_port | dst_port << 16, 10 protocol (bytes 41-43 padding).
__device__ __forceinline__ void key_to_words(const Key& k, uint32_t (&w)[kKeyWords]) {
    w[0] = k.ver;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        w[1 + j] = k.s[j];
        w[5 + j] = k.d[j];
    }
    w[9] = k.sport | k.dport << 16;
    w[10] = k.proto;
}
// Padding is dropped, and an IPv4 key's union bytes 4-15 with it.
__device__ __forceinline__ Key key_from_words(const uint32_t (&w)[kKeyWords]) {
    Key k;
    k.ver = w[0] & 0xFFu;
    const bool v6 = k.ver == 6u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        k.s[j] = v6 || j == 0 ? w[1 + j] : 0u;
        k.d[j] = v6 || j == 0 ? w[5 + j] : 0u;
    }
    k.sport = w[9] & 0xFFFFu;
    k.dport = w[9] >> 16;
    k.proto = w[10] & 0xFFu;
    return k;
}

__global__ void __launch_bounds__(kThreads) upe_parse_keys(const uint8_t* __restrict__ frames,
                                                           const uint64_t* __restrict__ desc,
                                                           uint32_t n, uint32_t* __restrict__ keys,
                                                           int32_t* __restrict__ rc) {
    __shared__ uint32_t s_key[kKeyWords * kThreads];
    const uint32_t tid = threadIdx.x;
    const uint32_t tiles = (n + kThreads - 1u) / kThreads;   // n <= kMaxKeys
    const size_t words = (size_t)n * kKeyWords;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t i = t * kThreads + tid;   // < n + kThreads: no wrap
        uint32_t w[24], len = 0;
#pragma unroll
        for (int j = 0; j < 24; ++j) w[j] = 0;
        if (i < n) {
            const uint64_t dsc = desc[i];
            len = (uint32_t)(dsc & 0xFFFFu);
            const uint4* q = reinterpret_cast<const uint4*>(frames + ((size_t)(dsc >> 20) << 4));
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                if (len > 16u * c) {   // chunks at or past len are not read
                    const uint4 v = q[c];
                    w[4 * c + 0] = v.x; w[4 * c + 1] = v.y; w[4 * c + 2] = v.z; w[4 * c + 3] = v.w;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 24; ++j) w[j] &= len_mask(len, j);
        Key k;
        const bool ok = parse_key(w, len, k);
        uint32_t kw[kKeyWords];
        key_to_words(k, kw);
#pragma unroll
        for (uint32_t j = 0; j < kKeyWords; ++j) s_key[kKeyWords * tid + j] = ok ? kw[j] : 0u;
        if (rc && i < n) rc[i] = ok ? 0 : -1;
        __syncthreads();
        tile_store(keys, s_key, (size_t)t * (kKeyWords * kThreads), words, tid);
        __syncthreads();   // the next tile's records overwrite s_key
    }
}

// What the matchers read of a compiled table (DeviceTable): the fields of upe_gpu.hip's Args that
// upe_match.h names.  Nothing is staged but the small table, so the *_lds flags are zero.
struct MatchArgs {
    const uint32_t* keys;
    int32_t* rule;
    uint32_t n;
    const RuleV4* rv4;
    const RuleV6* rv6;
    uint32_t nrules_pad;
    const uint4* fam;
    uint32_t fam4, fam6, fam6_lds, fam4_lds, fam_x1idx;
    const uint2* tree;
    uint32_t tree_loff;
    const TssGroup* tg4;
    const TssGroup* tg6;
    const uint4* tt4;
    const uint4* tt6;
    uint32_t ng4, ng6;
};
// How a table is matched: upe_classify's kScan 0-3 (upe_plan.h, plan_lds), and its tuple-space mode.
enum MatchKind { M_SMALL = 0, M_FAM = 1, M_WHOLE = 2, M_TREE = 3, M_TSS = 4 };

template <int kKind>
__global__ void __launch_bounds__(kThreads) upe_match_keys(MatchArgs a) {
    __shared__ uint32_t s_key[kKeyWords * kThreads];
    __shared__ u32x8 s_rv4[kKind == M_SMALL ? kSmallRules : 1];
    __shared__ u32x16 s_rv6[kKind == M_SMALL ? kSmallRules : 1];
    const uint32_t tid = threadIdx.x;
    if (kKind == M_SMALL) {   // nrules_pad <= kSmallRules (match_kind): the whole table
        const uint32_t nst = a.nrules_pad;
        const uint4* g4 = reinterpret_cast<const uint4*>(a.rv4);
        const uint4* g6 = reinterpret_cast<const uint4*>(a.rv6);
        uint4* d4 = reinterpret_cast<uint4*>(s_rv4);
        uint4* d6 = reinterpret_cast<uint4*>(s_rv6);
        for (uint32_t k = tid; k < 2 * nst; k += kThreads) d4[k] = g4[k];
        for (uint32_t k = tid; k < 4 * nst; k += kThreads) d6[k] = g6[k];
    }
    const uint32_t tiles = (a.n + kThreads - 1u) / kThreads;   // n <= kMaxKeys
    const size_t words = (size_t)a.n * kKeyWords;
    // every thread of the workgroup runs every pass (the barriers), and every lane of a wave
    // enters the matcher (their loops are wave-uniform): lanes past n carry no key
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t i = t * kThreads + tid;   // < n + kThreads: no wrap
        tile_load(s_key, a.keys, (size_t)t * (kKeyWords * kThreads), words, tid);
        __syncthreads();   // (the first pass: the small table's copy too)
        uint32_t kw[kKeyWords];
#pragma unroll
        for (uint32_t j = 0; j < kKeyWords; ++j) kw[j] = s_key[kKeyWords * tid + j];
        __syncthreads();   // the next tile's records overwrite s_key
        const Key k = key_from_words(kw);
        const bool is6 = k.ver == 6u;
        // an ip_ver other than 4 / 6 matches nothing (upe_rules_match_host's convention)
        const bool ok = i < a.n && (is6 || k.ver == 4u);
        const uint32_t k0 = key_k0(is6, k.proto, k.sport), k1 = key_k1(k.dport);
        const bool need_v6 = __any(ok && is6);
        uint32_t ri, act = 0;
        if (kKind == M_TSS) {
            ri = tss_match_both(a, ok, is6, k0, k1, k.s, k.d, act, nullptr);
        } else if (kKind == M_TREE) {
            ri = tree_match<false>(a, ok, is6, k0, k1, k.s, k.d, act, nullptr, nullptr, nullptr);
        } else if (kKind == M_FAM) {
            ri = need_v6 ? scan_fam<true>(a, !ok, is6, k0, k1, k.s, k.d, act, nullptr)
                         : scan_fam<false>(a, !ok, is6, k0, k1, k.s, k.d, act, nullptr);
        } else if (kKind == M_WHOLE) {
            ri = need_v6 ? scan_rules<true, false>(a, !ok, is6, k0, k1, k.s, k.d, act, s_rv4, s_rv6, 0u, a.nrules_pad)
                         : scan_rules<false, false>(a, !ok, is6, k0, k1, k.s, k.d, act, s_rv4, s_rv6, 0u, a.nrules_pad);
        } else {
            ri = need_v6 ? scan_rules<true, true>(a, !ok, is6, k0, k1, k.s, k.d, act, s_rv4, s_rv6, 0u, a.nrules_pad)
                         : scan_rules<false, true>(a, !ok, is6, k0, k1, k.s, k.d, act, s_rv4, s_rv6, 0u, a.nrules_pad);
        }
        // the family lists' and the tree's answer is an entry of the lists' index array
        if ((kKind == M_FAM || kKind == M_TREE) && ri != kNone) ri = fam_sorted_index(a, ri, act);
        if (i < a.n) a.rule[i] = ok && ri != kNone ? (int32_t)ri : -1;
    }
}

using namespace upe;

// The matcher upe_classify runs for the table (plan_lds, upe_plan.h: tuple space first, then the
// small table, the tree, the whole-table scan where a family's list is a single catch-all, else
// the family lists).
MatchKind match_kind(const DeviceTable& t) {
    return t.tss ? M_TSS
         : t.nrules_pad <= (uint32_t)kSmallRules ? M_SMALL
         : t.tree_ok ? M_TREE : t.fam_all ? M_WHOLE : M_FAM;
}

// (key_grid: upe_key_tile.h)
uint32_t keys_grid(const upe_gpu_ctx_t* c, size_t n) { return key_grid(c->cus, c->grid_cap, n); }

int keys_check(const upe_gpu_ctx_t* c, size_t n) {
    if (!c) return fail("null context");
    if (n > kMaxKeys) return fail("n must fit in 32 bits");
    return 0;
}

// Queue upe_match_keys over keys [0, n), n > 0, against `t` on `s`.
hipError_t match_launch(const DeviceTable& t, const upe_flow_key_t* d_keys, size_t n,
                        int32_t* d_rule, uint32_t grid, hipStream_t s) {
    MatchArgs a{};
    a.keys = reinterpret_cast<const uint32_t*>(d_keys);
    a.rule = d_rule;
    a.n = (uint32_t)n;
    a.rv4 = t.rv4;
    a.rv6 = t.rv6;
    a.nrules_pad = t.nrules_pad;
    a.fam = t.fam;
    a.fam4 = t.fam4;
    a.fam6 = t.fam6;
    a.fam_x1idx = t.fam_x1idx;
    a.tree = reinterpret_cast<const uint2*>(t.tree.p);
    a.tree_loff = t.tree_loff;
    a.tg4 = t.tg4;
    a.tg6 = t.tg6;
    a.tt4 = t.tt4;
    a.tt6 = t.tt6;
    a.ng4 = t.ng4;
    a.ng6 = t.ng6;
    const dim3 g(grid), b(kThreads);
    switch (match_kind(t)) {
    case M_TSS: hipLaunchKernelGGL(upe_match_keys<M_TSS>, g, b, 0, s, a); break;
    case M_TREE: hipLaunchKernelGGL(upe_match_keys<M_TREE>, g, b, 0, s, a); break;
    case M_FAM: hipLaunchKernelGGL(upe_match_keys<M_FAM>, g, b, 0, s, a); break;
    case M_WHOLE: hipLaunchKernelGGL(upe_match_keys<M_WHOLE>, g, b, 0, s, a); break;
    default: hipLaunchKernelGGL(upe_match_keys<M_SMALL>, g, b, 0, s, a); break;
    }
    return hipGetLastError();
}

}  // namespace

extern "C" {

// parse_flow_key (reference src/parser.c:6-111) per packet of a resident batch.
int upe_gpu_parse_keys(upe_gpu_ctx_t* c, const uint8_t* d_frames, const uint64_t* d_desc, size_t n,
                       upe_flow_key_t* d_keys, int32_t* d_rc, void* stream) {
    if (keys_check(c, n) != 0) return -1;
    if (n == 0) return 0;
    if (!d_frames || !d_desc || !d_keys) return fail("null buffer");
    if (((uintptr_t)d_frames & 15u) != 0) return fail("frames buffer must be 16-byte aligned");
    if (((uintptr_t)d_keys & 3u) != 0 || ((uintptr_t)d_rc & 3u) != 0)
        return fail("keys and rc must be 4-byte aligned");
    DEV_SCOPE(c->device);
    hipLaunchKernelGGL(upe_parse_keys, dim3(keys_grid(c, n)), dim3(kThreads), 0, pick(c, stream),
                       d_frames, d_desc, (uint32_t)n, reinterpret_cast<uint32_t*>(d_keys), d_rc);
    HIP_TRY(hipGetLastError());
    return 0;
}

// rule_table_match (reference src/rule_table.c:163-176) per key, against the loaded table or,
// with an image, against that table uploaded beside the loaded one for the call.
int upe_gpu_match_keys(upe_gpu_ctx_t* c, const upe_rule_image_t* image,
                       const upe_flow_key_t* d_keys, size_t n, int32_t* d_rule, void* stream) {
    if (keys_check(c, n) != 0) return -1;
    if (n == 0) return 0;
    if (!d_keys || !d_rule) return fail("null buffer");
    if (((uintptr_t)d_keys & 3u) != 0 || ((uintptr_t)d_rule & 3u) != 0)
        return fail("keys and rule must be 4-byte aligned");
    if (!image && c->table.nrules == 0) return fail("no rule table loaded");
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    if (!image) {
        HIP_TRY(match_launch(c->table, d_keys, n, d_rule, keys_grid(c, n), s));
        return 0;
    }
    // the dry run: a second DeviceTable value, uploaded as a reload uploads it (install_image,
    // upe_gpu.hip) and dropped, not swapped in; freed once the launch that reads it has finished
    DeviceTable dry;
    if (dry.upload(*image) != 0) return -1;
    HIP_TRY(match_launch(dry, d_keys, n, d_rule, keys_grid(c, n), s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
