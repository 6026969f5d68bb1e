// upe_neigh.hip — next hops on the device, apart from the classify launch (upe_gpu_resolve_keys,
// include/upe_gpu.h): the third table function process_packet calls, arp_get_mac (reference
// src/arp_table.c:55-80) / ndp_get_mac (src/ndp_table.c:67-86), over an array of flow keys, against
// the context's loaded snapshot or against a compiled image that is not loaded (a dry run before
// upe_gpu_load_neigh_image).
//
// The kernel: one key per lane, workgroups of 256 threads walking 256-key tiles a grid apart, no
// state between keys, no atomics; it touches nothing of the context's but the neighbour snapshot.
// A tile's 44-byte records come in through LDS (upe_key_tile.h, upe_keys.hip's mover); a lane then
// reads the five words it needs of its record (0: ip_ver, 5-8: dst_ip) at the odd stride, and
// stores its answer as one 8-byte word, a wave's 512 contiguous bytes.
//
// The lookup is the classify kernels' own (neigh_lookup, upe_neigh_lookup.h), reading the index
// from memory: both families' lanes of a wave issue their three slot loads together.  The index is
// not staged in LDS as upe_classify stages it: that would be up to 96 KB copied per workgroup for
// 256 keys at a time, where upe_classify's workgroups stage it once for thousands of packets
// (upe_match_keys reads its tree and lists from memory for the same reason).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "upe_ctx.h"
#include "upe_key_tile.h"
#include "upe_neigh_lookup.h"

namespace {

struct ResolveArgs {
    const uint32_t* keys;
    unsigned long long* mac;
    uint32_t n;
    NeighIndex arp, ndp;
};

__global__ void __launch_bounds__(kThreads) upe_resolve_keys(ResolveArgs a) {
    __shared__ uint32_t s_key[kKeyWords * kThreads];
    const uint32_t tid = threadIdx.x;
    const uint32_t tiles = (a.n + kThreads - 1u) / kThreads;   // n <= kMaxKeys
    const size_t words = (size_t)a.n * kKeyWords;
    // every thread of the workgroup runs every pass (the barriers); lanes past n carry a zero
    // record (tile_load), whose ip_ver asks for nothing
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t i = t * kThreads + tid;   // < n + kThreads: no wrap
        tile_load(s_key, a.keys, (size_t)t * (kKeyWords * kThreads), words, tid);
        __syncthreads();
        const uint32_t ver = s_key[kKeyWords * tid] & 0xFFu;
        uint32_t d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = s_key[kKeyWords * tid + 5 + j];
        __syncthreads();   // the next tile's records overwrite s_key
        const bool v6 = ver == 6u;
        // (of an IPv4 key, neigh_lookup reads d[0] alone: union bytes 4-15 never count)
        uint32_t lo = 0, hi = 0;
        const bool hit = (v6 || ver == 4u) && neigh_lookup(a.arp, a.ndp, v6, d, lo, hi);
        if (i < a.n)
            a.mac[i] = hit ? (unsigned long long)lo | (unsigned long long)(hi | 1u << 16) << 32
                           : 0ull;
    }
}

using namespace upe;

// Queue upe_resolve_keys over keys [0, n), n > 0, against `t` on `s`.
hipError_t resolve_launch(const upe_gpu_ctx_t* c, const NeighTable& t, const upe_flow_key_t* d_keys,
                          size_t n, uint64_t* d_mac, hipStream_t s) {
    const uint32_t grid = key_grid(c->cus, c->grid_cap, n);
    ResolveArgs a{};
    a.keys = reinterpret_cast<const uint32_t*>(d_keys);
    a.mac = reinterpret_cast<unsigned long long*>(d_mac);
    a.n = (uint32_t)n;
    a.arp = NeighIndex{t.arp, t.arp_bits, t.arp_seed};
    a.ndp = NeighIndex{t.ndp, t.ndp_bits, t.ndp_seed};
    hipLaunchKernelGGL(upe_resolve_keys, dim3(grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace

extern "C" {

// arp_get_mac / ndp_get_mac per key, against the loaded snapshot or, with an image, against that
// snapshot uploaded beside the loaded one for the call.
int upe_gpu_resolve_keys(upe_gpu_ctx_t* c, const upe_neigh_image_t* image,
                         const upe_flow_key_t* d_keys, size_t n, uint64_t* d_mac, void* stream) {
    if (!c) return fail("null context");
    if (n > kMaxKeys) return fail("n must fit in 32 bits");
    if (n == 0) return 0;
    if (!d_keys || !d_mac) return fail("null buffer");
    if (((uintptr_t)d_keys & 3u) != 0 || ((uintptr_t)d_mac & 7u) != 0)
        return fail("keys must be 4-byte and mac 8-byte aligned");
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    if (!image) {
        HIP_TRY(resolve_launch(c, c->neigh, d_keys, n, d_mac, s));
        return 0;
    }
    // the dry run: a second NeighTable value, uploaded as a load uploads it
    // (upe_gpu_load_neigh_image, upe_gpu.hip) and dropped, not swapped in; freed once the launch
    // that reads it has finished
    NeighTable dry;
    if (dry.upload(image->im) != 0) return -1;
    HIP_TRY(resolve_launch(c, dry, d_keys, n, d_mac, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
