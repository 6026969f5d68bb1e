// upe_scan.h — what the ordered-output stages share on the device: upe_rx.hip, upe_egress.hip,
// upe_ingress.hip, upe_ctrl.hip, upe_neigh_patch.hip and upe_release.hip each mark per tile, scan
// the tiles in one workgroup and write behind the prefix.  The wave-level primitives and the scan
// workgroup's step are defined here once; upe_neigh_learn.hip's one workgroup uses the step too.  HIP units only; internal linkage (an unnamed namespace,
// as upe_match.h and upe_neigh_lookup.h), so each unit compiles its own copies into its kernels.
#ifndef UPE_SCAN_H
#define UPE_SCAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t y = __shfl_xor(x, d);
        x = y < x ? y : x;
    }
    return x;
}

// Exclusive prefix of x over the wave's lanes, and the wave's total.
template <typename T>
__device__ __forceinline__ T wave_excl(T x, int lane, T& total) {
    T s = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(s, d);
        if (lane >= d) s += y;
    }
    total = __shfl(s, 63);
    return s - x;
}

// The word holding bytes first .. first + 3 of a frame or of a quad, with the bytes at or past
// len zeroed.
__device__ __forceinline__ uint32_t keep(uint32_t w, uint32_t len, uint32_t first) {
    if (len >= first + 4u) return w;
    if (len <= first) return 0u;
    return w & ((1u << (8u * (len - first))) - 1u);
}

// The waves' totals of a step, as block_excl's second barrier leaves them in s_w: those of the
// waves before this one go onto ex, all of them into `all`.
template <uint32_t kWaves, typename T>
__device__ __forceinline__ void add_waves(const T (&s_w)[kWaves], uint32_t wave, T& ex, T& all) {
    all = 0;
#pragma unroll
    for (uint32_t j = 0; j < kWaves; ++j) {
        const T y = s_w[j];
        if (j < wave) ex += y;
        all += y;
    }
}

// One step of a scan by a workgroup of kWaves whole waves, one value per thread (lane, wave: the
// thread's): returns the sum of x over the threads before this one and leaves the step's sum in
// `all`.  Every thread of the workgroup calls it, the same number of times.  Both barriers are
// inside — the first lets the readers of the call before finish with s_w (and orders whatever
// the kernel wrote to shared memory before its first call), the second publishes this call's wave
// totals — so the next call may reuse s_w without another barrier, and a caller that carries a
// running sum over steps adds `all` to it after each.
template <uint32_t kWaves, typename T>
__device__ __forceinline__ T block_excl(T x, int lane, uint32_t wave, T (&s_w)[kWaves], T& all) {
    T w;
    T ex = wave_excl(x, lane, w);
    __syncthreads();
    if (lane == 0) s_w[wave] = w;
    __syncthreads();
    add_waves(s_w, wave, ex, all);
    return ex;
}

// The same step for two values at once behind one pair of barriers (the packets and the 64-bit
// quads of upe_egress.hip): a and b become their exclusive prefixes.  upe_ingress_scan keeps the
// step written out, for its registers' sake (the comment there).
template <uint32_t kWaves, typename A, typename B>
__device__ __forceinline__ void block_excl(A& a, B& b, int lane, uint32_t wave, A (&s_a)[kWaves],
                                           B (&s_b)[kWaves], A& all_a, B& all_b) {
    A wa;
    B wb;
    a = wave_excl(a, lane, wa);
    b = wave_excl(b, lane, wb);
    __syncthreads();
    if (lane == 0) {
        s_a[wave] = wa;
        s_b[wave] = wb;
    }
    __syncthreads();
    add_waves(s_a, wave, a, all_a);
    add_waves(s_b, wave, b, all_b);
}

}  // namespace

#endif  // UPE_SCAN_H
