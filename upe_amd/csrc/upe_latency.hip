// upe_latency.hip — the worker's per-packet latency histogram on the device
// (upe_gpu_latency_record, include/upe_gpu.h): what process_packet does at each of its exits
// (reference src/worker.c:120-122 ... 249-251: latency_record(&w->latency_hist,
// rdtsc() - b->timestamp, g_cycles_per_ns) when b->timestamp > 0; src/latency.c:41-59) for a whole
// batch whose timestamps and verdicts are resident in GPU memory, with one `now` for the batch.
//
// One launch.  A workgroup of 256 threads walks the batch in passes of kBlock packets, a stride of
// the grid apart; in a pass a lane takes kPer packets kThreads apart, so every load instruction of
// a wave reads 64 consecutive timestamps (512 bytes) or verdicts (256 bytes), and a lane's kPer
// loads are issued before the first is used.  Each lane keeps its own tallies in registers:
//   below[j]   samples with ns < bound j, j = 0..6 (cumulative: the bounds ascend, so bucket j's
//              count is below[j] - below[j - 1], and the last bucket's is cnt - below[6]; no
//              register is indexed by a run-time value)
//   cnt, sum (modulo 2^64), mn, mx
// They are reduced across the wave with shuffles (64-bit values as two 32-bit halves), across the
// workgroup's waves through LDS, and a workgroup that sampled anything then issues at most 12
// 64-bit global atomics (adds, one min, one max) on the context's histogram.  Adds, min and max of
// integers commute, so the result does not depend on the order of lanes, waves or workgroups.
// The histogram is kept as 64 copies a line apart, a workgroup's atomics going to copy
// blockIdx % 64 (UPE_LATENCY_REPLICAS, upe_ctx.h): with all of a 1M-packet launch's 1024
// workgroups on one line the launch took 56 us, about 50 ns per workgroup queued behind the others.
//
// The sample's arithmetic is IEEE-754 double, each step rounded once: the conversion of the
// 64-bit cycle count (its halves are exact doubles, the high one scaled by 2^32 exactly, their sum
// rounded to nearest even — as one fused multiply-add or as a product and a sum), one division
// (correctly rounded: no reciprocal, no fast-math), truncation.  A quotient of 2^64 or more
// saturates; the conversion is given a value in range in every case.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cfloat>
#include <vector>

#include "upe_ctx.h"

namespace {

constexpr uint32_t kBlock = UPE_LATENCY_BLOCK;   // packets per workgroup pass
constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kPer = kBlock / kThreads;     // packets per thread and pass
constexpr uint32_t kCum = UPE_LATENCY_BUCKETS - 1;
constexpr uint32_t kWords = UPE_LATENCY_BUCKETS + 4;   // of a upe_latency_hist_t
constexpr double kTwo32 = 4294967296.0, kTwo64 = 18446744073709551616.0;
static_assert(kBlock % kThreads == 0, "pass shape");
static_assert(sizeof(upe_latency_hist_t) == kWords * sizeof(unsigned long long), "histogram words");
static_assert(kWords <= UPE_LATENCY_REPLICA_WORDS, "a replica holds a histogram");

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t x, int d) {
    const uint32_t lo = __shfl_xor((uint32_t)x, d);
    const uint32_t hi = __shfl_xor((uint32_t)(x >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t to_ns(uint64_t cycles, double cpn) {
    const double c = (double)(uint32_t)(cycles >> 32) * kTwo32 + (double)(uint32_t)cycles;
    const double q = c / cpn;   // >= 0, or +inf
    const bool over = !(q < kTwo64);
    const uint64_t t = (uint64_t)(over ? 0.0 : q);
    return over ? ~0ull : t;
}

__global__ void __launch_bounds__(kThreads) upe_latency_record(
    const uint64_t* __restrict__ timestamp, const uint32_t* __restrict__ verdict, uint32_t n,
    uint64_t now, double cpn, unsigned long long* hist_all) {
    constexpr uint64_t kBounds[UPE_LATENCY_BUCKETS] = {UPE_LATENCY_BOUNDS};
    __shared__ uint32_t s_c[kWaves][kCum + 1];   // below[0..6], cnt
    __shared__ uint64_t s_q[kWaves][3];          // sum, min, max
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    uint32_t below[kCum] = {}, cnt = 0;          // a lane sees fewer than 2^32 packets
    uint64_t sum = 0, mn = ~0ull, mx = 0;
    const uint32_t tiles = (n + kBlock - 1u) / kBlock;   // n <= 2^32 - 1 - kBlock
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t p0 = t * kBlock;
        uint64_t ts[kPer];
        uint32_t v[kPer];
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t i = p0 + k * kThreads + tid;   // < n + kBlock: no wrap
            const bool in = i < n;
            ts[k] = in ? timestamp[i] : 0ull;
            v[k] = in && verdict ? verdict[i] : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const bool take = ts[k] != 0ull && UPE_VERDICT_CODE(v[k]) != (uint32_t)UPE_V_CONSUMED;
            const uint64_t ns = to_ns(now - ts[k], cpn);
            const uint32_t one = take ? 1u : 0u;
#pragma unroll
            for (uint32_t j = 0; j < kCum; ++j) below[j] += ns < kBounds[j] ? one : 0u;
            cnt += one;
            sum += take ? ns : 0ull;
            mn = take && ns < mn ? ns : mn;
            mx = take && ns > mx ? ns : mx;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
        for (uint32_t j = 0; j < kCum; ++j) below[j] += __shfl_xor(below[j], d);
        cnt += __shfl_xor(cnt, d);
        sum += shfl_xor64(sum, d);
        const uint64_t a = shfl_xor64(mn, d), b = shfl_xor64(mx, d);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t j = 0; j < kCum; ++j) s_c[wave][j] = below[j];
        s_c[wave][kCum] = cnt;
        s_q[wave][0] = sum;
        s_q[wave][1] = mn;
        s_q[wave][2] = mx;
    }
    __syncthreads();
    if (tid >= kWords) return;
    // thread j < 8: bucket j; 8: total_count; 9: min_ns; 10: max_ns; 11: sum_ns
    uint64_t total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) total += s_c[w][kCum];
    if (total == 0) return;
    unsigned long long* hist =
        hist_all + (blockIdx.x % UPE_LATENCY_REPLICAS) * UPE_LATENCY_REPLICA_WORDS;
    if (tid <= UPE_LATENCY_BUCKETS) {
        // samples below bound tid (all of them for the last bucket and the total) less those
        // below the bound before it
        uint64_t hi = 0, lo = 0;
        for (uint32_t w = 0; w < kWaves; ++w) {
            hi += s_c[w][tid < kCum ? tid : kCum];
            lo += tid > 0 && tid < UPE_LATENCY_BUCKETS ? s_c[w][tid - 1u] : 0u;
        }
        if (hi - lo) atomicAdd(&hist[tid], (unsigned long long)(hi - lo));
    } else if (tid == UPE_LATENCY_BUCKETS + 1u) {
        uint64_t m = ~0ull;
        for (uint32_t w = 0; w < kWaves; ++w) m = s_q[w][1] < m ? s_q[w][1] : m;
        atomicMin(&hist[tid], (unsigned long long)m);
    } else if (tid == UPE_LATENCY_BUCKETS + 2u) {
        uint64_t m = 0;
        for (uint32_t w = 0; w < kWaves; ++w) m = s_q[w][2] > m ? s_q[w][2] : m;
        atomicMax(&hist[tid], (unsigned long long)m);
    } else {
        uint64_t m = 0;
        for (uint32_t w = 0; w < kWaves; ++w) m += s_q[w][0];
        if (m) atomicAdd(&hist[tid], (unsigned long long)m);
    }
}

// Queue the launch on `s`: the samples of packets [0, n) added to hist (the replicas, in device
// memory, 128-byte aligned), with the arguments as latency_check has checked them; at most
// max_grid > 0 workgroups, each walking the batch in strides of the grid.
hipError_t upe_latency_launch(const uint64_t* timestamp, const uint32_t* verdict, uint32_t n,
                              uint64_t now, double cycles_per_ns, unsigned long long* hist,
                              uint32_t max_grid, hipStream_t s) {
    const uint32_t tiles = (n + kBlock - 1u) / kBlock;
    const uint32_t grid = tiles < max_grid ? tiles : max_grid;
    hipLaunchKernelGGL(upe_latency_record, dim3(grid), dim3(kThreads), 0, s, timestamp, verdict, n,
                       now, cycles_per_ns, hist);
    return hipGetLastError();
}

using namespace upe;

constexpr size_t kLatWords = (size_t)UPE_LATENCY_REPLICAS * UPE_LATENCY_REPLICA_WORDS;

int latency_check(upe_gpu_ctx_t* c, const uint64_t* d_timestamp, size_t n) {
    if (!c) return fail("null context");
    if (n && !d_timestamp) return fail("null buffer");
    if (n > 0xFFFFFFFFull - UPE_LATENCY_BLOCK) return fail("n must fit in 32 bits");
    if (!(c->cycles_per_ns > 0.0))
        return fail("no calibration: upe_gpu_set_tsc has not succeeded on this context");
    return 0;
}

// at most four workgroups per CU, each striding over the batch; UPE_GPU_GRID_CAP lowers it
uint32_t latency_grid(const upe_gpu_ctx_t* c) {
    const uint32_t g = 4u * (uint32_t)c->cus;
    return c->grid_cap && c->grid_cap < g ? c->grid_cap : g;
}

}  // namespace

int upe::latency_init_image(std::vector<unsigned long long>& img) {
    upe_latency_hist_t h;
    upe_latency_init(&h);
    img.assign(kLatWords, 0);
    for (size_t r = 0; r < UPE_LATENCY_REPLICAS; ++r)
        memcpy(&img[r * UPE_LATENCY_REPLICA_WORDS], &h, sizeof h);
    return 0;
}

extern "C" {

// The worker's latency histogram (reference src/worker.c:120-122 ... 249-251 per packet,
// src/latency.c:41-59).
int upe_gpu_set_tsc(upe_gpu_ctx_t* c, double cycles_per_ns) {
    if (!c) return fail("null context");
    if (!(cycles_per_ns > 0.0 && cycles_per_ns <= DBL_MAX))
        return fail("cycles_per_ns must be finite and > 0");
    c->cycles_per_ns = cycles_per_ns;
    return 0;
}

int upe_gpu_latency_record(upe_gpu_ctx_t* c, const uint64_t* d_timestamp,
                           const uint32_t* d_verdict, size_t n, uint64_t now, void* stream) {
    if (latency_check(c, d_timestamp, n) != 0) return -1;
    if (n == 0) return 0;
    DEV_SCOPE(c->device);
    HIP_TRY(upe_latency_launch(d_timestamp, d_verdict, (uint32_t)n, now, c->cycles_per_ns,
                               c->lat_hist.p, latency_grid(c), pick(c, stream)));
    return 0;
}

// Diagnostic (tools/latency_time.py; not in the header): one upe_gpu_latency_record of n > 0
// packets between two HIP events, then a plain hipMemcpyAsync of copy_bytes (device to device) on
// the same stream between two more: the yardstick for the bytes the call reads.  ms[0] = the
// launch, ms[1] = the copy.  Synchronous.
int upe_gpu_latency_record_timed(upe_gpu_ctx_t* c, const uint64_t* d_timestamp,
                                 const uint32_t* d_verdict, size_t n, uint64_t now,
                                 const uint8_t* copy_src, uint8_t* copy_dst, size_t copy_bytes,
                                 void* stream, float* ms) {
    if (!ms || !copy_src || !copy_dst || n == 0) return fail("no output or an empty batch");
    if (latency_check(c, d_timestamp, n) != 0) return -1;
    DEV_SCOPE(c->device);
    hipStream_t s = pick(c, stream);
    Events<4> ev;
    if (ev.create() != 0) return -1;
    HIP_TRY(hipEventRecord(ev.e[0], s));
    HIP_TRY(upe_latency_launch(d_timestamp, d_verdict, (uint32_t)n, now, c->cycles_per_ns,
                               c->lat_hist.p, latency_grid(c), s));
    HIP_TRY(hipEventRecord(ev.e[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    return ev.yardstick(copy_dst, copy_src, copy_bytes, hipMemcpyDeviceToDevice, s,
                        "the yardstick copy", ms);
}

int upe_gpu_get_latency(upe_gpu_ctx_t* c, upe_latency_hist_t* out) {
    if (!c || !out) return fail("null argument");
    DEV_SCOPE(c->device);
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> img(kLatWords);
    HIP_TRY(hipMemcpy(img.data(), c->lat_hist.p, kLatWords * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost));
    upe_latency_init(out);
    for (size_t r = 0; r < UPE_LATENCY_REPLICAS; ++r) {
        upe_latency_hist_t h;
        memcpy(&h, &img[r * UPE_LATENCY_REPLICA_WORDS], sizeof h);
        upe_latency_merge(out, &h);
    }
    return 0;
}

int upe_gpu_reset_latency(upe_gpu_ctx_t* c) {
    if (!c) return fail("null context");
    DEV_SCOPE(c->device);
    HIP_TRY(hipDeviceSynchronize());   // launches on any stream have added what they add
    std::vector<unsigned long long> img;
    latency_init_image(img);
    HIP_TRY(hipMemcpy(c->lat_hist.p, img.data(), kLatWords * sizeof(unsigned long long),
                      hipMemcpyHostToDevice));
    return 0;
}

}  // extern "C"
