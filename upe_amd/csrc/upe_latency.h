/*
 * upe_latency.h — glue between upe_gpu.hip (the context, the C ABI) and upe_latency.hip (the
 * kernel of upe_gpu_latency_record).  Not part of the ABI.
 */
#ifndef UPE_LATENCY_H
#define UPE_LATENCY_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/upe_gpu.h"

/* The histogram on the device: UPE_LATENCY_REPLICAS copies of a upe_latency_hist_t,
 * UPE_LATENCY_REPLICA_WORDS 64-bit words (one 128-byte line) apart, each in the upe_latency_init
 * state when empty; their upe_latency_merge is the histogram.  A workgroup adds to the copy
 * blockIdx % UPE_LATENCY_REPLICAS, which keeps a launch's atomics from queueing on one line. */
#define UPE_LATENCY_REPLICAS 64
#define UPE_LATENCY_REPLICA_WORDS 16

/* Queue the launch on `s`: the samples of packets [0, n) added to hist (the replicas above, in
 * device memory, 128-byte aligned).  Arguments are checked by the caller: n > 0 and at most
 * 2^32 - 1 - UPE_LATENCY_BLOCK, timestamp of n entries, verdict NULL or of n entries,
 * cycles_per_ns finite and > 0, max_grid > 0 (the most workgroups; each walks the batch in
 * strides of the grid). */
__attribute__((visibility("hidden"))) hipError_t
upe_latency_launch(const uint64_t* timestamp, const uint32_t* verdict, uint32_t n, uint64_t now,
                   double cycles_per_ns, unsigned long long* hist, uint32_t max_grid,
                   hipStream_t s);

#endif /* UPE_LATENCY_H */
