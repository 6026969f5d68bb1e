/*
 * upe_rx.h — glue between upe_gpu.hip (the context, the C ABI) and upe_rx.hip (the RX dispatch
 * kernels of upe_gpu_rx_dispatch).  Not part of the ABI.
 */
#ifndef UPE_RX_H
#define UPE_RX_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

/* Bytes of scratch one dispatch of n packets over `rings` rings needs (n > 0). */
__attribute__((visibility("hidden"))) size_t upe_rx_scratch_bytes(uint32_t n, uint32_t rings);

/* Queue the three passes on `s`.  Arguments are checked by the caller: n > 0, rings a power of
 * two <= UPE_RX_RINGS_MAX, rr < rings, scratch of upe_rx_scratch_bytes(n, rings) bytes.  ev: NULL,
 * or four events recorded before the hash pass and after each pass (tools/rx_dispatch_time.py). */
__attribute__((visibility("hidden"))) hipError_t
upe_rx_launch(const uint8_t* frames, const uint64_t* desc, uint32_t n, uint32_t rings, uint32_t rr,
              uint32_t* ring, uint32_t* flow_hash, uint32_t* index, uint64_t* desc_out,
              uint64_t* counts, uint32_t* scratch, hipStream_t s, hipEvent_t* ev);

#endif /* UPE_RX_H */
