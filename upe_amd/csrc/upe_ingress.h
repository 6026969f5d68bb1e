/*
 * upe_ingress.h — glue between upe_gpu.hip (the context, the C ABI) and upe_ingress.hip (the
 * gather kernels of upe_gpu_ingress_gather).  Not part of the ABI.
 */
#ifndef UPE_INGRESS_H
#define UPE_INGRESS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/upe_gpu.h"

/* Bytes of scratch one gather of n packets needs (n > 0). */
__attribute__((visibility("hidden"))) size_t upe_ingress_scratch_bytes(uint32_t n);

/* Queue the passes on `s`.  Arguments are checked by the caller: n > 0, a known mode, pool 16-byte
 * aligned and loadable by the device, stride and pool_bytes within the header's rules, out 16-byte
 * aligned, apart from the pool and (WINDOW) of at least n * UPE_HDR_WINDOW bytes, scratch of
 * upe_ingress_scratch_bytes(n) bytes (8-byte aligned).  ev: NULL, or four events recorded before
 * the size pass and after each pass (tools/ingress_gather_time.py); a pass that a mode does not
 * launch leaves its pair of events back to back. */
__attribute__((visibility("hidden"))) hipError_t
upe_ingress_launch(const uint8_t* pool, uint64_t pool_bytes, uint64_t stride, const uint32_t* slot,
                   uint32_t n, int mode, uint8_t* out, uint64_t out_bytes, uint64_t* desc,
                   uint64_t* timestamp, uint32_t* ctrl, upe_ingress_info_t* info, void* scratch,
                   hipStream_t s, hipEvent_t* ev);

#endif /* UPE_INGRESS_H */
