/*
 * upe_egress.h — glue between upe_gpu.hip (the context, the C ABI) and upe_egress.hip (the pack
 * kernels of upe_gpu_egress_pack).  Not part of the ABI.
 */
#ifndef UPE_EGRESS_H
#define UPE_EGRESS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/upe_gpu.h"

/* Bytes of scratch one pack of n packets needs (n > 0). */
__attribute__((visibility("hidden"))) size_t upe_egress_scratch_bytes(uint32_t n);

/* Queue the three passes on `s`.  Arguments are checked by the caller: n > 0, out 16-byte aligned
 * and apart from frames, scratch of upe_egress_scratch_bytes(n) bytes (8-byte aligned).  hdr NULL:
 * the frames are copied; else each forwarded frame gets its record.  ev: NULL, or four events
 * recorded before the size pass and after each pass (tools/egress_pack_time.py). */
__attribute__((visibility("hidden"))) hipError_t
upe_egress_launch(const uint8_t* frames, const uint64_t* desc, const uint32_t* verdict,
                  const upe_hdr_rec_t* hdr, uint32_t n, uint8_t* out, uint64_t out_bytes,
                  uint64_t* out_desc, uint32_t* out_index, upe_egress_info_t* info, void* scratch,
                  hipStream_t s, hipEvent_t* ev);

#endif /* UPE_EGRESS_H */
