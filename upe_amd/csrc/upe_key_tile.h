// upe_key_tile.h — a tile of flow keys between a caller's array and LDS, for the units whose
// kernels take or leave upe_flow_key_t records one per lane: upe_keys.hip (upe_parse_keys,
// upe_match_keys) and upe_neigh.hip (upe_resolve_keys).  Device code only; internal linkage (an
// unnamed namespace, as upe_match.h).
//
// Keys are 44-byte records (upe_flow_key_t, 11 words), so a lane's record is neither 16-byte
// aligned nor a multiple of 16 bytes, and 64 lanes each moving their own words put 64 x 4 bytes
// 44 bytes apart with every memory instruction (eleven of them, each touching the wave's 22
// lines).  A tile's 256 records go through LDS instead: a lane writes (reads) its record's words at
// word 11 * lane + j (an odd stride: 64 lanes on 64 different banks), and the workgroup stores
// (loads) the tile's 2816 words row by row, 256 consecutive words per instruction — every wave
// instruction moves 256 contiguous bytes, whatever the alignment of the caller's array, and a
// ragged last tile is a bound on the word index.
#ifndef UPE_KEY_TILE_H
#define UPE_KEY_TILE_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/upe_gpu.h"

namespace {

constexpr uint32_t kThreads = 256;   // keys per tile
constexpr uint32_t kKeyWords = 11;   // of a upe_flow_key_t
static_assert(sizeof(upe_flow_key_t) == kKeyWords * sizeof(uint32_t), "flow key words");
static_assert(offsetof(upe_flow_key_t, src_ip) == 4 && offsetof(upe_flow_key_t, dst_ip) == 20 &&
                  offsetof(upe_flow_key_t, src_port) == 36 &&
                  offsetof(upe_flow_key_t, dst_port) == 38 &&
                  offsetof(upe_flow_key_t, protocol) == 40,
              "flow key layout");
// n + kThreads must not wrap (a tile's last lane index), and a tile index times kThreads neither
constexpr size_t kMaxKeys = 0xFFFFFFFFull - kThreads;

// A tile's records between LDS and the caller's array (see the top of the file).  base: the
// tile's first word in the array; words: the array's.
__device__ __forceinline__ void tile_store(uint32_t* g, const uint32_t* lds, size_t base,
                                           size_t words, uint32_t tid) {
#pragma unroll
    for (uint32_t j = 0; j < kKeyWords; ++j) {
        const uint32_t k = j * kThreads + tid;   // < kKeyWords * kThreads
        if (base + k < words) g[base + k] = lds[k];
    }
}
__device__ __forceinline__ void tile_load(uint32_t* lds, const uint32_t* g, size_t base,
                                          size_t words, uint32_t tid) {
#pragma unroll
    for (uint32_t j = 0; j < kKeyWords; ++j) {
        const uint32_t k = j * kThreads + tid;
        lds[k] = base + k < words ? g[base + k] : 0u;
    }
}

// The grid of a kernel that walks n keys' tiles: at most eight workgroups (32 waves) per CU, each
// striding over the tiles; a context's UPE_GPU_GRID_CAP (0: none) lowers it.
inline uint32_t key_grid(int cus, uint32_t grid_cap, size_t n) {
    const uint32_t tiles = (uint32_t)((n + kThreads - 1) / kThreads);
    uint32_t g = 8u * (uint32_t)cus;
    if (grid_cap && grid_cap < g) g = grid_cap;
    return tiles < g ? tiles : g;
}

}  // namespace

#endif  // UPE_KEY_TILE_H
