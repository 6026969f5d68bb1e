// upe_parse.h — parse_flow_key on the device (reference src/parser.c:6-111) over a frame's header
// window in registers: all of it for upe_keys.hip (upe_parse_keys), the byte helpers and the
// L4-word selection for general_path in upe_gpu.hip (its L4 gate and upe_rx.hip's rx_parse keep
// their own text and say why).  Device code only; internal linkage (an unnamed namespace, as
// upe_match.h), so each unit compiles its own copies into its own kernels.
//
// The window, w, is the frame's first 96 bytes as 24 little-endian dwords: every byte the parser
// reads (an IPv4 header of 60 bytes puts the TCP data-offset byte at 14 + 60 + 12 = 86).  How a
// unit loads it, and whether it clears the bytes at or past len, is the unit's business: a gate
// that succeeds has checked that the bytes it goes on to use lie below len.
// upe_classify's fast path (upe_gpu.hip) is fused with the rewrite and specialises these gates.
#ifndef UPE_PARSE_H
#define UPE_PARSE_H

#include "upe_match.h"   // vsel, and through it upe_dev.h

namespace {

using namespace upe;

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int k) { return (w >> (8 * k)) & 0xFFu; }
__device__ __forceinline__ uint32_t at2(uint32_t hi, uint32_t lo) {   // dword at byte 4q+2
    return __builtin_amdgcn_alignbit(hi, lo, 16);
}
__device__ __forceinline__ uint32_t be16_lo(uint32_t x) {             // BE u16 in bytes 0,1
    return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu);
}
// Mask of the bytes of dword j that lie below len (a zero-filled pktbuf reads 0 past len).
__device__ __forceinline__ uint32_t len_mask(uint32_t len, int j) {
    const uint32_t lo = 4u * (uint32_t)j;
    return len >= lo + 4 ? 0xFFFFFFFFu : len <= lo ? 0u : (1u << (8 * (len - lo))) - 1u;
}

// A flow key in registers: the address unions as little-endian words, IPv4 host order in word 0
// (src/parser.c:40-41), IPv6 the wire bytes.
struct Key {
    uint32_t ver, proto, sport, dport;
    uint32_t s[4], d[4];
};

// An L4 header that starts at byte 2 of window word q (both families put it at 2 mod 4): its
// dwords at bytes 0-3, 4-7 and 12-15, and x0 = w[q] (general_path's IPv4 checksum ends in its
// low half).
struct L4Words {
    uint32_t w0, w1, w3, x0;
};
__device__ __forceinline__ L4Words l4_at(const uint32_t (&w)[24], int q) {
    return L4Words{at2(w[q + 1], w[q]), at2(w[q + 2], w[q + 1]), at2(w[q + 4], w[q + 3]), w[q]};
}

// IPv4: L4 starts at byte 14 + 4 * ihl = 4 * (ihl + 3) + 2, and registers are not indexable, so
// the words are selected by IHL.  ihl < 5 has failed the parse before; it yields zeros (chain) or
// is not defined (barrel).
template <bool kBarrel>
__device__ __forceinline__ L4Words l4_select(const uint32_t (&w)[24], uint32_t ihl) {
    if constexpr (kBarrel) {
        // a four-stage barrel shift by ihl - 5 (31 selects; only shifts 0..10 matter).
        // Tuple-space kernels only: in the scan kernels it measured slower for config B, whose
        // waves never run this path (24.5 -> 26.7 us, an allocation effect;
        // profiles/r04/v4_wave_general_ab.txt)
        const uint32_t sh = ihl - 5u;
        const uint32_t m8 = (uint32_t)((int32_t)(sh << 28) >> 31);
        const uint32_t m4 = (uint32_t)((int32_t)(sh << 29) >> 31);
        const uint32_t m2 = (uint32_t)((int32_t)(sh << 30) >> 31);
        const uint32_t m1 = (uint32_t)((int32_t)(sh << 31) >> 31);
        uint32_t y[12], z[8], u[6], x[5];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            y[k] = 16 + k < 24 ? vsel(m8, w[16 + k < 24 ? 16 + k : 0], w[8 + k]) : w[8 + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) z[k] = vsel(m4, y[k + 4], y[k]);
#pragma unroll
        for (int k = 0; k < 6; ++k) u[k] = vsel(m2, z[k + 2], z[k]);
#pragma unroll
        for (int k = 0; k < 5; ++k) x[k] = vsel(m1, u[k + 1], u[k]);
        return L4Words{at2(x[1], x[0]), at2(x[2], x[1]), at2(x[4], x[3]), x[0]};
    } else {
        L4Words l{0, 0, 0, 0};
#pragma unroll
        for (int h = 5; h <= 15; ++h)
            if ((int)ihl == h) l = l4_at(w, h + 3);
        return l;
    }
}

// The L4 gate, src/parser.c:70-108: the header's length (TCP: and its data offset), and the ports.
// false: the key is not to be used, and sport / dport may hold anything.
__device__ __forceinline__ bool l4_gate(uint32_t proto, uint32_t l4len, const L4Words& l,
                                        uint32_t& sport, uint32_t& dport) {
    if (proto == 17u) {                                                 // UDP, parser.c:70-78
        sport = be16_lo(l.w0);
        dport = be16_lo(l.w0 >> 16);
        return l4len >= 8u;
    }
    if (proto == 6u) {                                                  // TCP, parser.c:79-94
        const uint32_t thl = (byte_of(l.w3, 0) >> 4) * 4u;
        sport = be16_lo(l.w0);
        dport = be16_lo(l.w0 >> 16);
        return l4len >= 20u && thl >= 20u && l4len >= thl;
    }
    if (proto == 1u) {                                                  // ICMP, parser.c:95-105
        sport = be16_lo(l.w1);                                          // id
        dport = be16_lo(l.w0);                                          // type << 8 | code
        return l4len >= 8u;
    }
    return false;                                                       // parser.c:106-108
}

// parse_flow_key (reference src/parser.c:6-111) over the window.  The gates in the reference's
// order: the Ethernet header, the ethertype, the IP header's length, version and IHL, the
// protocol, the L4 header's length.  false: the key is not to be used.
__device__ __forceinline__ bool parse_key(const uint32_t (&w)[24], uint32_t len, Key& k) {
    k.ver = k.proto = k.sport = k.dport = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) k.s[j] = k.d[j] = 0;
    if (len < 14u) return false;                                        // parser.c:8-10
    const uint32_t et = be16_lo(w[3]);                                  // bytes 12, 13
    const uint32_t iplen = len - 14u;
    L4Words l;
    uint32_t l4len;
    if (et == 0x0800u) {                                                // parser.c:18-44
        const uint32_t vihl = byte_of(w[3], 2), ihl = vihl & 0xFu, hl = ihl * 4u;
        if (iplen < 20u || (vihl >> 4) != 4u || hl < 20u || iplen < hl) return false;
        k.ver = 4;
        k.proto = byte_of(w[5], 3);                                     // byte 23
        k.s[0] = bswap32(at2(w[7], w[6]));                              // bytes 26..29, host order
        k.d[0] = bswap32(at2(w[8], w[7]));                              // bytes 30..33
        l4len = iplen - hl;
        l = l4_select<false>(w, ihl);
    } else if (et == 0x86DDu) {                                         // parser.c:46-64
        if (iplen < 40u) return false;
        k.ver = 6;
        k.proto = byte_of(w[5], 0);                                     // byte 20
        k.s[0] = at2(w[6], w[5]);   k.s[1] = at2(w[7], w[6]);           // bytes 22..37, wire order
        k.s[2] = at2(w[8], w[7]);   k.s[3] = at2(w[9], w[8]);
        k.d[0] = at2(w[10], w[9]);  k.d[1] = at2(w[11], w[10]);         // bytes 38..53
        k.d[2] = at2(w[12], w[11]); k.d[3] = at2(w[13], w[12]);
        l4len = iplen - 40u;
        l = l4_at(w, 13);                                               // L4 at byte 54
    } else {
        return false;                                                   // parser.c:66-68
    }
    return l4_gate(k.proto, l4len, l, k.sport, k.dport);
}

}  // namespace

#endif  // UPE_PARSE_H
