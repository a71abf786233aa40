// fc2_devcrc.h -- the gzip CRC-32 on the device, shared by the BGZF inflater (fc2_inflate.hip: the
// CRC of what it stored) and the DEFLATE compressor (fc2_deflate.hip: the CRC of a tile's input).
// Device code only; every translation unit gets its own copy (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// ---- CRC-32 of the output, as it is stored (gzip's CRC, RFC 1952; zlib's crc32_combine algebra) --
// raw(D) = the CRC register after D from 0 (linear in D); raw(A B) = x^(8|B|) raw(A) + raw(B) mod p,
// and the gzip CRC = raw(D) + x^(8|D|) 0xFFFFFFFF + 0xFFFFFFFF.  The output is stored in rows of
// 1024 bytes, 16 a lane: each lane's raw CRC of its 16 bytes, folded pairwise over the wave (lanes
// l and l + 2^s: x^(8 16 2^s) left + right), is the row's raw CRC, and the running one becomes
// R = x^8192 R + row.  The last, short row is folded in byte by byte.
constexpr uint32_t kPoly = 0xEDB88320u;        // reflected CRC-32 polynomial
__constant__ uint32_t kX2n[32] = {              // x^(2^k) mod p
    0x40000000, 0x20000000, 0x08000000, 0x00800000, 0x00008000, 0xedb88320, 0xb1e6b092, 0xa06a2517,
    0xed627dae, 0x88d14467, 0xd7bbfe6a, 0xec447f11, 0x8e7ea170, 0x6427800e, 0x4d47bae0, 0x09fe548f,
    0x83852d0f, 0x30362f1a, 0x7b5a9cc3, 0x31fec169, 0x9fec022a, 0x6c8dedc4, 0x15d6874d, 0x5fde7a4e,
    0xbad90e37, 0x2e4e5eef, 0x4eaba214, 0xa8a472c0, 0x429a969e, 0x148d302a, 0xc40ba6d0, 0xc4e22c3c};

__device__ __forceinline__ uint32_t mulx(uint32_t b) { return (b >> 1) ^ (kPoly & (0u - (b & 1u))); }
__device__ __forceinline__ uint32_t multmodp(uint32_t a, uint32_t b) {   // a b mod p
    uint32_t p = 0;
#pragma unroll
    for (int k = 31; k >= 0; --k) {
        p ^= b & (0u - ((a >> k) & 1u));
        b = mulx(b);
    }
    return p;
}
__device__ uint32_t x8n(uint32_t n) {                     // x^(8 n) mod p: n zero bytes' shift (uniform n)
    uint32_t p = 1u << 31;
    for (int k = 3; n; n >>= 1, ++k)
        if (n & 1u) p = multmodp(kX2n[k & 31], p);
    return p;
}
__device__ __forceinline__ uint32_t crc_word(uint32_t c, uint32_t w) {   // 4 bytes, little-endian
    c ^= w;
#pragma unroll
    for (int i = 0; i < 32; ++i) c = mulx(c);
    return c;
}
// the raw CRC of the wave's 64 consecutive 16-byte pieces (lane l: piece l's raw CRC), uniform
__device__ __forceinline__ uint32_t wave_fold(uint32_t v) {
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const uint32_t right = (uint32_t)__shfl_down((int)v, 1u << s);
        v = multmodp(kX2n[7 + s], v) ^ right;  // x^(8 16 2^s): the right half's length
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);   // (lane 0's: all 64 pieces)
}

}  // namespace
