// chan_words.hpp — the Fiat-Shamir channel's message words, built in registers
// (device only).  Frozen spec: a message is hex-encoded before
// it is hashed (channel.rs:35-44), so 4 bytes become 2 big-endian message
// words, and a root, which is sent as its own hex, is hex-encoded twice.
// Shared by the commit's channel wave (fri_tree_device.hpp) and the batched
// verifier's channel replay (fri_verify_kernels.hip).
#pragma once
#include <stdint.h>
#include "field.hpp"

namespace fri {

__device__ __forceinline__ uint32_t hexch(uint32_t nib) { return nib < 10u ? 0x30u + nib : 0x57u + nib; }
// 4 bytes -> 8 lowercase hex chars -> 2 big-endian message words
__device__ __forceinline__ void hex2(uint32_t x, uint32_t& hi, uint32_t& lo) {
    hi = (hexch(x >> 28) << 24) | (hexch((x >> 24) & 15u) << 16) | (hexch((x >> 20) & 15u) << 8) | hexch((x >> 16) & 15u);
    lo = (hexch((x >> 12) & 15u) << 24) | (hexch((x >> 8) & 15u) << 16) | (hexch((x >> 4) & 15u) << 8) | hexch(x & 15u);
}
// one byte -> hex(hex(byte)) = 4 chars = one message word.  For a nibble n,
// hexch(n) is '0'+n or 'a'+n-10, whose own hex is "3" '0'+n or "6" '0'+n-9:
// 0x3330 + n, plus 0x2F7 when n >= 10 (two 16-bit SWAR lanes).
__device__ __forceinline__ uint32_t hexhex(uint32_t b) {
    const uint32_t x = ((b & 0xF0u) << 12) | (b & 0x0Fu);
    const uint32_t ge = ((x + 0x00060006u) >> 4) & 0x00010001u;
    return 0x33303330u + x + ge * 0x2F7u;
}

// channel.rs:47-72: beta = U256(state) mod p  (the rehash is deferred).
// U256(state) = sum_i s_i 2^(32 (7-i)): eight independent products with the
// Montgomery weights 2^(32 (8-i)) mod p and a sum tree, instead of eight
// dependent Horner steps on the critical path after the root.
constexpr uint32_t pow2_32k_mod_p(int k) {
    uint64_t r = 1;
    for (int j = 0; j < k; j++) r = (r << 32) % P;
    return (uint32_t)r;
}
__device__ __forceinline__ uint32_t chan_beta(const uint32_t s[8]) {
    constexpr uint32_t W[8] = {pow2_32k_mod_p(8), pow2_32k_mod_p(7), pow2_32k_mod_p(6), pow2_32k_mod_p(5),
                               pow2_32k_mod_p(4), pow2_32k_mod_p(3), pow2_32k_mod_p(2), pow2_32k_mod_p(1)};
    uint32_t t[8];
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = mmul(s[i] >= P ? s[i] - P : s[i], W[i]);
    return add(add(add(t[0], t[1]), add(t[2], t[3])), add(add(t[4], t[5]), add(t[6], t[7])));
}

}  // namespace fri
