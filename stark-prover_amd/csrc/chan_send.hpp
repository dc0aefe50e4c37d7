// chan_send.hpp — one lane's Fiat-Shamir channel (channel.rs:35-84) in
// registers: the looped SHA-256 compression, Channel::send over a message of
// 32-byte nodes, a root or a value, and receive_random_int's draw (device
// only).  Shared by the batched verifier's replay (k_verify_chain,
// fri_verify_kernels.hip), which takes its nodes from the bytes of a record,
// and the batched prover's query phase (k_query_chain, fri_prover.hip), which
// takes them from the resident trees' digest words.  Every kernel that
// includes this keeps ONE call site of chan_send, and so of compress_c: both
// run a lane's compressions one after another, and the footprint in the
// instruction cache counts for more than the last percent of issue rate
// (DESIGN.md §4g).
#pragma once
#include "fri_internal.hpp"
#include "chan_words.hpp"
#include "sha256.hpp"

namespace fri {
namespace {

// SHA-256 compression, 16 rounds unrolled and looped four times.  K through
// scalar loads (the round index is wave-uniform).
__constant__ uint32_t VK[64] = {
    0x428a2f98u,0x71374491u,0xb5c0fbcfu,0xe9b5dba5u,0x3956c25bu,0x59f111f1u,0x923f82a4u,0xab1c5ed5u,
    0xd807aa98u,0x12835b01u,0x243185beu,0x550c7dc3u,0x72be5d74u,0x80deb1feu,0x9bdc06a7u,0xc19bf174u,
    0xe49b69c1u,0xefbe4786u,0x0fc19dc6u,0x240ca1ccu,0x2de92c6fu,0x4a7484aau,0x5cb0a9dcu,0x76f988dau,
    0x983e5152u,0xa831c66du,0xb00327c8u,0xbf597fc7u,0xc6e00bf3u,0xd5a79147u,0x06ca6351u,0x14292967u,
    0x27b70a85u,0x2e1b2138u,0x4d2c6dfcu,0x53380d13u,0x650a7354u,0x766a0abbu,0x81c2c92eu,0x92722c85u,
    0xa2bfe8a1u,0xa81a664bu,0xc24b8b70u,0xc76c51a3u,0xd192e819u,0xd6990624u,0xf40e3585u,0x106aa070u,
    0x19a4c116u,0x1e376c08u,0x2748774cu,0x34b0bcb5u,0x391c0cb3u,0x4ed8aa4au,0x5b9cca4fu,0x682e6ff3u,
    0x748f82eeu,0x78a5636fu,0x84c87814u,0x8cc70208u,0x90befffau,0xa4506cebu,0xbef9a3f7u,0xc67178f2u};

#define VK_ROUND(kw)                                                                \
    {                                                                               \
        const uint32_t t1 = h + (kw) + sha::bsig1(e) + sha::ch(e, f, g);            \
        const uint32_t t2 = sha::bsig0(a) + sha::maj(a, b, c);                      \
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;          \
    }
__device__ __forceinline__ void compress_c(uint32_t st[8], uint32_t w[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int i = 0; i < 16; i++) VK_ROUND(w[i] + VK[i]);
#pragma unroll 1
    for (int r = 1; r < 4; r++) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            w[i] = w[i] + sha::ssig0(w[(i + 1) & 15]) + w[(i + 9) & 15] + sha::ssig1(w[(i + 14) & 15]);
            VK_ROUND(w[i] + VK[16 * r + i]);
        }
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}
#undef VK_ROUND

// 32 bytes of a record as they were sent -> the eight big-endian words
__device__ __forceinline__ void load_node(const uint32_t* p, uint32_t out[8]) {
    const uint4 lo = reinterpret_cast<const uint4*>(p)[0], hi = reinterpret_cast<const uint4*>(p)[1];
    out[0] = __builtin_bswap32(lo.x); out[1] = __builtin_bswap32(lo.y);
    out[2] = __builtin_bswap32(lo.z); out[3] = __builtin_bswap32(lo.w);
    out[4] = __builtin_bswap32(hi.x); out[5] = __builtin_bswap32(hi.y);
    out[6] = __builtin_bswap32(hi.z); out[7] = __builtin_bswap32(hi.w);
}

// Where a message's nodes come from: node(i, out) gives node i's eight
// big-endian words, root_word(i) word i of a root's digest.
// The bytes of a record, as they were sent (the verifier).
struct RecordNodes {
    const uint32_t* p;
    __device__ __forceinline__ void node(uint32_t i, uint32_t out[8]) const { load_node(p + 8 * i, out); }
    __device__ __forceinline__ uint32_t root_word(uint32_t i) const { return p[i]; }
};
// An authentication path read where it lives (the prover): the sibling of
// `leaf` at every level of a resident tree of 2^L leaves (level_offset), whose
// digests are big-endian words already.  Sends no root.
struct TreeNodes {
    const uint32_t* tree;
    uint32_t L;
    uint64_t leaf;
    __device__ __forceinline__ void node(uint32_t i, uint32_t out[8]) const {
        const uint32_t* d = sibling_digest(tree, L, i, leaf);
        const uint4 lo = reinterpret_cast<const uint4*>(d)[0], hi = reinterpret_cast<const uint4*>(d)[1];
        out[0] = lo.x; out[1] = lo.y; out[2] = lo.z; out[3] = lo.w;
        out[4] = hi.x; out[5] = hi.y; out[6] = hi.z; out[7] = hi.w;
    }
    __device__ __forceinline__ uint32_t root_word(uint32_t) const { return 0u; }
};

// ------------------------------------------------------------ the channel ---
enum : uint32_t { MSG_PATH = 0, MSG_ROOT = 1, MSG_VALUE = 2 };

// One Channel::send (channel.rs:35-44): cs = sha256(hex(cs) || hex(message)).
// The state is "" or 64 hex characters and every data block below is 64 hex
// characters, so every message starts on a block boundary:
//   MSG_PATH   nd nodes of 32 bytes from src, one block each, then the padding
//              block; nd = 0 is send(b"") and also receive_random_int's
//              rehash (channel.rs:75-76), sha256(hex(cs));
//   MSG_ROOT   the root's 64-character hex, hex-encoded again: two blocks of
//              hexhex from the 8 digest words of src, then the padding block;
//   MSG_VALUE  the 8 bytes be64(vhi * 2^32 + v): 16 hex characters and the
//              padding in one block (vhi is 0 for a field element and a query
//              index; a grinding nonce is a full 64-bit number).
// kind and nd are wave-uniform; `has` and src are the lane's.  The next node
// is in flight under the current block's rounds.  The ONE call site of
// compress_c in a chain kernel.
template <class Src>
__device__ __forceinline__ void chan_send(uint32_t cs[8], uint32_t& has, uint32_t kind, const Src& src, uint32_t nd,
                                          uint32_t v, uint32_t vhi) {
    uint32_t X[8], nxt[8];
    sha::init(X);
    if (kind == MSG_PATH && nd) src.node(0u, nxt);
    const uint32_t chars = 64u * has + (kind == MSG_VALUE ? 16u : 64u * nd);
#pragma unroll 1
    for (int i = -1; i <= (int)nd; i++) {
        uint32_t w[16];
        if (i < 0) {
            if (!has) continue;
#pragma unroll
            for (int j = 0; j < 8; j++) hex2(cs[j], w[2 * j], w[2 * j + 1]);
        } else if (i < (int)nd) {
            if (kind == MSG_ROOT) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t r = src.root_word(4 * i + j);
                    w[4 * j] = hexhex(r >> 24);
                    w[4 * j + 1] = hexhex((r >> 16) & 255u);
                    w[4 * j + 2] = hexhex((r >> 8) & 255u);
                    w[4 * j + 3] = hexhex(r & 255u);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) hex2(nxt[j], w[2 * j], w[2 * j + 1]);
                if (i + 1 < (int)nd) src.node(i + 1, nxt);   // in flight under this block's rounds
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) w[j] = 0u;
            if (kind == MSG_VALUE) {
                hex2(vhi, w[0], w[1]);                    // "00000000" where the u64's high word is 0
                hex2(v, w[2], w[3]);
                w[4] = 0x80000000u;
            } else {
                w[0] = 0x80000000u;
            }
            w[15] = 8u * chars;
        }
        compress_c(X, w);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) cs[j] = X[j];
    has = 1u;
}

// U256(cs) mod range, range <= 2^32 (channel.rs:58-72 with min = 0)
__device__ __forceinline__ uint64_t chan_int(const uint32_t cs[8], uint64_t range) {
    uint64_t r = 0;
#pragma unroll 1
    for (int i = 0; i < 8; i++) r = ((r << 32) | cs[i]) % range;
    return r;
}

}  // namespace
}  // namespace fri
