// fri_prover.hip — prover slice around the FRI commit (SURVEY.md §8(f) rank 2,
// BASELINE configs[3]): the STARK-101 FibonacciSq composition polynomial in
// evaluation form on the LDE coset, the trace-tree decommitment gather, the
// batch's query phase and the proof-of-work grinding before it.
//
// The reference's src/prover, src/trace and src/composition are empty files;
// the constraint system is STARK-101's (the crate is `stark-101`,
// Cargo.toml:2), restated on the full trace subgroup G = <g>, |G| = T:
//     a_0 = 1,  a_{T-1} = A,  a_{i+2} = a_{i+1}^2 + a_i^2  (i <= T-3)
//     p0 = (f(x) - 1) / (x - 1)
//     p1 = (f(x) - A) / (x - g^{T-1})
//     p2 = (f(g^2 x) - f(g x)^2 - f(x)^2) * (x - g^{T-2})(x - g^{T-1}) / (x^T - 1)
//     CP = alpha0 p0 + alpha1 p1 + alpha2 p2            (deg CP <= T)
// On the LDE coset x_i = offset * w_n^i (n = B*T) the shifts are index shifts:
// g = w_n^B, so f(g x_i) = f[i + B], f(g^2 x_i) = f[i + 2B] (mod n), and
// x_i^T = offset^T * w_B^(i mod B) takes B values (host-inverted table).
// The two per-point divisions share one batch inversion (Montgomery's trick
// over CP_K consecutive points per lane, one Fermat inverse per lane).
#include "fri_internal.hpp"
#include "chan_send.hpp"
#include "sha256_fast.hpp"

namespace fri {

constexpr uint32_t CP_K = 16;     // points per lane

// One lane's CP_K points of one trace: f and out are that trace's n-word
// buffers, alpha_m / a_last its constants (the rest of q is the shape's).
__device__ __forceinline__ void fibsq_cp_lane(const uint32_t* __restrict__ f, uint32_t* __restrict__ out,
                                              const FibsqParams& q, uint32_t alpha0_m, uint32_t alpha1_m,
                                              uint32_t alpha2_m, uint32_t a_last) {
    const size_t n = (size_t)1 << q.log_n;
    const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * CP_K;
    if (i0 >= n) return;
    const size_t mask = n - 1;
    const uint32_t one_m = R_MOD_P;
    // x_{i0} = offset * w^{i0} (Montgomery), then x_{i+1} = x_i * w
    uint32_t x = mmul(q.offset_m, mpow(q.w_m, i0));
    uint32_t xa[CP_K], xb[CP_K], pre[CP_K];
    uint32_t acc = one_m;
#pragma unroll
    for (uint32_t k = 0; k < CP_K; k++) {
        xa[k] = sub(x, one_m);              // (x - 1)        Montgomery
        xb[k] = sub(x, q.glast_m);          // (x - g^{T-1})  Montgomery
        pre[k] = acc;
        acc = mmul(acc, mmul(xa[k], xb[k]));
        x = mmul(x, q.w_m);
    }
    // x_i != 1 and x_i != g^{T-1}: the coset is disjoint from G, so acc != 0
    uint32_t inv = mpow(acc, P - 2);
    x = mmul(q.offset_m, mpow(q.w_m, i0 + CP_K - 1));
#pragma unroll
    for (int k = CP_K - 1; k >= 0; k--) {
        const uint32_t dinv = mmul(inv, pre[k]);           // 1 / ((x-1)(x-g^{T-1}))
        inv = mmul(inv, mmul(xa[k], xb[k]));
        // n = 8 (log_t 2, blowup 2) is less than one lane's CP_K points: lane 0's
        // points 8..15 are points 0..7 again (w^n = 1), so the wrapped index reads
        // and writes the same words with the same values, inside the n-word buffers
        const size_t i = (i0 + k) & mask;
        const uint32_t fi = f[i], f1 = f[(i + q.B) & mask], f2 = f[(i + 2 * q.B) & mask];
        const uint32_t p0 = mmul(sub(fi, 1u), mmul(dinv, xb[k]));        // (f-1)/(x-1)
        const uint32_t p1 = mmul(sub(fi, a_last), mmul(dinv, xa[k]));  // (f-A)/(x-g^{T-1})
        const uint32_t sq = add(mmul(f1, to_mont(f1)), mmul(fi, to_mont(fi)));
        const uint32_t num2 = sub(f2, sq);
        const uint32_t zf = mmul(mmul(sub(x, q.gprev_m), xb[k]), q.zinv_m[i & (q.B - 1)]);
        const uint32_t p2 = mmul(num2, zf);
        out[i] = add(add(mmul(p0, alpha0_m), mmul(p1, alpha1_m)), mmul(p2, alpha2_m));
        x = mmul(x, q.winv_m);
    }
}

__global__ __launch_bounds__(256) void k_fibsq_cp(const uint32_t* __restrict__ f, uint32_t* __restrict__ out,
                                                  FibsqParams q) {
    fibsq_cp_lane(f, out, q, q.alpha_m[0], q.alpha_m[1], q.alpha_m[2], q.a_last);
}

void launch_fibsq_cp(const uint32_t* f_lde, uint32_t* out, const FibsqParams& q, hipStream_t s) {
    const size_t lanes = (((size_t)1 << q.log_n) + CP_K - 1) / CP_K;
    hipLaunchKernelGGL(k_fibsq_cp, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, f_lde, out, q);
}

// The batch (fri_fibsq_composition_commit_batch): trace blockIdx.y of one
// shape, its LDE and output at b * stride, its alphas and a_last in mem[b].
// The n = 8 wrap of fibsq_cp_lane stays inside the member's n words: the
// index is masked before the member's base is added.
__global__ __launch_bounds__(256) void k_fibsq_cp_batch(const uint32_t* __restrict__ f, size_t f_stride,
                                                        uint32_t* __restrict__ out, size_t out_stride,
                                                        const FibsqMember* __restrict__ mem, FibsqParams q) {
    const size_t b = blockIdx.y;
    const FibsqMember m = mem[b];
    fibsq_cp_lane(f + b * f_stride, out + b * out_stride, q, m.alpha_m[0], m.alpha_m[1], m.alpha_m[2], m.a_last);
}

void launch_fibsq_cp_batch(const uint32_t* f_lde, size_t f_stride, uint32_t* out, size_t out_stride,
                           const FibsqMember* mem, uint32_t batch, const FibsqParams& q, hipStream_t s) {
    const size_t lanes = (((size_t)1 << q.log_n) + CP_K - 1) / CP_K;
    hipLaunchKernelGGL(k_fibsq_cp_batch, dim3((unsigned)((lanes + 255) / 256), batch), dim3(256), 0, s, f_lde, f_stride,
                       out, out_stride, mem, q);
}

// Trace-tree decommitment (STARK-101 decommit_on_query): values at
// index + j*stride (j < count) and their authentication paths, sibling
// digests leaf -> root as big-endian bytes.  Block j, lane l = level l.
__global__ void k_trace_gather(const uint32_t* __restrict__ lde, const uint32_t* __restrict__ tree, uint32_t L,
                               uint64_t index, uint64_t stride, uint32_t* __restrict__ out, uint32_t count) {
    const uint32_t j = blockIdx.x;
    const uint64_t leaf = (index + j * stride) & (((uint64_t)1 << L) - 1);
    if (threadIdx.x == 0) out[j] = lde[leaf];
    const uint32_t l = threadIdx.x;
    if (l >= L) return;
    const uint32_t* d = sibling_digest(tree, L, l, leaf);
    store_digest_be(out + count + (size_t)j * 8 * L + 8 * l, d);
}

void launch_trace_gather(const uint32_t* lde, const uint32_t* tree, uint32_t L, uint64_t index, uint64_t stride,
                         uint32_t count, uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_trace_gather, dim3(count), dim3(64), 0, s, lde, tree, L, index, stride, out, count);
}

// ------------------------------------------------ the query phase (device) ---
// fri_batch_query_phase: every query of every member of a batch, the members'
// channels included.  The verifier's split, turned around:
// k_query_chain runs each member's Fiat-Shamir chain and leaves the indices it
// drew, then k_batch_query_all gathers the records of those indices.
// fri_batch_query_round is that gather alone, of one query at the host's indices.

// One lane per member, workgroups of one wave (k_verify_chain's shape).  The
// lane runs num_queries x { receive_random_int(0, range - 1, true), then the
// sends of prove_fibsq's query round } in units of a few sends:
//   0 the index, [1, 1 + tc) the trace openings (value, path), then per layer
//   (value, path, sibling value, sibling path), a one-element layer's value
//   once more first (fri_commit.rs:147-149).
// Values and sibling digests are read where they live, in the member's trace
// LDE and tree and its layers and trees (k_batch_query_all's addressing); nothing
// is staged.  Every address is formed from the drawn index masked to the
// layer's size.  Lanes past their member's last layer sit the unit out; a
// member with n_layers = 0 is left out and nothing of it is written.
__global__ __launch_bounds__(64) void k_query_chain(QueryPhase q) {
    const uint32_t m = blockIdx.x * 64u + threadIdx.x;
    if (m >= q.members) return;
    const uint32_t nl = q.n_layers[m];
    if (nl == 0) return;
    const size_t b = (size_t)q.first + m;
    const uint32_t L = q.log_n, ML = q.max_layers, tc = q.trace_count, Q = q.num_queries;
    const uint32_t* lay = q.layers + b * q.lay_stride;
    const uint32_t* tre = q.trees + b * q.tre_stride;
    const uint32_t* tlde = q.tlde + b * q.tlde_stride;
    const uint32_t* ttree = q.ttree + b * q.ttree_stride;
    uint32_t* chan = q.chan + (size_t)m * 9u;
    uint32_t cs[8], has;
#pragma unroll
    for (int j = 0; j < 8; j++) cs[j] = __builtin_bswap32(chan[j]);
    has = chan[8] ? 1u : 0u;
#pragma unroll 1
    for (uint32_t qi = 0; qi < Q; qi++) {
        uint64_t index = 0;
        const uint32_t units = 1u + tc + ML;
#pragma unroll 1
        for (uint32_t u = 0; u < units; u++) {
            const uint32_t nsub = u == 0 ? 1u : (u < 1u + tc ? 2u : (L - (u - 1u - tc) == 0u ? 5u : 4u));
#pragma unroll 1
            for (uint32_t s = 0; s < nsub; s++) {
                uint32_t kind = MSG_PATH, nd = 0u, v = 0u;
                TreeNodes src{tre, 0u, 0u};
                bool act = true;
                if (u == 0) {
                    // the draw, then its rehash: send(b"") is sha256(hex(cs))
                    index = chan_int(cs, q.range);
                    q.indices[(size_t)m * Q + qi] = index;
                } else if (u < 1u + tc) {
                    const uint64_t leaf = (index + (u - 1u) * q.trace_stride) & (((uint64_t)1 << L) - 1u);
                    if (s == 0) { kind = MSG_VALUE; v = tlde[leaf]; }
                    else { src = TreeNodes{ttree, L, leaf}; nd = L; }
                } else {
                    const uint32_t k = u - 1u - tc, depth = L - k;
                    const uint32_t s4 = depth ? s : s - 1u;      // depth 0: sub 0 is the doubled value
                    const uint64_t mk = (uint64_t)1 << depth;
                    const uint64_t idx = index & (mk - 1u);
                    const uint64_t leaf = (s4 == 2u || s4 == 3u) ? ((idx + mk / 2u) & (mk - 1u)) : idx;
                    act = k < nl;
                    if (s4 == 0u || s4 == 2u || s4 == ~0u) { kind = MSG_VALUE; v = act ? lay[q.layer_off[k] + leaf] : 0u; }
                    else { src = TreeNodes{tre + q.tree_off[k], depth, leaf}; nd = depth; }
                }
                if (!act) continue;
                chan_send(cs, has, kind, src, nd, v, 0u);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) chan[j] = __builtin_bswap32(cs[j]);
    chan[8] = has;
}

// The openings of every (member, query): block (x + openings * query, member),
// lane l = tree level l, the index the one in q.indices.  x < trace_count opens
// the member's trace LDE at index + x * trace_stride (k_trace_gather's value and
// path); above, x - trace_count is a FRI layer k of the member: the values at
// idx = index mod m_k and its sibling and their two paths (k_decommit_gather).
// THE RECORD of (member, query) is rec_words words at out + (member *
// num_queries + query) * rec_words:
//   [trace values][2 * max_layers FRI values][trace paths, 8 L words each]
//   [FRI paths, layer k's two at 16 (k L - k (k - 1) / 2)]
// of which a member with fewer layers fills a prefix of each part (the sizes:
// RecordShape, fri_host.hpp).  A member with n_layers = 0 (skipped, or its
// commit failed) writes nothing.
__global__ __launch_bounds__(64) void k_batch_query_all(QueryPhase q) {
    const uint32_t L = q.log_n, tc = q.trace_count, opens = tc + q.max_layers;
    const uint32_t x = blockIdx.x % opens, qi = blockIdx.x / opens, l = threadIdx.x;
    const uint32_t m = blockIdx.y;
    const uint32_t nl = q.n_layers[m];
    if (nl == 0) return;
    const size_t b = (size_t)q.first + m;
    const uint64_t index = q.indices[(size_t)m * q.num_queries + qi];
    uint32_t* rec = q.out + ((size_t)m * q.num_queries + qi) * q.rec_words;
    uint32_t* tpaths = rec + tc + 2 * q.max_layers;
    if (x < tc) {
        const uint64_t leaf = (index + x * q.trace_stride) & (((uint64_t)1 << L) - 1);
        if (l == 0) rec[x] = q.tlde[b * q.tlde_stride + leaf];
        if (l >= L) return;
        const uint32_t* d = sibling_digest(q.ttree + b * q.ttree_stride, L, l, leaf);
        store_digest_be(tpaths + (size_t)x * 8 * L + 8 * l, d);
        return;
    }
    const uint32_t k = x - tc;
    if (k >= nl) return;
    const uint32_t Lk = L - k;
    const uint64_t mk = (uint64_t)1 << Lk;
    const uint64_t idx = index % mk, sib = (idx + mk / 2) % mk;
    const uint32_t* lay = q.layers + b * q.lay_stride + q.layer_off[k];
    if (l == 0) {
        rec[tc + 2 * k] = lay[idx];
        rec[tc + 2 * k + 1] = lay[sib];
    }
    if (l >= Lk) return;
    const uint32_t* tr = q.trees + b * q.tre_stride + q.tree_off[k];
    uint32_t* paths = tpaths + (size_t)tc * 8 * L + 16 * ((size_t)k * L - (size_t)k * (k - 1) / 2);
#pragma unroll
    for (int which = 0; which < 2; which++) {
        const uint32_t* d = sibling_digest(tr, Lk, l, which ? sib : idx);
        store_digest_be(paths + (size_t)which * 8 * Lk + 8 * l, d);
    }
}

void launch_query_chain(const QueryPhase& q, hipStream_t s) {
    if (!q.members || !q.num_queries) return;
    hipLaunchKernelGGL(k_query_chain, dim3((q.members + 63u) / 64u), dim3(64), 0, s, q);
}
void launch_query_gather(const QueryPhase& q, hipStream_t s) {
    if (!q.members || !q.num_queries) return;
    hipLaunchKernelGGL(k_batch_query_all, dim3((q.trace_count + q.max_layers) * q.num_queries, q.members), dim3(64), 0,
                       s, q);
}

// ------------------------------------------------- grinding ---
// fri_grind / fri_grind_batch: the smallest nonce v such that
//     SHA256(ascii(state) || ascii(hex(be64(v))))
// has its `bits` most significant bits zero (the state after channel.send of
// the 8-byte nonce, channel.rs:35-44).  The state's 64 hex characters are the
// first block of every candidate, so a candidate costs one compression, from
// the member's midstate, of a block of which only W0..W3 (the nonce's 16 hex
// characters) vary: W4 is the padding bit, W15 the length, the rest zero.

// 16 bits -> 4 lowercase hex characters, one big-endian message word (SWAR:
// the nibbles spread to bytes, '0' + n, and 0x27 more from 10 up)
__device__ __forceinline__ uint32_t hex4(uint32_t x) {
    const uint32_t t = ((x & 0xF000u) << 12) | ((x & 0x0F00u) << 8) | ((x & 0x00F0u) << 4) | (x & 0x000Fu);
    return t + 0x30303030u + (((t + 0x06060606u) >> 4) & 0x01010101u) * 0x27u;
}

// One lane per member: the midstate of its channel state and its length word.
__global__ __launch_bounds__(256) void k_grind_prep(const uint32_t* __restrict__ chan, GrindMember* __restrict__ mem,
                                                    unsigned long long* __restrict__ best, uint32_t members) {
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;
    if (m >= members) return;
    const uint32_t* c = chan + (size_t)m * 9u;
    uint32_t st[8];
    sha::init(st);
    uint32_t len = 128u;
    if (c[8]) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 8; j++) hex2(__builtin_bswap32(c[j]), w[2 * j], w[2 * j + 1]);
        sha::compress(st, w);
        len = 640u;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) mem[m].mid[j] = st[j];
    mem[m].len_bits = len;
    best[m] = ~0ull;
}

// Digest word 0 of the nonce's block from the midstate.  The rate-ordered
// rounds of the leaf kernels (sha256_fast.hpp); the schedule stays in C so
// that its zero words fold and what depends on m0, m1 and the length alone
// leaves the caller's loop.  Rounds 0-1 see only m0 and m1 (the same for a
// whole window) and stay in C for the same reason; round 63 does so that the
// unused e of the last round goes.  k15 = K[15] + len_bits, in an SGPR.
__device__ __forceinline__ uint32_t grind_word0(const uint32_t mid[8], uint32_t m0, uint32_t m1, uint32_t m2,
                                                uint32_t m3, uint32_t len_bits, uint32_t k15) {
    using namespace shaf;
    uint32_t w[16] = {m0, m1, m2, m3, 0x80000000u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, len_bits};
    uint32_t a = mid[0], b = mid[1], c = mid[2], d = mid[3], e = mid[4], f = mid[5], g = mid[6], h = mid[7];
#pragma unroll
    for (int t = 0; t < 64; t += 8) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int tt = t + u;
            if (tt < 2) {
                SHAF_ROUND8(SHAF_RND_C, u, sha::K(tt) + w[tt])
            } else if (tt < 4) {
                SHAF_ROUND8(SHAF_RND_W, u, w[tt], sha::K(tt))
            } else if (tt < 15) {
                SHAF_ROUND8(SHAF_RND_K, u, sha::K(tt) + w[tt])
            } else if (tt == 15) {
                SHAF_ROUND8(SHAF_RND_K, u, k15)
            } else {
                const uint32_t wt = w[tt & 15] + s0(w[(tt - 15) & 15]) + w[(tt - 7) & 15] + s1(w[(tt - 2) & 15]);
                w[tt & 15] = wt;
                if (tt < 63) {
                    SHAF_ROUND8(SHAF_RND_W, u, wt, sha::K(tt))
                } else {
                    SHAF_ROUND8(SHAF_RND_C, u, sha::K(tt) + wt)
                }
            }
        }
    }
    return mid[0] + a;
}

// Block (x, j): member j of the active list, waves blockIdx.x * 4 .. + 3 of
// gridDim.x * 4.  The window is cut into rows of 64 consecutive nonces, one
// per lane, aligned to 64 (the lanes below lo0 in the first row and past the
// end in the last sit out), so a nonce's low six bits are its lane: the last
// hex character is the lane's own and W2 and half of W3 are the row's.  Wave
// v takes rows v, v + waves, ..: ascending, so after its first hit nothing it
// could still find is smaller, and a row that starts above the member's
// current minimum (a relaxed load, issued a row ahead) cannot lower it.  Both
// exits only save work: a row is skipped only when all of it lies above a
// value the minimum has already reached.  The lowest hit lane of a row holds
// the row's smallest hit and alone goes to the atomic.
__global__ __launch_bounds__(256) void k_grind(GrindTask q) {
    const uint32_t j = blockIdx.y;
    const uint32_t m = q.active ? q.active[j] : j;
    const GrindMember* gm = q.mem + m;
    uint32_t mid[8];
#pragma unroll
    for (int i = 0; i < 8; i++) mid[i] = __builtin_amdgcn_readfirstlane(gm->mid[i]);
    const uint32_t len_bits = __builtin_amdgcn_readfirstlane(gm->len_bits);
    const uint32_t k15 = __builtin_amdgcn_readfirstlane(sha::K(15) + len_bits);
    unsigned long long* best = q.best + m;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t waves = gridDim.x * 4u;
    uint32_t m0, m1;
    hex2(q.hi, m0, m1);
    const uint32_t base = q.lo0 & ~63u, skew = q.lo0 & 63u;
    const uint32_t c0 = hexch(lane & 15u);
    unsigned long long cur = __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll 1
    for (uint32_t row = wave; row < q.rows; row += waves) {
        const uint32_t rel0 = row * 64u;                       // lane 0's nonce, counted from base
        if ((unsigned long long)(rel0 > skew ? rel0 - skew : 0u) > cur) break;
        const unsigned long long nxt = __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t lo_u = base + rel0;                     // low six bits zero: the lanes'
        const uint32_t m2 = hex4(lo_u >> 16);
        const uint32_t n1 = ((lo_u >> 4) & 0xCu) | (lane >> 4);
        const uint32_t m3 = (hex4(lo_u & 0xFFFFu) & 0xFFFF0000u) | (hexch(n1) << 8) | c0;
        const uint32_t h0 = grind_word0(mid, m0, m1, m2, m3, len_bits, k15);
        const uint32_t idx = rel0 + lane;
        const bool hit = idx >= skew && idx - skew <= q.last_idx && (h0 & q.mask) == 0u;
        const unsigned long long hits = __ballot(hit);
        if (hits) {
            if (lane == (uint32_t)__builtin_ctzll(hits))
                __hip_atomic_fetch_min(best, (unsigned long long)(idx - skew), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        cur = nxt;
    }
}

// One lane per active member: the whole digest of the nonce it found, if any,
// as its channel state after the send.
__global__ __launch_bounds__(64) void k_grind_finish(GrindTask q) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= q.n_active) return;
    const uint32_t m = q.active ? q.active[j] : j;
    const unsigned long long b = q.best[m];
    if (b == ~0ull) return;
    const GrindMember gm = q.mem[m];
    uint32_t w[16] = {0u, 0u, 0u, 0u, 0x80000000u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, gm.len_bits};
    hex2(q.hi, w[0], w[1]);
    hex2(q.lo0 + (uint32_t)b, w[2], w[3]);
    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = gm.mid[i];
    sha::compress(st, w);
    uint32_t* c = q.chan + (size_t)m * 9u;
#pragma unroll
    for (int i = 0; i < 8; i++) c[i] = __builtin_bswap32(st[i]);
    c[8] = 1u;
}

void launch_grind_prep(const uint32_t* chan, GrindMember* mem, unsigned long long* best, uint32_t members,
                       hipStream_t s) {
    hipLaunchKernelGGL(k_grind_prep, dim3((members + 255u) / 256u), dim3(256), 0, s, chan, mem, best, members);
}

// The search of one window, then the states of the members that found a nonce.
// 2048 workgroups of four waves fill the chip at eight waves per SIMD; a batch
// shares them among its members, at least one workgroup each.
void launch_grind(const GrindTask& q, hipStream_t s) {
    if (!q.n_active || !q.rows) return;
    const uint32_t share = 2048u / q.n_active ? 2048u / q.n_active : 1u, want = (q.rows + 3u) / 4u;
    const uint32_t gx = want < share ? want : share;
    hipLaunchKernelGGL(k_grind, dim3(gx, q.n_active), dim3(256), 0, s, q);
    hipLaunchKernelGGL(k_grind_finish, dim3((q.n_active + 63u) / 64u), dim3(64), 0, s, q);
}

}  // namespace fri
