// fri_poly_kernels.hip — gfx950 kernels of the polynomial layer: polynomial
// arithmetic (fri_poly.hip), the product tree and the Lagrange basis
// (fri_roots.hip), multipoint evaluation and interpolation on the retained
// tree (fri_multipoint.hip).  The transforms between them are the NTT passes of
// fri_kernels.hip; the commit path launches nothing from this file.
//
// Data in HBM is canonical u32 (value < p) unless a section says Montgomery;
// constants are Montgomery (field.hpp).
#include "fri_internal.hpp"

namespace fri {

// ================================================= polynomial arithmetic ==
// fri_poly_mul / fri_poly_div_rem (fri_poly.hip; ops.rs:114-191).
//
// Pointwise kernels on NTT outputs.  The transforms leave canonical values,
// so every mmul of two of them carries one R^-1: the product kernel leaves
// A*B*R^-1, the Newton kernel G*(2 - F*G)*R^-2 (2*R^-1 - F*G*R^-1 is
// (2 - F*G)*R^-1).  The caller folds R (R^2) and N^-1 into the inverse
// transform's post-scale table, so there is no conversion pass.  16-byte
// loads and stores when the three pointers are aligned; out may alias a or b
// (each element is read, then written, by the same lane).
template <bool NEWTON>
__device__ __forceinline__ uint32_t poly_pw(uint32_t a, uint32_t b, uint32_t two_rinv) {
    const uint32_t t = mmul(a, b);
    return NEWTON ? mmul(b, sub(two_rinv, t)) : t;
}
template <bool NEWTON>
__global__ __launch_bounds__(256) void k_poly_pointwise(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n,
                                                        size_t n4, uint32_t two_rinv) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint4* a4 = reinterpret_cast<const uint4*>(a);
    const uint4* b4 = reinterpret_cast<const uint4*>(b);
    uint4* o4 = reinterpret_cast<uint4*>(out);
    for (size_t i = t0; i < n4; i += stride) {
        const uint4 x = a4[i], y = b4[i];
        uint4 r;
        r.x = poly_pw<NEWTON>(x.x, y.x, two_rinv);
        r.y = poly_pw<NEWTON>(x.y, y.y, two_rinv);
        r.z = poly_pw<NEWTON>(x.z, y.z, two_rinv);
        r.w = poly_pw<NEWTON>(x.w, y.w, two_rinv);
        o4[i] = r;
    }
    for (size_t i = 4 * n4 + t0; i < n; i += stride) out[i] = poly_pw<NEWTON>(a[i], b[i], two_rinv);
}
template <bool NEWTON>
static void launch_pointwise(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, hipStream_t s) {
    if (!n) return;
    const bool vec = ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)out)) & 15u) == 0;
    const size_t n4 = vec ? n / 4 : 0;
    const size_t work = n4 ? n4 : n;
    size_t blocks = (work + 255) / 256;
    if (blocks > 8192) blocks = 8192;                              // grid-stride beyond 2^21 lanes
    const uint32_t rinv = from_mont(1u);
    hipLaunchKernelGGL((k_poly_pointwise<NEWTON>), dim3((unsigned)blocks), dim3(256), 0, s, a, b, out, n, n4,
                       add(rinv, rinv));
}
void launch_poly_pointwise_mul(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, hipStream_t s) {
    launch_pointwise<false>(a, b, out, n, s);
}
void launch_poly_newton(const uint32_t* f, const uint32_t* g, uint32_t* out, size_t n, hipStream_t s) {
    launch_pointwise<true>(f, g, out, n, s);
}

// Direct convolution with a short operand (`* (x - c)`, the products of a
// small composition): out[i] = sum_j sht[j] * lng[i - j] for i < n_out, one
// lane per output coefficient, no transform.  The short operand is staged in
// LDS in Montgomery form (so each product comes out canonical), next to the
// window of the long operand the workgroup's 256 outputs read, zero-filled
// outside [0, ll): the inner loop has no bounds test, the short operand is an
// LDS broadcast and the window is read at consecutive addresses across lanes.
// Terms are canonical (< 2^32), at most POLY_DIRECT_LIMIT = 2^12 of them, so
// a 64-bit sum stays below 2^44 and is reduced once (two REDCs).
__global__ __launch_bounds__(256) void k_poly_conv_direct(const uint32_t* __restrict__ lng, size_t ll,
                                                          const uint32_t* __restrict__ sht, uint32_t ls,
                                                          uint32_t* __restrict__ out, size_t n_out) {
    extern __shared__ uint32_t poly_sm[];
    uint32_t* sh = poly_sm;                 // ls words
    uint32_t* win = poly_sm + ls;           // 256 + ls - 1 words: lng[i0 - (ls - 1) .. i0 + 255]
    const size_t i0 = (size_t)blockIdx.x * 256;
    for (uint32_t j = threadIdx.x; j < ls; j += 256) sh[j] = to_mont(sht[j]);
    const uint32_t wn = 256 + ls - 1;
    for (uint32_t t = threadIdx.x; t < wn; t += 256) {
        const size_t pos = i0 + t;          // index + (ls - 1)
        win[t] = (pos >= ls - 1 && pos - (ls - 1) < ll) ? lng[pos - (ls - 1)] : 0u;
    }
    __syncthreads();
    const size_t i = i0 + threadIdx.x;
    if (i >= n_out) return;
    const uint32_t* w = win + threadIdx.x + (ls - 1);   // w[-j] = lng[i - j]
    uint64_t acc = 0;
#pragma unroll 4
    for (uint32_t j = 0; j < ls; j++) acc += mmul(w[-(int)j], sh[j]);
    out[i] = mmul(redc(acc), R2_MOD_P);
}
void launch_poly_conv_direct(const uint32_t* lng, size_t ll, const uint32_t* sht, size_t ls, uint32_t* out,
                             size_t n_out, hipStream_t s) {
    if (!n_out || !ls || ls > POLY_DIRECT_LIMIT) return;
    const size_t lds = (2 * ls + 255) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_poly_conv_direct, dim3((unsigned)((n_out + 255) / 256)), dim3(256), lds, s, lng, ll, sht,
                       (uint32_t)ls, out, n_out);
}

// Division helpers.  Reverse-truncate-pad: dst[i] = src[top - i] for
// i < cnt (cnt <= top + 1), 0 for cnt <= i < n.  Remainder: r = a - t on the
// low n coefficients.
__global__ __launch_bounds__(256) void k_poly_reverse(const uint32_t* __restrict__ src, size_t top, size_t cnt,
                                                      uint32_t* __restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dst[i] = i < cnt ? src[top - i] : 0u;
}
__global__ __launch_bounds__(256) void k_poly_sub(const uint32_t* __restrict__ a, const uint32_t* __restrict__ t,
                                                  uint32_t* __restrict__ r, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) r[i] = sub(a[i], t[i]);
}
static unsigned poly_blocks(size_t n) {
    const size_t b = (n + 255) / 256;
    return (unsigned)(b > 8192 ? 8192 : b);
}
void launch_poly_reverse(const uint32_t* src, size_t top, size_t cnt, uint32_t* dst, size_t n, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_poly_reverse, dim3(poly_blocks(n)), dim3(256), 0, s, src, top, cnt, dst, n);
}
void launch_poly_sub(const uint32_t* a, const uint32_t* t, uint32_t* r, size_t n, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_poly_sub, dim3(poly_blocks(n)), dim3(256), 0, s, a, t, r, n);
}

// ===================================== product tree and the Lagrange basis ==
// fri_poly_from_roots / fri_lagrange_basis (fri_roots.hip; interpolation.rs:
// 9-23, 46-115).  Z = prod (x - r_i) over 2^log_np roots (the list padded
// with zero roots) as a binary product tree.  Every node is monic with the
// leading 1 implicit: a node of degree m is its m low coefficients, in
// Montgomery form, and a level is the 2^log_np words of its nodes side by side.
//   (x^m + a)(x^m + b) = x^2m + (a + b) x^m + a b.
//
// Leaf kernel: one workgroup builds the subtree over 2^log_leaf consecutive
// roots in LDS, level by level between two buffers.  A work item owns the
// output coefficients k and m + k of one node: for i = 0..m-1 the term
// a_i * b_((k - i) mod m) belongs to coefficient k when i <= k and to m + k
// otherwise, so every item runs exactly m products; m + k also takes
// a_k + b_k.  A level keeps its even nodes (the a's of the next level) in the
// buffer's first half and the odd nodes in the second: consecutive lanes then
// read one a word (a broadcast) or, below m = 64, words of neighbouring nodes
// that lie side by side, and consecutive b words (mod m): no two lanes of a
// wave meet in a bank at different addresses.  Sums of <= 2^10 Montgomery
// products (< 2^32 each) stay below 2^42 in 64 bits and are reduced once.
//
// WITH_F (interpolation, fri_multipoint.hip): F_S = sum_{i in S} c_i M_S /
// (x - x_i) is carried along in a second pair of buffers with the layout of
// the nodes, so the bank behaviour is the same.  Level 0 is F_i = c_i; the
// item owning coefficients k and m + k adds, to the m products of the node
// itself, the 2m of F_L b + F_R a (M_L = x^m + a, M_R = x^m + b), and m + k
// also takes F_L[k] + F_R[k]; sums of <= 2^11 products stay below 2^43.  The
// level written out is F's, and the last level's node product is skipped (the
// caller retains the tree); without F it is the node's, canonical on request.
// LDS: two buffers of the 2048-word limit per carried polynomial, 16 KiB (ten
// workgroups per CU) without F, 32 KiB with it.
template <bool WITH_F>
__device__ __forceinline__ void leaf_subtree(const uint32_t* __restrict__ roots, const uint32_t* __restrict__ c,
                                             size_t n, uint32_t log_leaf, uint32_t canon,
                                             uint32_t* __restrict__ out) {
    __shared__ uint32_t buf[WITH_F ? 4 : 2][1u << ROOTS_LEAF_LOG_MAX];   // nodes in [0], [1]; F in [2], [3]
    constexpr uint32_t FB = WITH_F ? 2 : 0;
    const uint32_t L = 1u << log_leaf, H = L >> 1, tid = threadIdx.x;
    const size_t r0 = (size_t)blockIdx.x << log_leaf;
    // level 0: node i is the constant -r_i; even nodes first
    for (uint32_t i = tid; i < L; i += blockDim.x) {
        const bool in = r0 + i < n;
        const uint32_t pos = log_leaf ? (i & 1u) * H + (i >> 1) : 0u;
        buf[0][pos] = to_mont(neg(in ? roots[r0 + i] : 0u));
        if (WITH_F) buf[FB][pos] = in ? c[r0 + i] : 0u;
    }
    uint32_t cur = 0;
    for (uint32_t lm = 0; lm < log_leaf; lm++, cur ^= 1u) {
        const uint32_t m = 1u << lm;
        const bool last = lm + 1 == log_leaf;
        const bool nodes = !(WITH_F && last);
        const uint32_t* a = buf[cur];          // node j of the even half, m words at j*m
        const uint32_t* b = buf[cur] + H;
        __syncthreads();
        for (uint32_t t = tid; t < H; t += blockDim.x) {
            const uint32_t nd = t >> lm, k = t & (m - 1);
            const uint32_t* an = a + nd * m;
            const uint32_t* bn = b + nd * m;
            const uint32_t* fan = buf[FB + cur] + nd * m;
            const uint32_t* fbn = fan + H;
            uint64_t lo = 0, hi = 0, flo = 0, fhi = 0;
            for (uint32_t i = 0; i < m; i++) {
                const uint32_t bv = bn[(k - i) & (m - 1)];
                if (WITH_F) {
                    const uint64_t fp = (uint64_t)mmul(fan[i], bv) + mmul(fbn[i], an[(k - i) & (m - 1)]);
                    flo += i <= k ? fp : 0;
                    fhi += i <= k ? 0 : fp;
                }
                if (nodes) {
                    const uint64_t p = mmul(an[i], bv);
                    lo += i <= k ? p : 0;
                    hi += i <= k ? 0 : p;
                }
            }
            // output node `nd` (2m words): even nodes in the first half; the
            // last level's single node fills the whole buffer
            const uint32_t o = last ? 0u : (nd & 1u) * H + (nd >> 1) * 2 * m;
            if (nodes) {
                buf[cur ^ 1u][o + k] = mmul(redc(lo), R2_MOD_P);
                buf[cur ^ 1u][o + m + k] = add(mmul(redc(hi), R2_MOD_P), add(an[k], bn[k]));
            }
            if (WITH_F) {
                buf[FB + (cur ^ 1u)][o + k] = mmul(redc(flo), R2_MOD_P);
                buf[FB + (cur ^ 1u)][o + m + k] = add(mmul(redc(fhi), R2_MOD_P), add(fan[k], fbn[k]));
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < L; i += blockDim.x) {
        const uint32_t v = buf[FB + cur][i];
        out[r0 + i] = !WITH_F && canon ? from_mont(v) : v;
    }
}
__global__ __launch_bounds__(256) void k_roots_leaf(const uint32_t* __restrict__ roots, size_t n, uint32_t log_leaf,
                                                    uint32_t canon, uint32_t* __restrict__ out) {
    leaf_subtree<false>(roots, nullptr, n, log_leaf, canon, out);
}
// a work item per output pair of a node: half the leaf's roots, within 64..256 threads
static uint32_t leaf_threads(uint32_t log_leaf) {
    const uint32_t half = log_leaf ? 1u << (log_leaf - 1) : 1u;
    return half < 64 ? 64 : half > 256 ? 256 : half;
}
void launch_roots_leaf(const uint32_t* roots, size_t n, uint32_t log_np, uint32_t log_leaf, bool canon, uint32_t* out,
                       hipStream_t s) {
    hipLaunchKernelGGL(k_roots_leaf, dim3(1u << (log_np - log_leaf)), dim3(leaf_threads(log_leaf)), 0, s, roots, n,
                       log_leaf, canon ? 1u : 0u, out);
}

// One level above the leaves whose products (2m = 2^lg words) fit LDS: a
// workgroup takes a tile of `tile` consecutive words of the level (tile / 2m
// pairs of nodes), and the whole tile runs as one batched transform, because
// the stages s < lg of a DIT over the tile are independent transforms of its
// aligned 2^lg blocks (the twiddles are stage-packed, size-independent).
// a and b of a pair are gathered bit-reversed into two arrays, zero-padded to
// 2m (the odd positions: stage 0 is then a copy), transformed, multiplied as
// (A + s)(B + s) - 1 with s = x^m at w_2m^k = (-1)^k (the monic factors; the
// product's x^2m wraps to the constant 1), scaled by (2m)^-1, scattered
// bit-reversed, transformed back and stored: one launch per level, no
// intermediate in HBM.  `scale` is Montgomery((2m)^-1), or the canonical
// value when the level is the top and leaves canonical coefficients.
//
// The same tile scheme carries the levels of the multipoint descent and
// ascent (k_mp_down_level, k_mp_up_level below); its steps are these helpers.

// The leading 1 of a monic node of degree m is x^m = (-1)^k at w_2m^k:
// Montgomery(+1) at an even transform index, Montgomery(-1) at an odd one.
__device__ __forceinline__ uint32_t monic_sign(uint32_t k) { return (k & 1u) ? P - R_MOD_P : R_MOD_P; }
// a times the monic node (x^m + node), at one transform point
__device__ __forceinline__ uint32_t mul_monic(uint32_t a, uint32_t node, uint32_t sg) { return mmul(a, add(node, sg)); }

constexpr uint32_t TILE_REGS = (1u << ROOTS_LDS_LOG_MAX) / 256;   // a thread's share of a tile: elements k * 256 + tid
template <class F>
__device__ __forceinline__ void tile_regs(uint32_t tile, F f) {
#pragma unroll
    for (uint32_t k = 0; k < TILE_REGS; k++) {
        const uint32_t e = k * 256 + threadIdx.x;
        if (e < tile) f(k, e);
    }
}
// where element e of a tile goes in the bit-reversed order of its 2^lg block
__device__ __forceinline__ uint32_t tile_brev(uint32_t e, uint32_t lg) {
    const uint32_t mask = (1u << lg) - 1;
    return (e & ~mask) + (__brev(e & mask) >> (32 - lg));
}
// One child (side 0: left) of every node pair of the tile, gathered
// bit-reversed and zero-padded to 2^lg: the padding is the odd positions, so
// stage 0 is the copy made here.
__device__ __forceinline__ void tile_load_child(uint32_t* dst, const uint32_t* __restrict__ src, uint32_t tile,
                                                uint32_t lg, uint32_t side) {
    const uint32_t h = 1u << (lg - 1);
    for (uint32_t e = threadIdx.x; e < tile / 2; e += 256) {
        const uint32_t nb = (e >> (lg - 1)) << lg, i = e & (h - 1);
        const uint32_t pos = nb + (__brev(i) >> (32 - lg));
        const uint32_t v = src[nb + side * h + i];
        dst[pos] = v;
        dst[pos + 1] = v;
    }
}
__device__ __forceinline__ void tile_stage(uint32_t* v, uint32_t tile, uint32_t s, const uint32_t* __restrict__ tw) {
    const uint32_t h = 1u << s;
    for (uint32_t e = threadIdx.x; e < tile / 2; e += blockDim.x) {
        const uint32_t lo = e & (h - 1), i = ((e >> s) << (s + 1)) | lo;
        const uint32_t u = v[i], t = mmul(v[i + h], tw[h + lo]);
        v[i] = add(u, t);
        v[i + h] = sub(u, t);
    }
}
// DIT stages s0..lg-1 on one array or two, a barrier ahead of each stage
__device__ __forceinline__ void tile_stages(uint32_t tile, uint32_t s0, uint32_t lg, const uint32_t* __restrict__ tw,
                                            uint32_t* a, uint32_t* b = nullptr) {
    for (uint32_t s = s0; s < lg; s++) {
        __syncthreads();
        tile_stage(a, tile, s, tw);
        if (b) tile_stage(b, tile, s, tw);
    }
}
// a thread's register tile to the bit-reversed positions of an array
__device__ __forceinline__ void tile_scatter(uint32_t* dst, const uint32_t (&r)[TILE_REGS], uint32_t tile,
                                             uint32_t lg) {
    tile_regs(tile, [&](uint32_t k, uint32_t e) { dst[tile_brev(e, lg)] = r[k]; });
}
// what the launchers of the level kernels share: the tile, and the scale
// (2^lg)^-1 of a level's inverse transform (Montgomery, or canonical)
static uint32_t level_tile(uint32_t log_np) { return 1u << (log_np < ROOTS_LDS_LOG_MAX ? log_np : ROOTS_LDS_LOG_MAX); }
static uint32_t level_scale(uint32_t lg, bool canon = false) {
    const uint32_t ninv = inv_std((uint32_t)(((size_t)1 << lg) % P));
    return canon ? ninv : to_mont(ninv);
}

__device__ __forceinline__ uint32_t roots_pw(uint32_t a, uint32_t b, uint32_t sg, uint32_t scale) {
    return mmul(sub(mmul(add(a, sg), add(b, sg)), R_MOD_P), scale);
}
__global__ __launch_bounds__(256) void k_roots_level(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                     uint32_t tile, uint32_t lg, const uint32_t* __restrict__ tw_f,
                                                     const uint32_t* __restrict__ tw_i, uint32_t scale) {
    __shared__ uint32_t A[1u << ROOTS_LDS_LOG_MAX], B[1u << ROOTS_LDS_LOG_MAX];
    const size_t base = (size_t)blockIdx.x * tile;
    tile_load_child(A, in + base, tile, lg, 0);
    tile_load_child(B, in + base, tile, lg, 1);
    tile_stages(tile, 1, lg, tw_f, A, B);
    __syncthreads();
    uint32_t r[TILE_REGS];
    tile_regs(tile, [&](uint32_t k, uint32_t e) { r[k] = roots_pw(A[e], B[e], monic_sign(e), scale); });
    __syncthreads();
    tile_scatter(A, r, tile, lg);
    tile_stages(tile, 0, lg, tw_i, A);
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < tile; e += 256) out[base + e] = A[e];
}
void launch_roots_level_lds(const uint32_t* in, uint32_t* out, uint32_t log_np, uint32_t lg, bool canon,
                            const uint32_t* tw_fwd, const uint32_t* tw_inv, hipStream_t s) {
    const uint32_t tile = level_tile(log_np);
    hipLaunchKernelGGL(k_roots_level, dim3((unsigned)(((size_t)1 << log_np) / tile)), dim3(256), 0, s, in, out, tile, lg,
                       tw_fwd, tw_inv, level_scale(lg, canon));
}

// Larger levels: the transforms are batched launches of the NTT passes
// (NttPlan::batch) around a pointwise step, elementwise over the level because
// k mod 2 is the word index mod 2.  Its loop, one 16-byte vector of each input
// per lane and step: f(x, sg, y) makes the outputs' word y from the inputs'
// word x and the sign of that word.  Every input vector is read before an
// output is written, so an output may be one of the inputs.
template <int NIN, int NOUT, class F>
__device__ __forceinline__ void monic_pointwise(const uint4* const (&in)[NIN], uint4* const (&out)[NOUT], size_t n4,
                                                F f) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        uint32_t v[NIN][4], r[NOUT][4];
#pragma unroll
        for (int j = 0; j < NIN; j++) {
            const uint4 t = in[j][i];
            v[j][0] = t.x, v[j][1] = t.y, v[j][2] = t.z, v[j][3] = t.w;
        }
#pragma unroll
        for (int w = 0; w < 4; w++) {
            uint32_t x[NIN], y[NOUT];
#pragma unroll
            for (int j = 0; j < NIN; j++) x[j] = v[j][w];
            f(x, monic_sign(w), y);
#pragma unroll
            for (int j = 0; j < NOUT; j++) r[j][w] = y[j];
        }
#pragma unroll
        for (int j = 0; j < NOUT; j++) out[j][i] = make_uint4(r[j][0], r[j][1], r[j][2], r[j][3]);
    }
}
// out = ((A + s)(B + s) - 1) * scale, A and B the transforms of the even and
// the odd nodes.
__global__ __launch_bounds__(256) void k_roots_pointwise(const uint4* a, const uint4* __restrict__ b, uint4* out,
                                                         size_t n4, uint32_t scale) {
    monic_pointwise<2, 1>({a, b}, {out}, n4, [&](const uint32_t (&x)[2], uint32_t sg, uint32_t (&y)[1]) {
        y[0] = roots_pw(x[0], x[1], sg, scale);
    });
}
void launch_roots_pointwise(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t words, uint32_t lg, bool canon,
                            hipStream_t s) {
    hipLaunchKernelGGL(k_roots_pointwise, dim3(poly_blocks(words / 4)), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(a), reinterpret_cast<const uint4*>(b),
                       reinterpret_cast<uint4*>(out), words / 4, level_scale(lg, canon));
}

// Lagrange rows: L_i = w_i * Z / (x - x_i), the quotient by synthetic
// division, q_i[n-1] = 1, q_i[j-1] = z_j + x_i q_i[j].  A wave takes 64 rows
// (one lane each) and a segment of LAGRANGE_SEG columns, 64 columns at a
// time: the lanes run the chain downwards and put w_i q_i[j] into an LDS tile
// (row stride 65 words: 64 banks, no conflict), then the tile goes out row by
// row, 64 consecutive words (256 bytes) per store instruction, instead of 64
// stores at stride n.  The chain of segment [c0, c1) starts from
//   q_i[c1 - 1] = T(c1),  T(c) = sum_{k >= c} z_k x_i^(k - c)  (z_n = 1),
// which the lane folds together from the segment values P_s(x_i) of a first
// kernel (P_s the slice of Z on segment s): T(s SEG) = P_s + x^len_s T(end_s).
constexpr uint32_t LAGRANGE_SEG = 256;
static uint32_t lagrange_segments(size_t n) {
    return n >= 1024 ? (uint32_t)((n + LAGRANGE_SEG - 1) / LAGRANGE_SEG) : 1u;
}
size_t lagrange_tmp_words(size_t n) { return (size_t)(lagrange_segments(n) - 1) * n; }
__global__ __launch_bounds__(256) void k_lagrange_parts(const uint32_t* __restrict__ xs, const uint32_t* __restrict__ z,
                                                        uint32_t n, uint32_t* __restrict__ part) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, sgm = blockIdx.y + 1;
    if (i >= n) return;
    const uint32_t lo = sgm * LAGRANGE_SEG, hi = lo + LAGRANGE_SEG < n ? lo + LAGRANGE_SEG : n;
    const uint32_t xm = to_mont(xs[i]);
    uint32_t h = 0;
    for (uint32_t k = hi; k-- > lo;) h = add(mmul(h, xm), z[k]);
    part[(size_t)(sgm - 1) * n + i] = h;
}
__global__ __launch_bounds__(64) void k_lagrange_rows(const uint32_t* __restrict__ xs, const uint32_t* __restrict__ z,
                                                      const uint32_t* __restrict__ w, uint32_t n,
                                                      const uint32_t* __restrict__ part, uint32_t* __restrict__ out) {
    __shared__ uint32_t tile[64 * 65];
    __shared__ uint32_t zs[64];
    const uint32_t lane = threadIdx.x, row0 = blockIdx.x * 64, i = row0 + lane;
    const uint32_t sgm = blockIdx.y, S = gridDim.y;
    const uint32_t c0 = S > 1 ? sgm * LAGRANGE_SEG : 0u;
    const uint32_t c1 = S > 1 && c0 + LAGRANGE_SEG < n ? c0 + LAGRANGE_SEG : n;
    const uint32_t xm = i < n ? to_mont(xs[i]) : 0u, wm = i < n ? w[i] : 0u;
    uint32_t q = 1u;                                                // T(n) = z_n
    if (i < n && c1 < n) {
        const uint32_t xseg = mpow(xm, LAGRANGE_SEG);
        for (uint32_t sp = S - 1; sp > sgm; sp--) {
            const uint32_t len = n - sp * LAGRANGE_SEG < LAGRANGE_SEG ? n - sp * LAGRANGE_SEG : LAGRANGE_SEG;
            q = add(part[(size_t)(sp - 1) * n + i], mmul(q, len == LAGRANGE_SEG ? xseg : mpow(xm, len)));
        }
    }
    for (int cb = (int)((c1 - 1) & ~63u); cb >= (int)c0; cb -= 64) {
        const uint32_t ce = (uint32_t)cb + 64 < c1 ? (uint32_t)cb + 64 : c1;
        zs[lane] = (uint32_t)cb + lane < ce ? z[cb + lane] : 0u;
        __syncthreads();
        for (int j = (int)ce - 1; j >= cb; j--) {
            tile[lane * 65 + (j - cb)] = mmul(q, wm);               // w_i q_i[j], canonical
            q = add(zs[j - cb], mmul(q, xm));                       // q_i[j - 1]
        }
        __syncthreads();
        if ((uint32_t)cb + lane < ce) {
            const uint32_t rows = n - row0 < 64 ? n - row0 : 64;
            for (uint32_t r = 0; r < rows; r++) out[(size_t)(row0 + r) * n + cb + lane] = tile[r * 65 + lane];
        }
        __syncthreads();
    }
}
void launch_lagrange_rows(const uint32_t* xs, const uint32_t* z, const uint32_t* w, size_t n, uint32_t* out,
                          uint32_t* tmp, hipStream_t s) {
    if (!n) return;
    const uint32_t S = lagrange_segments(n);
    if (S > 1)
        hipLaunchKernelGGL(k_lagrange_parts, dim3((unsigned)((n + 255) / 256), S - 1), dim3(256), 0, s, xs, z,
                           (uint32_t)n, tmp);
    hipLaunchKernelGGL(k_lagrange_rows, dim3((unsigned)((n + 63) / 64), S), dim3(64), 0, s, xs, z, w, (uint32_t)n, tmp,
                       out);
}

// ============================ multipoint evaluation and interpolation ==
// fri_evaluate_ex / fri_interpolate_points_ex on the retained product tree
// (fri_multipoint.hip).  Evaluation goes down the tree with
// the vector a_S of a node S (|S| = m words; the coefficients of x^-m..x^-1
// of f / M_S, lowest power first), interpolation comes up with F_S =
// sum_{i in S} c_i M_S / (x - x_i).  Both are cyclic products of size m with
// the children's nodes, whose leading 1 is x^(m/2) = (-1)^k in the transform
// domain, as in k_roots_pointwise:
//   down   a_L = (M_R * a_S)[m/2..m),  a_R = (M_L * a_S)[m/2..m)
//   up     F_S = F_L M_R + F_R M_L
// a and F are canonical, the tree's nodes Montgomery, so each product of one
// of each comes out canonical; `scale` is Montgomery(m^-1).

// g = F^-1 mod x^cnt for a series with F[0] = 1 (cnt <= 64, F of lf words):
// the recurrence g_i = -sum_{j=1..i} F_j g_(i-j) on one lane, the seed of the
// Newton steps (which would each be four launches on a handful of words).
__global__ void k_mp_series_seed(const uint32_t* __restrict__ F, uint32_t lf, uint32_t cnt, uint32_t* __restrict__ g) {
    __shared__ uint32_t gm[64];
    if (threadIdx.x) return;
    gm[0] = R_MOD_P;
    g[0] = 1u;
    for (uint32_t i = 1; i < cnt; i++) {
        uint32_t acc = 0;
        for (uint32_t j = 1; j <= i && j < lf; j++) acc = add(acc, mmul(F[j], gm[i - j]));
        g[i] = neg(acc);
        gm[i] = to_mont(neg(acc));
    }
}
void launch_mp_series_seed(const uint32_t* F, size_t lf, uint32_t cnt, uint32_t* g, hipStream_t s) {
    hipLaunchKernelGGL(k_mp_series_seed, dim3(1), dim3(64), 0, s, F, (uint32_t)(lf < 64 ? lf : 64), cnt, g);
}

// out[j] = (j + 1) z[j + 1], j < n: the derivative of the monic Z of degree n
// given by its n low coefficients (z[n] = 1 implied).
__global__ __launch_bounds__(256) void k_mp_derivative(const uint32_t* __restrict__ z, size_t n,
                                                       uint32_t* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride)
        out[j] = mmul(to_mont((uint32_t)(j + 1)), j + 1 < n ? z[j + 1] : 1u);
}
void launch_mp_derivative(const uint32_t* z, size_t n, uint32_t* out, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_mp_derivative, dim3(poly_blocks(n)), dim3(256), 0, s, z, n, out);
}

// Leaf subtrees, evaluation: node S of the leaf level (m = 2^log_leaf points)
// and its a_S give f(x_i) = sum_u q_i[u] a_S[m-1-u], q_i = M_S / (x - x_i) by
// the synthetic-division chain of k_lagrange_rows (q[m-1] = 1, q[u-1] =
// M_S[u] + x_i q[u]).  One lane per point; M_S and a_S are staged in LDS and
// every lane of a wave reads the same word of each per step (broadcasts).
// `canon`: the level is the tree's top (one leaf subtree) and holds canonical
// coefficients.
__global__ __launch_bounds__(256) void k_mp_leaf_eval(const uint32_t* __restrict__ xs, size_t count,
                                                      const uint32_t* __restrict__ node, uint32_t canon,
                                                      const uint32_t* __restrict__ a, uint32_t log_leaf,
                                                      uint32_t* __restrict__ out) {
    __shared__ uint32_t Ms[1u << ROOTS_LEAF_LOG_MAX], As[1u << ROOTS_LEAF_LOG_MAX];
    const uint32_t m = 1u << log_leaf, tid = threadIdx.x;
    const size_t p0 = (size_t)blockIdx.x * blockDim.x, n0 = (p0 >> log_leaf) << log_leaf;
    for (uint32_t u = tid; u < m; u += blockDim.x) {
        const uint32_t v = node[n0 + u];
        Ms[u] = canon ? to_mont(v) : v;
        As[u] = a[n0 + u];
    }
    __syncthreads();
    const size_t i = p0 + tid;
    if (i >= count || i >= n0 + m) return;
    const uint32_t xm = to_mont(xs[i]);
    uint32_t q = R_MOD_P, acc = 0;
    for (uint32_t u = m; u-- > 0;) {
        acc = add(acc, mmul(q, As[m - 1 - u]));
        q = add(Ms[u], mmul(q, xm));
    }
    out[i] = acc;
}
void launch_mp_leaf_eval(const uint32_t* xs, size_t count, const uint32_t* node, bool canon, const uint32_t* a,
                         uint32_t log_np, uint32_t log_leaf, uint32_t* out, hipStream_t s) {
    const uint32_t L = 1u << log_leaf, tpb = L < 64 ? 64 : L > 256 ? 256 : L;
    const size_t np = (size_t)1 << log_np;
    hipLaunchKernelGGL(k_mp_leaf_eval, dim3((unsigned)((np + tpb - 1) / tpb)), dim3(tpb), 0, s, xs, count, node,
                       canon ? 1u : 0u, a, log_leaf, out);
}

// Leaf subtrees, interpolation: the leaf kernel of the product tree with F
// carried along (leaf_subtree<true>): level 0 is M_i = x - x_i, F_i = c_i.
__global__ __launch_bounds__(256) void k_mp_leaf_up(const uint32_t* __restrict__ xs, const uint32_t* __restrict__ c,
                                                    size_t n, uint32_t log_leaf, uint32_t* __restrict__ out) {
    leaf_subtree<true>(xs, c, n, log_leaf, 0u, out);
}
void launch_mp_leaf_up(const uint32_t* xs, const uint32_t* c, size_t n, uint32_t log_np, uint32_t log_leaf,
                       uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_mp_leaf_up, dim3(1u << (log_np - log_leaf)), dim3(leaf_threads(log_leaf)), 0, s, xs, c, n,
                       log_leaf, out);
}

// One level in LDS, products of 2^lg <= 2^ROOTS_LDS_LOG_MAX words, on
// k_roots_level's tile scheme (a tile of the level is one batched transform).
// Down: the transform of a_S (all 2^lg words), the two children's, the two
// middle products, two inverse transforms of which the upper halves are
// kept: a_L beside a_R, the layout of the tree's level below.  Its loops over
// the two arrays and the two register tiles stay spelled out: written through
// tile_stages, tile_regs and tile_scatter, as its two neighbours are, this
// kernel cost the evaluation 3-6 us per call at 2^12..2^14 points
// (profiles/poly_refactor_ab.txt).
__global__ __launch_bounds__(256) void k_mp_down_level(const uint32_t* __restrict__ a_in,
                                                       const uint32_t* __restrict__ nodes, uint32_t* __restrict__ a_out,
                                                       uint32_t tile, uint32_t lg, const uint32_t* __restrict__ tw_f,
                                                       const uint32_t* __restrict__ tw_i, uint32_t scale) {
    __shared__ uint32_t A[1u << ROOTS_LDS_LOG_MAX], B[1u << ROOTS_LDS_LOG_MAX];
    const uint32_t tid = threadIdx.x, h = 1u << (lg - 1), mask = 2 * h - 1;
    const size_t base = (size_t)blockIdx.x * tile;
    for (uint32_t e = tid; e < tile; e += 256) A[(e & ~mask) + (__brev(e & mask) >> (32 - lg))] = a_in[base + e];
    tile_load_child(B, nodes + base, tile, lg, 1);
    __syncthreads();
    tile_stage(A, tile, 0, tw_f);
    for (uint32_t s = 1; s < lg; s++) {
        __syncthreads();
        tile_stage(A, tile, s, tw_f);
        tile_stage(B, tile, s, tw_f);
    }
    __syncthreads();
    uint32_t pl[TILE_REGS], pr[TILE_REGS];
#pragma unroll
    for (uint32_t k = 0; k < TILE_REGS; k++) {
        const uint32_t e = k * 256 + tid;
        if (e >= tile) continue;
        pl[k] = mmul(mul_monic(A[e], B[e], monic_sign(e)), scale);   // a_S (M_R)
    }
    __syncthreads();
    tile_load_child(B, nodes + base, tile, lg, 0);
    for (uint32_t s = 1; s < lg; s++) {
        __syncthreads();
        tile_stage(B, tile, s, tw_f);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < TILE_REGS; k++) {
        const uint32_t e = k * 256 + tid;
        if (e >= tile) continue;
        pr[k] = mmul(mul_monic(A[e], B[e], monic_sign(e)), scale);   // a_S (M_L)
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < TILE_REGS; k++) {
        const uint32_t e = k * 256 + tid;
        if (e >= tile) continue;
        const uint32_t pos = (e & ~mask) + (__brev(e & mask) >> (32 - lg));
        A[pos] = pl[k];
        B[pos] = pr[k];
    }
    for (uint32_t s = 0; s < lg; s++) {
        __syncthreads();
        tile_stage(A, tile, s, tw_i);
        tile_stage(B, tile, s, tw_i);
    }
    __syncthreads();
    for (uint32_t e = tid; e < tile; e += 256) {
        const uint32_t r = e & mask;
        a_out[base + e] = r < h ? A[e + h] : B[e];
    }
}
void launch_mp_down_level_lds(const uint32_t* a_in, const uint32_t* nodes, uint32_t* a_out, uint32_t log_np,
                              uint32_t lg, const uint32_t* tw_fwd, const uint32_t* tw_inv, hipStream_t s) {
    const uint32_t tile = level_tile(log_np);
    hipLaunchKernelGGL(k_mp_down_level, dim3((unsigned)(((size_t)1 << log_np) / tile)), dim3(256), 0, s, a_in, nodes,
                       a_out, tile, lg, tw_fwd, tw_inv, level_scale(lg));
}
// Up: F_L with M_R, then F_R with M_L through the same two arrays, the sum
// held in registers between them; one inverse transform.
__global__ __launch_bounds__(256) void k_mp_up_level(const uint32_t* __restrict__ f_in,
                                                     const uint32_t* __restrict__ nodes, uint32_t* __restrict__ f_out,
                                                     uint32_t tile, uint32_t lg, const uint32_t* __restrict__ tw_f,
                                                     const uint32_t* __restrict__ tw_i, uint32_t scale) {
    __shared__ uint32_t A[1u << ROOTS_LDS_LOG_MAX], B[1u << ROOTS_LDS_LOG_MAX];
    const size_t base = (size_t)blockIdx.x * tile;
    uint32_t r[TILE_REGS];
    for (uint32_t side = 0; side < 2; side++) {
        if (side) __syncthreads();
        tile_load_child(A, f_in + base, tile, lg, side);
        tile_load_child(B, nodes + base, tile, lg, side ^ 1u);
        tile_stages(tile, 1, lg, tw_f, A, B);
        __syncthreads();
        tile_regs(tile, [&](uint32_t k, uint32_t e) {
            const uint32_t t = mul_monic(A[e], B[e], monic_sign(e));
            r[k] = side ? mmul(add(r[k], t), scale) : t;
        });
    }
    __syncthreads();
    tile_scatter(A, r, tile, lg);
    tile_stages(tile, 0, lg, tw_i, A);
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < tile; e += 256) f_out[base + e] = A[e];
}
void launch_mp_up_level_lds(const uint32_t* f_in, const uint32_t* nodes, uint32_t* f_out, uint32_t log_np, uint32_t lg,
                            const uint32_t* tw_fwd, const uint32_t* tw_inv, hipStream_t s) {
    const uint32_t tile = level_tile(log_np);
    hipLaunchKernelGGL(k_mp_up_level, dim3((unsigned)(((size_t)1 << log_np) / tile)), dim3(256), 0, s, f_in, nodes,
                       f_out, tile, lg, tw_fwd, tw_inv, level_scale(lg));
}

// Larger levels: batched NTT passes around these pointwise kernels
// (monic_pointwise).  Down reads the parents' transform ta and the children's
// tl, tr and leaves ta (M_R) over tr and ta (M_L) over tl; the upper halves of
// their inverse transforms are the children's vectors, and k_mp_take_high
// moves a_L's to its place beside a_R.
__global__ __launch_bounds__(256) void k_mp_down_pointwise(const uint4* __restrict__ ta, uint4* tl, uint4* tr,
                                                           size_t n4, uint32_t scale) {
    monic_pointwise<3, 2>({ta, tl, tr}, {tl, tr}, n4, [&](const uint32_t (&x)[3], uint32_t sg, uint32_t (&y)[2]) {
        y[0] = mmul(mul_monic(x[0], x[1], sg), scale);
        y[1] = mmul(mul_monic(x[0], x[2], sg), scale);
    });
}
void launch_mp_down_pointwise(const uint32_t* ta, uint32_t* tl, uint32_t* tr, size_t words, uint32_t lg,
                              hipStream_t s) {
    hipLaunchKernelGGL(k_mp_down_pointwise, dim3(poly_blocks(words / 4)), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(ta), reinterpret_cast<uint4*>(tl), reinterpret_cast<uint4*>(tr),
                       words / 4, level_scale(lg));
}
__global__ __launch_bounds__(256) void k_mp_take_high(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n4,
                                                      uint32_t lg4) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, h4 = (size_t)1 << (lg4 - 1);
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4 / 2; e += stride) {
        const size_t o = ((e >> (lg4 - 1)) << lg4) + (e & (h4 - 1));
        dst[o] = src[o + h4];
    }
}
void launch_mp_take_high(const uint32_t* src, uint32_t* dst, size_t words, uint32_t lg, hipStream_t s) {
    hipLaunchKernelGGL(k_mp_take_high, dim3(poly_blocks(words / 8)), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), words / 4, lg - 2);
}
// Up: out = (fl (br + s) + fr (bl + s)) / 2^lg; out may be fl.
__global__ __launch_bounds__(256) void k_mp_up_pointwise(const uint4* fl, const uint4* __restrict__ fr,
                                                         const uint4* __restrict__ bl, const uint4* __restrict__ br,
                                                         uint4* out, size_t n4, uint32_t scale) {
    monic_pointwise<4, 1>({fl, fr, bl, br}, {out}, n4, [&](const uint32_t (&x)[4], uint32_t sg, uint32_t (&y)[1]) {
        y[0] = mmul(add(mul_monic(x[0], x[3], sg), mul_monic(x[1], x[2], sg)), scale);
    });
}
void launch_mp_up_pointwise(const uint32_t* fl, const uint32_t* fr, const uint32_t* bl, const uint32_t* br,
                            uint32_t* out, size_t words, uint32_t lg, hipStream_t s) {
    hipLaunchKernelGGL(k_mp_up_pointwise, dim3(poly_blocks(words / 4)), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(fl), reinterpret_cast<const uint4*>(fr),
                       reinterpret_cast<const uint4*>(bl), reinterpret_cast<const uint4*>(br),
                       reinterpret_cast<uint4*>(out), words / 4, level_scale(lg));
}

}  // namespace fri
