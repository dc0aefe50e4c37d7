// fri_internal.hpp — device state layout and kernel launchers shared by
// the kernel files (fri_kernels.hip, fri_poly_kernels.hip, fri_layer.hip, ...) and the host code of
// the C ABI (fri_host.hpp and the files it lists).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <functional>
#include "field.hpp"

namespace fri {

constexpr int MAXR = 32;            // == FRI_MAX_ROUNDS
constexpr uint32_t TOP_LOG = 9;         // single-workgroup tree top: <= 512 inputs
constexpr uint32_t TAIL_LOG = TOP_LOG;  // layers of <= 2^TAIL_LOG elements run in the fused tail
constexpr uint32_t POW_LO_LOG = 12;     // two-level power tables s^j = lo[j&4095]*hi[j>>12]

// Device-resident commit state (one per context).  Every per-round kernel
// reads its gate (active[r]) and operands (beta, degrees) from here, so the
// whole commit is a static launch sequence that a hipGraph can replay and
// that needs no host round trip between Fiat-Shamir rounds.
struct DevState {
    uint32_t chan[8];            // channel state digest (src/channel/channel.rs:19)
    uint32_t chan_has;           // 0 => state == ""
    uint32_t chan_pending;       // 1 => true state = sha256_hex(hex(chan)) (receive's rehash deferred)
    uint32_t n_layers;
    uint32_t n_rounds;
    uint32_t final_value;
    int32_t  final_degree;
    uint32_t status;             // 0 ok, else FRI_E* raised on device
    uint32_t forced;             // FRI_FLAG_FORCE_BETAS
    int32_t  deg0max;            // max nonzero index of the input coefficients
    uint32_t active[MAXR + 1];   // active[r]: fold round r runs (deg_r >= 1)
    int32_t  deg[MAXR + 1];      // degree of poly_k (reference degree field)
    int32_t  newmax[MAXR];       // per round: max j with folded c'_j != 0
    int32_t  evenmax[MAXR];      //            max j with c_{2j}   != 0
    int32_t  oddmax[MAXR];       //            max j with c_{2j+1} != 0
    uint32_t beta[MAXR];
    uint32_t beta_mont[MAXR];
    uint32_t forced_beta[MAXR];
    uint32_t roots[MAXR + 1][8];
#ifdef FRI_STAMPS
    uint64_t stamps[MAXR + 1][64];   // diagnostic build only: s_memrealtime (100 MHz) per phase
#endif
};

// Tree layout: layer with 2^L leaves stores levels 0..L contiguously,
// level l at digest offset 2^(L+1) - 2^(L+1-l) (8 words per digest).
__host__ __device__ inline size_t level_offset(uint32_t L, uint32_t l) {
    return ((size_t)2 << L) - ((size_t)2 << (L - l));
}
// What an authentication path takes at level l: the sibling of `leaf`'s
// ancestor there, in a tree of 2^D leaves; and its eight words stored as the
// big-endian bytes a path is sent as.
__device__ __forceinline__ const uint32_t* sibling_digest(const uint32_t* tree, uint32_t D, uint32_t l, uint64_t leaf) {
    return tree + 8 * (level_offset(D, l) + ((leaf >> l) ^ 1u));
}
__device__ __forceinline__ void store_digest_be(uint32_t* o, const uint32_t* d) {
#pragma unroll
    for (int w = 0; w < 8; w++) o[w] = __builtin_bswap32(d[w]);
}

// ---- launchers (fri_kernels.hip); all asynchronous on `s` ----------------
struct NttPlan {
    uint32_t log_n;              // transform size 2^log_n
    const uint32_t* tw;          // stage-packed Montgomery twiddles: tw[2^s + j] = w_{2^(s+1)}^j
    const uint32_t* pre_lo;      // optional input scale s^j (Montgomery, two-level)
    const uint32_t* pre_hi;
    const uint32_t* post_lo;     // optional output scale t^j (Montgomery, two-level)
    const uint32_t* post_hi;
    // Batch (the product tree's levels, fri_roots.hip): 0 or 1 is one
    // transform; else `batch` transforms in the same launches (grid y),
    // transform b reading src + b*src_stride (d words each) and writing
    // dst + b*dst_stride.  log_n >= 13 (whole tiles), strides multiples of 4
    // words, batch <= 65535, no pre/post tables (they are indexed per transform).
    uint32_t batch;
    size_t src_stride, dst_stride;
};
// dst[k] = post(k) * sum_{j<d} src[j]*pre(j)*w^(jk); src may alias nothing in dst.
void launch_ntt(const NttPlan& p, const uint32_t* src, size_t d, uint32_t* dst, hipStream_t s);

// tw[2^s + j] = Montgomery(w_{2^(s+1)}^{+-j}), s < log_max, j < 2^s (2^log_max entries)
void launch_twiddles(uint32_t* tw, uint32_t log_max, bool inverse, hipStream_t s);
void launch_pow_table(uint32_t* lo, uint32_t* hi, uint32_t log_n, uint32_t base_std,
                      uint32_t scale_std, hipStream_t s);
void launch_batch_inverse(const uint32_t* in, uint32_t* out, size_t n, int out_mont,
                          hipStream_t s);
void launch_coset_points(uint32_t* out, size_t count, uint32_t offset, uint32_t log_n,
                         hipStream_t s);
void launch_square_mont(const uint32_t* in, uint32_t* out, size_t count, hipStream_t s);
// Arbitrary-point interpolation (fri_interpolate_points): prod_{i!=j}(x_j - x_i)
// into acc; c_j = y_j * w_j (w Montgomery) in place over w; f(w_N^k) for k < N.
// tmp: interp_tmp_words(n, log_N) words of segment partials.
size_t interp_tmp_words(size_t n, uint32_t log_N);
void launch_interp_weights(const uint32_t* xs, size_t n, uint32_t* acc, uint32_t* tmp, hipStream_t s);
void launch_interp_coeffs(const uint32_t* ys, uint32_t* w_to_c, size_t n, hipStream_t s);
void launch_interp_eval(const uint32_t* xs, const uint32_t* c, size_t n, uint32_t log_N, uint32_t* f, uint32_t* tmp,
                        hipStream_t s);
// Horner at arbitrary points; with few points and many coefficients (tmp of
// evaluate_tmp_words(d, count) > 0 words) the coefficients are split over lanes.
size_t evaluate_tmp_words(size_t d, size_t count);
void launch_evaluate(const uint32_t* coeffs, size_t d, const uint32_t* xs, size_t count, uint32_t* out,
                     uint32_t* tmp, hipStream_t s);

// ---- launchers (fri_poly_kernels.hip): the polynomial layer ---------------
// Polynomial arithmetic (fri_poly.hip).  Pointwise on two transforms of n
// canonical values: out = a*b*R^-1, and the Newton step out = g*(2 - f*g)*R^-2
// (the caller's inverse transform scales by R or R^2, and N^-1); out may
// alias an operand.
void launch_poly_pointwise_mul(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, hipStream_t s);
void launch_poly_newton(const uint32_t* f, const uint32_t* g, uint32_t* out, size_t n, hipStream_t s);
// out[i] = sum_j sht[j]*lng[i - j], i < n_out, canonical; ls <= POLY_DIRECT_LIMIT
// (the short operand and the long operand's window are staged in LDS).
constexpr size_t POLY_DIRECT_LIMIT = 4096;   // == FRI_POLY_DIRECT_LIMIT
void launch_poly_conv_direct(const uint32_t* lng, size_t ll, const uint32_t* sht, size_t ls, uint32_t* out,
                             size_t n_out, hipStream_t s);
// dst[i] = src[top - i] for i < cnt (cnt <= top + 1), 0 for cnt <= i < n.
void launch_poly_reverse(const uint32_t* src, size_t top, size_t cnt, uint32_t* dst, size_t n, hipStream_t s);
// r[i] = a[i] - t[i], i < n.
void launch_poly_sub(const uint32_t* a, const uint32_t* t, uint32_t* r, size_t n, hipStream_t s);
// Product tree and Lagrange rows (fri_roots.hip).  A level is 2^log_np words:
// its monic nodes' low coefficients (Montgomery), side by side.
// leaf: out = the level of nodes of degree 2^log_leaf (<= 2^ROOTS_LEAF_LOG_MAX)
// over roots[0..n) padded with zero roots; canon: canonical output (the top).
constexpr uint32_t ROOTS_LEAF_LOG_MAX = 11;
void launch_roots_leaf(const uint32_t* roots, size_t n, uint32_t log_np, uint32_t log_leaf, bool canon, uint32_t* out,
                       hipStream_t s);
// one level, products of 2^lg <= 2^ROOTS_LDS_LOG_MAX words (nodes of degree 2^(lg-1) in, 2^lg out), in LDS
constexpr uint32_t ROOTS_LDS_LOG_MAX = 12;
void launch_roots_level_lds(const uint32_t* in, uint32_t* out, uint32_t log_np, uint32_t lg, bool canon,
                            const uint32_t* tw_fwd, const uint32_t* tw_inv, hipStream_t s);
// out = ((a + s)(b + s) - 1) / 2^lg on `words` (a multiple of 4) transform values, s = (-1)^index
void launch_roots_pointwise(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t words, uint32_t lg, bool canon,
                            hipStream_t s);
// out[i*n + j] = w[i] * (Z / (x - xs[i]))[j], i, j < n; z: Z's n low coefficients (canonical, z_n = 1 implied),
// w Montgomery; tmp: lagrange_tmp_words(n) words.
size_t lagrange_tmp_words(size_t n);
void launch_lagrange_rows(const uint32_t* xs, const uint32_t* z, const uint32_t* w, size_t n, uint32_t* out,
                          uint32_t* tmp, hipStream_t s);
// Multipoint evaluation and interpolation on the retained tree
// (fri_multipoint.hip).  a and F levels are canonical, 2^log_np words laid out
// like the tree's levels; `nodes` is the tree's level below the products.
// g = F^-1 mod x^cnt (cnt <= 64) for a series of lf words with F[0] = 1
void launch_mp_series_seed(const uint32_t* F, size_t lf, uint32_t cnt, uint32_t* g, hipStream_t s);
// out[j] = (j + 1) z[j + 1], j < n (z[n] = 1 implied)
void launch_mp_derivative(const uint32_t* z, size_t n, uint32_t* out, hipStream_t s);
// out[i] = f(xs[i]), i < count, from the leaf level's nodes (canonical if canon) and vectors a
void launch_mp_leaf_eval(const uint32_t* xs, size_t count, const uint32_t* node, bool canon, const uint32_t* a,
                         uint32_t log_np, uint32_t log_leaf, uint32_t* out, hipStream_t s);
// out = the F level of the leaf subtrees over xs[0..n), c[0..n) (zero roots and c = 0 beyond n)
void launch_mp_leaf_up(const uint32_t* xs, const uint32_t* c, size_t n, uint32_t log_np, uint32_t log_leaf,
                       uint32_t* out, hipStream_t s);
// one level, products of 2^lg <= 2^ROOTS_LDS_LOG_MAX words: parents' a -> children's a; children's F -> parents' F
void launch_mp_down_level_lds(const uint32_t* a_in, const uint32_t* nodes, uint32_t* a_out, uint32_t log_np,
                              uint32_t lg, const uint32_t* tw_fwd, const uint32_t* tw_inv, hipStream_t s);
void launch_mp_up_level_lds(const uint32_t* f_in, const uint32_t* nodes, uint32_t* f_out, uint32_t log_np, uint32_t lg,
                            const uint32_t* tw_fwd, const uint32_t* tw_inv, hipStream_t s);
// larger levels, on transforms of `words` values: tr = ta (tr + s) / 2^lg, tl = ta (tl + s) / 2^lg;
// dst's low half of every 2^lg words = src's high half; out = (fl (br + s) + fr (bl + s)) / 2^lg
void launch_mp_down_pointwise(const uint32_t* ta, uint32_t* tl, uint32_t* tr, size_t words, uint32_t lg,
                              hipStream_t s);
void launch_mp_take_high(const uint32_t* src, uint32_t* dst, size_t words, uint32_t lg, hipStream_t s);
void launch_mp_up_pointwise(const uint32_t* fl, const uint32_t* fr, const uint32_t* bl, const uint32_t* br,
                            uint32_t* out, size_t words, uint32_t lg, hipStream_t s);

// ---- launchers (fri_kernels.hip): decommitment gather, standalone fold ----
struct DecommitPlan {
    uint64_t index;
    uint32_t log_n, n_layers;
    uint64_t layer_off[MAXR + 1];
    uint64_t tree_off[MAXR + 1];
    uint32_t path_off[MAXR + 1];   // word offset of layer k's two paths (16 * L_j per earlier layer)
    // Sharded layers (fri_decommit_query_sharded): layer k with shard_lb1[k] =
    // log2(block size) + 1 (0: an ordinary whole layer) is held block-wise: this rank writes an opening
    // only when it owns the opened element's block (owned[k], bit b), taking
    // the path's lower log2(block) levels from its block-local tree and the
    // top log G levels from the layer's top tree (top + top_off[k]); openings
    // of blocks it does not hold are written as zeros (the ranks' outputs are
    // then combined by a max-reduction).  val_block[k]: the value slot holds
    // only this rank's block (index i mod B), else the whole layer (index i).
    uint32_t logG;
    uint8_t shard_lb1[MAXR + 1];    // log2(block size) + 1; 0: an ordinary (whole) layer
    uint8_t val_block[MAXR + 1];
    uint64_t owned[MAXR + 1];
    uint64_t top_off[MAXR + 1];
};
void launch_decommit_gather(const uint32_t* layers, const uint32_t* trees, const DecommitPlan& dp, uint32_t* out,
                            hipStream_t s, const uint32_t* top = nullptr);
void launch_fold_plain(const uint32_t* in, uint32_t* out, uint32_t log_m, const uint32_t* xinv_m,
                       uint32_t beta, hipStream_t s);

// Sharded layer k (run_commit_sharded), device-resident per layer: what
// the block top and the replicated top kernels of a coset-sharded layer read
// besides their LayerTask (k_tree_top<..., SHARD>, fri_layer.hip).
constexpr uint32_t REC_WORDS = 16;   // per-rank record: root (8), m0, m1, m2, first coefficient, 0 x 4
struct ShardTop {
    // block top (this rank): the record it writes
    uint32_t* rec_out;
    const int32_t* rec_mx;     // rec_R workgroup maxima triples of this rank's coefficient task
    const uint32_t* rec_c0;    // this rank's first coefficient of poly_k
    uint32_t rec_R;
    // replicated top: the G all-gathered records (rank order)
    uint32_t G;
    const uint32_t* recs_in;
    int32_t sched_deg;         // loopback rehearsal (sched_on): the recorded degree of this layer
    uint32_t sched_on;
    uint8_t rank_of_block[64]; // block b's root is in the record of rank rank_of_block[b]
};

// One FRI layer (fri_layer.hip): optional fold of the previous layer, leaf
// hashes, every tree level, and (commit mode, st != nullptr) the coefficient
// fold slice, degree resolution and Fiat-Shamir step of layer k.
struct LayerTask {
    const uint32_t* prev;      // layer k-1 values (fold) or nullptr
    const uint32_t* xinv;      // Montgomery (x_i)^-1 of layer k-1's domain, i < 2^L
    uint32_t* values;          // layer k values (written when folding)
    uint32_t* tree;            // layer k tree: levels 0..L (level_offset)
    uint32_t L;                // log2 |layer k|
    int k;                     // layer index (commit mode)
    uint32_t beta_m;           // Montgomery beta for a standalone fold (no state)
    const uint32_t* coef_in;   // k == 0: input coefficients; else poly_{k-1}
    uint32_t* coef_out;        // poly_k coefficients (k >= 1)
    size_t d0;                 // k == 0: input length
    int32_t* wgmax;            // [3 * workgroups] coefficient maxima
    DevState* st;              // nullptr: standalone Merkle tree (no degree / channel)
    const DevState* gst;       // gate for standalone trees inside a commit (sharded
    int gidx;                  //   layers): skip when !gst->active[gidx]
    // Sharded coefficient fold (run_commit_sharded, k_coef only): this rank
    // handles the coefficients j in [jlo, jhi) of poly_k (jhi == 0: all of
    // them); coef_in[0] holds global coefficient ibase of poly_{k-1} (of the
    // input at k == 0), coef_out[0] global coefficient obase of poly_k.
    size_t jlo, jhi, ibase, obase;
    const ShardTop* shard;     // sharded layer (device): nullptr otherwise
    // Sharded block tree with the pair fold fused in (run_commit_sharded):
    // the fold's second operand is prev2[i] (the partner's half-block)
    // instead of prev[i + 2^L]; beta is gst->beta_mont[gidx].  The leaf
    // kernel then runs as two launches, the half-block the next exchange
    // sends (send_half: 0 first half, 1 second half) first.
    const uint32_t* prev2;
    uint32_t send_half;
    uint32_t wg_base;          // (set per launch) first workgroup of a split launch
    uint32_t wg_total;         // (set per launch) workgroups of the whole layer
};
// after_leaf: called right after the leaf kernel is enqueued (and
// ev_leaf_end recorded), so the caller can start work on another stream
// behind it; ev_before_top: the stream waits for it before the top kernel
// (a sharded block top reads the coefficient maxima made on that stream).
// after_part1 (a fused sharded layer, t.prev2 set): called right after the
// leaf launch of the half-block the next exchange sends, so the caller can
// enqueue that exchange while the other half is hashed.
void launch_layer(const LayerTask& t, hipStream_t s, hipEvent_t ev_leaf_end = nullptr,
                  const std::function<void()>& after_leaf = {}, hipEvent_t ev_before_top = nullptr,
                  const std::function<void()>& after_part1 = {});
// Layers ts[0..n) (consecutive, 2^L <= 2^TAIL_LOG elements, commit mode) in
// one single-workgroup launch (k_tree_tail), n <= TAIL_LOG + 1.
void launch_tail(const LayerTask* ts, uint32_t n, hipStream_t s);
// Coefficient task of layer t.k alone (grid G): k == 0 scans the input for
// deg_0, k >= 1 folds poly_{k-1} -> poly_k; maxima into t.wgmax[3*G].
void launch_coef(const LayerTask& t, uint32_t G, hipStream_t s);
// fri_dist_kernels.hip
void launch_coset_coeffs(const uint32_t* a, size_t d, uint32_t* out, size_t M, uint32_t c_std, hipStream_t s);
void launch_decimate(const uint32_t* a, size_t d, uint32_t* ev, uint32_t* od, hipStream_t s);
void launch_radix2_block(const uint32_t* E, const uint32_t* O, const uint32_t* tlo, const uint32_t* thi,
                         uint32_t* out, size_t M, uint32_t negate, hipStream_t s);
void launch_cyclic_to_block(const uint32_t* recv, uint32_t* block, size_t B, uint32_t G, hipStream_t s);
// layer[block_of[r] * B ..] = gath[r * B ..] for r < G (B a multiple of 4).
void launch_place_blocks(const uint32_t* gath, uint32_t* layer, size_t B, uint32_t G, const uint32_t* block_of,
                         hipStream_t s);
// In-process peer transport: dst[p * words ..] = src[p][0 .. words) for p < n
// (n <= 64 sources, each another rank's buffer); vec4: every pointer 16-byte
// aligned and words % 4 == 0.
struct PeerPull {
    const uint32_t* src[64];
    uint32_t* dst;
    size_t words;
    uint32_t n;
    uint32_t vec4;
};
void launch_peer_pull(const PeerPull& pp, hipStream_t s);
// *out = position-sensitive 64-bit checksum of v[0..n) (FRI_FLAG_RANK_INPUTS).
void launch_checksum(const uint32_t* v, size_t n, uint64_t* out, hipStream_t s);
// Loopback rehearsal: dst = G copies of src (words each), one launch.
void launch_replicate(const uint32_t* src, uint32_t* dst, size_t words, uint32_t G, hipStream_t s);
// Tree top + degree + channel step for a layer whose level `l` (2^(L-l)
// nodes, <= 512) is already in t.tree; mx/G: coefficient maxima.
void launch_top(const LayerTask& t, uint32_t l, const int32_t* mx, uint32_t G, hipStream_t s);

// Batched commit (fri_commit_batch; k_commit_batch, fri_batch_kernels.hip): `batch`
// independent commits of one shape, one 512-thread workgroup each.  Member b
// owns the slice b of every buffer (layers + b * lay_stride, ...), laid out
// inside like a one-GPU plan (layer_off / tree_off, in words); the x^-1 tables
// are shared (fold k reads xinv + xinv_off[k]).  st: one DevState per member.
constexpr uint32_t BATCH_MAX_LOG = 18;   // tiles of 2^9 leaves, <= 2^9 tile roots
constexpr uint32_t BATCH_LDS_LDE_MAX_LOG = 12;   // LDE in LDS up to here, NttPlan::batch above
struct BatchTask {
    uint32_t* layers;
    uint32_t* trees;
    uint32_t* coefA;           // poly_k of odd k (layers above 2^TAIL_LOG only: smaller ones stay in LDS)
    uint32_t* coefB;           // poly_k of even k >= 2
    const uint32_t* coef_in;   // member b's d0 input coefficients at coef_in + b * in_stride
    const uint32_t* xinv;
    DevState* st;
    size_t lay_stride, tre_stride, coef_stride, in_stride;
    uint32_t log_n, d0;
    int rmax;
    uint32_t layer_off[BATCH_MAX_LOG + 2], tree_off[BATCH_MAX_LOG + 2], xinv_off[BATCH_MAX_LOG + 2];
};
void launch_commit_batch(const BatchTask& bt, uint32_t batch, hipStream_t s);
// LDE of every member, layer 0 := the member's coefficients on offset * <w_n>.
// dst[b * dst_stride + j] = src[b * src_stride + j] * offset^j, j < d (lo / hi: launch_pow_table)
void launch_batch_scale(const uint32_t* src, size_t src_stride, uint32_t* dst, size_t dst_stride, size_t d,
                        uint32_t batch, const uint32_t* lo, const uint32_t* hi, hipStream_t s);
// log_n <= BATCH_LDS_LDE_MAX_LOG: scale and transform in LDS, one workgroup per member
void launch_batch_lde_lds(const uint32_t* src, size_t src_stride, size_t d, uint32_t* layers, size_t lay_stride,
                          uint32_t log_n, uint32_t batch, const uint32_t* tw, const uint32_t* lo, const uint32_t* hi,
                          hipStream_t s);
// The inverse: dst[b * dst_stride + j] = t^j sum_i src[b * src_stride + i] w^-ij, j < 2^log_n, in LDS
// (log_n <= BATCH_LDS_LDE_MAX_LOG; tw_inv the inverse twiddles, lo / hi the post-scale table of t)
void launch_batch_intt_lds(const uint32_t* src, size_t src_stride, uint32_t* dst, size_t dst_stride, uint32_t log_n,
                           uint32_t batch, const uint32_t* tw_inv, const uint32_t* lo, const uint32_t* hi,
                           hipStream_t s);
// Merkle tree of every member's 2^L values (fri_trace_commit_batch), one 512-thread
// workgroup each: every level into trees + b * tre_stride (level_offset(L, l),
// tre_stride in words), the root's 8 words into roots + 8 * b.
void launch_trace_trees_batch(const uint32_t* lde, size_t lde_stride, uint32_t* trees, size_t tre_stride, uint32_t L,
                              uint32_t batch, uint32_t* roots, hipStream_t s);

// fri_prover.hip — STARK-101 FibonacciSq composition on the LDE coset.
constexpr uint32_t FIBSQ_MAX_B = 16;   // blowup <= 2^4
struct FibsqParams {
    uint32_t log_n;              // LDE size n = B * T
    uint32_t B;                  // blowup (power of two, 2..16): g = w_n^B
    uint32_t offset_m;           // Montgomery(offset)
    uint32_t w_m, winv_m;        // Montgomery(w_n^{+-1})
    uint32_t glast_m, gprev_m;   // Montgomery(g^{T-1}), Montgomery(g^{T-2})
    uint32_t a_last;             // canonical a_{T-1}
    uint32_t alpha_m[3];         // Montgomery(alpha_0..2)
    uint32_t zinv_m[FIBSQ_MAX_B];// Montgomery((offset^T w_B^j - 1)^-1), j < B
};
void launch_fibsq_cp(const uint32_t* f_lde, uint32_t* out, const FibsqParams& q, hipStream_t s);
// The batch: trace b's LDE at f_lde + b * f_stride, its CP at out + b * out_stride,
// its constants in mem[b] (device); q carries the shape (its alpha_m / a_last are not read).
struct FibsqMember {
    uint32_t alpha_m[3];         // Montgomery(alpha_0..2)
    uint32_t a_last;             // canonical a_{T-1}
};
void launch_fibsq_cp_batch(const uint32_t* f_lde, size_t f_stride, uint32_t* out, size_t out_stride,
                           const FibsqMember* mem, uint32_t batch, const FibsqParams& q, hipStream_t s);
// out[j] = lde[(index + j*stride) mod 2^L], then count paths of L big-endian digests
void launch_trace_gather(const uint32_t* lde, const uint32_t* tree, uint32_t L, uint64_t index, uint64_t stride,
                         uint32_t count, uint32_t* out, hipStream_t s);
// The queries of `members` members of the resident batch, from member `first`
// on.  fri_batch_query_phase: k_query_chain draws every index from the member's
// channel and absorbs the openings from the resident buffers
// (launch_query_chain), then k_batch_query_all gathers the records
// (launch_query_gather), both on `s`.  fri_batch_query_round: the gather alone,
// of one query whose indices the host uploaded.  The per-member arrays are the
// chunk's (member first + m at m); n_layers[m] = 0 leaves a member out.
struct QueryPhase {
    const uint32_t* layers;      // the FRI batch (BatchTask's slices and offsets)
    const uint32_t* trees;
    size_t lay_stride, tre_stride;
    const uint32_t* tlde;        // the trace batch (trace_count > 0)
    const uint32_t* ttree;
    size_t tlde_stride, ttree_stride;
    const uint32_t* n_layers;    // [members]
    uint32_t* chan;              // [members] fri_channel_state, 9 words: in, and out after the last send
    uint64_t* indices;           // [members][num_queries]: the chain's output, the gather's input
    uint32_t* out;               // [members][num_queries] records of rec_words words (k_batch_query_all has the layout)
    size_t rec_words;
    uint64_t trace_stride;
    uint64_t range;              // max_index + 1, <= 2^32
    uint32_t first, members, num_queries;
    uint32_t log_n, trace_count, max_layers;
    uint32_t layer_off[BATCH_MAX_LOG + 2], tree_off[BATCH_MAX_LOG + 2];
};
void launch_query_chain(const QueryPhase& q, hipStream_t s);
void launch_query_gather(const QueryPhase& q, hipStream_t s);

// Proof-of-work grinding (fri_grind, fri_grind_batch): the
// smallest nonce whose send leaves the channel state with leading zero bits.
// A member's record is what every candidate shares: the SHA-256 state before
// the nonce's block (the midstate after the state's 64 hex characters, or the
// IV for an empty state) and the message length in bits (640 or 128).
struct GrindMember {
    uint32_t mid[8];
    uint32_t len_bits;
};
// One window of consecutive nonces hi * 2^32 + lo0 + i, i <= last_idx, that
// does not cross a multiple of 2^32, searched for every member j < n_active
// (member active[j], or j itself when active is null).  best[m] takes the
// smallest i whose digest word 0 has no bit of `mask` set (64-bit atomic min;
// ~0 = none so far); the members that found one get their channel state after
// the send in chan[m] (9 words, fri_channel_state).
struct GrindTask {
    const GrindMember* mem;
    unsigned long long* best;
    const uint32_t* active;
    uint32_t* chan;
    uint32_t hi, lo0, last_idx;
    uint32_t rows;               // ceil(((lo0 & 63) + last_idx + 1) / 64): the window in rows of one nonce per lane
    uint32_t mask;
    uint32_t n_active;
};
// chan: `members` channel states; fills mem and sets best to ~0
void launch_grind_prep(const uint32_t* chan, GrindMember* mem, unsigned long long* best, uint32_t members,
                       hipStream_t s);
void launch_grind(const GrindTask& q, hipStream_t s);

// fri_verify_kernels.hip — the batched verifier (fri_verify_batch_pow): `members`
// transcripts of one shape, packed as fri_amd.h describes, in device memory
// with compact strides.  Both kernels OR what they find into verdict[b]
// (FRI_VERIFY_* bits); neither reads what the other writes.
constexpr uint32_t VERIFY_MAX_LOG = 30;
enum : uint32_t {                // FRI_VERIFY_* of fri_amd.h (fri_verify.hip asserts they agree)
    VB_CHANNEL = 1, VB_TRACE_PATH = 2, VB_COMPOSITION = 4, VB_FRI_PATH = 8, VB_FOLD = 16, VB_FINAL = 32,
    VB_MALFORMED = 64, VB_POW = 128
};
struct VerifyTask {
    const uint32_t* head;        // per member: [trace root 8, alphas 3] roots 8 * max_layers, betas, final
    const uint32_t* chan;        // per member: fri_channel_state, 9 words (digest bytes, has_state)
    const uint32_t* n_layers;    // per member, 1..max_layers
    const uint32_t* a_last;      // per member (trace_count = 3)
    const uint64_t* indices;     // [member][query], claimed
    const uint32_t* values;      // [member][query] records of val_words words
    const uint32_t* paths;       // [member][query] records of path_words words (the bytes as they are sent)
    uint32_t* verdict;
    uint32_t head_words, val_words, path_words;
    uint32_t members, log_n, max_layers, num_queries, trace_count, log_t, log_blowup;
    uint64_t range;              // max_index + 1, <= 2^32
    uint32_t glast_m, gprev_m;   // Montgomery(g^{T-1}), Montgomery(g^{T-2}), g = w_T (trace_count = 3)
    // Montgomery(w_{2^(log_n-k)}) and Montgomery(offset^(2^k)): layer k lives on offset^(2^k) <w_{2^(log_n-k)}>
    uint32_t w_m[VERIFY_MAX_LOG + 1], off_m[VERIFY_MAX_LOG + 1];
    // the grinding nonce (fri_verify_batch_pow), behind everything else: the kernels without it keep their argument layout
    const uint64_t* nonces;      // per member (pow_bits > 0; not read otherwise)
    uint32_t pow_bits;           // grinding bits, 0..32: 0 = the transcripts carry no nonce
};
void launch_verify_chain(const VerifyTask& t, hipStream_t s);
void launch_verify_open(const VerifyTask& t, hipStream_t s);

}  // namespace fri
