// fri_batch_kernels.hip — the batched commit's kernels on gfx950, one
// workgroup per member: the members' LDE and coset interpolation
// (k_batch_scale, k_batch_lde_lds, k_batch_intt_lds), their FRI commits
// (k_commit_batch) and their trace trees (k_trace_trees_batch), the last two
// built from the per-layer helpers of fri_tree_device.hpp.
#include <cassert>
#include "fri_tree_device.hpp"

namespace fri {

// ------------------------------------------------------------ batch ----
// fri_commit_batch: member blockIdx.x's whole commit in ONE workgroup of ONE
// launch: k_tree_tail generalised to start at layer 0 of a codeword of up to
// 2^BATCH_MAX_LOG elements.  Per layer, as in the tail: fold, leaves, tree,
// coefficient fold, degree, channel step, beta; the loop ends (uniformly per
// workgroup) when the member's degree drops below 1, so members of one batch
// end at different layers.
//   L <= TAIL_LOG: the tail's LDS path (values and coefficients of the
//       previous layer in LDS, whole tree in one level loop).
//   L >  TAIL_LOG: tiles of 2^TAIL_LOG leaves: fold, store, hash, climb nine
//       levels in LDS; then the level loop runs over the 2^(L - TAIL_LOG) tile
//       roots.  Values, coefficients and digests of these layers go through
//       the member's own slots in HBM.
// Producer and consumer of every such word are this workgroup, so a
// workgroup barrier is the only synchronisation: nothing here waits for
// another workgroup (no flag, no atomic, no cooperative launch), whatever the
// batch size and however the workgroups are scheduled.
__global__ __launch_bounds__(512) void k_commit_batch(BatchTask bt) {
    constexpr uint32_t NMAX = 1u << TAIL_LOG;
    __shared__ uint4 lds[2 * NMAX + NMAX];
    __shared__ uint32_t vals[2][NMAX];         // this / previous layer's values (layers of <= NMAX)
    __shared__ uint32_t coefs[2][NMAX];        // this / previous round's polynomial (the same layers)
    __shared__ int32_t red[24];
    __shared__ uint32_t s_beta_m, s_active;      // hand_off
    __shared__ int32_t s_deg;
    __shared__ uint32_t s_fbeta[BATCH_MAX_LOG + 2];   // the test hook's betas by layer (chan_open)
    __shared__ SchedLds sl;
    sched_init(&sl);
    uint32_t ord = 0;                            // levels so far (schedule producer flag)
    const uint32_t tid = threadIdx.x;
    const bool chan_wave = tid >= 448;
    const size_t mb = blockIdx.x;
    DevState* st = bt.st + mb;
    uint32_t* layers = bt.layers + mb * bt.lay_stride;
    uint32_t* trees = bt.trees + mb * bt.tre_stride;
    const uint32_t* input = bt.coef_in + mb * bt.in_stride;
    uint32_t* cA = bt.coefA + mb * bt.coef_stride;
    uint32_t* cB = bt.coefB + mb * bt.coef_stride;
    auto cbuf = [&](int r) -> uint32_t* { return (r & 1) ? cA : cB; };   // poly_r, r >= 1 (fri::coef_buf)
    Chan ch;
    chan_open(ch, st, chan_wave, s_fbeta, (uint32_t)bt.rmax + 2, 0);
    uint32_t beta_m = 0u;
    int prev_deg = -1;
    const shaq::Role R = shaq::role_of(tid);
#pragma unroll 1
    for (int k = 0; k <= bt.rmax; k++) {
        const uint32_t L = bt.log_n - (uint32_t)k, N = 1u << L;
        LayerTask t{};                           // what the shared helpers read of it
        t.st = st;
        t.k = k;
        t.L = L;
        const bool big = L > TAIL_LOG;
        const bool prev_lds = k > 0 && L + 1 <= TAIL_LOG;    // layer k-1 ran the LDS path
        const uint32_t* xl = k ? bt.xinv + bt.xinv_off[k - 1] : nullptr;
        const uint32_t* prev = k ? layers + bt.layer_off[k - 1] : nullptr;
        uint32_t* values = layers + bt.layer_off[k];
        uint32_t* tr = trees + bt.tree_off[k];
        uint4* A = lds;
        uint4* B = lds + 2 * NMAX;
        // ---- coefficient fold of round k-1 (or the input scan at k == 0), all waves ----
        // poly_{k-1}: in LDS where layer k-1 folded it there, else the input or its HBM buffer
        uint32_t* cout = big ? cbuf(k) : coefs[k & 1];
        const uint32_t* cin = (k >= 2 && prev_lds) ? coefs[(k & 1) ^ 1] : (k == 1 ? input : cbuf(k - 1));
        if (k == 0) coef_scan(input, bt.d0, red, 0, blockDim.x);
        else coef_fold(false, nullptr, cin, cout, (uint32_t)(prev_deg + 1), beta_m, red, 0, blockDim.x);
        // ---- fold + leaves (+ the tiles' nine levels): the digests of level lvl0 in A ----
        uint32_t lvl0 = 0;
        if (big) {
            lvl0 = tiled_leaves(t, tr, lds, R, &sl, ord, [&](uint32_t i) {
                if (!k) return values[i];
                const uint32_t v = fold_one(prev[i], prev[i + N], xl[i], beta_m);
                values[i] = v;
                return v;
            });
        } else {
            folded_leaves(N, tr, A, k > 0, prev_lds, vals[(k & 1) ^ 1], prev, xl, beta_m, values, vals[k & 1]);
        }
        lds_barrier();
        // ---- degree of poly_k, uniform: is this the member's last layer? ----
        const Settled s = settle(k, red, 8, chan_wave, k == 0 ? input : cout);
        levels_and_channel(t, false, A, B, tr, lvl0, ch, chan_wave, s, R, &sl, ord);
        hand_off(t, s, ch, chan_wave, s_fbeta[k], A, s_beta_m, s_active, s_deg);
        // not lds_barrier(): the next layer's fold reads this layer's values
        // (and coefficients) from HBM, so vmcnt drains here
        __syncthreads();
        if (!s_active) break;                           // uniform
        beta_m = s_beta_m;
        prev_deg = s_deg;
    }
}

void launch_commit_batch(const BatchTask& bt, uint32_t batch, hipStream_t s) {
    assert(bt.log_n >= 1 && bt.log_n <= BATCH_MAX_LOG && bt.rmax <= (int)bt.log_n);
    hipLaunchKernelGGL(k_commit_batch, dim3(batch), dim3(512), 0, s, bt);
}

// The members' LDE.  Pointwise c_j * offset^j, for the batched transform
// (NttPlan::batch takes no pre-scale table) ...
__global__ __launch_bounds__(256) void k_batch_scale(const uint32_t* __restrict__ src, size_t src_stride,
                                                     uint32_t* __restrict__ dst, size_t dst_stride, size_t d,
                                                     const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    const uint32_t v = src[blockIdx.y * src_stride + j];
    dst[blockIdx.y * dst_stride + j] = mmul(mmul(v, hi[j >> POW_LO_LOG]), lo[j & ((1u << POW_LO_LOG) - 1)]);
}
void launch_batch_scale(const uint32_t* src, size_t src_stride, uint32_t* dst, size_t dst_stride, size_t d,
                        uint32_t batch, const uint32_t* lo, const uint32_t* hi, hipStream_t s) {
    if (!d) return;
    hipLaunchKernelGGL(k_batch_scale, dim3((unsigned)((d + 255) / 256), batch), dim3(256), 0, s, src, src_stride, dst,
                       dst_stride, d, lo, hi);
}

// ... and, for transforms of <= 2^BATCH_LDS_LDE_MAX_LOG points (below the
// batched transform's whole tiles), scale and a radix-2 DIT in LDS, one
// workgroup per member: bit-reversed load, stage s with tw[2^s + j]
// (launch_twiddles), natural-order canonical output into the member's layer 0.
__global__ __launch_bounds__(256) void k_batch_lde_lds(const uint32_t* __restrict__ src, size_t src_stride, uint32_t d,
                                                       uint32_t* __restrict__ layers, size_t lay_stride, uint32_t log_n,
                                                       const uint32_t* __restrict__ tw, const uint32_t* __restrict__ lo,
                                                       const uint32_t* __restrict__ hi) {
    __shared__ uint32_t a[1u << BATCH_LDS_LDE_MAX_LOG];
    const uint32_t n = 1u << log_n;
    const uint32_t* in = src + blockIdx.x * src_stride;
    uint32_t* out = layers + blockIdx.x * lay_stride;
    for (uint32_t j = threadIdx.x; j < n; j += 256) {
        uint32_t v = 0u;
        if (j < d) v = mmul(mmul(in[j], hi[j >> POW_LO_LOG]), lo[j & ((1u << POW_LO_LOG) - 1)]);
        a[__brev(j) >> (32 - log_n)] = v;
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = 0; s < log_n; s++) {
        const uint32_t half = 1u << s;
        for (uint32_t idx = threadIdx.x; idx < n / 2; idx += 256) {
            const uint32_t j = idx & (half - 1), p0 = ((idx >> s) << (s + 1)) + j;
            const uint32_t u = a[p0], w = mmul(a[p0 + half], tw[half + j]);
            a[p0] = add(u, w);
            a[p0 + half] = sub(u, w);
        }
        __syncthreads();
    }
    for (uint32_t j = threadIdx.x; j < n; j += 256) out[j] = a[j];
}
void launch_batch_lde_lds(const uint32_t* src, size_t src_stride, size_t d, uint32_t* layers, size_t lay_stride,
                          uint32_t log_n, uint32_t batch, const uint32_t* tw, const uint32_t* lo, const uint32_t* hi,
                          hipStream_t s) {
    assert(log_n >= 1 && log_n <= BATCH_LDS_LDE_MAX_LOG && d <= ((size_t)1 << log_n));
    hipLaunchKernelGGL(k_batch_lde_lds, dim3(batch), dim3(256), 0, s, src, src_stride, (uint32_t)d, layers, lay_stride,
                       log_n, tw, lo, hi);
}

// Its mirror image, the members' coset interpolation (fri_trace_commit_batch,
// fri_fibsq_composition_commit_batch): the same DIT with the inverse twiddles,
// then the post-scale t^j (lo / hi: launch_pow_table with the 1/n factor in
// hi) on the way out.  dst[b * dst_stride + j] = t^j sum_i src[b * src_stride + i] w^-ij.
__global__ __launch_bounds__(256) void k_batch_intt_lds(const uint32_t* __restrict__ src, size_t src_stride,
                                                        uint32_t* __restrict__ dst, size_t dst_stride, uint32_t log_n,
                                                        const uint32_t* __restrict__ tw, const uint32_t* __restrict__ lo,
                                                        const uint32_t* __restrict__ hi) {
    __shared__ uint32_t a[1u << BATCH_LDS_LDE_MAX_LOG];
    const uint32_t n = 1u << log_n;
    const uint32_t* in = src + blockIdx.x * src_stride;
    uint32_t* out = dst + blockIdx.x * dst_stride;
    for (uint32_t j = threadIdx.x; j < n; j += 256) a[__brev(j) >> (32 - log_n)] = in[j];
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = 0; s < log_n; s++) {
        const uint32_t half = 1u << s;
        for (uint32_t idx = threadIdx.x; idx < n / 2; idx += 256) {
            const uint32_t j = idx & (half - 1), p0 = ((idx >> s) << (s + 1)) + j;
            const uint32_t u = a[p0], w = mmul(a[p0 + half], tw[half + j]);
            a[p0] = add(u, w);
            a[p0 + half] = sub(u, w);
        }
        __syncthreads();
    }
    for (uint32_t j = threadIdx.x; j < n; j += 256)
        out[j] = mmul(mmul(a[j], hi[j >> POW_LO_LOG]), lo[j & ((1u << POW_LO_LOG) - 1)]);
}
void launch_batch_intt_lds(const uint32_t* src, size_t src_stride, uint32_t* dst, size_t dst_stride, uint32_t log_n,
                           uint32_t batch, const uint32_t* tw_inv, const uint32_t* lo, const uint32_t* hi,
                           hipStream_t s) {
    assert(log_n >= 1 && log_n <= BATCH_LDS_LDE_MAX_LOG);
    hipLaunchKernelGGL(k_batch_intt_lds, dim3(batch), dim3(256), 0, s, src, src_stride, dst, dst_stride, log_n, tw_inv,
                       lo, hi);
}

// The members' trace trees (fri_trace_commit_batch): k_commit_batch's layer 0
// without fold, coefficients or channel.  Member blockIdx.x hashes its 2^L LDE
// values and stores every level in its tree slice (level_offset(L, l), what
// k_trace_gather reads) and its root in roots[8 * member ..].  L <= TAIL_LOG:
// one level loop from the leaves; above, tiles of 2^TAIL_LOG leaves climb nine
// levels in LDS and the level loop runs over the tile roots.  As in
// k_commit_batch every word is produced and consumed by this workgroup.
__global__ __launch_bounds__(512) void k_trace_trees_batch(const uint32_t* __restrict__ lde, size_t lde_stride,
                                                           uint32_t* __restrict__ trees, size_t tre_stride, uint32_t L,
                                                           uint32_t* __restrict__ roots) {
    constexpr uint32_t NMAX = 1u << TAIL_LOG;
    __shared__ uint4 lds[2 * NMAX + NMAX];
    __shared__ SchedLds sl;
    sched_init(&sl);
    uint32_t ord = 0;
    const uint32_t tid = threadIdx.x;
    const size_t mb = blockIdx.x;
    const uint32_t* values = lde + mb * lde_stride;
    uint32_t* tr = trees + mb * tre_stride;
    if (tid >= 384 && tid < 448) kcache_touch_sha_tables();
    const shaq::Role R = shaq::role_of(tid);
    const uint32_t N = 1u << L;
    LayerTask t{};
    t.L = L;
    uint4* A = lds;
    uint4* B = lds + 2 * NMAX;
    uint32_t lvl0 = 0;
    if (L > TAIL_LOG) lvl0 = tiled_leaves(t, tr, lds, R, &sl, ord, [&](uint32_t i) { return values[i]; });
    else leaf_loop(N, tr, A, [&](uint32_t j, bool) { return values[j]; });
    lds_barrier();
    uint32_t cnt = N >> lvl0;
#pragma unroll 1
    for (uint32_t it = 0; it < L - lvl0; it++) {
        cnt >>= 1;
        level_step(t, false, it, A, B, tr + 8 * level_offset(L, lvl0 + 1 + it), cnt, R, &sl, ord++);
        lds_barrier();
        uint4* tmp = A; A = B; B = tmp;
    }
    if (tid == 0) {
        Dg root;
        dg_lds_load(A, root);
        dg_store(roots + 8 * mb, root);
    }
}
void launch_trace_trees_batch(const uint32_t* lde, size_t lde_stride, uint32_t* trees, size_t tre_stride, uint32_t L,
                              uint32_t batch, uint32_t* roots, hipStream_t s) {
    assert(L >= 1 && L <= BATCH_MAX_LOG);
    hipLaunchKernelGGL(k_trace_trees_batch, dim3(batch), dim3(512), 0, s, lde, lde_stride, trees, tre_stride, L, roots);
}

}  // namespace fri
