// fri_roots.hip — src/polynomial/interpolation.rs on the device:
// gen_polynomial_from_roots (:9-23) and gen_lagrange_polynomials (:46-78,
// == gen_lagrange_polynomials_parallel, :80-115).  The reference multiplies
// the linear factors one after the other and divides Z by each (x - x_i) with
// div_rem; field arithmetic is exact, so a product tree and synthetic
// division give the same coefficients:
//   from_roots  leaf subtrees in LDS (k_roots_leaf), then one level per step:
//               products that fit LDS in one launch (k_roots_level), larger
//               ones as batched NTT passes around a pointwise kernel
//   lagrange    Z from the tree, the weights of fri_interpolate_points, one
//               row kernel (k_lagrange_rows)
// Everything is enqueued on ctx->stream with one synchronisation at the end.
#include "fri_host.hpp"

static_assert((FRI_ROOTS_LEAF & (FRI_ROOTS_LEAF - 1)) == 0 && FRI_ROOTS_LEAF >= 128 &&
                  FRI_ROOTS_LEAF <= (1 << ROOTS_LEAF_LOG_MAX),
              "FRI_ROOTS_LEAF: a power of two in 128..2048");

namespace fri {

uint32_t roots_leaf_log(const fri_ctx* ctx, bool small_leaf) {
    if (small_leaf) return 6;
    return ceil_log2(ctx->roots_leaf ? ctx->roots_leaf : FRI_ROOTS_LEAF);
}

// Enqueues the product tree over d_roots[0..n), n >= 1, padded with zero roots
// to 2^log_np = next_pow2(n) (<= 2^log_n_max); returns where the n low
// coefficients of Z will be (canonical; the padding's x^pad is skipped).  The
// levels move between the three context buffers; d_roots is read by the leaf
// kernel only and may be scratch_b or lie outside them.  With `keep`
// (fri_multipoint.hip) every level stays instead: the level of nodes of degree
// 2^lg at keep + (lg - lf_log) * 2^log_np, lf_log clamped to log_np, Montgomery
// but for the canonical top; scratch_a and scratch_b are still work space.
const uint32_t* product_tree(fri_ctx* ctx, const uint32_t* d_roots, size_t n, uint32_t lf_log, uint32_t* keep) {
    hipStream_t s = ctx->stream;
    const uint32_t log_np = ceil_log2(n);
    const size_t np = (size_t)1 << log_np;
    if (lf_log > log_np) lf_log = log_np;
    uint32_t *cur = keep ? keep : ctx->scratch_c, *x = ctx->scratch_a, *y = ctx->scratch_b;
    launch_roots_leaf(d_roots, n, log_np, lf_log, lf_log == log_np, cur, s);
    for (uint32_t lg = lf_log + 1; lg <= log_np; lg++) {            // nodes of 2^(lg-1) words -> 2^lg
        const bool top = lg == log_np;
        uint32_t* kept = keep ? keep + (size_t)(lg - lf_log) * np : nullptr;
        if (lg <= ROOTS_LDS_LOG_MAX) {
            launch_roots_level_lds(cur, keep ? kept : x, log_np, lg, top, ctx->tw_fwd, ctx->tw_inv, s);
            if (keep) cur = kept;
            else std::swap(cur, x);
            continue;
        }
        // even nodes -> x, odd nodes -> y, each zero-padded to 2^lg and
        // transformed; the product's inverse transform lands in cur again.
        const size_t two_m = (size_t)1 << lg, m = two_m >> 1;
        batched_ntt(ctx, lg, false, cur, m, x, np);
        batched_ntt(ctx, lg, false, cur + m, m, y, np);
        launch_roots_pointwise(x, y, x, np, lg, top, s);
        if (keep) cur = kept;
        batched_ntt(ctx, lg, true, x, two_m, cur, np);
    }
    return cur + (np - n);
}

}  // namespace fri

extern "C" int fri_debug_set_roots_leaf(fri_ctx* ctx, uint32_t leaf) {
    if (!ctx) return FRI_EINVAL;
    if (leaf && ((leaf & (leaf - 1)) || leaf < 64 || leaf > (1u << ROOTS_LEAF_LOG_MAX)))
        return fail(ctx, FRI_EINVAL, "roots per leaf subtree: a power of two in 64..2048, or 0");
    ctx->roots_leaf = leaf;
    return FRI_OK;
}

extern "C" int fri_poly_from_roots(fri_ctx* ctx, const uint32_t* roots, size_t n, uint32_t flags, uint32_t* out,
                                   size_t out_cap, size_t* len_out) {
    if (!ctx || !len_out || (n && !roots)) return fail(ctx, FRI_EINVAL, "null argument");
    if (flags & ~FRI_ROOTS_SMALL_LEAF) return fail(ctx, FRI_EINVAL, "flags: 0 or FRI_ROOTS_SMALL_LEAF");
    if (!check_canonical(roots, n)) return fail(ctx, FRI_EINVAL, "root not canonical (>= p)");
    *len_out = 0;
    if (n == 0) return FRI_OK;                                     // Polynomial::zero() (interpolation.rs:10-12)
    if (n > ((size_t)1 << ctx->log_n_max))
        return fail(ctx, FRI_EINVAL, "root count exceeds context capacity (next_pow2(n) <= 2^log_n_max)");
    *len_out = n + 1;
    if (out_cap < n + 1 || !out) return fail(ctx, FRI_EINVAL, "output capacity too small (needed length in *len_out)");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_b, roots, n * 4, hipMemcpyHostToDevice, s));
    const uint32_t* z = product_tree(ctx, ctx->scratch_b, n, roots_leaf_log(ctx, flags & FRI_ROOTS_SMALL_LEAF));
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipMemcpyAsync(out, z, n * 4, hipMemcpyDeviceToHost, s));
    FRI_HIP(ctx, hipStreamSynchronize(s));
    out[n] = 1u;                                                   // monic: never trims
    return FRI_OK;
}

extern "C" int fri_lagrange_basis(fri_ctx* ctx, const uint32_t* xs, size_t n, uint32_t* out, size_t out_cap) {
    if (!ctx || (n && (!xs || !out))) return fail(ctx, FRI_EINVAL, "null argument");
    if (n > FRI_LAGRANGE_MAX) return fail(ctx, FRI_EINVAL, "Lagrange basis: n <= FRI_LAGRANGE_MAX");
    if (n > ((size_t)1 << ctx->log_n_max))
        return fail(ctx, FRI_EINVAL, "point count exceeds context capacity (next_pow2(n) <= 2^log_n_max)");
    if (out_cap < n * n) return fail(ctx, FRI_EINVAL, "output capacity too small (n*n words)");
    if (!check_canonical(xs, n)) return fail(ctx, FRI_EINVAL, "value not canonical (>= p)");
    if (n == 0) return FRI_OK;
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // scratch: the n x n rows, the points, the weights' products and inverses,
    // the weight kernel's segment partials, the row kernel's segment values
    const size_t oM = 0, oX = oM + round4(n * n), oA = oX + round4(n), oW = oA + round4(n), oT = oW + round4(n),
                 oP = oT + round4(interp_tmp_words(n, 0)), end = oP + round4(lagrange_tmp_words(n));
    const int rc = ensure_tmp(ctx, end);
    if (rc) return rc;
    uint32_t* t = ctx->interp_tmp;
    FRI_HIP(ctx, hipMemcpyAsync(t + oX, xs, n * 4, hipMemcpyHostToDevice, s));
    launch_interp_weights(t + oX, n, t + oA, t + oT, s);            // prod_{j!=i}(x_i - x_j)
    launch_batch_inverse(t + oA, t + oW, n, 1, s);                  // w_i (Montgomery; 0 -> 0)
    const uint32_t* z = product_tree(ctx, t + oX, n, roots_leaf_log(ctx, false));
    launch_lagrange_rows(t + oX, z, t + oW, n, t + oM, t + oP, s);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipMemcpyAsync(out, t + oM, n * n * 4, hipMemcpyDeviceToHost, s));
    FRI_HIP(ctx, hipStreamSynchronize(s));
    tmp_trim(ctx);
    return FRI_OK;
}
