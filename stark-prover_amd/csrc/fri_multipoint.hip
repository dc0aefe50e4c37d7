// fri_multipoint.hip — Polynomial::evaluate at many points (ops.rs:76-83) and
// Polynomial::interpolate on arbitrary points (ops.rs:239-241 ->
// interpolation.rs:121-152) through the product tree of fri_roots.hip, all of
// whose levels are retained.  Field arithmetic is exact, so
// the values equal Horner's and the coefficients the Lagrange sum's:
//   evaluate     tree; g = rev(Z_pad)^-1 mod x^d (Newton); the root vector
//                a[k] = (rev(f) g)[d-1-k]; one middle-product level per tree
//                level down to the leaf subtrees; one lane per point there
//   interpolate  tree; Z' at every point by the evaluation; w = 1/Z'(x_i)
//                (0 -> 0: the copies of a repeated x); c = y w; F up the tree
// Below FRI_MP_EVAL_MIN / FRI_MP_INTERP_MIN the direct kernels of fri_ops.hip
// run as before.  Everything is enqueued on ctx->stream with one
// synchronisation at the end.
#include "fri_host.hpp"

static_assert((FRI_MP_EVAL_MIN & (FRI_MP_EVAL_MIN - 1)) == 0 && (FRI_MP_INTERP_MIN & (FRI_MP_INTERP_MIN - 1)) == 0,
              "the crossovers are powers of two");
static_assert(FRI_MP_INTERP_MIN <= (1 << 17), "every n the direct kernels refuse takes the tree");

namespace {

const uint32_t ONE = 1u;

// Where the call's pieces lie in the partials scratch (word offsets).
struct Layout {
    uint32_t log_np = 0, lf_log = 0;
    size_t np = 0;
    size_t xs = 0, lev = 0, F = 0, G = 0, f = 0, rf = 0, a0 = 0, a1 = 0, end = 0;
    uint32_t levels() const { return log_np - lf_log + 1; }
    // the retained level of nodes of degree 2^lg, lf_log <= lg <= log_np (np
    // words; the children of a product of 2^lg words are level lg - 1)
    size_t level(uint32_t lg) const { return lev + (size_t)(lg - lf_log) * np; }
};
// count points, a polynomial of d coefficients (0: none uploaded or reversed)
Layout layout(fri_ctx* ctx, size_t count, size_t d, bool small_leaf, size_t base) {
    Layout L;
    L.log_np = ceil_log2(count);
    L.np = (size_t)1 << L.log_np;
    L.lf_log = roots_leaf_log(ctx, small_leaf);
    if (L.lf_log > L.log_np) L.lf_log = L.log_np;
    L.xs = base;
    L.lev = L.xs + round4(count);
    L.F = L.lev + round4(L.levels() * L.np + 1);  // the top level is followed by Z_pad's leading 1
    L.G = L.F + round4(L.np + 1);
    L.f = L.G + series_words(newton_steps(d), d);
    L.rf = L.f + round4(d);
    L.a0 = L.rf + round4(d);
    L.a1 = L.a0 + round4(L.np);
    L.end = L.a1 + round4(L.np);
    return L;
}
// The tree path's sizes (include/fri_amd.h): the root product and the last Newton step.
bool eval_fits(const fri_ctx* ctx, size_t d, size_t count) {
    const size_t cap = (size_t)1 << ctx->log_n_max, np = (size_t)1 << ceil_log2(count);
    return d <= cap && np <= cap && d + np - 1 <= cap && ((size_t)2 << ceil_log2(d)) <= cap;
}

int build_tree(fri_ctx* ctx, const Layout& L, size_t count) {
    uint32_t* t = ctx->interp_tmp;
    product_tree(ctx, t + L.xs, count, L.lf_log, t + L.lev);
    FRI_HIP(ctx, hipMemcpyAsync(t + L.level(L.log_np) + L.np, &ONE, 4, hipMemcpyHostToDevice, ctx->stream));
    return FRI_OK;
}

// out[i] = f(xs[i]), i < count, on the tree already enqueued: f is d >= 1
// canonical coefficients on the device (outside the three context buffers),
// out a device pointer.
void evaluate_on_tree(fri_ctx* ctx, const Layout& L, const uint32_t* f, size_t d, size_t count, uint32_t* out) {
    hipStream_t s = ctx->stream;
    uint32_t* t = ctx->interp_tmp;
    const size_t np = L.np;
    uint32_t *F = t + L.F, *G = t + L.G, *a = t + L.a0, *b = t + L.a1;
    launch_poly_reverse(t + L.level(L.log_np), np, np + 1, F, np + 1, s);   // rev(Z_pad): F[0] = 1
    // g = F^-1 mod x^d
    launch_mp_series_seed(F, np + 1, (uint32_t)(d < 64 ? d : 64), G, s);
    series_inverse(ctx, F, np + 1, G, newton_steps(d), [&](size_t, const uint32_t* src, uint32_t log_N, uint32_t* dst) {
        inverse(ctx, src, log_N, 2, dst);
    });
    // the root vector: the d + np - 1 wide cyclic product keeps the wrap off
    // the np coefficients read
    {
        const uint32_t log_N = ceil_log2(d + np - 1);
        launch_poly_reverse(f, d - 1, d, t + L.rf, d, s);
        forward(ctx, t + L.rf, d, log_N, ctx->scratch_a);
        forward(ctx, G, d, log_N, ctx->scratch_b);
        launch_poly_pointwise_mul(ctx->scratch_a, ctx->scratch_b, ctx->scratch_a, (size_t)1 << log_N, s);
        inverse(ctx, ctx->scratch_a, log_N, 1, ctx->scratch_c);
        launch_poly_reverse(ctx->scratch_c, d - 1, d < np ? d : np, a, np, s);
    }
    for (uint32_t lg = L.log_np; lg > L.lf_log; lg--) {             // parents of 2^lg words -> children
        const uint32_t* nodes = t + L.level(lg - 1);
        if (lg <= ROOTS_LDS_LOG_MAX) {
            launch_mp_down_level_lds(a, nodes, b, L.log_np, lg, ctx->tw_fwd, ctx->tw_inv, s);
            std::swap(a, b);
            continue;
        }
        const size_t m2 = (size_t)1 << lg, h = m2 >> 1;
        batched_ntt(ctx, lg, false, a, m2, ctx->scratch_a, np);
        batched_ntt(ctx, lg, false, nodes, h, ctx->scratch_b, np);
        batched_ntt(ctx, lg, false, nodes + h, h, ctx->scratch_c, np);
        launch_mp_down_pointwise(ctx->scratch_a, ctx->scratch_b, ctx->scratch_c, np, lg, s);
        // a_R lands in place; a_L's product goes through the old level's buffer
        batched_ntt(ctx, lg, true, ctx->scratch_b, m2, b, np);
        batched_ntt(ctx, lg, true, ctx->scratch_c, m2, a, np);
        launch_mp_take_high(a, b, np, lg, s);
        std::swap(a, b);
    }
    launch_mp_leaf_eval(t + L.xs, count, t + L.level(L.lf_log), L.lf_log == L.log_np, a, L.log_np, L.lf_log, out, s);
}

int check_flags(fri_ctx* ctx, uint32_t flags) {
    if ((flags & ~(FRI_MP_FORCE_TREE | FRI_MP_FORCE_DIRECT | FRI_MP_SMALL_LEAF)) ||
        (flags & (FRI_MP_FORCE_TREE | FRI_MP_FORCE_DIRECT)) == (FRI_MP_FORCE_TREE | FRI_MP_FORCE_DIRECT))
        return fail(ctx, FRI_EINVAL, "flags: FRI_MP_FORCE_TREE or FRI_MP_FORCE_DIRECT, and FRI_MP_SMALL_LEAF");
    return FRI_OK;
}

}  // namespace

extern "C" int fri_evaluate_ex(fri_ctx* ctx, const uint32_t* coeffs, size_t d, const uint32_t* xs, size_t count,
                               uint32_t flags, uint32_t* out) {
    if (!ctx || (d && !coeffs) || (count && (!xs || !out))) return fail(ctx, FRI_EINVAL, "null argument");
    if (check_flags(ctx, flags)) return FRI_EINVAL;
    const size_t cap = (size_t)1 << ctx->log_n_max;
    if (d > cap || count > cap) return fail(ctx, FRI_EINVAL, "size exceeds context capacity");
    if (!check_canonical(coeffs, d) || !check_canonical(xs, count))
        return fail(ctx, FRI_EINVAL, "value not canonical (>= p)");
    const bool fits = d && count && eval_fits(ctx, d, count);
    if ((flags & FRI_MP_FORCE_TREE) && d && count && !fits)
        return fail(ctx, FRI_EINVAL,
                    "FRI_MP_FORCE_TREE: evaluation exceeds the tree path's sizes (d + next_pow2(count) - 1 <= "
                    "2^log_n_max, next_pow2(d) <= 2^(log_n_max-1))");
    const bool tree = fits && ((flags & FRI_MP_FORCE_TREE) ||
                               (!(flags & FRI_MP_FORCE_DIRECT) && (d < count ? d : count) >= FRI_MP_EVAL_MIN));
    if (!tree) return evaluate_direct(ctx, coeffs, d, xs, count, out);
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const Layout L = layout(ctx, count, d, flags & FRI_MP_SMALL_LEAF, 0);
    const int rc = ensure_tmp(ctx, L.end);
    if (rc) return rc;
    uint32_t* t = ctx->interp_tmp;
    FRI_HIP(ctx, hipMemcpyAsync(t + L.xs, xs, count * 4, hipMemcpyHostToDevice, s));
    FRI_HIP(ctx, hipMemcpyAsync(t + L.f, coeffs, d * 4, hipMemcpyHostToDevice, s));
    if (const int rt = build_tree(ctx, L, count)) return rt;
    evaluate_on_tree(ctx, L, t + L.f, d, count, ctx->scratch_c);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipMemcpyAsync(out, ctx->scratch_c, count * 4, hipMemcpyDeviceToHost, s));
    FRI_HIP(ctx, hipStreamSynchronize(s));
    tmp_trim(ctx);
    return FRI_OK;
}

extern "C" int fri_evaluate(fri_ctx* ctx, const uint32_t* coeffs, size_t d, const uint32_t* xs, size_t count,
                            uint32_t* out) {
    return fri_evaluate_ex(ctx, coeffs, d, xs, count, 0, out);
}

extern "C" int fri_interpolate_points_ex(fri_ctx* ctx, const uint32_t* xs, const uint32_t* ys, size_t n,
                                         uint32_t flags, uint32_t* coeffs_out, size_t* len_out) {
    if (!ctx || !len_out || (n && (!xs || !ys || !coeffs_out))) return fail(ctx, FRI_EINVAL, "null argument");
    if (check_flags(ctx, flags)) return FRI_EINVAL;
    const uint32_t log_N = ceil_log2(n);
    // Z' has n coefficients, evaluated at next_pow2(n) points
    const bool fits = n && log_N + 1 <= ctx->log_n_max;
    const bool direct_ok = log_N <= 17 && log_N <= ctx->log_n_max;
    if (n && (flags & FRI_MP_FORCE_TREE) && !fits)
        return fail(ctx, FRI_EINVAL,
                    "FRI_MP_FORCE_TREE: interpolation exceeds the tree path's sizes (next_pow2(n) <= 2^(log_n_max-1))");
    const bool tree = fits && ((flags & FRI_MP_FORCE_TREE) ||
                               (!(flags & FRI_MP_FORCE_DIRECT) && n >= FRI_MP_INTERP_MIN));
    if (n && !tree && !direct_ok)
        return fail(ctx, FRI_EINVAL,
                    "arbitrary-point interpolation: next_pow2(n) <= 2^(log_n_max-1) on the tree path; the direct "
                    "kernels are O(n^2) and take n <= 2^17 and <= 2^log_n_max");
    if (!check_canonical(xs, n) || !check_canonical(ys, n)) return fail(ctx, FRI_EINVAL, "value not canonical (>= p)");
    *len_out = 0;
    if (n == 0) return FRI_OK;                                   // Polynomial::zero() (interpolation.rs:133-136)
    if (!tree) return interpolate_points_direct(ctx, xs, ys, n, log_N, coeffs_out, len_out);
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // ahead of the evaluation's pieces: ys, Z', its values, the weights that
    // become c, a fourth transform buffer; F climbs between the evaluation's
    // two vector buffers once they are free
    const size_t np = (size_t)1 << log_N;
    const size_t oY = 0, oD = oY + round4(n), oV = oD + round4(n), oC = oV + round4(n), oT = oC + round4(np),
                 base = oT + round4(np);
    const Layout L = layout(ctx, n, n, flags & FRI_MP_SMALL_LEAF, base);
    const int rc = ensure_tmp(ctx, L.end);
    if (rc) return rc;
    uint32_t* t = ctx->interp_tmp;
    FRI_HIP(ctx, hipMemcpyAsync(t + L.xs, xs, n * 4, hipMemcpyHostToDevice, s));
    FRI_HIP(ctx, hipMemcpyAsync(t + oY, ys, n * 4, hipMemcpyHostToDevice, s));
    if (const int rt = build_tree(ctx, L, n)) return rt;
    const uint32_t* z = t + L.level(log_N) + (np - n);              // Z's n low coefficients
    launch_mp_derivative(z, n, t + oD, s);
    evaluate_on_tree(ctx, L, t + oD, n, n, t + oV);                // Z'(x_i) = prod_{j!=i}(x_i - x_j)
    launch_batch_inverse(t + oV, t + oC, n, 1, s);                  // w_i (Montgomery; 0 -> 0)
    launch_interp_coeffs(t + oY, t + oC, n, s);                     // c_i = y_i w_i; the leaf kernel pads with 0
    uint32_t *F = t + L.a0, *Fn = t + L.a1;
    launch_mp_leaf_up(t + L.xs, t + oC, n, log_N, L.lf_log, F, s);
    for (uint32_t lg = L.lf_log + 1; lg <= log_N; lg++) {           // children of 2^(lg-1) words -> parents
        const uint32_t* nodes = t + L.level(lg - 1);
        if (lg <= ROOTS_LDS_LOG_MAX) {
            launch_mp_up_level_lds(F, nodes, Fn, log_N, lg, ctx->tw_fwd, ctx->tw_inv, s);
            std::swap(F, Fn);
            continue;
        }
        const size_t h = (size_t)1 << (lg - 1);
        batched_ntt(ctx, lg, false, F, h, ctx->scratch_a, np);
        batched_ntt(ctx, lg, false, F + h, h, ctx->scratch_b, np);
        batched_ntt(ctx, lg, false, nodes, h, ctx->scratch_c, np);
        batched_ntt(ctx, lg, false, nodes + h, h, t + oT, np);
        launch_mp_up_pointwise(ctx->scratch_a, ctx->scratch_b, ctx->scratch_c, t + oT, ctx->scratch_a, np, lg, s);
        batched_ntt(ctx, lg, true, ctx->scratch_a, (size_t)1 << lg, Fn, np);
        std::swap(F, Fn);
    }
    FRI_HIP(ctx, hipGetLastError());
    // the padding's x^pad is skipped, as for Z
    FRI_HIP(ctx, hipMemcpyAsync(coeffs_out, F + (np - n), n * 4, hipMemcpyDeviceToHost, s));
    FRI_HIP(ctx, hipStreamSynchronize(s));
    tmp_trim(ctx);
    *len_out = trimmed(coeffs_out, n);                           // Polynomial::new trim (ops.rs:19-37)
    return FRI_OK;
}

extern "C" int fri_interpolate_points(fri_ctx* ctx, const uint32_t* xs, const uint32_t* ys, size_t n,
                                      uint32_t* coeffs_out, size_t* len_out) {
    return fri_interpolate_points_ex(ctx, xs, ys, n, 0, coeffs_out, len_out);
}
