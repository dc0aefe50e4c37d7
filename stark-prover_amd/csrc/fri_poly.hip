// fri_poly.hip — polynomial arithmetic entry points of include/fri_amd.h:
// mul_assign (ops.rs:114-138), div_rem (ops.rs:141-191) and compose
// (ops.rs:214-237).  The reference's algorithms are schoolbook (O(n*m)
// products, long division with one Fermat inverse per quotient step, Horner
// over polynomials); field arithmetic is exact and quotient and remainder are
// unique, so any exact algorithm gives the same coefficients:
//   mul      two forward NTTs, a pointwise product, one inverse NTT; or the
//            direct convolution kernel when one operand is short
//   div_rem  Newton inversion of the reversed divisor, then two products
//   compose  NTT of q, Horner of p at those N values, inverse NTT
// Everything is enqueued on ctx->stream with one synchronisation at the end.
#include "fri_host.hpp"

static_assert(POLY_DIRECT_LIMIT == FRI_POLY_DIRECT_LIMIT, "direct kernel limit");
static_assert(FRI_POLY_DIRECT_MAX <= FRI_POLY_DIRECT_LIMIT, "crossover within the direct kernel's limit");

namespace {

// The post-scale tables of a division's inverse transforms, made once for the
// whole call instead of one table launch per transform: every table has base
// 1, so the low level (Montgomery(1) throughout, ctx->pow_lo) is shared, and a
// transform's high level is max(1, N / 2^POW_LO_LOG) copies of
// Montgomery(N^-1 * R^r_pow), uploaded together.
struct PostScales {
    std::vector<uint32_t> host;
    std::vector<size_t> offset;                       // of the i-th planned table in host
    const uint32_t* dev = nullptr;
    size_t plan(uint32_t log_N, uint32_t r_pow) {     // returns the table's index
        offset.push_back(host.size());
        const size_t nhi = log_N > POW_LO_LOG ? (size_t)1 << (log_N - POW_LO_LOG) : 1;
        host.insert(host.end(), nhi, to_mont(post_scale(log_N, r_pow)));
        return offset.size() - 1;
    }
    const uint32_t* table(size_t i) const { return dev + offset[i]; }
};
// scratch_c[0..2^log_N) = x * y (cyclic, size 2^log_N); x and y anywhere but
// scratch_a / scratch_b.
void product(fri_ctx* ctx, const uint32_t* x, size_t lx, const uint32_t* y, size_t ly, uint32_t log_N,
             const uint32_t* post_hi) {
    forward(ctx, x, lx, log_N, ctx->scratch_a);
    forward(ctx, y, ly, log_N, ctx->scratch_b);
    launch_poly_pointwise_mul(ctx->scratch_a, ctx->scratch_b, ctx->scratch_a, (size_t)1 << log_N, ctx->stream);
    inverse_with(ctx, ctx->scratch_a, log_N, ctx->pow_lo, post_hi, ctx->scratch_c);
}

}  // namespace

extern "C" int fri_poly_mul(fri_ctx* ctx, const uint32_t* a, size_t la, const uint32_t* b, size_t lb, uint32_t flags,
                            uint32_t* out, size_t out_cap, size_t* len_out) {
    if (!ctx || !len_out || (la && !a) || (lb && !b)) return fail(ctx, FRI_EINVAL, "null argument");
    if ((flags & ~(FRI_POLY_FORCE_NTT | FRI_POLY_FORCE_DIRECT)) ||
        flags == (FRI_POLY_FORCE_NTT | FRI_POLY_FORCE_DIRECT))
        return fail(ctx, FRI_EINVAL, "flags: FRI_POLY_FORCE_NTT or FRI_POLY_FORCE_DIRECT");
    if (!check_canonical(a, la) || !check_canonical(b, lb))
        return fail(ctx, FRI_EINVAL, "coefficient not canonical (>= p)");
    la = trimmed(a, la);
    lb = trimmed(b, lb);
    *len_out = 0;
    if (la == 0 || lb == 0) return FRI_OK;                        // ops.rs:115-121
    const size_t cap = (size_t)1 << ctx->log_n_max;
    if (la > cap || lb > cap || la + lb - 1 > cap)
        return fail(ctx, FRI_EINVAL, "product exceeds context capacity (next_pow2(la + lb - 1) <= 2^log_n_max)");
    const size_t n = la + lb - 1;
    *len_out = n;
    if (out_cap < n || !out) return fail(ctx, FRI_EINVAL, "output capacity too small (needed length in *len_out)");
    const size_t ls = la < lb ? la : lb;
    if ((flags & FRI_POLY_FORCE_DIRECT) && ls > FRI_POLY_DIRECT_LIMIT)
        return fail(ctx, FRI_EINVAL, "FRI_POLY_FORCE_DIRECT: short operand exceeds FRI_POLY_DIRECT_LIMIT");
    const bool direct = (flags & FRI_POLY_FORCE_DIRECT) || (!(flags & FRI_POLY_FORCE_NTT) && ls <= FRI_POLY_DIRECT_MAX);
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (direct) {
        const uint32_t* lng = la < lb ? b : a;
        const uint32_t* sht = la < lb ? a : b;
        FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_a, lng, (n + 1 - ls) * 4, hipMemcpyHostToDevice, s));
        FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_b, sht, ls * 4, hipMemcpyHostToDevice, s));
        launch_poly_conv_direct(ctx->scratch_a, n + 1 - ls, ctx->scratch_b, ls, ctx->scratch_c, n, s);
    } else {
        // both operands pass through scratch_c: the second upload is ordered
        // after the first transform on the stream
        const uint32_t log_N = ceil_log2(n);
        FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_c, a, la * 4, hipMemcpyHostToDevice, s));
        forward(ctx, ctx->scratch_c, la, log_N, ctx->scratch_a);
        FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_c, b, lb * 4, hipMemcpyHostToDevice, s));
        forward(ctx, ctx->scratch_c, lb, log_N, ctx->scratch_b);
        launch_poly_pointwise_mul(ctx->scratch_a, ctx->scratch_b, ctx->scratch_a, (size_t)1 << log_N, s);
        inverse(ctx, ctx->scratch_a, log_N, 1, ctx->scratch_c);
    }
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipMemcpyAsync(out, ctx->scratch_c, n * 4, hipMemcpyDeviceToHost, s));
    FRI_HIP(ctx, hipStreamSynchronize(s));
    return FRI_OK;                                                 // lead(a) * lead(b) != 0: n is the trimmed length
}

extern "C" int fri_poly_div_rem(fri_ctx* ctx, const uint32_t* a, size_t la, const uint32_t* b, size_t lb,
                                uint32_t* q_out, size_t q_cap, size_t* q_len, uint32_t* r_out, size_t r_cap,
                                size_t* r_len) {
    if (!ctx || !q_len || !r_len || (la && !a) || (lb && !b)) return fail(ctx, FRI_EINVAL, "null argument");
    if (!check_canonical(a, la) || !check_canonical(b, lb))
        return fail(ctx, FRI_EINVAL, "coefficient not canonical (>= p)");
    la = trimmed(a, la);
    lb = trimmed(b, lb);
    *q_len = 0;
    *r_len = 0;
    if (lb == 0) return fail(ctx, FRI_EINVAL, "Division by zero polynomial");   // ops.rs:143
    if (la < lb) {                                                 // ops.rs:145-147: q = 0, r = a
        *r_len = la;
        if (la && (r_cap < la || !r_out))
            return fail(ctx, FRI_EINVAL, "remainder capacity too small (needed length in *r_len)");
        if (la) memcpy(r_out, a, la * 4);
        return FRI_OK;
    }
    const size_t K = la - lb + 1, nr = lb - 1;                     // quotient length; remainder bound
    const size_t cap = (size_t)1 << ctx->log_n_max;
    if (la > cap || ((size_t)2 << ceil_log2(K)) > cap)
        return fail(ctx, FRI_EINVAL,
                    "division exceeds context capacity (la <= 2^log_n_max, next_pow2(la - lb + 1) <= 2^(log_n_max-1))");
    *q_len = K;
    *r_len = nr;
    if (q_cap < K || !q_out || (nr && (r_cap < nr || !r_out)))
        return fail(ctx, FRI_EINVAL, "output capacity too small (needed lengths in *q_len, *r_len: la-lb+1, lb-1)");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // the inverse transforms of the call and their post-scale tables: Newton
    // step k's is table k, then the quotient product's, the remainder product's
    const std::vector<NewtonStep> steps = newton_steps(K);
    const size_t lq_r = K < nr ? K : nr;                           // q and b cut to the low nr coefficients
    const bool r_direct = lq_r <= FRI_POLY_DIRECT_MAX;
    const uint32_t log_Q = ceil_log2(2 * K - 1), log_R = nr ? ceil_log2(lq_r + nr - 1) : 0;
    PostScales ps;
    for (const NewtonStep& st : steps) ps.plan(st.log_N, 2);
    const size_t ps_q = ps.plan(log_Q, 1);
    const size_t ps_r = nr && !r_direct ? ps.plan(log_R, 1) : 0;
    // operands and the running results live in the partials scratch; the three
    // context buffers are the transforms' work space
    const size_t oA = 0, oB = oA + round4(la), oF = oB + round4(lb), oG = oF + round4(lb),
                 oQ = oG + series_words(steps, K), oS = oQ + round4(K);
    const int rc = ensure_tmp(ctx, oS + ps.host.size());
    if (rc) return rc;
    uint32_t* A = ctx->interp_tmp + oA;
    uint32_t* B = ctx->interp_tmp + oB;
    uint32_t* F = ctx->interp_tmp + oF;                            // rev(b): F[0] = lead(b) != 0
    uint32_t* G = ctx->interp_tmp + oG;                            // F^-1 mod x^m, m -> K (room for a whole iNTT)
    uint32_t* Q = ctx->interp_tmp + oQ;
    ps.dev = ctx->interp_tmp + oS;
    FRI_HIP(ctx, hipMemcpyAsync(ctx->interp_tmp + oS, ps.host.data(), ps.host.size() * 4, hipMemcpyHostToDevice, s));
    launch_pow_table(ctx->pow_lo, ctx->pow_hi, 0, 1u, 1u, s);      // the shared low level: Montgomery(1)
    FRI_HIP(ctx, hipMemcpyAsync(A, a, la * 4, hipMemcpyHostToDevice, s));
    FRI_HIP(ctx, hipMemcpyAsync(B, b, lb * 4, hipMemcpyHostToDevice, s));
    launch_poly_reverse(B, lb - 1, lb, F, lb, s);
    // g mod x^m0 by the power-series recurrence on the host (m0 <= 64: the
    // Newton steps below would each be four launches on a handful of words)
    const size_t m0 = K < 64 ? K : 64;
    uint32_t g0[64];
    g0[0] = inv_std(b[lb - 1]);
    for (size_t i = 1; i < m0; i++) {
        uint64_t acc = 0;
        for (size_t j = 1; j <= i && j < lb; j++) acc = (acc + (uint64_t)b[lb - 1 - j] * g0[i - j] % P) % P;
        g0[i] = (uint32_t)((uint64_t)(P - (uint32_t)acc) % P * g0[0] % P);
    }
    FRI_HIP(ctx, hipMemcpyAsync(G, g0, m0 * 4, hipMemcpyHostToDevice, s));
    series_inverse(ctx, F, lb, G, steps, [&](size_t k, const uint32_t* src, uint32_t log_N, uint32_t* dst) {
        inverse_with(ctx, src, log_N, ctx->pow_lo, ps.table(k), dst);
    });
    // q = rev((rev(a) mod x^K) * g mod x^K)
    launch_poly_reverse(A, la - 1, K, Q, K, s);
    product(ctx, Q, K, G, K, log_Q, ps.table(ps_q));
    launch_poly_reverse(ctx->scratch_c, K - 1, K, Q, K, s);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipMemcpyAsync(q_out, Q, K * 4, hipMemcpyDeviceToHost, s));
    // r = (a - q b) mod x^(lb-1): only the low nr coefficients of q and b count
    if (nr) {
        if (r_direct) {
            launch_poly_conv_direct(B, nr, Q, lq_r, ctx->scratch_c, nr, s);
        } else {
            product(ctx, Q, lq_r, B, nr, log_R, ps.table(ps_r));
        }
        launch_poly_sub(A, ctx->scratch_c, ctx->scratch_b, nr, s);
        FRI_HIP(ctx, hipGetLastError());
        FRI_HIP(ctx, hipMemcpyAsync(r_out, ctx->scratch_b, nr * 4, hipMemcpyDeviceToHost, s));
    }
    FRI_HIP(ctx, hipStreamSynchronize(s));
    tmp_trim(ctx);
    *r_len = trimmed(r_out, nr);                                   // lead(a) / lead(b) != 0: K needs no trim
    return FRI_OK;
}

extern "C" int fri_poly_compose(fri_ctx* ctx, const uint32_t* p, size_t lp, const uint32_t* q, size_t lq,
                                uint32_t* out, size_t out_cap, size_t* len_out) {
    if (!ctx || !len_out || (lp && !p) || (lq && !q)) return fail(ctx, FRI_EINVAL, "null argument");
    if (!check_canonical(p, lp) || !check_canonical(q, lq))
        return fail(ctx, FRI_EINVAL, "coefficient not canonical (>= p)");
    lp = trimmed(p, lp);
    lq = trimmed(q, lq);
    *len_out = 0;
    if (lp == 0) return FRI_OK;                                    // ops.rs:214-237: the zero polynomial
    const size_t cap = (size_t)1 << ctx->log_n_max;
    if (lp > cap || lq > cap) return fail(ctx, FRI_EINVAL, "size exceeds context capacity");
    // q zero or constant: N = 1 and the result is the constant p(q_0)
    const size_t n = lq <= 1 ? 1 : (lp - 1) * (lq - 1) + 1;
    if (n > cap)
        return fail(ctx, FRI_EINVAL, "composition exceeds context capacity (next_pow2(deg p * deg q + 1) <= 2^log_n_max)");
    *len_out = n;
    if (out_cap < n || !out) return fail(ctx, FRI_EINVAL, "output capacity too small (needed length in *len_out)");
    const uint32_t log_N = ceil_log2(n);
    const size_t N = (size_t)1 << log_N;
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t tw = evaluate_tmp_words(lp, N);
    if (tw) {
        const int rc = ensure_tmp(ctx, tw);
        if (rc) return rc;
    }
    if (lq) FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_a, q, lq * 4, hipMemcpyHostToDevice, s));
    forward(ctx, ctx->scratch_a, lq, log_N, ctx->scratch_b);       // q(w_N^k)
    FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_a, p, lp * 4, hipMemcpyHostToDevice, s));   // after the transform
    launch_evaluate(ctx->scratch_a, lp, ctx->scratch_b, N, ctx->scratch_c, ctx->interp_tmp, s);   // p(q(w_N^k))
    inverse(ctx, ctx->scratch_c, log_N, 0, ctx->scratch_a);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipMemcpyAsync(out, ctx->scratch_a, n * 4, hipMemcpyDeviceToHost, s));
    FRI_HIP(ctx, hipStreamSynchronize(s));
    tmp_trim(ctx);
    *len_out = trimmed(out, n);                                    // a constant p(c) may be zero
    return FRI_OK;
}
