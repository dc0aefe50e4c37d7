// fri_fibsq.hip — the single-proof STARK-101 prover entry points: trace
// commit (interpolation, LDE, Merkle tree), the FibonacciSq composition
// commit on that trace, the trace itself and its decommitment.  fibsq_shape,
// the shape's checks and constants, also serves the batched composition
// commit (fri_batch.hip); fri_prover.hip has the constraint system.
#include "fri_host.hpp"

// Trace side of the prover (the reference's
// src/trace and src/prover are empty): interpolate the trace on its subgroup
// <w_t> (Polynomial::interpolate, ops.rs:239 -> interpolation.rs:121-152),
// evaluate it on the blown-up coset offset*<w_n> (the LDE, as
// fri_commit.rs:78 evaluates), and Merkle-commit the LDE (merkle/mod.rs:10-26),
// all device-resident.  The LDE tree stays in the context (trace_tree).
extern "C" int fri_trace_commit(fri_ctx* ctx, const uint32_t* trace, uint32_t log_t, uint32_t log_blowup,
                                uint32_t offset, uint8_t root32[32], uint32_t* coeffs_out, size_t* coeff_len,
                                uint32_t* lde_out) {
    if (!ctx || !trace || !root32) return fail(ctx, FRI_EINVAL, "null argument");
    const uint32_t L = log_t + log_blowup;
    if (L > ctx->log_n_max || L < 1) return fail(ctx, FRI_EINVAL, "log_t + log_blowup out of range for context");
    if (offset == 0 || offset >= P) return fail(ctx, FRI_EINVAL, "offset must be a nonzero canonical element");
    const size_t nt = (size_t)1 << log_t, n = (size_t)1 << L;
    if (!check_canonical(trace, nt)) return fail(ctx, FRI_EINVAL, "trace value not canonical (>= p)");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    ctx->trace_valid = false;
    if (ctx->trace_tree_cap < n) {
        dfree(ctx, ctx->trace_tree);
        dfree(ctx, ctx->trace_lde);
        ctx->trace_tree = nullptr;
        ctx->trace_lde = nullptr;
        ctx->trace_tree_cap = 0;
        FRI_HIP(ctx, dalloc(ctx, &ctx->trace_tree, (n * 2) * 32));
        FRI_HIP(ctx, dalloc(ctx, &ctx->trace_lde, n * 4));
        ctx->trace_tree_cap = n;
    }
    hipStream_t s = ctx->stream;
    FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_a, trace, nt * 4, hipMemcpyHostToDevice, s));
    coset_inverse(ctx, ctx->scratch_a, log_t, 1u, 0, ctx->scratch_b);       // c_j = nt^-1 sum_i trace_i w_t^-ij
    coset_forward(ctx, ctx->scratch_b, nt, L, offset, ctx->trace_lde);      // the LDE on offset * <w_n>
    // Merkle tree of the LDE, every level kept
    LayerTask t{};
    t.values = ctx->trace_lde;
    t.tree = ctx->trace_tree;
    t.L = L;
    launch_layer(t, s);
    FRI_HIP(ctx, hipGetLastError());
    uint32_t w[8];
    FRI_HIP(ctx, hipMemcpyAsync(w, ctx->trace_tree + 8 * level_offset(L, L), 32, hipMemcpyDeviceToHost, s));
    if (coeffs_out) FRI_HIP(ctx, hipMemcpyAsync(coeffs_out, ctx->scratch_b, nt * 4, hipMemcpyDeviceToHost, s));
    if (lde_out) FRI_HIP(ctx, hipMemcpyAsync(lde_out, ctx->trace_lde, n * 4, hipMemcpyDeviceToHost, s));
    FRI_HIP(ctx, hipStreamSynchronize(s));
    digest_to_bytes(w, root32);
    ctx->trace_valid = true;
    ctx->trace_log_t = log_t;
    ctx->trace_log_b = log_blowup;
    ctx->trace_offset = offset;
    if (coeffs_out && coeff_len) *coeff_len = trimmed(coeffs_out, nt);
    ctx->err.clear();
    return FRI_OK;
}

int fri::fibsq_shape(fri_ctx* ctx, uint32_t log_t, uint32_t log_blowup, uint32_t offset, bool batch_caps,
                     FibsqParams* q) {
    if (log_blowup < 1 || ((uint32_t)1 << log_blowup) > FIBSQ_MAX_B)
        return fail(ctx, FRI_EINVAL, "log_blowup must be 1..4 (deg CP = T needs n > T)");
    if (log_t < 2) return fail(ctx, FRI_EINVAL, "trace needs at least 4 rows");
    const uint32_t L = log_t + log_blowup;
    if (batch_caps) {
        if (log_t > FRI_BATCH_MAX_LOG_N || L > FRI_BATCH_MAX_LOG_N)
            return fail(ctx, FRI_EINVAL, "log_t + log_blowup above FRI_BATCH_MAX_LOG_N");
        if (L > ctx->log_n_max) return fail(ctx, FRI_EINVAL, "log_t + log_blowup out of range for context");
    }
    if (offset == 0 || offset >= P) return fail(ctx, FRI_EINVAL, "offset must be a nonzero canonical element");
    const size_t T = (size_t)1 << log_t;
    const uint32_t B = 1u << log_blowup;
    const uint32_t w = root_of_unity(L), g = root_of_unity(log_t), wB = root_of_unity(log_blowup);
    const uint32_t offT = pow_std(offset, T);
    *q = FibsqParams{};
    for (uint32_t j = 0; j < B; j++) {
        const uint32_t z = sub(mul_std(offT, pow_std(wB, j)), 1u);
        if (z == 0) return fail(ctx, FRI_EINVAL, "offset^T lies in <w_B>: the coset meets the trace domain");
        q->zinv_m[j] = to_mont(inv_std(z));
    }
    q->log_n = L;
    q->B = B;
    q->offset_m = to_mont(offset);
    q->w_m = to_mont(w);
    q->winv_m = to_mont(inv_std(w));
    q->glast_m = to_mont(pow_std(g, T - 1));
    q->gprev_m = to_mont(pow_std(g, T - 2));
    return FRI_OK;
}

// ------------------------------------------------------------- prover ----
// STARK-101 FibonacciSq composition + FRI commit of the composition
// polynomial (fri_prover.hip has the constraint system).  Reads the trace LDE
// kept by the last fri_trace_commit; CP evaluations -> coset iNTT -> the
// commit of fri_commit_device (layer 0 re-extends exactly those evaluations).
extern "C" int fri_fibsq_composition_commit(fri_ctx* ctx, uint32_t log_t, uint32_t log_blowup, uint32_t offset,
                                            uint32_t a_last, const uint32_t alphas[3],
                                            const fri_channel_state* chan_in, uint32_t flags,
                                            fri_commit_result* out) {
    if (!ctx || !alphas || !out) return fail(ctx, FRI_EINVAL, "null argument");
    if (!ctx->trace_valid || ctx->trace_log_t != log_t || ctx->trace_log_b != log_blowup ||
        ctx->trace_offset != offset)
        return fail(ctx, FRI_ESTATE, "no resident trace commit with this (log_t, log_blowup, offset)");
    FibsqParams q;
    int rc = fibsq_shape(ctx, log_t, log_blowup, offset, false, &q);
    if (rc) return rc;
    if (a_last >= P || alphas[0] >= P || alphas[1] >= P || alphas[2] >= P)
        return fail(ctx, FRI_EINVAL, "a_last / alphas not canonical");
    if (flags & FRI_FLAG_FORCE_BETAS) return fail(ctx, FRI_EINVAL, "forced betas are not supported here");
    q.a_last = a_last;
    for (int j = 0; j < 3; j++) q.alpha_m[j] = to_mont(alphas[j]);
    const uint32_t L = log_t + log_blowup;
    const size_t n = (size_t)1 << L, T = (size_t)1 << log_t;
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = use_lane(ctx, 0))) return rc;            // the commit below runs on lane 0: so does its input
    size_t sp = span_begin(ctx, "composition", (uint64_t)n * 8);
    launch_fibsq_cp(ctx->trace_lde, ctx->scratch_c, q, ctx->stream);
    // coefficients: c_j = n^-1 offset^-j sum_i cp_i w^-ij   (fri_interpolate)
    coset_inverse(ctx, ctx->scratch_c, L, inv_std(offset), 0, ctx->scratch_b);
    span_end(ctx, sp);
    FRI_HIP(ctx, hipGetLastError());
    rc = run_commit(ctx, nullptr, ctx->scratch_b, n, L, offset, chan_in, flags, nullptr, out);
    if (rc) return rc;
    if (ctx->h_state->deg[0] > (int32_t)T) {
        ctx->h_state->n_layers = 0;      // no proof of a violated trace is served
        return fail(ctx, FRI_EDEGREE, "composition polynomial degree exceeds T: the trace violates the constraints");
    }
    return FRI_OK;
}

// STARK-101 FibonacciSq trace.  The recurrence is one serial dependency
// chain (each row needs the previous two), so it runs on the host: ~2
// 64-bit mulmods per row, far below one kernel launch for any T here.
extern "C" int fri_fibsq_trace(uint32_t a1, uint32_t log_t, uint32_t* out) {
    if (!out || log_t > 30) return FRI_EINVAL;
    if (a1 >= P) return FRI_EINVAL;
    const size_t T = (size_t)1 << log_t;
    uint64_t x = 1, y = a1;
    out[0] = 1;
    if (T > 1) out[1] = a1;
    for (size_t i = 2; i < T; i++) {
        const uint64_t z = (x * x % P + y * y % P) % P;
        out[i] = (uint32_t)z;
        x = y;
        y = z;
    }
    return FRI_OK;
}

extern "C" int fri_trace_decommit(fri_ctx* ctx, uint64_t index, uint64_t stride, uint32_t count, uint32_t* values,
                                  uint8_t* paths, size_t paths_cap) {
    if (!ctx || !values || !paths) return fail(ctx, FRI_EINVAL, "null argument");
    if (!ctx->trace_valid) return fail(ctx, FRI_ESTATE, "no resident trace commit");
    if (count < 1 || count > 8) return fail(ctx, FRI_EINVAL, "count must be 1..8");
    const uint32_t L = ctx->trace_log_t + ctx->trace_log_b;
    if (index >> L) return fail(ctx, FRI_EINVAL, "index out of range");
    const size_t words = (size_t)count * 8 * L;
    if (paths_cap < words * 4) return fail(ctx, FRI_EINVAL, "paths buffer too small (32 bytes per level per value)");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    int rc = dq_alloc(ctx);
    if (rc) return rc;
    launch_trace_gather(ctx->trace_lde, ctx->trace_tree, L, index, stride, count, ctx->dq_dev, ctx->stream);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(values, ctx->dq_host, count * 4);
    memcpy(paths, ctx->dq_host + count, words * 4);
    return FRI_OK;
}
