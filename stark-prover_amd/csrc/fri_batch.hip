// fri_batch.hip — fri_commit_batch: B independent commits of one shape
// (src/fri/fri_commit.rs:72-122 each) in one call.  The LDE of every member
// is a fixed number of launches, then ONE launch commits them all, one
// workgroup per member (k_commit_batch, fri_batch_kernels.hip).  The batch has its
// own buffers (Batch, fri_host.hpp): no lane's plan or graph is touched, so a
// single commit afterwards replays what it captured.  The member-wise
// read-backs are fri_readback.hip's.  Below the commit the batched prover:
// B x fri_trace_commit, B x fri_fibsq_composition_commit on that trace batch
// (the shape's checks and constants: fibsq_shape, fri_fibsq.hip), and one
// query of every member in one launch (fri_batch_query_round).
#include "fri_host.hpp"

static_assert(FRI_BATCH_MAX_LOG_N >= 14 && FRI_BATCH_MAX_LOG_N <= (int)BATCH_MAX_LOG, "the kernel's tiles");
static_assert(FRI_BATCH_LDE_LDS_MAX_LOG_N == (int)BATCH_LDS_LDE_MAX_LOG, "the LDE's switch point");

static void bufs_release(fri_ctx* ctx, BatchBufs& b) {
    for (int i = 0; i < BB_N; i++) dfree(ctx, b.dev[i]);
    if (b.h_states) hipHostFree(b.h_states);
    b = BatchBufs();
}

void fri::batch_free(fri_ctx* ctx) {
    Batch& B = ctx->batch;
    bufs_release(ctx, B.b);
    dfree(ctx, B.xinv); dfree(ctx, B.pre_lo); dfree(ctx, B.pre_hi);
    if (B.h_q) hipHostFree(B.h_q);
    B = Batch();
}

// Every buffer at least want[i] bytes.  The larger ones are all allocated
// before any old one is freed: a failure leaves the buffers (and a resident
// batch in them) as they were.
static int bufs_grow(fri_ctx* ctx, BatchBufs& b, const size_t want[BB_N], size_t members) {
    BatchBufs nb;
    bool ok = true;
    for (int i = 0; i < BB_N && ok; i++)
        if (want[i] > b.cap[i]) {
            ok = dalloc(ctx, &nb.dev[i], want[i]) == hipSuccess;
            if (ok) nb.cap[i] = want[i];
        }
    if (ok && members > b.h_cap) {
        ok = hipHostMalloc(&nb.h_states, members * sizeof(DevState), hipHostMallocDefault) == hipSuccess;
        if (ok) nb.h_cap = members;
        else nb.h_states = nullptr;
    }
    if (!ok) {
        (void)hipGetLastError();
        bufs_release(ctx, nb);
        return fail(ctx, FRI_ENOMEM, "device allocation failed for the batch's buffers");
    }
    for (int i = 0; i < BB_N; i++)
        if (nb.dev[i]) {
            dfree(ctx, b.dev[i]);
            b.dev[i] = nb.dev[i];
            b.cap[i] = nb.cap[i];
        }
    if (nb.h_states) {
        if (b.h_states) hipHostFree(b.h_states);
        b.h_states = nb.h_states;
        b.h_cap = nb.h_cap;
    }
    return FRI_OK;
}

// x^-1 of every fold of a 2^log_n codeword on offset * <w_n> (fold k at
// n - (n >> k), as plan_layout lays them out) and the LDE's pre-scale powers.
static int batch_tables(fri_ctx* ctx, uint32_t log_n, uint32_t offset) {
    Batch& B = ctx->batch;
    if (B.xinv && B.tab_log_n == log_n && B.tab_offset == offset) return FRI_OK;
    dfree(ctx, B.xinv); dfree(ctx, B.pre_lo); dfree(ctx, B.pre_hi);
    B.xinv = B.pre_lo = B.pre_hi = nullptr;
    B.tab_log_n = 0;
    const size_t n = (size_t)1 << log_n;
    const size_t nhi = log_n > POW_LO_LOG ? ((size_t)1 << (log_n - POW_LO_LOG)) : 1;
    if (dalloc(ctx, &B.xinv, n * 4) != hipSuccess || dalloc(ctx, &B.pre_lo, ((size_t)1 << POW_LO_LOG) * 4) != hipSuccess ||
        dalloc(ctx, &B.pre_hi, nhi * 4) != hipSuccess) {
        dfree(ctx, B.xinv); dfree(ctx, B.pre_lo); dfree(ctx, B.pre_hi);
        B.xinv = B.pre_lo = B.pre_hi = nullptr;
        return fail(ctx, FRI_ENOMEM, "device allocation failed for the batch's tables");
    }
    hipStream_t s = ctx->stream;
    launch_pow_table(B.pre_lo, B.pre_hi, log_n, offset, 1u, s);
    // xinv_0[i] = (offset*w_n^i)^-1, xinv_k[i] = xinv_{k-1}[i]^2 (plan_build)
    launch_coset_points(ctx->scratch_a, n / 2, offset, log_n, s);
    launch_batch_inverse(ctx->scratch_a, B.xinv, n / 2, 1, s);
    for (uint32_t k = 1; k < log_n; k++)
        launch_square_mont(B.xinv + (n - (n >> (k - 1))), B.xinv + (n - (n >> k)), (n >> k) / 2, s);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipStreamSynchronize(s));
    B.tab_log_n = log_n;
    B.tab_offset = offset;
    return FRI_OK;
}

// Batches run on one-device contexts, outside profiling.
static int batch_ctx_ok(fri_ctx* ctx) {
    if (ctx->team_root || ctx->tp.team)
        return fail(ctx, FRI_EINVAL, "multi-GPU context: batched commits run on one-device contexts");
    if (ctx->profiling) return fail(ctx, FRI_ESTATE, "profiling: time commits with fri_commit_device");
    return FRI_OK;
}

// Pending pipelined commits first, on whichever lane (the batch's tables use the context's scratch).
static int batch_quiesce(fri_ctx* ctx) {
    settle(ctx);
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (Lane& ln : ctx->lanes)
        if (ln.stream) FRI_HIP(ctx, hipStreamSynchronize(ln.stream));
    ctx->async_unsettled = false;
    return FRI_OK;
}

// The members' LDE on offset * <w_n> (batch_tables' powers): member b's d
// coefficients at src + b * src_stride into dst + b * dst_stride, a fixed
// number of launches.  Above the LDS transform it goes through BB_SCALED
// (batch * round4(d) words).
static void batch_lde(fri_ctx* ctx, const uint32_t* src, size_t src_stride, size_t d, uint32_t* dst, size_t dst_stride,
                      uint32_t log_n, uint32_t batch, hipStream_t s) {
    Batch& B = ctx->batch;
    if (log_n <= BATCH_LDS_LDE_MAX_LOG) {
        launch_batch_lde_lds(src, src_stride, d, dst, dst_stride, log_n, batch, ctx->tw_fwd, B.pre_lo, B.pre_hi, s);
        return;
    }
    const size_t sc_stride = round4(d);
    uint32_t* scaled = B.b.words(BB_SCALED);
    launch_batch_scale(src, src_stride, scaled, sc_stride, d, batch, B.pre_lo, B.pre_hi, s);
    NttPlan np = lde_plan(ctx, log_n);
    np.batch = batch;
    np.src_stride = sc_stride;
    np.dst_stride = dst_stride;
    launch_ntt(np, scaled, d, dst, s);
}

// The members' coset interpolation: dst_b[j] = 2^-lg base^j sum_i src_b[i] w^-ij,
// j < 2^lg (strides in words, multiples of 4 above the LDS transform).  The
// post-scale table is the context's (pow_lo / pow_hi), made on the stream.
static void batch_intt(fri_ctx* ctx, const uint32_t* src, size_t src_stride, uint32_t* dst, size_t dst_stride,
                       uint32_t lg, uint32_t batch, uint32_t base, hipStream_t s) {
    if (lg > BATCH_LDS_LDE_MAX_LOG) {
        coset_inverse(ctx, src, lg, base, 0, dst, batch, src_stride, dst_stride);
        return;
    }
    launch_pow_table(ctx->pow_lo, ctx->pow_hi, lg, base, post_scale(lg, 0), s);
    launch_batch_intt_lds(src, src_stride, dst, dst_stride, lg, batch, ctx->tw_inv, ctx->pow_lo, ctx->pow_hi, s);
}

// keep_trace: the commit of a resident trace batch's composition (the trace
// batch stays); deg0_max != 0: a member whose input has a larger degree fails
// with FRI_EDEGREE (the composition of a trace that violates its constraints).
static int run_batch(fri_ctx* ctx, const uint32_t* host_coeffs, const uint32_t* dev_coeffs, size_t d, uint32_t batch,
                     uint32_t log_n, uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
                     const uint32_t* forced_betas, fri_commit_result* out, int* status, bool keep_trace = false,
                     uint32_t deg0_max = 0) {
    if (!ctx || !out || !status) return fail(ctx, FRI_EINVAL, "null argument");
    if (d && !host_coeffs && !dev_coeffs) return fail(ctx, FRI_EINVAL, "null coefficients");
    int rc = batch_ctx_ok(ctx);
    if (rc) return rc;
    if (flags & ~(FRI_FLAG_FORCE_BETAS | FRI_FLAG_NO_GRAPH))
        return fail(ctx, FRI_EINVAL, "fri_commit_batch takes FRI_FLAG_FORCE_BETAS and FRI_FLAG_NO_GRAPH only");
    if (batch < 1 || batch > 65535) return fail(ctx, FRI_EINVAL, "batch must be 1..65535");
    if (log_n > FRI_BATCH_MAX_LOG_N) return fail(ctx, FRI_EINVAL, "log_n above FRI_BATCH_MAX_LOG_N");
    if ((rc = commit_validate(ctx, d, log_n, offset, 0u, nullptr))) return rc;
    const bool forced = (flags & FRI_FLAG_FORCE_BETAS) != 0;
    if (forced && !forced_betas) return fail(ctx, FRI_EINVAL, "forced betas missing");
    if (forced && !check_canonical(forced_betas, (size_t)batch * MAXR))
        return fail(ctx, FRI_EINVAL, "forced beta not canonical");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = batch_quiesce(ctx))) return rc;

    Batch& B = ctx->batch;
    Plan lay;
    size_t lw, tw, xw;
    plan_layout(lay, d, log_n, 1, 0, lw, tw, xw);
    const size_t lay_stride = round4(lw), tre_stride = tw, coef_stride = round4(d / 2 + 1);
    const size_t sc_stride = round4(d ? d : 1);
    const bool lds_lde = log_n <= BATCH_LDS_LDE_MAX_LOG;
    size_t want[BB_N] = {};
    want[BB_LAYERS] = batch * lay_stride * 4;
    want[BB_TREES] = batch * tre_stride * 4;
    want[BB_COEFA] = want[BB_COEFB] = batch * coef_stride * 4;
    want[BB_IN] = host_coeffs && d ? (size_t)batch * d * 4 : 0;
    want[BB_SCALED] = !lds_lde && d ? batch * sc_stride * 4 : 0;
    want[BB_STATES] = batch * sizeof(DevState);
    if ((rc = batch_tables(ctx, log_n, offset))) return rc;
    if ((rc = bufs_grow(ctx, B.b, want, batch))) return rc;

    // from here on the batch is the context's commit
    ctx->commit_gen++;
    ctx->h_state = ctx->h_sync;
    memset(ctx->h_sync, 0, sizeof(DevState));        // the single-commit read-backs find no layers
    ctx->res_lane = ctx->cur_lane;
    ctx->sharded_layers = 0;
    B.resident = true;
    if (!keep_trace) B.trace_resident = false;
    B.count = batch;
    B.log_n = log_n;
    B.lay = lay;
    B.lay_stride = lay_stride;
    B.tre_stride = tre_stride;
    B.coef_stride = coef_stride;
    DevState* hs = B.b.h_states;
    for (uint32_t b = 0; b < batch; b++)
        state_reset(&hs[b], chan_in ? &chan_in[b] : nullptr, flags, forced ? forced_betas + (size_t)b * MAXR : nullptr);

    hipStream_t s = ctx->stream;
    const uint32_t* src = dev_coeffs;
    if (host_coeffs && d) {
        FRI_HIP(ctx, hipMemcpyAsync(B.b.dev[BB_IN], host_coeffs, (size_t)batch * d * 4, hipMemcpyHostToDevice, s));
        src = B.b.words(BB_IN);
    }
    if (!d) src = B.b.words(BB_LAYERS);              // (never read: d0 == 0)
    DevState* ds = static_cast<DevState*>(B.b.dev[BB_STATES]);
    FRI_HIP(ctx, hipMemcpyAsync(ds, hs, batch * sizeof(DevState), hipMemcpyHostToDevice, s));
    // ---- LDE: layer 0 of every member, a fixed number of launches ----
    uint32_t* layers = B.b.words(BB_LAYERS);
    if (!d) {
        FRI_HIP(ctx, hipMemsetAsync(layers, 0, batch * lay_stride * 4, s));
    } else {
        batch_lde(ctx, src, d, d, layers, lay_stride, log_n, batch, s);
    }
    // ---- every member's commit: one launch ----
    BatchTask bt{};
    bt.layers = layers;
    bt.trees = B.b.words(BB_TREES);
    bt.coefA = B.b.words(BB_COEFA);
    bt.coefB = B.b.words(BB_COEFB);
    bt.coef_in = src;
    bt.xinv = B.xinv;
    bt.st = ds;
    bt.lay_stride = lay_stride;
    bt.tre_stride = tre_stride;
    bt.coef_stride = coef_stride;
    bt.in_stride = d;
    bt.log_n = log_n;
    bt.d0 = (uint32_t)d;
    bt.rmax = lay.rmax;
    const size_t n = (size_t)1 << log_n;
    for (int k = 0; k <= lay.rmax + 1; k++) {
        bt.layer_off[k] = (uint32_t)lay.layer_off[k];
        bt.tree_off[k] = (uint32_t)lay.tree_off[k];
        bt.xinv_off[k] = (uint32_t)(n - (n >> k));
    }
    launch_commit_batch(bt, batch, s);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipMemcpyAsync(hs, ds, batch * sizeof(DevState), hipMemcpyDeviceToHost, s));
    FRI_HIP(ctx, hipStreamSynchronize(s));

    int first = FRI_OK;
    uint32_t first_b = 0;
    bool first_degree = false, degree_b = false;
    for (uint32_t b = 0; b < batch; b++) {
        memset(&out[b], 0, sizeof out[b]);
        status[b] = commit_finish(ctx, &hs[b], log_n, &out[b]);     // (a failed member serves nothing: n_layers = 0)
        if (!status[b] && deg0_max && hs[b].deg[0] > (int32_t)deg0_max) {
            status[b] = FRI_EDEGREE;
            hs[b].status = FRI_EDEGREE;
            hs[b].n_layers = 0;          // no proof of a violated trace is served
            memset(&out[b], 0, sizeof out[b]);
            degree_b = true;
        } else {
            degree_b = false;
        }
        if (status[b] && !first) { first = status[b]; first_b = b; first_degree = degree_b; }
    }
    if (first)
        return fail(ctx, first,
                    "member " + std::to_string(first_b) + ": " +
                        (first_degree ? "composition polynomial degree exceeds T: the trace violates the constraints"
                                      : status_message((uint32_t)first)));
    return FRI_OK;
}

extern "C" int fri_commit_batch(fri_ctx* ctx, const uint32_t* coeffs, size_t d, uint32_t batch, uint32_t log_n,
                                uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
                                const uint32_t* forced_betas, fri_commit_result* out, int* status) {
    if (d && !coeffs) return fail(ctx, FRI_EINVAL, "null coefficients");
    return run_batch(ctx, coeffs, nullptr, d, batch, log_n, offset, chan_in, flags, forced_betas, out, status);
}

extern "C" int fri_commit_batch_device(fri_ctx* ctx, const uint32_t* d_coeffs, size_t d, uint32_t batch,
                                       uint32_t log_n, uint32_t offset, const fri_channel_state* chan_in,
                                       uint32_t flags, const uint32_t* forced_betas, fri_commit_result* out,
                                       int* status) {
    if (d && !d_coeffs) return fail(ctx, FRI_EINVAL, "null coefficients");
    return run_batch(ctx, nullptr, d_coeffs, d, batch, log_n, offset, chan_in, flags, forced_betas, out, status);
}

extern "C" int fri_batch_info(fri_ctx* ctx, uint64_t* generation, uint32_t* batch, uint32_t* log_n) {
    if (!ctx || !generation || !batch || !log_n) return fail(ctx, FRI_EINVAL, "null argument");
    *generation = ctx->commit_gen;
    *batch = ctx->batch.resident ? ctx->batch.count : 0u;
    *log_n = ctx->batch.resident ? ctx->batch.log_n : 0u;
    return FRI_OK;
}

// ------------------------------------------------------ batched prover ----
// B proofs of one shape (log_t, log_blowup, offset): what fri_trace_commit,
// fri_fibsq_composition_commit and the per-query read-backs do for one proof,
// for every member of a batch in a fixed number of launches.

// Pinned staging of at least `bytes` (allocated before the old one is freed).
static int hq_grow(fri_ctx* ctx, size_t bytes) {
    Batch& B = ctx->batch;
    if (bytes <= B.h_q_cap) return FRI_OK;
    uint8_t* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, FRI_ENOMEM, "pinned host allocation failed for the batch's staging");
    }
    if (B.h_q) hipHostFree(B.h_q);
    B.h_q = p;
    B.h_q_cap = bytes;
    return FRI_OK;
}

extern "C" int fri_trace_commit_batch(fri_ctx* ctx, const uint32_t* traces, uint32_t log_t, uint32_t log_blowup,
                                      uint32_t offset, uint32_t batch, uint8_t* roots32) {
    if (!ctx || !traces || !roots32) return fail(ctx, FRI_EINVAL, "null argument");
    int rc = batch_ctx_ok(ctx);
    if (rc) return rc;
    if (batch < 1 || batch > 65535) return fail(ctx, FRI_EINVAL, "batch must be 1..65535");
    FibsqParams q;                                   // (the checks are what the trace commit needs of it)
    if ((rc = fibsq_shape(ctx, log_t, log_blowup, offset, true, &q))) return rc;
    const uint32_t L = log_t + log_blowup;
    const size_t T = (size_t)1 << log_t, n = (size_t)1 << L;
    for (uint32_t b = 0; b < batch; b++)
        if (!check_canonical(traces + b * T, T))
            return fail(ctx, FRI_EINVAL, "member " + std::to_string(b) + ": trace value not canonical (>= p)");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = batch_quiesce(ctx))) return rc;
    Batch& B = ctx->batch;
    if ((rc = batch_tables(ctx, L, offset))) return rc;
    const size_t tree_stride = 8 * (2 * n);          // levels 0..L: 2n - 1 digests
    size_t want[BB_N] = {};
    want[BB_IN] = (size_t)batch * T * 4;
    want[BB_TCOEF] = (size_t)batch * T * 4;
    want[BB_SCALED] = L > BATCH_LDS_LDE_MAX_LOG ? (size_t)batch * T * 4 : 0;
    want[BB_TLDE] = (size_t)batch * n * 4;
    want[BB_TTREE] = (size_t)batch * tree_stride * 4;
    want[BB_TROOTS] = (size_t)batch * 32;
    if ((rc = hq_grow(ctx, (size_t)batch * 32))) return rc;
    if ((rc = bufs_grow(ctx, B.b, want, 0))) return rc;      // (a failure leaves an older trace batch resident)
    B.trace_resident = false;
    hipStream_t s = ctx->stream;
    uint32_t* in = B.b.words(BB_IN);
    uint32_t* coef = B.b.words(BB_TCOEF);
    uint32_t* lde = B.b.words(BB_TLDE);
    uint32_t* trees = B.b.words(BB_TTREE);
    uint32_t* roots = B.b.words(BB_TROOTS);
    FRI_HIP(ctx, hipMemcpyAsync(in, traces, (size_t)batch * T * 4, hipMemcpyHostToDevice, s));
    batch_intt(ctx, in, T, coef, T, log_t, batch, 1u, s);              // c_j = T^-1 sum_i trace_i w_T^-ij
    batch_lde(ctx, coef, T, T, lde, n, L, batch, s);                   // on offset * <w_n>
    launch_trace_trees_batch(lde, n, trees, tree_stride, L, batch, roots, s);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipMemcpyAsync(B.h_q, roots, (size_t)batch * 32, hipMemcpyDeviceToHost, s));
    FRI_HIP(ctx, hipStreamSynchronize(s));
    for (uint32_t b = 0; b < batch; b++)
        digest_to_bytes(reinterpret_cast<const uint32_t*>(B.h_q) + 8 * (size_t)b, roots32 + 32 * (size_t)b);
    B.trace_resident = true;
    B.trace_count = batch;
    B.trace_log_t = log_t;
    B.trace_log_b = log_blowup;
    B.trace_offset = offset;
    B.tlde_stride = n;
    B.ttree_stride = tree_stride;
    ctx->err.clear();
    return FRI_OK;
}

extern "C" int fri_fibsq_composition_commit_batch(fri_ctx* ctx, uint32_t log_t, uint32_t log_blowup, uint32_t offset,
                                                  uint32_t batch, const uint32_t* a_last, const uint32_t* alphas,
                                                  const fri_channel_state* chan_in, uint32_t flags,
                                                  fri_commit_result* out, int* status) {
    if (!ctx || !a_last || !alphas || !chan_in || !out || !status) return fail(ctx, FRI_EINVAL, "null argument");
    int rc = batch_ctx_ok(ctx);
    if (rc) return rc;
    Batch& B = ctx->batch;
    if (!B.trace_resident || B.trace_log_t != log_t || B.trace_log_b != log_blowup || B.trace_offset != offset ||
        B.trace_count != batch)
        return fail(ctx, FRI_ESTATE, "no resident trace batch with this (log_t, log_blowup, offset, batch)");
    if (flags & ~FRI_FLAG_NO_GRAPH)
        return fail(ctx, FRI_EINVAL, "fri_fibsq_composition_commit_batch takes FRI_FLAG_NO_GRAPH only");
    FibsqParams q;
    if (batch < 1 || batch > 65535) return fail(ctx, FRI_EINVAL, "batch must be 1..65535");
    if ((rc = fibsq_shape(ctx, log_t, log_blowup, offset, true, &q))) return rc;
    for (uint32_t b = 0; b < batch; b++)
        if (a_last[b] >= P || alphas[3 * b] >= P || alphas[3 * b + 1] >= P || alphas[3 * b + 2] >= P)
            return fail(ctx, FRI_EINVAL, "member " + std::to_string(b) + ": a_last / alphas not canonical");
    const uint32_t L = log_t + log_blowup;
    const size_t n = (size_t)1 << L, T = (size_t)1 << log_t;
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = batch_quiesce(ctx))) return rc;
    size_t want[BB_N] = {};
    want[BB_CP] = (size_t)batch * n * 4;
    want[BB_IN] = (size_t)batch * n * 4;
    want[BB_FIB] = (size_t)batch * sizeof(FibsqMember);
    if ((rc = hq_grow(ctx, (size_t)batch * sizeof(FibsqMember)))) return rc;
    if ((rc = bufs_grow(ctx, B.b, want, 0))) return rc;
    FibsqMember* hm = reinterpret_cast<FibsqMember*>(B.h_q);
    for (uint32_t b = 0; b < batch; b++) {
        for (int j = 0; j < 3; j++) hm[b].alpha_m[j] = to_mont(alphas[3 * b + j]);
        hm[b].a_last = a_last[b];
    }
    hipStream_t s = ctx->stream;
    FibsqMember* dm = static_cast<FibsqMember*>(B.b.dev[BB_FIB]);
    uint32_t* cp = B.b.words(BB_CP);
    uint32_t* coef = B.b.words(BB_IN);
    FRI_HIP(ctx, hipMemcpyAsync(dm, hm, (size_t)batch * sizeof(FibsqMember), hipMemcpyHostToDevice, s));
    launch_fibsq_cp_batch(B.b.words(BB_TLDE), B.tlde_stride, cp, n, dm, batch, q, s);
    // coefficients: c_j = n^-1 offset^-j sum_i cp_i w^-ij, all n of them (the
    // commit's degree scan then sees a composition of degree above T)
    batch_intt(ctx, cp, n, coef, n, L, batch, inv_std(offset), s);
    FRI_HIP(ctx, hipGetLastError());
    return run_batch(ctx, nullptr, coef, n, batch, L, offset, chan_in, flags, nullptr, out, status, true, (uint32_t)T);
}

// ------------------------------------------------ the queries of a batch ----
// fri_batch_query_round (one query of every member at the caller's indices)
// and fri_batch_query_phase (all the queries of every member, the channels'
// draws and sends included) are one run (run_queries) in chunks of members
// under a staging budget; per chunk one upload, the phase's k_query_chain,
// k_batch_query_all and one read-back on the context stream.  Reads and
// changes nothing of the resident batch.
namespace {
constexpr size_t QUERY_CHUNK_BYTES = (size_t)256 << 20;   // device and pinned staging of one chunk
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
// Sections of a chunk's staging for m members: the first three in BB_QMETA, the
// records in BB_QOUT; the pinned buffer holds all four, the records last.
struct QuerySections {
    size_t chan, nl, idx, meta, rec, total;
    QuerySections(size_t m, size_t q, size_t rec_words) {
        size_t o = 0;
        chan = o; o += al256(m * sizeof(fri_channel_state));
        nl = o;   o += al256(m * 4);
        idx = o;  o += al256(m * q * 8);
        meta = o;
        rec = m * q * rec_words * 4;
        total = meta + rec;
    }
};
}  // namespace

extern "C" int fri_debug_set_query_chunk(fri_ctx* ctx, uint32_t members) {
    if (!ctx) return FRI_EINVAL;
    ctx->batch.query_chunk = members;
    return FRI_OK;
}

// The resident batch the queries are served from, and the trace batch behind it.
static int query_batch_ok(fri_ctx* ctx, uint32_t trace_count) {
    const Batch& B = ctx->batch;
    if (!B.resident)
        return fail(ctx, FRI_ESTATE,
                    "no resident batch: fri_batch_* serve the last fri_commit_batch until the next commit");
    if (trace_count > 8) return fail(ctx, FRI_EINVAL, "trace_count must be 0..8");
    if (trace_count && (!B.trace_resident || B.trace_count != B.count || B.trace_log_t + B.trace_log_b != B.log_n))
        return fail(ctx, FRI_ESTATE, "no resident trace batch behind this batch (fri_trace_commit_batch)");
    return FRI_OK;
}

// The layers member b is served with: none when it is skipped or its commit failed.
static uint32_t served_layers(const Batch& B, const uint8_t* skip, uint32_t b) {
    return (skip && skip[b]) ? 0u : B.b.h_states[b].n_layers;
}

// Q queries of every served member into the caller's records, which it scatters
// from the chunks' staging.  The round: Q = 1 at idx_in[b], the gather alone.
// The phase (chan != nullptr): the indices are drawn below `range` from chan[b],
// which takes the openings and is written back with the indices (idx_out).
// The arguments are the entry points', checked by them but for the strides.
static int run_queries(fri_ctx* ctx, uint32_t Q, const uint64_t* idx_in, fri_channel_state* chan, uint64_t range,
                       const uint8_t* skip, uint32_t trace_count, uint64_t trace_stride, uint64_t* idx_out,
                       uint32_t* values, size_t values_stride, uint8_t* paths, size_t paths_stride, size_t* paths_len) {
    Batch& B = ctx->batch;
    const uint32_t batch = B.count;
    // who is served, and the record's shape
    RecordShape rs{B.log_n, trace_count, 0};
    uint32_t served = 0;
    for (uint32_t b = 0; b < batch; b++) {
        const uint32_t nl = served_layers(B, skip, b);
        if (!nl) continue;
        rs.max_layers = std::max(rs.max_layers, nl);
        served++;
    }
    const size_t val_words = rs.val_words(), rec_words = rs.rec_words();
    if (served && (values_stride < val_words || paths_stride < rs.path_words(rs.max_layers) * 4)) {
        paths_len[0] = rs.path_words(rs.max_layers) * 4;
        return fail(ctx, FRI_EINVAL,
                    "record strides too small (values: trace_count + 2 per layer words; paths: see paths_len[0])");
    }
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    // members per chunk: what the byte budget holds, or the hook's count; halved while the staging does not fit
    size_t chunk = B.query_chunk ? B.query_chunk
                                 : std::max<size_t>(QUERY_CHUNK_BYTES / QuerySections(1, Q, rec_words).total, 1);
    chunk = std::min<size_t>(chunk, batch);
    if (served)
        for (;;) {
            const QuerySections S(chunk, Q, rec_words);
            size_t want[BB_N] = {};
            want[BB_QMETA] = S.meta;
            want[BB_QOUT] = S.rec;
            rc = hq_grow(ctx, S.total);
            if (!rc) rc = bufs_grow(ctx, B.b, want, 0);
            if (!rc) break;
            if (rc != FRI_ENOMEM || B.query_chunk || chunk == 1) return rc;
            chunk = (chunk + 1) / 2;
        }
    for (uint32_t b = 0; b < batch; b++) paths_len[b] = 0;
    if (!served) {
        if (chan) ctx->err.clear();          // (the round leaves the last error's text)
        return FRI_OK;
    }

    QueryPhase qp{};
    qp.layers = B.b.words(BB_LAYERS);
    qp.trees = B.b.words(BB_TREES);
    qp.lay_stride = B.lay_stride;
    qp.tre_stride = B.tre_stride;
    qp.tlde = B.b.words(BB_TLDE);
    qp.ttree = B.b.words(BB_TTREE);
    qp.tlde_stride = B.tlde_stride;
    qp.ttree_stride = B.ttree_stride;
    qp.rec_words = rec_words;
    qp.trace_stride = trace_stride;
    qp.range = range;
    qp.num_queries = Q;
    qp.log_n = B.log_n;
    qp.trace_count = trace_count;
    qp.max_layers = rs.max_layers;
    for (int k = 0; k <= B.lay.rmax + 1; k++) {
        qp.layer_off[k] = (uint32_t)B.lay.layer_off[k];
        qp.tree_off[k] = (uint32_t)B.lay.tree_off[k];
    }
    hipStream_t s = ctx->stream;
    uint8_t* dmeta = static_cast<uint8_t*>(B.b.dev[BB_QMETA]);
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t m = std::min<size_t>(chunk, batch - b0);
        const QuerySections S(m, Q, rec_words);
        fri_channel_state* hchan = reinterpret_cast<fri_channel_state*>(B.h_q + S.chan);
        uint32_t* hnl = reinterpret_cast<uint32_t*>(B.h_q + S.nl);
        uint64_t* hidx = reinterpret_cast<uint64_t*>(B.h_q + S.idx);
        const uint32_t* hrec = reinterpret_cast<const uint32_t*>(B.h_q + S.meta);
        bool any = false;
        for (size_t i = 0; i < m; i++) {
            if (chan) hchan[i] = chan[b0 + i];
            else hidx[i] = idx_in[b0 + i];
            hnl[i] = served_layers(B, skip, (uint32_t)(b0 + i));
            any = any || hnl[i];
        }
        if (!any) continue;
        // up: the phase's states and n_layers (it draws the indices), the round's n_layers and indices
        const size_t up0 = chan ? S.chan : S.nl, up1 = chan ? S.idx : S.meta;
        FRI_HIP(ctx, hipMemcpyAsync(dmeta + up0, B.h_q + up0, up1 - up0, hipMemcpyHostToDevice, s));
        qp.n_layers = reinterpret_cast<const uint32_t*>(dmeta + S.nl);
        qp.chan = reinterpret_cast<uint32_t*>(dmeta + S.chan);
        qp.indices = reinterpret_cast<uint64_t*>(dmeta + S.idx);
        qp.out = B.b.words(BB_QOUT);
        qp.first = (uint32_t)b0;
        qp.members = (uint32_t)m;
        if (chan) launch_query_chain(qp, s);
        launch_query_gather(qp, s);
        FRI_HIP(ctx, hipGetLastError());
        if (chan) FRI_HIP(ctx, hipMemcpyAsync(B.h_q, dmeta, S.meta, hipMemcpyDeviceToHost, s));
        FRI_HIP(ctx, hipMemcpyAsync(B.h_q + S.meta, qp.out, S.rec, hipMemcpyDeviceToHost, s));
        // the next chunk reuses the staging
        FRI_HIP(ctx, hipStreamSynchronize(s));
        for (size_t i = 0; i < m; i++) {
            const uint32_t nl = hnl[i];
            if (!nl) continue;
            const size_t b = b0 + i;
            if (chan) chan[b] = hchan[i];
            for (size_t qi = 0; qi < Q; qi++) {
                const uint32_t* rec = hrec + (i * Q + qi) * rec_words;
                if (idx_out) idx_out[b * Q + qi] = hidx[i * Q + qi];
                memcpy(values + (b * Q + qi) * values_stride, rec, (trace_count + 2 * (size_t)nl) * 4);
                memcpy(paths + (b * Q + qi) * paths_stride, rec + val_words, rs.path_words(nl) * 4);
            }
            paths_len[b] = rs.path_words(nl) * 4;
        }
    }
    ctx->err.clear();
    return FRI_OK;
}

extern "C" int fri_batch_query_round(fri_ctx* ctx, const uint64_t* indices, const uint8_t* skip, uint32_t trace_count,
                                     uint64_t trace_stride, uint32_t* values, size_t values_stride, uint8_t* paths,
                                     size_t paths_stride, size_t* paths_len) {
    if (!ctx || !indices || !values || !paths || !paths_len) return fail(ctx, FRI_EINVAL, "null argument");
    int rc = query_batch_ok(ctx, trace_count);       // (no batch_ctx_ok: a profiling context serves rounds)
    if (rc) return rc;
    const Batch& B = ctx->batch;
    // (the FRI openings take any index, mod the layer's size, as fri_decommit_query; the trace's do not)
    for (uint32_t b = 0; trace_count && b < B.count; b++)
        if (served_layers(B, skip, b) && (indices[b] >> B.log_n))
            return fail(ctx, FRI_EINVAL, "member " + std::to_string(b) + ": index out of range");
    return run_queries(ctx, 1, indices, nullptr, 0, skip, trace_count, trace_stride, nullptr, values, values_stride,
                       paths, paths_stride, paths_len);
}

extern "C" int fri_batch_query_phase(fri_ctx* ctx, uint32_t num_queries, uint64_t max_index, fri_channel_state* chan,
                                     const uint8_t* skip, uint32_t trace_count, uint64_t trace_stride,
                                     uint64_t* indices, uint32_t* values, size_t values_stride, uint8_t* paths,
                                     size_t paths_stride, size_t* paths_len) {
    static_assert(sizeof(fri_channel_state) == 36, "k_query_chain reads a channel state as 9 words");
    if (!ctx || !chan || !paths_len || (num_queries && (!indices || !values || !paths)))
        return fail(ctx, FRI_EINVAL, "null argument");
    int rc = batch_ctx_ok(ctx);
    if (!rc) rc = query_batch_ok(ctx, trace_count);
    if (rc) return rc;
    const Batch& B = ctx->batch;
    if (max_index >> 32) return fail(ctx, FRI_EINVAL, "max_index must be below 2^32");
    // (the FRI openings take any index, mod the layer's size; the trace's do not)
    if (trace_count && (max_index >> B.log_n))
        return fail(ctx, FRI_EINVAL, "max_index must be below 2^log_n with trace_count > 0");
    if (num_queries > FRI_VERIFY_MAX_QUERIES) return fail(ctx, FRI_EINVAL, "num_queries above FRI_VERIFY_MAX_QUERIES");
    if (num_queries == 0) {
        ctx->err.clear();
        return FRI_OK;
    }
    for (uint32_t b = 0; b < B.count; b++)
        if (served_layers(B, skip, b) && !chan[b].has_state)
            return fail(ctx, FRI_EINVAL,
                        "member " + std::to_string(b) + ": an empty channel state draws no index (channel.rs:65)");
    return run_queries(ctx, num_queries, nullptr, chan, max_index + 1, skip, trace_count, trace_stride, indices, values,
                       values_stride, paths, paths_stride, paths_len);
}
