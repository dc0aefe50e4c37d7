// fri_batch.hip — fri_commit_batch: B independent commits of one shape
// (src/fri/fri_commit.rs:72-122 each) in one call.  The LDE of every member
// is a fixed number of launches, then ONE launch commits them all, one
// workgroup per member (k_commit_batch, fri_layer.hip).  The batch has its
// own buffers (Batch, fri_host.hpp): no lane's plan or graph is touched, so a
// single commit afterwards replays what it captured.  Member-wise read-backs.
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

static int run_batch(fri_ctx* ctx, const uint32_t* host_coeffs, const uint32_t* dev_coeffs, size_t d, uint32_t batch,
                     uint32_t log_n, uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
                     const uint32_t* forced_betas, fri_commit_result* out, int* status) {
    if (!ctx || !out || !status) return fail(ctx, FRI_EINVAL, "null argument");
    if (d && !host_coeffs && !dev_coeffs) return fail(ctx, FRI_EINVAL, "null coefficients");
    if (ctx->team_root || ctx->tp.team)
        return fail(ctx, FRI_EINVAL, "multi-GPU context: batched commits run on one-device contexts");
    if (ctx->profiling) return fail(ctx, FRI_ESTATE, "profiling: time commits with fri_commit_device");
    if (flags & ~(FRI_FLAG_FORCE_BETAS | FRI_FLAG_NO_GRAPH))
        return fail(ctx, FRI_EINVAL, "fri_commit_batch takes FRI_FLAG_FORCE_BETAS and FRI_FLAG_NO_GRAPH only");
    if (batch < 1 || batch > 65535) return fail(ctx, FRI_EINVAL, "batch must be 1..65535");
    if (log_n > FRI_BATCH_MAX_LOG_N) return fail(ctx, FRI_EINVAL, "log_n above FRI_BATCH_MAX_LOG_N");
    int rc = commit_validate(ctx, d, log_n, offset, 0u, nullptr);
    if (rc) return rc;
    const bool forced = (flags & FRI_FLAG_FORCE_BETAS) != 0;
    if (forced && !forced_betas) return fail(ctx, FRI_EINVAL, "forced betas missing");
    if (forced && !check_canonical(forced_betas, (size_t)batch * MAXR))
        return fail(ctx, FRI_EINVAL, "forced beta not canonical");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    // pending pipelined commits first, on whichever lane (the tables below use the context's scratch)
    settle(ctx);
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (Lane& ln : ctx->lanes)
        if (ln.stream) FRI_HIP(ctx, hipStreamSynchronize(ln.stream));
    ctx->async_unsettled = false;

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
    } else if (lds_lde) {
        launch_batch_lde_lds(src, d, d, layers, lay_stride, log_n, batch, ctx->tw_fwd, B.pre_lo, B.pre_hi, s);
    } else {
        uint32_t* scaled = B.b.words(BB_SCALED);
        launch_batch_scale(src, d, scaled, sc_stride, d, batch, B.pre_lo, B.pre_hi, s);
        NttPlan np = lde_plan(ctx, log_n);
        np.batch = batch;
        np.src_stride = sc_stride;
        np.dst_stride = lay_stride;
        launch_ntt(np, scaled, d, layers, s);
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
    for (uint32_t b = 0; b < batch; b++) {
        memset(&out[b], 0, sizeof out[b]);
        status[b] = commit_finish(ctx, &hs[b], log_n, &out[b]);     // (a failed member serves nothing: n_layers = 0)
        if (status[b] && !first) { first = status[b]; first_b = b; }
    }
    if (first)
        return fail(ctx, first, "member " + std::to_string(first_b) + ": " + status_message((uint32_t)first));
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

// The resident batch's member: its copied-out state (n_layers = 0 when it failed).
static int batch_member(fri_ctx* ctx, uint32_t member, const DevState** h) {
    if (!ctx) return FRI_EINVAL;
    const Batch& B = ctx->batch;
    if (!B.resident)
        return fail(ctx, FRI_ESTATE, "no resident batch: fri_batch_* serve the last fri_commit_batch until the next commit");
    if (member >= B.count) return fail(ctx, FRI_EINVAL, "no such member");
    *h = &B.b.h_states[member];
    return FRI_OK;
}

extern "C" int fri_batch_layer_copy(fri_ctx* ctx, uint32_t member, uint32_t layer, uint32_t* out, size_t cap) {
    if (!ctx || !out) return fail(ctx, FRI_EINVAL, "null argument");
    const DevState* h;
    int rc = batch_member(ctx, member, &h);
    if (rc) return rc;
    const Batch& B = ctx->batch;
    if (layer >= h->n_layers) return fail(ctx, FRI_ESTATE, "no such committed layer of this member");
    const size_t m = (size_t)1 << (B.log_n - layer);
    if (cap < m) return fail(ctx, FRI_EINVAL, "output buffer too small");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    FRI_HIP(ctx, hipMemcpyAsync(out, B.b.words(BB_LAYERS) + member * B.lay_stride + B.lay.layer_off[layer], m * 4,
                                hipMemcpyDeviceToHost, ctx->stream));
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FRI_OK;
}

extern "C" int fri_batch_tree_level_copy(fri_ctx* ctx, uint32_t member, uint32_t layer, uint32_t level, uint8_t* out,
                                         size_t cap) {
    if (!ctx || !out) return fail(ctx, FRI_EINVAL, "null argument");
    const DevState* h;
    int rc = batch_member(ctx, member, &h);
    if (rc) return rc;
    const Batch& B = ctx->batch;
    if (layer >= h->n_layers) return fail(ctx, FRI_ESTATE, "no such committed layer of this member");
    const uint32_t L = B.log_n - layer;
    if (level > L) return fail(ctx, FRI_EINVAL, "level above root");
    const size_t cnt = (size_t)1 << (L - level);
    if (cap < cnt * 32) return fail(ctx, FRI_EINVAL, "output buffer too small");
    std::vector<uint32_t> w(cnt * 8);
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    FRI_HIP(ctx, hipMemcpyAsync(w.data(),
                                B.b.words(BB_TREES) + member * B.tre_stride + B.lay.tree_off[layer] +
                                    8 * level_offset(L, level),
                                cnt * 32, hipMemcpyDeviceToHost, ctx->stream));
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < cnt; i++) digest_to_bytes(&w[8 * i], out + 32 * i);
    return FRI_OK;
}

extern "C" int fri_batch_commit_degrees(fri_ctx* ctx, uint32_t member, int32_t* out, size_t cap, uint32_t* n_out) {
    if (!ctx || !n_out) return fail(ctx, FRI_EINVAL, "null argument");
    const DevState* h;
    int rc = batch_member(ctx, member, &h);
    if (rc) return rc;
    if (h->status) return fail(ctx, FRI_ESTATE, "this member's commit failed");
    const uint32_t n = h->n_layers;
    *n_out = n;
    if (n && (!out || cap < n)) return fail(ctx, FRI_EINVAL, "degree buffer too small (n_layers entries)");
    for (uint32_t k = 0; k < n; k++) out[k] = h->deg[k];
    return FRI_OK;
}

// fri_decommit_query on the member's slices (its layout is the plan's).
extern "C" int fri_batch_decommit_query(fri_ctx* ctx, uint32_t member, uint64_t index, uint32_t* values,
                                        size_t values_cap, uint8_t* paths, size_t paths_cap, size_t* paths_len) {
    if (!ctx || !values || !paths_len) return fail(ctx, FRI_EINVAL, "null argument");
    const DevState* h;
    int rc = batch_member(ctx, member, &h);
    if (rc) return rc;
    const Batch& B = ctx->batch;
    if (h->n_layers == 0) return fail(ctx, FRI_ESTATE, "no committed layers of this member");
    DecommitPlan dp{};
    dp.index = index;
    dp.log_n = B.log_n;
    dp.n_layers = h->n_layers;
    uint32_t words = 0;
    for (uint32_t k = 0; k < dp.n_layers; k++) {
        dp.layer_off[k] = B.lay.layer_off[k];
        dp.tree_off[k] = B.lay.tree_off[k];
        dp.path_off[k] = words;
        words += 16 * (B.log_n - k);
    }
    *paths_len = (size_t)words * 4;
    if (values_cap < 2 * (size_t)dp.n_layers) return fail(ctx, FRI_EINVAL, "values buffer too small (2 per layer)");
    if (!paths || paths_cap < (size_t)words * 4) return fail(ctx, FRI_EINVAL, "paths buffer too small (see paths_len)");
    if ((2 * (size_t)dp.n_layers + words) * 4 > 65536) return fail(ctx, FRI_EINVAL, "decommitment too large");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = dq_alloc(ctx))) return rc;
    launch_decommit_gather(B.b.words(BB_LAYERS) + member * B.lay_stride, B.b.words(BB_TREES) + member * B.tre_stride, dp,
                           ctx->dq_dev, ctx->stream);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(values, ctx->dq_host, 2 * dp.n_layers * 4);
    memcpy(paths, ctx->dq_host + 2 * dp.n_layers, (size_t)words * 4);
    return FRI_OK;
}
