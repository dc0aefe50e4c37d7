// fri_readback.hip — what a commit leaves in HBM, read back: layers and
// tree levels (FRIProof, fri_commit.rs:9-13), authentication paths and whole
// query decommitments (decommit_fri_layers, fri_commit.rs:137-163).  One set
// of bodies reads a ProofView (fri_host.hpp): the single commit's entry points
// and the member-wise ones (fri_batch_*, the resident batch's members) are
// argument checks around them.
#include "fri_host.hpp"

// After fri_commit_batch the context holds the members' proofs, not a single
// commit's: the single-commit read-backs refuse and say where to look.
int fri::no_layer(fri_ctx* ctx, const char* what) {
    return fail(ctx, FRI_ESTATE,
                ctx->batch.resident ? "the resident commit is a batch: read it with fri_batch_* (member-wise)" : what);
}

// ------------------------------------------------------------ the views ----
ProofView fri::single_view(fri_ctx* ctx) {
    settle(ctx);
    const Plan& p = ctx->plan;
    const DevState* st = ctx->h_state;
    return ProofView{p.layers, p.trees, p.layer_off, p.tree_off, p.log_n, p.valid ? st->n_layers : 0, st, false};
}

// Member `member` of the resident batch (n_layers = 0 when its commit failed).
static int member_view(fri_ctx* ctx, uint32_t member, ProofView* v) {
    const Batch& B = ctx->batch;
    if (!B.resident)
        return fail(ctx, FRI_ESTATE, "no resident batch: fri_batch_* serve the last fri_commit_batch until the next commit");
    if (member >= B.count) return fail(ctx, FRI_EINVAL, "no such member");
    const DevState* st = &B.b.h_states[member];
    *v = ProofView{B.b.words(BB_LAYERS) + member * B.lay_stride, B.b.words(BB_TREES) + member * B.tre_stride,
                   B.lay.layer_off, B.lay.tree_off, B.log_n, st->n_layers, st, true};
    return FRI_OK;
}

static int no_such(fri_ctx* ctx, const ProofView& v, const char* what) {
    return v.member ? fail(ctx, FRI_ESTATE, std::string(what) + " of this member") : no_layer(ctx, what);
}

// A layer of the single commit that is held block-wise across ranks
// (fri_commit_sharded): a team root reads it through its ranks, a lone rank
// refuses with only_block.
static bool on_ranks(fri_ctx* ctx, const ProofView& v, uint32_t layer) {
    return layer < v.n_layers && layer < ctx->sharded_layers;
}
static int only_block(fri_ctx* ctx) {
    return fail(ctx, FRI_ESTATE, "layer was committed sharded: this rank holds only its block (fri_commit_sharded)");
}

// ----------------------------------------------------------- the bodies ----
static int layer_copy(fri_ctx* ctx, const ProofView& v, uint32_t layer, uint32_t* out, size_t cap) {
    if (layer >= v.n_layers) return no_such(ctx, v, "no such committed layer");
    const size_t m = (size_t)1 << (v.log_n - layer);
    if (cap < m) return fail(ctx, FRI_EINVAL, "output buffer too small");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    // on the context stream: the null stream would hold a hardware queue of
    // its own (GPU_MAX_HW_QUEUES) for the rest of the process, one fewer for
    // the commit lanes and other contexts
    FRI_HIP(ctx, hipMemcpyAsync(out, v.layers + v.layer_off[layer], m * 4, hipMemcpyDeviceToHost, ctx->stream));
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FRI_OK;
}

// The checks of a tree-level read; *cnt = the level's digests.
static int level_count(fri_ctx* ctx, const ProofView& v, uint32_t layer, uint32_t level, size_t cap, size_t* cnt) {
    if (layer >= v.n_layers) return no_such(ctx, v, "no such committed layer");
    const uint32_t L = v.log_n - layer;
    if (level > L) return fail(ctx, FRI_EINVAL, "level above root");
    *cnt = (size_t)1 << (L - level);
    if (cap < *cnt * 32) return fail(ctx, FRI_EINVAL, "output buffer too small");
    return FRI_OK;
}
static void digests_out(const std::vector<uint32_t>& w, uint8_t* out) {
    for (size_t i = 0; i < w.size() / 8; i++) digest_to_bytes(&w[8 * i], out + 32 * i);
}

static int tree_level_copy(fri_ctx* ctx, const ProofView& v, uint32_t layer, uint32_t level, uint8_t* out, size_t cap) {
    size_t cnt;
    const int rc = level_count(ctx, v, layer, level, cap, &cnt);
    if (rc) return rc;
    std::vector<uint32_t> w(cnt * 8);
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    FRI_HIP(ctx, hipMemcpyAsync(w.data(), v.trees + v.tree_off[layer] + 8 * level_offset(v.log_n - layer, level),
                                cnt * 32, hipMemcpyDeviceToHost, ctx->stream));   // (not the null stream: layer_copy)
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    digests_out(w, out);
    return FRI_OK;
}

static int commit_degrees(fri_ctx* ctx, const ProofView& v, int32_t* out, size_t cap, uint32_t* n_out) {
    const uint32_t n = v.st->n_layers;
    *n_out = n;
    if (n && (!out || cap < n)) return fail(ctx, FRI_EINVAL, "degree buffer too small (n_layers entries)");
    for (uint32_t k = 0; k < n; k++) out[k] = v.st->deg[k];
    return FRI_OK;
}

int fri::decommit_plan(fri_ctx* ctx, const ProofView& v, uint64_t index, size_t values_cap, const uint8_t* paths,
                       size_t paths_cap, size_t* paths_len, DecommitPlan* dp, uint32_t* words) {
    *dp = DecommitPlan{};
    dp->index = index;
    dp->log_n = v.log_n;
    dp->n_layers = v.n_layers;
    uint32_t w = 0;
    for (uint32_t k = 0; k < v.n_layers; k++) {
        dp->layer_off[k] = v.layer_off[k];
        dp->tree_off[k] = v.tree_off[k];
        dp->path_off[k] = w;
        w += 16 * (v.log_n - k);
    }
    *words = w;
    *paths_len = (size_t)w * 4;
    if (values_cap < 2 * (size_t)v.n_layers) return fail(ctx, FRI_EINVAL, "values buffer too small (2 per layer)");
    if (!paths || paths_cap < (size_t)w * 4) return fail(ctx, FRI_EINVAL, "paths buffer too small (see paths_len)");
    if ((2 * (size_t)v.n_layers + w) * 4 > 65536) return fail(ctx, FRI_EINVAL, "decommitment too large");
    return FRI_OK;
}

// The gather kernel writes a query's values and paths (<= 64 KiB) straight
// into coherent pinned host memory: no device-to-host copy per query (a copy
// of that size took either ~25 or ~130 us per query, varying from process to
// process; the zero-copy write does not go through the copy engines).
int fri::dq_alloc(fri_ctx* ctx) {
    if (!ctx->dq_host) FRI_HIP(ctx, hipHostMalloc(&ctx->dq_host, 65536, hipHostMallocMapped | hipHostMallocCoherent));
    if (!ctx->dq_dev) {
        void* d = nullptr;
        FRI_HIP(ctx, hipHostGetDevicePointer(&d, ctx->dq_host, 0));
        ctx->dq_dev = static_cast<uint32_t*>(d);
    }
    return FRI_OK;
}

static int decommit_query(fri_ctx* ctx, const ProofView& v, uint64_t index, uint32_t* values, size_t values_cap,
                          uint8_t* paths, size_t paths_cap, size_t* paths_len) {
    if (v.n_layers == 0) return no_such(ctx, v, "no committed layers");
    DecommitPlan dp;
    uint32_t words;
    int rc = decommit_plan(ctx, v, index, values_cap, paths, paths_cap, paths_len, &dp, &words);
    if (rc) return rc;
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = dq_alloc(ctx))) return rc;
    launch_decommit_gather(v.layers, v.trees, dp, ctx->dq_dev, ctx->stream);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(values, ctx->dq_host, 2 * dp.n_layers * 4);
    memcpy(paths, ctx->dq_host + 2 * dp.n_layers, (size_t)words * 4);
    return FRI_OK;
}

// ------------------------------------------------------ the single commit ----
extern "C" int fri_layer_copy(fri_ctx* ctx, uint32_t layer, uint32_t* out, size_t cap) {
    if (!ctx || !out) return fail(ctx, FRI_EINVAL, "null argument");
    const ProofView v = single_view(ctx);
    if (on_ranks(ctx, v, layer)) {
        if (!ctx->team_root) return only_block(ctx);
        if (cap < (size_t)1 << (v.log_n - layer)) return fail(ctx, FRI_EINVAL, "output buffer too small");
        return team_layer_copy(ctx, layer, out);     // the ranks' blocks
    }
    return layer_copy(ctx, v, layer, out, cap);
}

extern "C" int fri_tree_level_copy(fri_ctx* ctx, uint32_t layer, uint32_t level, uint8_t* out, size_t cap) {
    if (!ctx || !out) return fail(ctx, FRI_EINVAL, "null argument");
    const ProofView v = single_view(ctx);
    if (on_ranks(ctx, v, layer)) {
        if (!ctx->team_root) return only_block(ctx);
        size_t cnt;
        int rc = level_count(ctx, v, layer, level, cap, &cnt);
        if (rc) return rc;
        std::vector<uint32_t> w(cnt * 8);
        if ((rc = team_tree_level_copy(ctx, layer, level, w.data()))) return rc;     // block trees + top tree
        digests_out(w, out);
        return FRI_OK;
    }
    return tree_level_copy(ctx, v, layer, level, out, cap);
}

// One query's value and path through the decommitment gather kernel (a
// one-layer DecommitPlan): one launch that writes the big-endian path
// straight into the pinned host buffer, instead of one blocking copy per
// tree level.
extern "C" int fri_auth_path(fri_ctx* ctx, uint32_t layer, uint64_t index, uint32_t* value_out, uint8_t* path,
                             uint32_t* depth_out) {
    if (!ctx || !value_out || !depth_out) return fail(ctx, FRI_EINVAL, "null argument");
    const ProofView v = single_view(ctx);
    if (layer >= v.n_layers) return no_layer(ctx, "no such committed layer");
    if (on_ranks(ctx, v, layer) && !ctx->team_root) return only_block(ctx);
    uint32_t L = v.log_n - layer;
    if (index >> L) return fail(ctx, FRI_EINVAL, "index out of range");
    if (on_ranks(ctx, v, layer)) {
        // a team commit: the decommitment of `index` (idx_k = index mod m_k =
        // index for this layer) through the ranks, then this layer's part
        const uint32_t nl = v.n_layers;
        size_t total = 0, off = 0;
        for (uint32_t k = 0; k < nl; k++) {
            if (k == layer) off = total;
            total += (size_t)64 * (v.log_n - k);
        }
        std::vector<uint32_t> vals(2 * (size_t)nl);
        std::vector<uint8_t> pb(total);
        size_t plen = 0;
        const int rc = team_decommit(ctx, index, vals.data(), vals.size(), pb.data(), pb.size(), &plen);
        if (rc) return rc;
        *value_out = vals[2 * layer];
        if (path) memcpy(path, pb.data() + off, (size_t)32 * L);
        *depth_out = L;
        return FRI_OK;
    }
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    int rc = dq_alloc(ctx);
    if (rc) return rc;
    DecommitPlan dp{};
    dp.index = index;
    dp.log_n = L;
    dp.n_layers = 1;
    dp.layer_off[0] = v.layer_off[layer];
    dp.tree_off[0] = v.tree_off[layer];
    launch_decommit_gather(v.layers, v.trees, dp, ctx->dq_dev, ctx->stream);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *value_out = ctx->dq_host[0];
    if (path) memcpy(path, ctx->dq_host + 2, (size_t)32 * L);     // [value, sibling value, path(index), ...]
    *depth_out = L;
    return FRI_OK;
}

extern "C" int fri_decommit_query(fri_ctx* ctx, uint64_t index, uint32_t* values, size_t values_cap,
                                  uint8_t* paths, size_t paths_cap, size_t* paths_len) {
    if (!ctx || !values || !paths_len) return fail(ctx, FRI_EINVAL, "null argument");
    const ProofView v = single_view(ctx);
    if (v.n_layers && ctx->sharded_layers && ctx->team_root)
        return team_decommit(ctx, index, values, values_cap, paths, paths_cap, paths_len);
    if (v.n_layers && ctx->sharded_layers)
        return fail(ctx, FRI_ESTATE, "last commit was sharded: each rank holds only its blocks of the large layers");
    return decommit_query(ctx, v, index, values, values_cap, paths, paths_cap, paths_len);
}

extern "C" int fri_commit_degrees(fri_ctx* ctx, int32_t* out, size_t cap, uint32_t* n_out) {
    if (!ctx || !n_out) return fail(ctx, FRI_EINVAL, "null argument");
    return commit_degrees(ctx, single_view(ctx), out, cap, n_out);
}

// ------------------------------------------- a member of the resident batch ----
extern "C" int fri_batch_layer_copy(fri_ctx* ctx, uint32_t member, uint32_t layer, uint32_t* out, size_t cap) {
    if (!ctx || !out) return fail(ctx, FRI_EINVAL, "null argument");
    ProofView v;
    const int rc = member_view(ctx, member, &v);
    return rc ? rc : layer_copy(ctx, v, layer, out, cap);
}

extern "C" int fri_batch_tree_level_copy(fri_ctx* ctx, uint32_t member, uint32_t layer, uint32_t level, uint8_t* out,
                                         size_t cap) {
    if (!ctx || !out) return fail(ctx, FRI_EINVAL, "null argument");
    ProofView v;
    const int rc = member_view(ctx, member, &v);
    return rc ? rc : tree_level_copy(ctx, v, layer, level, out, cap);
}

extern "C" int fri_batch_commit_degrees(fri_ctx* ctx, uint32_t member, int32_t* out, size_t cap, uint32_t* n_out) {
    if (!ctx || !n_out) return fail(ctx, FRI_EINVAL, "null argument");
    ProofView v;
    const int rc = member_view(ctx, member, &v);
    if (rc) return rc;
    if (v.st->status) return fail(ctx, FRI_ESTATE, "this member's commit failed");
    return commit_degrees(ctx, v, out, cap, n_out);
}

// fri_decommit_query on the member's slices (its layout is the plan's).
extern "C" int fri_batch_decommit_query(fri_ctx* ctx, uint32_t member, uint64_t index, uint32_t* values,
                                        size_t values_cap, uint8_t* paths, size_t paths_cap, size_t* paths_len) {
    if (!ctx || !values || !paths_len) return fail(ctx, FRI_EINVAL, "null argument");
    ProofView v;
    const int rc = member_view(ctx, member, &v);
    return rc ? rc : decommit_query(ctx, v, index, values, values_cap, paths, paths_cap, paths_len);
}
