// fri_grind.hip — proof-of-work grinding before the query phase (fri_grind,
// fri_grind_batch, include/fri_amd.h): argument checks, the
// staging buffers and the walk over windows of nonces (kernels in
// fri_prover.hip).  Reads and changes nothing of the resident commit, batch or
// trace batch.
#include "fri_host.hpp"

static_assert(sizeof(fri_channel_state) == 36, "the grind kernels read a channel state as 9 words");

void fri::grind_free(fri_ctx* ctx) {
    GrindBufs& G = ctx->grind;
    dfree(ctx, G.dev);
    if (G.host) hipHostFree(G.host);
    G = GrindBufs();
}

namespace {
// The automatic window is 8 * 2^bits nonces (a window that holds no hit is
// then a 1-in-3000 event), at least 2^12 and at most 2^GRIND_MAX_LOG_WINDOW:
// 2^30 nonces are one launch of 35 ms at the 31.0 G nonces/s measured for the
// kernel alone on an MI355X (profiles/grind.txt, table (ii): 8.7 ms per 2^28).
constexpr uint32_t GRIND_MIN_LOG_WINDOW = 12, GRIND_MAX_LOG_WINDOW = 30;

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
// Sections of the device buffer for m members (offsets in bytes); the pinned
// mirror has the same layout.  [0, back) is what a launch's read-back brings.
struct Sections {
    size_t best, chan, back, mem, active, total;
    explicit Sections(size_t m) {
        size_t o = 0;
        best = o;   o += al256(m * 8);
        chan = o;   o += al256(m * sizeof(fri_channel_state));
        back = o;
        mem = o;    o += al256(m * sizeof(GrindMember));
        active = o; o += al256(m * 4);
        total = o;
    }
};

int grind_bufs(fri_ctx* ctx, size_t members) {
    GrindBufs& G = ctx->grind;
    if (members <= G.cap) return FRI_OK;
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    dfree(ctx, G.dev);
    if (G.host) hipHostFree(G.host);
    G.dev = G.host = nullptr;
    G.cap = 0;
    const size_t bytes = Sections(members).total;
    if (dalloc(ctx, &G.dev, bytes) != hipSuccess || hipHostMalloc(&G.host, bytes, hipHostMallocDefault) != hipSuccess) {
        dfree(ctx, G.dev);
        G.dev = nullptr;
        G.host = nullptr;
        return fail(ctx, FRI_ENOMEM, "grind staging");
    }
    G.cap = members;
    return FRI_OK;
}

// `batch` members from `first`: windows in rising order, cut at the multiples
// of 2^32 (a window's nonces share their high word), every unfinished member
// in each launch.  The first window in which a member has a hit gives its
// smallest nonce; nonces[b], found[b] and (for the found ones) chan_out[b] are
// written once the walk has ended without an error.  (The walk is a lambda so
// that a HIP error leaves through one place, after the profiling spans.)
int grind_walk(fri_ctx* ctx, uint32_t batch, const fri_channel_state* chan_in, uint32_t bits, uint64_t first,
               uint64_t last, uint64_t* nonces, uint32_t* found, fri_channel_state* chan_out) {
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    int rc = grind_bufs(ctx, batch);
    if (rc) return rc;
    GrindBufs& G = ctx->grind;
    const Sections S(batch);
    hipStream_t s = ctx->stream;
    uint64_t* h_best = reinterpret_cast<uint64_t*>(G.host + S.best);
    fri_channel_state* h_chan = reinterpret_cast<fri_channel_state*>(G.host + S.chan);
    uint32_t* h_active = reinterpret_cast<uint32_t*>(G.host + S.active);
    if (chan_in) memcpy(h_chan, chan_in, (size_t)batch * sizeof(fri_channel_state));
    else memset(h_chan, 0, (size_t)batch * sizeof(fri_channel_state));
    FRI_HIP(ctx, hipMemcpyAsync(G.dev + S.chan, h_chan, (size_t)batch * sizeof(fri_channel_state),
                                hipMemcpyHostToDevice, s));
    GrindTask t{};
    t.mem = reinterpret_cast<const GrindMember*>(G.dev + S.mem);
    t.best = reinterpret_cast<unsigned long long*>(G.dev + S.best);
    t.chan = reinterpret_cast<uint32_t*>(G.dev + S.chan);
    t.mask = bits ? ~0u << (32 - bits) : 0u;
    launch_grind_prep(t.chan, reinterpret_cast<GrindMember*>(G.dev + S.mem), t.best, batch, s);

    const uint32_t auto_log = std::min(std::max(bits + 3, GRIND_MIN_LOG_WINDOW), GRIND_MAX_LOG_WINDOW);
    const uint64_t window = (uint64_t)1 << (G.log_window ? G.log_window : auto_log);
    std::vector<uint64_t> start(batch, 0);       // the window in which member b found its nonce began here
    uint32_t n_active = batch;
    const auto walk = [&]() -> int {
        for (uint64_t w0 = first;;) {
            // the window's last nonce: the window's size, the range's end, the next carry into the high word
            const uint64_t wl1 =
                std::min(std::min(window - 1, last - w0), (uint64_t)(0xFFFFFFFFu - (uint32_t)w0));
            t.active = n_active == batch ? nullptr : reinterpret_cast<const uint32_t*>(G.dev + S.active);
            t.n_active = n_active;
            t.hi = (uint32_t)(w0 >> 32);
            t.lo0 = (uint32_t)w0;
            t.last_idx = (uint32_t)wl1;
            t.rows = (uint32_t)(((uint64_t)(t.lo0 & 63u) + wl1 + 64) / 64);
            const size_t sp = span_begin(ctx, "grind", 0);
            launch_grind(t, s);
            span_end(ctx, sp);
            FRI_HIP(ctx, hipGetLastError());
            FRI_HIP(ctx, hipMemcpyAsync(G.host, G.dev, S.back, hipMemcpyDeviceToHost, s));
            FRI_HIP(ctx, hipStreamSynchronize(s));
            // the members still without a nonce go on, in member order
            uint32_t left = 0;
            for (uint32_t j = 0; j < n_active; j++) {
                const uint32_t b = n_active == batch ? j : h_active[j];
                if (h_best[b] == ~(uint64_t)0) h_active[left++] = b;
                else start[b] = w0;
            }
            if (left == 0 || w0 + wl1 == last) break;
            if (left != n_active)
                FRI_HIP(ctx,
                        hipMemcpyAsync(G.dev + S.active, h_active, (size_t)left * 4, hipMemcpyHostToDevice, s));
            n_active = left;
            w0 += wl1 + 1;
        }
        return FRI_OK;
    };
    rc = walk();
    if (ctx->profiling) spans_collect(ctx);      // also what an error left recorded
    if (rc) return rc;
    for (uint32_t b = 0; b < batch; b++) {
        found[b] = h_best[b] != ~(uint64_t)0;
        if (!found[b]) continue;
        nonces[b] = start[b] + h_best[b];
        if (chan_out) chan_out[b] = h_chan[b];
    }
    ctx->err.clear();
    return FRI_OK;
}
}  // namespace

extern "C" int fri_debug_set_grind_window(fri_ctx* ctx, uint32_t log_window) {
    if (!ctx) return FRI_EINVAL;
    if (log_window > 32) return fail(ctx, FRI_EINVAL, "log_window must be 0 (automatic) or 1..32");
    ctx->grind.log_window = log_window;
    return FRI_OK;
}

extern "C" int fri_grind(fri_ctx* ctx, const fri_channel_state* chan_in, uint32_t bits, uint64_t first, uint64_t last,
                         uint64_t* nonce, uint32_t* found, fri_channel_state* chan_out) {
    if (!ctx || !nonce || !found) return fail(ctx, FRI_EINVAL, "null argument");
    if (bits > 32) return fail(ctx, FRI_EINVAL, "bits must be 0..32");
    if (first > last) return fail(ctx, FRI_EINVAL, "empty range (first > last)");
    return grind_walk(ctx, 1, chan_in, bits, first, last, nonce, found, chan_out);
}

extern "C" int fri_grind_batch(fri_ctx* ctx, uint32_t batch, fri_channel_state* chan, uint32_t bits, uint64_t last,
                               uint64_t* nonces, uint32_t* found) {
    if (!ctx || !chan || !nonces || !found) return fail(ctx, FRI_EINVAL, "null argument");
    if (bits > 32) return fail(ctx, FRI_EINVAL, "bits must be 0..32");
    if (batch < 1 || batch > 65535) return fail(ctx, FRI_EINVAL, "batch must be 1..65535");
    if (ctx->team_root || ctx->tp.team)
        return fail(ctx, FRI_EINVAL, "multi-GPU context: batched grinding runs on one-device contexts");
    if (ctx->profiling) return fail(ctx, FRI_ESTATE, "profiling: time grinding with fri_grind");
    return grind_walk(ctx, batch, chan, bits, 0, last, nonces, found, chan);
}
