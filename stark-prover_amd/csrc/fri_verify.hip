// fri_verify.hip — the batched verifier's host side (fri_verify_batch and
// fri_verify_batch_pow, include/fri_amd.h): argument checks, the staging buffer, the
// upload of a chunk of members and its launch pair (fri_verify_kernels.hip).
// Reads and changes nothing of the resident commit, batch or trace batch.
#include "fri_host.hpp"

static_assert(VB_CHANNEL == FRI_VERIFY_CHANNEL && VB_TRACE_PATH == FRI_VERIFY_TRACE_PATH &&
                  VB_COMPOSITION == FRI_VERIFY_COMPOSITION && VB_FRI_PATH == FRI_VERIFY_FRI_PATH &&
                  VB_FOLD == FRI_VERIFY_FOLD && VB_FINAL == FRI_VERIFY_FINAL && VB_MALFORMED == FRI_VERIFY_MALFORMED &&
                  VB_POW == FRI_VERIFY_POW,
              "verdict bits");
static_assert(sizeof(fri_channel_state) == 36, "k_verify_chain reads a channel state as 9 words");

void fri::verify_free(fri_ctx* ctx) {
    VerifyBufs& V = ctx->verify;
    if (V.side) { hipStreamSynchronize(V.side); hipStreamDestroy(V.side); }
    if (V.ev_up) hipEventDestroy(V.ev_up);
    if (V.ev_open) hipEventDestroy(V.ev_open);
    dfree(ctx, V.dev);
    V = VerifyBufs();
}

namespace {
constexpr size_t VERIFY_CHUNK_BYTES = (size_t)2 << 30;   // staging budget of one launch pair (2 GiB)
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// Sections of the staging buffer for m members (offsets in bytes); the nonces
// have one only with grinding bits, so without them the size is what it was
struct Sections {
    size_t head, chan, nl, alast, idx, vals, paths, verdict, nonce, total;
    Sections(size_t m, size_t hw, size_t q, size_t vw, size_t pw, bool pow) {
        size_t o = 0;
        head = o;    o += al256(m * hw * 4);
        chan = o;    o += al256(m * sizeof(fri_channel_state));
        nl = o;      o += al256(m * 4);
        alast = o;   o += al256(m * 4);
        idx = o;     o += al256(m * q * 8);
        vals = o;    o += al256(m * q * vw * 4);
        paths = o;   o += al256(m * q * pw * 4);
        verdict = o; o += al256(m * 4);
        nonce = o;   o += pow ? al256(m * 8) : 0;
        total = o;
    }
};

// rows of `width` bytes, `pitch` apart at src, packed at dst
hipError_t upload_rows(void* dst, const void* src, size_t width, size_t pitch, size_t rows, hipStream_t s) {
    if (!width || !rows) return hipSuccess;
    if (pitch == width) return hipMemcpyAsync(dst, src, width * rows, hipMemcpyHostToDevice, s);
    return hipMemcpy2DAsync(dst, width, src, pitch, width, rows, hipMemcpyHostToDevice, s);
}
}  // namespace

extern "C" int fri_debug_set_verify_chunk(fri_ctx* ctx, uint32_t members) {
    if (!ctx) return FRI_EINVAL;
    ctx->verify.chunk = members;
    return FRI_OK;
}

extern "C" int fri_verify_batch(fri_ctx* ctx, const fri_verify_shape* shape, uint32_t batch,
                                const fri_channel_state* chan_in, const uint32_t* n_layers, const uint32_t* a_last,
                                const uint32_t* head, size_t head_stride, const uint64_t* indices,
                                const uint32_t* values, size_t values_stride, const uint8_t* paths,
                                size_t paths_stride, uint32_t* verdict) {
    return fri_verify_batch_pow(ctx, shape, batch, chan_in, n_layers, a_last, head, head_stride, indices, values,
                                values_stride, paths, paths_stride, 0, nullptr, verdict);
}

extern "C" int fri_verify_batch_pow(fri_ctx* ctx, const fri_verify_shape* shape, uint32_t batch,
                                    const fri_channel_state* chan_in, const uint32_t* n_layers,
                                    const uint32_t* a_last, const uint32_t* head, size_t head_stride,
                                    const uint64_t* indices, const uint32_t* values, size_t values_stride,
                                    const uint8_t* paths, size_t paths_stride, uint32_t grinding_bits,
                                    const uint64_t* nonces, uint32_t* verdict) {
    if (!ctx || !shape || !chan_in || !n_layers || !head || !verdict) return fail(ctx, FRI_EINVAL, "null argument");
    if (grinding_bits > 32) return fail(ctx, FRI_EINVAL, "grinding_bits must be 0..32");
    if (grinding_bits && !nonces) return fail(ctx, FRI_EINVAL, "null argument (nonces with grinding_bits > 0)");
    const bool pow = grinding_bits != 0;
    if (ctx->team_root || ctx->tp.team)
        return fail(ctx, FRI_EINVAL, "multi-GPU context: the batched verifier runs on one-device contexts");
    const fri_verify_shape& sh = *shape;
    const uint32_t L = sh.log_n, ML = sh.max_layers, Q = sh.num_queries, tc = sh.trace_count;
    if (L < 1 || L > VERIFY_MAX_LOG || L > ctx->log_n_max)
        return fail(ctx, FRI_EINVAL, "log_n must be 1..min(30, the context's log_n_max)");
    if (ML < 1 || ML > L + 1) return fail(ctx, FRI_EINVAL, "max_layers must be 1..log_n + 1");
    if (Q > FRI_VERIFY_MAX_QUERIES) return fail(ctx, FRI_EINVAL, "num_queries above FRI_VERIFY_MAX_QUERIES");
    if (tc != 0 && tc != 3) return fail(ctx, FRI_EINVAL, "trace_count must be 0 (FRI only) or 3 (FibonacciSq)");
    if (sh.offset >= P) return fail(ctx, FRI_EINVAL, "offset not canonical (>= p)");
    if (sh.max_index >> 32) return fail(ctx, FRI_EINVAL, "max_index must be below 2^32");
    if (tc) {
        if (sh.log_t < 2 || sh.log_blowup < 1 || sh.log_blowup > 4 || sh.log_t + sh.log_blowup != L)
            return fail(ctx, FRI_EINVAL, "log_t >= 2, log_blowup 1..4 and log_t + log_blowup = log_n");
        if (sh.max_index != ((uint64_t)1 << L) - ((uint64_t)2 << sh.log_blowup) - 1)
            return fail(ctx, FRI_EINVAL, "max_index must be 2^log_n - 2 * 2^log_blowup - 1 with trace_count = 3");
        if (!a_last) return fail(ctx, FRI_EINVAL, "null argument");
    }
    if (batch < 1 || batch > 65535) return fail(ctx, FRI_EINVAL, "batch must be 1..65535");
    if (Q && (!indices || !values || !paths)) return fail(ctx, FRI_EINVAL, "null argument");
    const RecordShape rs{L, tc, ML};
    const size_t hw = (tc ? 11 : 0) + 9 * (size_t)ML, vw = rs.val_words(), pw = rs.path_words(ML);
    if (head_stride < hw || (Q && (values_stride < vw || paths_stride < pw * 4)))
        return fail(ctx, FRI_EINVAL,
                    "record strides too small (head: [11 +] 9 max_layers words; values: trace_count + 2 max_layers "
                    "words; paths: fri_batch_query_round's)");
    for (uint32_t b = 0; b < batch; b++) {
        if (n_layers[b] < 1 || n_layers[b] > ML)
            return fail(ctx, FRI_EINVAL, "member " + std::to_string(b) + ": n_layers must be 1..max_layers");
        if (tc && a_last[b] >= P)
            return fail(ctx, FRI_EINVAL, "member " + std::to_string(b) + ": a_last not canonical (>= p)");
    }

    FRI_HIP(ctx, hipSetDevice(ctx->device));
    VerifyBufs& V = ctx->verify;
    if (!V.side) {
        FRI_HIP(ctx, hipStreamCreateWithFlags(&V.side, hipStreamNonBlocking));
        FRI_HIP(ctx, hipEventCreateWithFlags(&V.ev_up, hipEventDisableTiming));
        FRI_HIP(ctx, hipEventCreateWithFlags(&V.ev_open, hipEventDisableTiming));
    }
    // members per launch pair: what the byte budget holds, or the hook's count
    const size_t per_member = Sections(1, hw, Q, vw, pw, pow).total;
    size_t chunk = V.chunk ? V.chunk : std::max<size_t>(VERIFY_CHUNK_BYTES / per_member, 1);
    chunk = std::min<size_t>(chunk, batch);
    while (Sections(chunk, hw, Q, vw, pw, pow).total > V.cap) {
        const size_t need = Sections(chunk, hw, Q, vw, pw, pow).total;
        FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        dfree(ctx, V.dev);
        V.dev = nullptr;
        V.cap = 0;
        if (dalloc(ctx, &V.dev, need) == hipSuccess) {
            V.cap = need;
            break;
        }
        if (V.chunk || chunk == 1) return fail(ctx, FRI_ENOMEM, "verifier staging: one member does not fit");
        chunk = (chunk + 1) / 2;
    }

    VerifyTask t{};
    t.head_words = (uint32_t)hw;
    t.val_words = (uint32_t)vw;
    t.path_words = (uint32_t)pw;
    t.log_n = L;
    t.max_layers = ML;
    t.num_queries = Q;
    t.trace_count = tc;
    t.log_t = sh.log_t;
    t.log_blowup = sh.log_blowup;
    t.range = sh.max_index + 1;
    t.pow_bits = grinding_bits;
    for (uint32_t k = 0; k <= L; k++) {
        t.w_m[k] = to_mont(root_of_unity(L - k));
        t.off_m[k] = to_mont(pow_std(sh.offset, (uint64_t)1 << k));
    }
    if (tc) {
        const uint32_t g = root_of_unity(sh.log_t);
        const uint64_t T = (uint64_t)1 << sh.log_t;
        t.glast_m = to_mont(pow_std(g, T - 1));
        t.gprev_m = to_mont(pow_std(g, T - 2));
    }
    // one stream, chain then open, while profiling (the spans time the context
    // stream) and under FRI_VERIFY_SERIAL=1 (measurement: tools/batch_probe.py)
    const char* serial_env = getenv("FRI_VERIFY_SERIAL");
    const bool serial = ctx->profiling || (serial_env && serial_env[0] == '1');
    hipStream_t s = ctx->stream;
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t m = std::min<size_t>(chunk, batch - b0);
        const Sections S(m, hw, Q, vw, pw, pow);
        uint8_t* d = V.dev;
        FRI_HIP(ctx, upload_rows(d + S.head, head + b0 * head_stride, hw * 4, head_stride * 4, m, s));
        FRI_HIP(ctx, upload_rows(d + S.chan, chan_in + b0, sizeof(fri_channel_state), sizeof(fri_channel_state), m, s));
        FRI_HIP(ctx, upload_rows(d + S.nl, n_layers + b0, 4, 4, m, s));
        if (tc) FRI_HIP(ctx, upload_rows(d + S.alast, a_last + b0, 4, 4, m, s));
        if (Q) {
            FRI_HIP(ctx, upload_rows(d + S.idx, indices + b0 * Q, 8, 8, m * Q, s));
            FRI_HIP(ctx, upload_rows(d + S.vals, values + b0 * Q * values_stride, vw * 4, values_stride * 4, m * Q, s));
            FRI_HIP(ctx, upload_rows(d + S.paths, paths + b0 * Q * paths_stride, pw * 4, paths_stride, m * Q, s));
        }
        if (pow) FRI_HIP(ctx, upload_rows(d + S.nonce, nonces + b0, 8, 8, m, s));
        FRI_HIP(ctx, hipMemsetAsync(d + S.verdict, 0, m * 4, s));
        t.head = reinterpret_cast<const uint32_t*>(d + S.head);
        t.chan = reinterpret_cast<const uint32_t*>(d + S.chan);
        t.n_layers = reinterpret_cast<const uint32_t*>(d + S.nl);
        t.a_last = reinterpret_cast<const uint32_t*>(d + S.alast);
        t.indices = reinterpret_cast<const uint64_t*>(d + S.idx);
        t.values = reinterpret_cast<const uint32_t*>(d + S.vals);
        t.paths = reinterpret_cast<const uint32_t*>(d + S.paths);
        t.nonces = pow ? reinterpret_cast<const uint64_t*>(d + S.nonce) : nullptr;
        t.verdict = reinterpret_cast<uint32_t*>(d + S.verdict);
        t.members = (uint32_t)m;
        if (serial) {
            size_t sp = span_begin(ctx, "verify_chain", 0);
            launch_verify_chain(t, s);
            span_end(ctx, sp);
            sp = span_begin(ctx, "verify_open", 0);
            launch_verify_open(t, s);
            span_end(ctx, sp);
        } else {
            // the two kernels share no data but the verdict words they OR into
            FRI_HIP(ctx, hipEventRecord(V.ev_up, s));
            FRI_HIP(ctx, hipStreamWaitEvent(V.side, V.ev_up, 0));
            launch_verify_open(t, V.side);
            FRI_HIP(ctx, hipEventRecord(V.ev_open, V.side));
            launch_verify_chain(t, s);
            FRI_HIP(ctx, hipStreamWaitEvent(s, V.ev_open, 0));
        }
        FRI_HIP(ctx, hipGetLastError());
        FRI_HIP(ctx, hipMemcpyAsync(verdict + b0, t.verdict, m * 4, hipMemcpyDeviceToHost, s));
        // the next chunk reuses the staging buffer, and `verdict` is pageable
        FRI_HIP(ctx, hipStreamSynchronize(s));
    }
    if (ctx->profiling) spans_collect(ctx);
    ctx->err.clear();
    return FRI_OK;
}
