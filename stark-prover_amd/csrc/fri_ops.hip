// fri_ops.hip — kernel-level entry points of include/fri_amd.h: batch
// inverse (element.rs:54-57), coset LDE (fri_commit.rs:78), interpolation on
// a coset and through arbitrary points (ops.rs:239-241 ->
// interpolation.rs:121-152), evaluation (ops.rs:76-83), one fold
// (fri_commit.rs:53-65) and the Merkle root of any n (merkle/mod.rs:10-26).
#include "fri_host.hpp"
#include "sha256.hpp"

// ------------------------------------------------------- kernel-level ----
extern "C" int fri_batch_inverse(fri_ctx* ctx, const uint32_t* in, uint32_t* out, size_t n) {
    if (!ctx || (!in && n) || (!out && n)) return fail(ctx, FRI_EINVAL, "null argument");
    if (!check_canonical(in, n)) return fail(ctx, FRI_EINVAL, "input not canonical (>= p)");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cap = (size_t)1 << ctx->log_n_max;
    for (size_t off = 0; off < n; off += cap) {
        size_t m = n - off < cap ? n - off : cap;
        FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_a, in + off, m * 4, hipMemcpyHostToDevice, ctx->stream));
        launch_batch_inverse(ctx->scratch_a, ctx->scratch_b, m, 0, ctx->stream);
        FRI_HIP(ctx, hipGetLastError());
        FRI_HIP(ctx, hipMemcpyAsync(out + off, ctx->scratch_b, m * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FRI_OK;
}


extern "C" int fri_lde(fri_ctx* ctx, const uint32_t* coeffs, size_t d, uint32_t log_n, uint32_t offset,
                       uint32_t* evals_out) {
    if (!ctx || !evals_out || (d && !coeffs)) return fail(ctx, FRI_EINVAL, "null argument");
    if (log_n > ctx->log_n_max) return fail(ctx, FRI_EINVAL, "log_n exceeds context capacity");
    const size_t n = (size_t)1 << log_n;
    if (d > n) return fail(ctx, FRI_EINVAL, "more coefficients than domain points");
    if (offset == 0 || offset >= P) return fail(ctx, FRI_EINVAL, "offset must be a nonzero canonical element");
    if (!check_canonical(coeffs, d)) return fail(ctx, FRI_EINVAL, "coefficient not canonical (>= p)");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    if (d) FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_a, coeffs, d * 4, hipMemcpyHostToDevice, ctx->stream));
    coset_forward(ctx, ctx->scratch_a, d, log_n, offset, ctx->scratch_b);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipMemcpyAsync(evals_out, ctx->scratch_b, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FRI_OK;
}

extern "C" int fri_interpolate(fri_ctx* ctx, const uint32_t* ys, uint32_t log_n, uint32_t offset,
                               uint32_t* coeffs_out, size_t* len_out) {
    if (!ctx || !ys || !coeffs_out || !len_out) return fail(ctx, FRI_EINVAL, "null argument");
    if (log_n > ctx->log_n_max) return fail(ctx, FRI_EINVAL, "log_n exceeds context capacity");
    if (offset == 0 || offset >= P) return fail(ctx, FRI_EINVAL, "offset must be a nonzero canonical element");
    const size_t n = (size_t)1 << log_n;
    if (!check_canonical(ys, n)) return fail(ctx, FRI_EINVAL, "value not canonical (>= p)");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_a, ys, n * 4, hipMemcpyHostToDevice, ctx->stream));
    // coeff_j = n^-1 * offset^-j * sum_i ys_i w^-ij
    coset_inverse(ctx, ctx->scratch_a, log_n, inv_std(offset), 0, ctx->scratch_b);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipMemcpyAsync(coeffs_out, ctx->scratch_b, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *len_out = trimmed(coeffs_out, n);                           // Polynomial::new trim (ops.rs:19-37)
    return FRI_OK;
}

// The direct kernels of fri_interpolate_points_ex / fri_evaluate_ex
// (fri_multipoint.hip validates the arguments and chooses the path).
namespace fri {

// interpolate_lagrange_polynomials (interpolation.rs:121-152) on arbitrary
// points: weights, c_j = y_j w_j, f on the 2^k-th roots of unity, iNTT
// (fri_kernels.hip "arbitrary-point interpolate").  n >= 1, 2^log_N >= n.
int interpolate_points_direct(fri_ctx* ctx, const uint32_t* xs, const uint32_t* ys, size_t n, uint32_t log_N,
                              uint32_t* coeffs_out, size_t* len_out) {
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int rc = ensure_tmp(ctx, interp_tmp_words(n, log_N));
    if (rc) return rc;
    FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_a, xs, n * 4, hipMemcpyHostToDevice, s));
    launch_interp_weights(ctx->scratch_a, n, ctx->scratch_b, ctx->interp_tmp, s);   // prod_{i!=j}(x_j - x_i)
    launch_batch_inverse(ctx->scratch_b, ctx->scratch_c, n, 1, s);          // w_j (Montgomery; 0 -> 0)
    FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_b, ys, n * 4, hipMemcpyHostToDevice, s));   // after the inverse (stream order)
    launch_interp_coeffs(ctx->scratch_b, ctx->scratch_c, n, s);             // c_j = y_j w_j
    launch_interp_eval(ctx->scratch_a, ctx->scratch_c, n, log_N, ctx->scratch_b, ctx->interp_tmp, s);   // f(w_N^k)
    inverse(ctx, ctx->scratch_b, log_N, 0, ctx->scratch_a);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipMemcpyAsync(coeffs_out, ctx->scratch_a, n * 4, hipMemcpyDeviceToHost, s));   // deg f < n
    FRI_HIP(ctx, hipStreamSynchronize(s));
    tmp_trim(ctx);
    *len_out = trimmed(coeffs_out, n);                           // Polynomial::new trim (ops.rs:19-37)
    return FRI_OK;
}

// Horner at every point (ops.rs:76-83); d, count <= 2^log_n_max.
int evaluate_direct(fri_ctx* ctx, const uint32_t* coeffs, size_t d, const uint32_t* xs, size_t count, uint32_t* out) {
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    if (d) FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_a, coeffs, d * 4, hipMemcpyHostToDevice, ctx->stream));
    if (count) FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_b, xs, count * 4, hipMemcpyHostToDevice, ctx->stream));
    const size_t tw = evaluate_tmp_words(d, count);
    if (tw) {
        const int rc = ensure_tmp(ctx, tw);
        if (rc) return rc;
    }
    launch_evaluate(ctx->scratch_a, d, ctx->scratch_b, count, ctx->scratch_c, ctx->interp_tmp, ctx->stream);
    FRI_HIP(ctx, hipGetLastError());
    if (count) FRI_HIP(ctx, hipMemcpyAsync(out, ctx->scratch_c, count * 4, hipMemcpyDeviceToHost, ctx->stream));
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    tmp_trim(ctx);
    return FRI_OK;
}

}  // namespace fri

extern "C" int fri_fold(fri_ctx* ctx, const uint32_t* layer, uint32_t log_m, uint32_t layer_offset, uint32_t beta,
                        uint32_t* out) {
    if (!ctx || !layer || !out) return fail(ctx, FRI_EINVAL, "null argument");
    if (log_m < 1 || log_m > ctx->log_n_max) return fail(ctx, FRI_EINVAL, "log_m out of range");
    if (layer_offset == 0 || layer_offset >= P || beta >= P) return fail(ctx, FRI_EINVAL, "bad offset/beta");
    const size_t m = (size_t)1 << log_m;
    if (!check_canonical(layer, m)) return fail(ctx, FRI_EINVAL, "value not canonical (>= p)");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_a, layer, m * 4, hipMemcpyHostToDevice, ctx->stream));
    launch_coset_points(ctx->scratch_b, m / 2, layer_offset, log_m, ctx->stream);
    launch_batch_inverse(ctx->scratch_b, ctx->scratch_c, m / 2, 1, ctx->stream);
    launch_fold_plain(ctx->scratch_a, ctx->scratch_b, log_m, ctx->scratch_c, beta, ctx->stream);
    FRI_HIP(ctx, hipGetLastError());
    FRI_HIP(ctx, hipMemcpyAsync(out, ctx->scratch_b, (m / 2) * 4, hipMemcpyDeviceToHost, ctx->stream));
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FRI_OK;
}

// Non-power-of-two trees (rs_merkle promotes a lone right-most node).
__global__ void k_leaf_generic(const uint32_t* v, uint32_t* out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sha::leaf(v[i], out + 8 * i);
}
__global__ void k_level_generic(const uint32_t* in, uint32_t* out, size_t cnt) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t pc = (cnt + 1) / 2;
    if (j >= pc) return;
    if (2 * j + 1 < cnt) sha::node(in + 16 * j, in + 16 * j + 8, out + 8 * j);
    else for (int i = 0; i < 8; i++) out[8 * j + i] = in[16 * j + i];
}

extern "C" int fri_merkle_root(fri_ctx* ctx, const uint32_t* values, size_t n, uint8_t root32[32]) {
    if (!ctx || !values || !root32) return fail(ctx, FRI_EINVAL, "null argument");
    if (n == 0) return fail(ctx, FRI_EINVAL, "empty tree has no root (merkle/mod.rs:25)");
    const size_t cap = (size_t)1 << ctx->log_n_max;
    if (n > cap) return fail(ctx, FRI_EINVAL, "size exceeds context capacity");
    if (!check_canonical(values, n)) return fail(ctx, FRI_EINVAL, "value not canonical (>= p)");
    FRI_HIP(ctx, hipSetDevice(ctx->device));
    FRI_HIP(ctx, hipMemcpyAsync(ctx->scratch_a, values, n * 4, hipMemcpyHostToDevice, ctx->stream));
    // the tree lives in the context's partials scratch (no hipMalloc / hipFree,
    // which synchronises the device, per MerkleTree::new)
    uint32_t* root_dev;
    uint32_t* tree = nullptr;
    bool pow2 = (n & (n - 1)) == 0;
    if (pow2) {
        const uint32_t L = ceil_log2(n);
        const int rc = ensure_tmp(ctx, ((size_t)2 << L) * 8);
        if (rc) return rc;
        tree = ctx->interp_tmp;
        LayerTask t{};
        t.values = ctx->scratch_a;
        t.tree = tree;
        t.L = L;
        launch_layer(t, ctx->stream);
        root_dev = tree + 8 * level_offset(L, L);
    } else {
        size_t total = 0;
        for (size_t m = n;; m = (m + 1) / 2) { total += m; if (m == 1) break; }
        const int rc = ensure_tmp(ctx, total * 8);
        if (rc) return rc;
        tree = ctx->interp_tmp;
        uint32_t* cur = tree;
        hipLaunchKernelGGL(k_leaf_generic, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                           ctx->scratch_a, cur, n);
        size_t cnt = n;
        while (cnt > 1) {
            size_t pc = (cnt + 1) / 2;
            uint32_t* nxt = cur + 8 * cnt;
            hipLaunchKernelGGL(k_level_generic, dim3((unsigned)((pc + 255) / 256)), dim3(256), 0, ctx->stream, cur,
                               nxt, cnt);
            cur = nxt;
            cnt = pc;
        }
        root_dev = cur;
    }
    FRI_HIP(ctx, hipGetLastError());
    uint32_t w[8];
    hipError_t e1 = hipMemcpyAsync(w, root_dev, 32, hipMemcpyDeviceToHost, ctx->stream);
    hipError_t e2 = hipStreamSynchronize(ctx->stream);
    tmp_trim(ctx);
    FRI_HIP(ctx, e1);
    FRI_HIP(ctx, e2);
    digest_to_bytes(w, root32);
    return FRI_OK;
}
