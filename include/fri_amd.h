/*
 * fri_amd.h — C ABI of the MI355X-native FRI commit path (libfri_amd.so).
 *
 * Drop-in boundary for the reference crate `stark-101`
 * (RazorClient/Stark-prover).  Each entry point names the reference function
 * it replaces (path:line in the reference tree).  Plain pointers and sizes
 * only; no torch / HIP types in any signature.
 *
 * Field: p = 3*2^30 + 1 = 3221225473, generator g = 5 (frozen spec,
 * SURVEY.md §8).  Field elements cross the boundary as canonical uint32_t
 * (value < p) — the reference's FieldElement<M>{value: u64} is not repr(C),
 * so the Rust shim copies `.value() as u32`.
 *
 * Host buffers are caller-owned and only borrowed for the duration of a call.
 * Device memory, streams and graphs are owned by the fri_ctx.  A context is
 * not re-entrant: use one per host thread.  Every call returns FRI_OK (0) or
 * a FRI_E* code; fri_last_error() describes the last failure on the context.
 * The reference panics where these return an error (ops.rs:143,
 * interpolation.rs:127, merkle/mod.rs:25, channel.rs:65); the Rust shim maps
 * non-zero codes back to panic!().
 */
#ifndef FRI_AMD_H
#define FRI_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRI_P          3221225473u   /* 3*2^30 + 1 */
#define FRI_GENERATOR  5u
#define FRI_MAX_ROUNDS 32
#define FRI_MAX_LAYERS (FRI_MAX_ROUNDS + 1)

enum {
    FRI_OK      = 0,
    FRI_EINVAL  = 1,   /* bad argument (sizes, d > n, value >= p, ...)      */
    FRI_ENOMEM  = 2,   /* device or host allocation failed                  */
    FRI_EHIP    = 3,   /* HIP runtime error                                 */
    FRI_ENODEV  = 4,   /* no usable gfx950 device                           */
    FRI_ERCCL   = 5,   /* collective failure (multi-GPU)                    */
    FRI_ESTATE  = 6,   /* call out of order (e.g. no committed layers)      */
    FRI_EDEGREE = 7    /* polynomial degree too large for the domain: the
                          reference would exhaust the domain and panic in
                          MerkleTree::root() (merkle/mod.rs:25)             */
};

/* Fiat-Shamir transcript state — src/channel/channel.rs:14-20.
 * The reference keeps `state: String` = "" or the 64-char lowercase hex of
 * a SHA-256 digest; here it is the 32 raw digest bytes + has_state flag. */
typedef struct {
    uint8_t  digest[32];
    uint32_t has_state;   /* 0 => state == "" (Channel::new, channel.rs:24-30) */
} fri_channel_state;

/* Result of fri_commit — the transcript-visible part of FRIProof
 * (src/fri/fri_commit.rs:9-13) plus the channel messages it produced.
 * Layer evaluations and Merkle levels stay on the device and are read back
 * on demand with fri_layer_copy / fri_tree_level_copy. */
typedef struct {
    uint32_t n_layers;                       /* R+1 committed layers          */
    uint32_t n_rounds;                       /* R folds (= betas drawn)       */
    uint32_t log_n;                          /* layer k has 2^(log_n-k) elems */
    uint32_t final_value;                    /* fri_commit.rs:109-113         */
    int32_t  final_degree;                   /* 0, or -1 for the zero poly    */
    uint32_t reserved;
    uint8_t  roots[FRI_MAX_LAYERS][32];      /* Merkle root bytes per layer   */
    uint32_t betas[FRI_MAX_ROUNDS];          /* beta_k, canonical             */
    fri_channel_state channel_out;           /* channel state after the final send */
} fri_commit_result;

typedef struct fri_ctx fri_ctx;

/* flags for fri_commit* */
#define FRI_FLAG_FORCE_BETAS 1u   /* test hook: use forced_betas[k] instead of the
                                     channel's draw (transcript still absorbs roots) */
#define FRI_FLAG_NO_GRAPH    2u   /* run eagerly instead of replaying a hipGraph   */
#define FRI_FLAG_RANK_INPUTS 4u   /* multi-GPU context, fri_commit_device with
                                     fri_ctx_input_buffer(): ranks 1..n-1 commit the
                                     copy of rank 0's buffer their plan staged at the
                                     last team commit of this shape instead of
                                     copying it again over xGMI.  Verified, not
                                     trusted: every rank hashes the input it would
                                     commit (a position-sensitive 64-bit checksum)
                                     and the call returns FRI_ESTATE, committing
                                     nothing, when a rank's copy differs from rank
                                     0's buffer (rewritten since it was staged) or
                                     no copy of this shape was staged yet */

/* ---------------------------------------------------------------- context */
/* Opens `device` (HIP ordinal) and sizes scratch for codewords up to
 * 2^log_n_max.  Returns FRI_ENODEV when no gfx950 device is present. */
int         fri_ctx_create(int device, uint32_t log_n_max, fri_ctx** out);
int         fri_ctx_destroy(fri_ctx* ctx);
const char* fri_last_error(const fri_ctx* ctx);    /* never NULL; "" if none */
const char* fri_version(void);

/* ------------------------------------------------------- field / batch ops */
/* Batch inverse with inverse(0) = 0 — same results as element-wise
 * FieldElement::inverse (src/fields/element.rs:54-57, Fermat a^(p-2)). */
int fri_batch_inverse(fri_ctx* ctx, const uint32_t* in, uint32_t* out, size_t n);

/* ------------------------------------------------------ polynomial layer */
/* Low-degree extension: evals[i] = P(offset * w_n^i), i < n = 2^log_n,
 * P given by d <= n coefficients (coefficient j = x^j).  Replaces
 * `domain.map(|x| poly.evaluate(x))` (src/fri/fri_commit.rs:78,
 * src/polynomial/ops.rs:76-83) on the coset domain of
 * src/fri/coset_fri.rs:32-36.  offset = 1 gives the plain subgroup. */
int fri_lde(fri_ctx* ctx, const uint32_t* coeffs, size_t d, uint32_t log_n,
            uint32_t offset, uint32_t* evals_out);

/* Interpolation on the same coset: the unique P, deg P < n, with
 * P(offset*w_n^i) = ys[i].  Replaces Polynomial::interpolate
 * (src/polynomial/ops.rs:239-241 -> interpolation.rs:121-152) for coset
 * domains.  coeffs_out holds n entries; *len_out = trimmed length
 * (Polynomial::new semantics, ops.rs:19-37). */
int fri_interpolate(fri_ctx* ctx, const uint32_t* ys, uint32_t log_n, uint32_t offset,
                    uint32_t* coeffs_out, size_t* len_out);

/* Interpolation through n arbitrary points: Polynomial::interpolate(xs, ys)
 * (src/polynomial/ops.rs:239-241 -> interpolate_lagrange_polynomials,
 * interpolation.rs:121-152) for point sets that are not a coset.  Same
 * result as the reference's Lagrange sum, duplicates included (their basis
 * polynomials vanish through inverse(0) = 0, element.rs:54-57).  Two paths,
 * the same coefficients (field arithmetic is exact):
 *   direct  O(n^2): weights w_j = 1/prod_{i!=j}(x_j - x_i), then f at the
 *           2^k-th roots of unity (2^k >= n) as sum_j y_j w_j prod_{i!=j}(x - x_i)
 *           without any division, then an iNTT.  n <= 2^17, n <= 2^log_n_max.
 *   tree    O(n log^2 n), from n >= FRI_MP_INTERP_MIN: the product tree of
 *           fri_poly_from_roots with every level retained, the weights as
 *           1/Z'(x_i) by the tree evaluation below, then sum_i y_i w_i Z/(x - x_i)
 *           combined up the tree.  Accepted sizes are exactly
 *             next_pow2(n) <= 2^(log_n_max - 1)
 *           (Z' has n coefficients and is evaluated at next_pow2(n) points).
 * fri_interpolate_points is fri_interpolate_points_ex with flags 0: the tree
 * from FRI_MP_INTERP_MIN points where the sizes fit, else the direct kernels with the
 * launches they always had.  coeffs_out holds n entries; *len_out = trimmed
 * length; n = 0 gives length 0. */
int fri_interpolate_points(fri_ctx* ctx, const uint32_t* xs, const uint32_t* ys, size_t n,
                           uint32_t* coeffs_out, size_t* len_out);

/* Evaluation of P (d coefficients) at `count` arbitrary points
 * (src/polynomial/ops.rs:76-83, Horner semantics): fri_evaluate_ex with
 * flags 0.  d = 0 gives zeros, count = 0 writes nothing. */
int fri_evaluate(fri_ctx* ctx, const uint32_t* coeffs, size_t d, const uint32_t* xs,
                 size_t count, uint32_t* out);

/* The two calls above with a choice of path.  The tree path pads the point
 * list with zero roots to N = next_pow2(count), builds the product tree with
 * every level from the leaf subtrees up retained in the context's grown
 * scratch, inverts rev(Z_pad) as a power series to d terms (Newton, as
 * fri_poly_div_rem), takes the vector of f / Z_pad from one product of cyclic
 * size next_pow2(d + N - 1) and goes down the tree with one batched set of
 * cyclic middle products per level (a fixed number of launches whatever the
 * node count); in a leaf subtree one lane per point finishes with a synthetic
 * division chain.  Values equal Horner's bit for bit.  Accepted sizes of the
 * tree path are exactly
 *   d + next_pow2(count) - 1 <= 2^log_n_max  and  next_pow2(d) <= 2^(log_n_max - 1)
 * (the root product and the last Newton step).  FRI_MP_FORCE_TREE outside
 * them gives FRI_EINVAL; flags 0 then runs the direct kernels where they
 * accept the call.  Both FORCE flags together, or an unknown flag, give
 * FRI_EINVAL.  The leaf subtrees hold FRI_ROOTS_LEAF points
 * (fri_debug_set_roots_leaf applies).  Memory: the retained levels are
 * (log2 N - log2 leaf + 1) * N words, 48 MiB at N = 2^20 and 1 GiB at 2^24
 * with leaves of 512, next to about 8 N words of vectors and operands (13 N
 * for interpolation); a failed allocation gives FRI_ENOMEM and leaves the
 * context usable.  On a multi-GPU context the calls run on rank 0. */
#define FRI_MP_FORCE_TREE   1u   /* test/measurement hook: never the direct kernels */
#define FRI_MP_FORCE_DIRECT 2u   /* test/measurement hook: always them (FRI_EINVAL past their limits) */
#define FRI_MP_SMALL_LEAF   4u   /* test hook: leaf subtrees of 64 points */
/* Evaluation takes the tree when min(d, count) >= FRI_MP_EVAL_MIN,
 * interpolation when n >= FRI_MP_INTERP_MIN (and the sizes fit): the measured
 * crossovers (profiles/poly_multipoint.txt, from tools/poly_arith_probe.py
 * --multipoint) — the smallest power of two from which the tree is not slower
 * than the direct kernels, whole call, the same in both runs of the table.
 * Evaluation, d = count: 0.601 ms direct against 1.535 tree at 2^15, 5.002
 * against 1.731 at 2^16, 21.8 against 2.30 at 2^18.  Interpolation: 1.251
 * against 2.057 at 2^15, 4.438 against 2.314 at 2^16, 16.1 against 2.63 at
 * 2^17.  The tree's cost below 2^15 is its launches (0.5 ms at 2^10). */
#define FRI_MP_EVAL_MIN     65536
#define FRI_MP_INTERP_MIN   65536
int fri_evaluate_ex(fri_ctx* ctx, const uint32_t* coeffs, size_t d, const uint32_t* xs, size_t count,
                    uint32_t flags, uint32_t* out);
int fri_interpolate_points_ex(fri_ctx* ctx, const uint32_t* xs, const uint32_t* ys, size_t n,
                              uint32_t flags, uint32_t* coeffs_out, size_t* len_out);

/* ------------------------------------------------- polynomial arithmetic */
/* Polynomial<M>::mul_assign, div_rem and compose (src/polynomial/ops.rs) on
 * the device.  Operands are host arrays of canonical coefficients
 * (coefficient j = x^j; a value >= p gives FRI_EINVAL) and may carry
 * trailing zeros: they are trimmed first, as Polynomial::new does
 * (ops.rs:19-37).  Every length written back is a trimmed length, 0 for the
 * zero polynomial.  An output capacity that is too small gives FRI_EINVAL
 * with the needed length in the length output.  Field arithmetic is exact
 * and quotient and remainder are unique, so the coefficients equal the
 * reference's whatever algorithm computes them.  On a multi-GPU context the
 * calls run on rank 0. */
#define FRI_POLY_FORCE_NTT    1u   /* test/measurement hook: never take the direct kernel */
#define FRI_POLY_FORCE_DIRECT 2u   /* test/measurement hook: take it (FRI_EINVAL if the
                                      short operand exceeds FRI_POLY_DIRECT_LIMIT) */
/* The direct convolution kernel stages the short operand in LDS: its hard
 * limit, in coefficients of the shorter operand. */
#define FRI_POLY_DIRECT_LIMIT 4096
/* fri_poly_mul takes the direct kernel when min(la, lb) <= this: the
 * measured crossover (profiles/poly_arith.txt, table (i)) — the largest
 * short length, rounded down to a power of two, at which the direct kernel
 * is not slower than the NTT path against a long operand of 2^16
 * coefficients (0.10 ms against 0.12 ms at 1024; 0.14 against 0.12 at 2048;
 * the same in three runs). */
#define FRI_POLY_DIRECT_MAX   1024

/* a * b — Polynomial::mul_assign (ops.rs:114-138, schoolbook O(la*lb)).
 * A zero operand gives *len_out = 0 (ops.rs:115-121); otherwise the product
 * has la + lb - 1 coefficients (trimmed lengths) and needs
 * next_pow2(la + lb - 1) <= 2^log_n_max.  Two forward NTTs of that size, a
 * pointwise product and one inverse NTT; with min(la, lb) <=
 * FRI_POLY_DIRECT_MAX one direct convolution kernel, O(la*lb), instead.
 * flags: 0 or one FRI_POLY_FORCE_*. */
int fri_poly_mul(fri_ctx* ctx, const uint32_t* a, size_t la, const uint32_t* b, size_t lb,
                 uint32_t flags, uint32_t* out, size_t out_cap, size_t* len_out);

/* (q, r) with a = q*b + r, deg r < deg b — Polynomial::div_rem
 * (ops.rs:141-191, long division with one Fermat inverse per quotient
 * step).  b zero: FRI_EINVAL, "Division by zero polynomial" (ops.rs:143).
 * deg a < deg b: q = 0 and r = a (ops.rs:145-147).  Otherwise q has
 * la - lb + 1 coefficients and q_cap >= la - lb + 1, r_cap >= lb - 1 are
 * required (*r_len is then the trimmed length, <= lb - 1).  Newton inversion
 * of the reversed divisor, O(n log n): accepted sizes (trimmed) are exactly
 *   la <= 2^log_n_max  and  next_pow2(la - lb + 1) <= 2^(log_n_max - 1),
 * which holds for every la <= 2^(log_n_max - 2) and every la <= 2^(log_n_max
 * - 1) + lb - 1. */
int fri_poly_div_rem(fri_ctx* ctx, const uint32_t* a, size_t la, const uint32_t* b, size_t lb,
                     uint32_t* q_out, size_t q_cap, size_t* q_len,
                     uint32_t* r_out, size_t r_cap, size_t* r_len);

/* p(q(x)) — Polynomial::compose (ops.rs:214-237, Horner over polynomials).
 * p zero gives zero; q zero or a constant c gives the constant p(c), which
 * may trim to zero (ops.rs:993-1019); otherwise the result has
 * deg p * deg q + 1 coefficients and needs N = next_pow2(deg p * deg q + 1)
 * <= 2^log_n_max.  One NTT of q, Horner of p at those N values, one inverse
 * NTT: the cost is O(lp * N) field products, so this is for compositions
 * with a short p or a low-degree q (f(g*x): N = next_pow2(lp)). */
int fri_poly_compose(fri_ctx* ctx, const uint32_t* p, size_t lp, const uint32_t* q, size_t lq,
                     uint32_t* out, size_t out_cap, size_t* len_out);

/* ------------------------------------- polynomial from roots, Lagrange basis */
/* src/polynomial/interpolation.rs on the device, with the conventions of the
 * block above: host arrays, canonical values (a value >= p gives
 * FRI_EINVAL), the needed length in *len_out when a capacity is too small,
 * rank 0 on a multi-GPU context.  The reference multiplies the linear
 * factors one by one (O(n^2)); here Z is a binary product tree: subtrees of
 * FRI_ROOTS_LEAF roots are built by one workgroup each in LDS, and every
 * level above is one batched set of cyclic NTT products, a fixed number of
 * launches per level whatever its node count. */
#define FRI_ROOTS_SMALL_LEAF 1u   /* test/measurement hook: leaf subtrees of 64 roots */
/* Roots per LDS leaf subtree: the measured choice (profiles/poly_roots.txt,
 * table (iii), from tools/poly_arith_probe.py --roots) — the power of two in
 * 128..2048 with the lowest whole-call median at n = 2^16 (0.435 ms at 512
 * against 0.448 at 256, 0.465 at 128, 0.520 at 1024 and 0.955 at 2048; 512
 * in two runs).  At n = 2^20 the candidates 128, 256 and 512 lie within
 * 0.012 ms of each other (0.981, 0.980, 0.992 ms), so the 2^16 winner stands. */
#define FRI_ROOTS_LEAF       512
#define FRI_LAGRANGE_MAX     4096

/* Z(x) = prod_i (x - roots[i]) — gen_polynomial_from_roots
 * (interpolation.rs:9-23).  n = 0 gives *len_out = 0 (Polynomial::zero(),
 * :10-12); otherwise *len_out = n + 1: Z is monic and never trims.  Repeated
 * roots and the roots 0 and p - 1 are ordinary inputs.  Any n with
 * next_pow2(n) <= 2^log_n_max (the list is padded with zero roots to a power
 * of two and the padding's factor x^pad is dropped from the result).
 * flags: 0 or FRI_ROOTS_SMALL_LEAF. */
int fri_poly_from_roots(fri_ctx* ctx, const uint32_t* roots, size_t n, uint32_t flags,
                        uint32_t* out, size_t out_cap, size_t* len_out);

/* L_i = Z/(x - xs[i]) / prod_{j!=i}(xs[i] - xs[j]) — gen_lagrange_polynomials
 * (interpolation.rs:46-78; gen_lagrange_polynomials_parallel, :80-115, gives
 * the same).  out is row-major n x n: row i holds L_i's coefficients
 * x^0..x^(n-1), untrimmed.  n = 0 writes nothing.  A repeated x gives
 * all-zero rows for every copy: the denominator is 0 and inverse(0) = 0
 * (element.rs:54-57).  n <= FRI_LAGRANGE_MAX and out_cap >= n*n, else
 * FRI_EINVAL; the n^2 words are built in the context's grown scratch (64 MiB
 * at the limit).  Z from the product tree, the weights from the kernels of
 * fri_interpolate_points, then one kernel of synthetic divisions that writes
 * w_i * Z/(x - x_i) row by row. */
int fri_lagrange_basis(fri_ctx* ctx, const uint32_t* xs, size_t n, uint32_t* out, size_t out_cap);

/* Measurement hook (tools/poly_arith_probe.py): roots per leaf subtree of
 * this context's later fri_poly_from_roots / fri_lagrange_basis calls, a
 * power of two in 64..2048; 0 restores FRI_ROOTS_LEAF. */
int fri_debug_set_roots_leaf(fri_ctx* ctx, uint32_t leaf);

/* ---------------------------------------------------------------- FRI ops */
/* One FRI fold of a layer of size m = 2^log_m living on the coset
 * layer_offset * <w_m> (natural order): out[i] = P'(x_i^2), i < m/2, with
 * P' = even(P) + beta*odd(P).  Bit-identical to next_fri_layer's
 * coefficient fold + re-evaluation (src/fri/fri_commit.rs:53-65). */
int fri_fold(fri_ctx* ctx, const uint32_t* layer, uint32_t log_m, uint32_t layer_offset,
             uint32_t beta, uint32_t* out);

/* Merkle root of n field elements: MerkleTree::new(values).root()
 * (src/merkle/mod.rs:10-26 over rs_merkle 1.4.2, SHA-256, leaf =
 * SHA256(u64 big-endian)).  root32 = raw digest bytes; the reference's
 * `root() -> String` is their lowercase hex.  n must be >= 1. */
int fri_merkle_root(fri_ctx* ctx, const uint32_t* values, size_t n, uint8_t root32[32]);

/* Trace side of the prover (the reference's src/trace and src/prover are
 * empty): interpolate 2^log_t trace values on the subgroup
 * <w_{2^log_t}> (Polynomial::interpolate, src/polynomial/ops.rs:239-241),
 * evaluate the polynomial on the coset offset*<w_n>, n = 2^(log_t+log_blowup)
 * (the low-degree extension), and Merkle-commit the LDE (merkle/mod.rs:10-26).
 * root32 = LDE tree root.  Optional: coeffs_out (2^log_t entries, *coeff_len
 * = trimmed length), lde_out (n entries).  The tree stays on the device. */
int fri_trace_commit(fri_ctx* ctx, const uint32_t* trace, uint32_t log_t, uint32_t log_blowup,
                     uint32_t offset, uint8_t root32[32], uint32_t* coeffs_out, size_t* coeff_len,
                     uint32_t* lde_out);

/* Prover slice (BASELINE configs[3]; src/prover, src/composition are empty in
 * the reference, so the constraint system is STARK-101's FibonacciSq — the
 * crate is `stark-101`, Cargo.toml:2 — on the full trace subgroup G = <g>,
 * |G| = T = 2^log_t):  a_0 = 1, a_{T-1} = a_last, a_{i+2} = a_{i+1}^2 + a_i^2.
 * From the trace LDE kept by the last fri_trace_commit (same log_t,
 * log_blowup, offset) computes, on the coset offset*<w_n>,
 *   CP = alphas[0] (f-1)/(x-1) + alphas[1] (f-a_last)/(x-g^{T-1})
 *      + alphas[2] (f(g^2 x) - f(g x)^2 - f^2) (x-g^{T-2})(x-g^{T-1}) / (x^T-1)
 * (two divisions per point through one batch inversion), interpolates it and
 * runs fri_commit on it: the FRI of fri_commit.rs:72-122 over the composition
 * polynomial, channel continued from chan_in (after the trace root and the
 * three alphas were drawn).  FRI_EDEGREE if deg CP > T (trace violates the
 * constraints).  log_blowup 1..4.  Layers stay resident for fri_decommit_query. */
int fri_fibsq_composition_commit(fri_ctx* ctx, uint32_t log_t, uint32_t log_blowup, uint32_t offset,
                                 uint32_t a_last, const uint32_t alphas[3],
                                 const fri_channel_state* chan_in, uint32_t flags,
                                 fri_commit_result* out);

/* The FibonacciSq trace itself: out[0] = 1, out[1] = a1,
 * out[i+2] = out[i+1]^2 + out[i]^2 mod p, 2^log_t rows.  Host-side (a serial
 * recurrence); needs no context or device.  a1 must be canonical. */
int fri_fibsq_trace(uint32_t a1, uint32_t log_t, uint32_t* out);

/* Trace-tree decommitment (STARK-101 decommit_on_query: f(x), f(gx), f(g^2x)
 * with their paths): values[j] = LDE[(index + j*stride) mod n], j < count
 * (1..8); paths = count authentication paths of log2(n) sibling digests
 * (leaf -> root, 32 bytes each), as fri_auth_path formats them. */
int fri_trace_decommit(fri_ctx* ctx, uint64_t index, uint64_t stride, uint32_t count, uint32_t* values,
                       uint8_t* paths, size_t paths_cap);

/* ---------------------------------------------------------- FRI commit */
/* Full FRI commit — fri_commit(poly, domain, &mut channel)
 * (src/fri/fri_commit.rs:72-122): LDE of `coeffs` on offset*<w_n>,
 * n = 2^log_n; per layer SHA-256 Merkle tree, channel.send(root_hex),
 * beta = channel.receive_random_field_element(), fold; loop while the
 * folded polynomial's degree >= 1; channel.send(final.to_bytes()).
 * chan_in may be NULL (fresh Channel::new()).  Layers and trees stay on the
 * device until the next commit on this context.  A coefficient >= p gives
 * FRI_EINVAL: the device checks the coefficients in layer 0's coefficient
 * scan, so the call returns only after the commit has run, with nothing
 * served.  There is no host pass over the input. */
int fri_commit(fri_ctx* ctx, const uint32_t* coeffs, size_t d, uint32_t log_n,
               uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
               const uint32_t* forced_betas, fri_commit_result* out);

/* Same, with the coefficients already resident in device memory
 * (d_coeffs: a device pointer; may be fri_ctx_input_buffer()). */
int fri_commit_device(fri_ctx* ctx, const uint32_t* d_coeffs, size_t d, uint32_t log_n,
                      uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
                      const uint32_t* forced_betas, fri_commit_result* out);

/* The context's input buffer: a device buffer of >= d words (on rank 0's
 * device for a multi-GPU context) that fri_commit_device and
 * fri_commit_device_async read in place, on any commit lane, without a copy.
 * It belongs to the caller, as `poly` does in fri_commit(poly, domain,
 * &mut channel) (src/fri/fri_commit.rs:72-76): no commit ever writes it, so a
 * commit from it commits exactly what the caller last wrote there (with its
 * own kernels or copies, or fri_ctx_input_upload), whatever was committed
 * before or on which lane.  Commits from any other pointer stage their
 * coefficients in the plan's private buffer instead.  Created on first call;
 * valid until a call with a larger d moves it (contents kept) or
 * fri_ctx_destroy.  d <= 2^log_n_max. */
int fri_ctx_input_buffer(fri_ctx* ctx, size_t d, uint32_t** d_ptr);
/* Fills the input buffer (grown to >= d words as fri_ctx_input_buffer does)
 * with d host coefficients, after the pending pipelined commits that read it
 * have finished; returns when the copy is complete. */
int fri_ctx_input_upload(fri_ctx* ctx, const uint32_t* coeffs, size_t d);

/* Pipelined commits: a prover that commits many codewords in a row calls
 * fri_commit (src/fri/fri_commit.rs:72-122) in a loop; here it enqueues them.
 * fri_commit_device_async validates the arguments, enqueues the whole commit
 * of fri_commit_device on the context stream and returns at once with a
 * ticket; fri_commit_wait(ticket) waits for that commit and returns its
 * result, with the same errors fri_commit_device would have returned.  Up to
 * FRI_MAX_INFLIGHT commits may be pending (FRI_ESTATE beyond that).  They run
 * on separate lanes (fri_ctx_set_lanes): concurrently, with no host round
 * trip between one commit's kernels and the next one's.  A commit with another
 * (d, log_n, offset) first waits for the pending ones.  The read-backs
 * (fri_commit_info .. fri_decommit_query) serve the most recently enqueued
 * commit and wait for it.  Not while profiling (FRI_ESTATE).
 * d_coeffs is read when the commit runs on the device, not when the call
 * returns: it must stay unchanged until fri_commit_wait(ticket) has returned.
 * fri_ctx_input_buffer() is one buffer, read in place by every pending commit
 * handed it: refill it only through fri_ctx_input_upload (which waits for
 * them), give each pending commit its own device buffer, or use
 * fri_commit_async, which copies host coefficients into the ticket's own
 * pinned buffer before returning. */
#define FRI_MAX_INFLIGHT 4
int fri_commit_device_async(fri_ctx* ctx, const uint32_t* d_coeffs, size_t d, uint32_t log_n,
                            uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
                            const uint32_t* forced_betas, uint64_t* ticket);
/* Same, from host coefficients: copied into a pinned buffer of the result
 * slot before the call returns (the caller may reuse `coeffs` at once), then
 * to the device as an asynchronous copy on the context stream. */
int fri_commit_async(fri_ctx* ctx, const uint32_t* coeffs, size_t d, uint32_t log_n,
                     uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
                     const uint32_t* forced_betas, uint64_t* ticket);
int fri_commit_wait(fri_ctx* ctx, uint64_t ticket, fri_commit_result* out);

/* Commit lanes of pipelined commits.  Each lane is a stream with its own
 * commit plan (input and coefficient buffers, layers, trees, x^-1 tables,
 * graphs, device state), created on first use.  A pipelined commit goes to
 * the lane with the fewest pending (un-waited) commits, ties to the lane
 * dealt a commit longest ago (an unused lane first, lower index first); a
 * lane that gets no HBM for its plan is dropped from the rotation until the
 * next fri_ctx_set_lanes or plan change (the commit runs on another lane;
 * FRI_ENOMEM only when lane 0 itself cannot get one).  Commits on different lanes run
 * concurrently, so one commit's serial tree tops (the Fiat-Shamir chain,
 * one workgroup) overlap the next commit's leaf hashing on the otherwise
 * idle chip.  Default FRI_DEFAULT_LANES (3) lanes: a caller keeping k <= 3
 * commits pending uses k lanes and k plans of HBM (about 2.3 GB per 2^24
 * plan, 38 GB per 2^28 plan); max_lanes = 1 runs them one after another on
 * one stream.  Three, because HIP spreads a process's streams over its
 * hardware queues (GPU_MAX_HW_QUEUES, 4 by default) in creation order: a
 * fourth lane shared a queue with another and ran serialised with it
 * (2^24: 3.41-3.45 ms per commit with 3 lanes and 3 pending, 3.75-3.86 with
 * 4 and 4; profiles/r04_lanes_queues.txt).  Lanes already created keep their
 * memory until the next plan change or fri_ctx_destroy.  FRI_ESTATE while
 * commits are pending. */
#define FRI_DEFAULT_LANES 3
int fri_ctx_set_lanes(fri_ctx* ctx, uint32_t max_lanes);
/* Diagnostic: the lane a pending pipelined commit was dealt to (0-based);
 * FRI_EINVAL for a ticket that is not pending. */
int fri_debug_ticket_lane(fri_ctx* ctx, uint64_t ticket, int* lane);

/* Batched commit: `batch` independent fri_commit calls (src/fri/fri_commit.rs:
 * 72-122) of one shape in one call, for the many small codewords of
 * per-transaction proofs and recursion leaves, whose single commits are a
 * serial chain of one-workgroup launches on an otherwise idle chip.
 * Member b: coefficients coeffs + b*d (d each, trailing zeros allowed), channel
 * chan_in[b] (chan_in NULL: every member starts from Channel::new()), forced
 * betas forced_betas + b*FRI_MAX_ROUNDS (with FRI_FLAG_FORCE_BETAS), result
 * out[b], status[b].  out[b] is word for word what fri_commit returns for the
 * same arguments, and the member's stored layers, tree levels, degrees and
 * decommitments (fri_batch_*) are what the single commit's read-backs return.
 *
 * How it runs: the LDE of all members is a fixed number of launches, in LDS
 * (one workgroup per member) for log_n <= FRI_BATCH_LDE_LDS_MAX_LOG_N and as
 * one pointwise launch plus the batched transform above it; then ONE launch
 * commits every member, one 512-thread workgroup each, from layer 0 to its
 * last layer (layers above 2^9 elements in tiles of 2^9 leaves through the
 * member's HBM slots, smaller ones in LDS).  No workgroup ever waits for
 * another.  One CU hashes a whole member, so a small batch is slower than a
 * loop of fri_commit_device: batch where there are tens of members or more
 * (the table below).
 *
 * 1 <= log_n <= FRI_BATCH_MAX_LOG_N (and the context's log_n_max), d <= 2^log_n
 * (else FRI_EDEGREE), 1 <= batch <= 65535.  Flags: FRI_FLAG_FORCE_BETAS, and
 * FRI_FLAG_NO_GRAPH (accepted, no effect: a batch replays no graph); any other
 * is FRI_EINVAL.  A multi-GPU context gives FRI_EINVAL, a profiling context
 * FRI_ESTATE.  Argument errors write nothing.  The call first waits for
 * pending pipelined commits.  A member with a coefficient >= p (found on the
 * device) gets status[b] = FRI_EINVAL and serves no read-backs (FRI_ESTATE);
 * every other member is served.  The call returns FRI_OK when every member
 * succeeded, else the first failing member's code.
 *
 * Memory per member: the one-GPU plan's layers and trees,
 *   4 * (2^(log_n+1) - 2^(log_n-R)) + 32 * sum_{k<=R} (2^(log_n-k+1) - 1) bytes
 * (R = the rounds bound of d: ceil(log2 d), at most log_n), two coefficient
 * buffers of 4 * (d/2 + 1) bytes, 4 * d more for host input and 4 * d more
 * above FRI_BATCH_LDE_LDS_MAX_LOG_N, and a 2.2 KB state: 8.6 MiB at 2^16 with
 * d = 2^13.  The x^-1, power and twiddle tables are shared by the members.
 * The buffers belong to the batch, grow on demand and stay until a larger
 * batch or fri_ctx_destroy; no single commit's plan or graph is touched.
 * FRI_ENOMEM leaves the context usable and what was resident readable.
 *
 * Residency: a batch bumps the commit generation; after it fri_commit_info
 * reports n_layers = 0 and the single-commit read-backs give FRI_ESTATE
 * (their message names fri_batch_*); after any later commit the fri_batch_*
 * read-backs give FRI_ESTATE.
 *
 * FRI_BATCH_MAX_LOG_N: the largest measured log_n in 14..18 at which a batch
 * of 256 is faster per commit than three pipelined commits pending
 * (tools/batch_probe.py, profiles/commit_batch.txt; us per commit, d = n/8):
 *   log_n   loop of fri_commit_device   3 pipelined pending   batch of 16     64    256   1024
 *     8              225                     79                   14.4    3.9    1.3    0.9
 *    10              329                    115                   23.3    6.1    1.8    1.3
 *    12              445                    155                   54.6   14.1    3.9    2.7
 *    14              570                    203                    171   43.3   11.2    8.2
 *    16              710                    264                    627    157   40.1   29.7
 *    18              911                    359                   2440    614    156      -
 * A batch of 1 costs 215 us at 2^8 and 38.9 ms at 2^18 (one CU hashes the whole
 * member): a batch beats the loop from 16 members on (64 at 2^18), the
 * pipelined commits from 16 up to 2^14, 64 at 2^16 and 256 at 2^18.  At 256
 * members it is 63x (2^10) to 2.3x (2^18) faster per commit than three
 * pipelined commits, so the cap is 18.  The first call of a shape also
 * allocates: 0.9 ms (2^10, B = 256) to 41 ms (2^18, B = 256) in all.
 */
#define FRI_BATCH_MAX_LOG_N          18
#define FRI_BATCH_LDE_LDS_MAX_LOG_N  12
int fri_commit_batch(fri_ctx* ctx, const uint32_t* coeffs, size_t d, uint32_t batch, uint32_t log_n,
                     uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
                     const uint32_t* forced_betas, fri_commit_result* out, int* status);
/* Same, d_coeffs a device pointer to batch*d words, read in place. */
int fri_commit_batch_device(fri_ctx* ctx, const uint32_t* d_coeffs, size_t d, uint32_t batch, uint32_t log_n,
                            uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
                            const uint32_t* forced_betas, fri_commit_result* out, int* status);
/* The resident batch: the commit generation, its members and log_n (batch = 0:
 * the last commit call was not a batch). */
int fri_batch_info(fri_ctx* ctx, uint64_t* generation, uint32_t* batch, uint32_t* log_n);
/* fri_layer_copy, fri_tree_level_copy, fri_commit_degrees and
 * fri_decommit_query of one member of the resident batch. */
int fri_batch_layer_copy(fri_ctx* ctx, uint32_t member, uint32_t layer, uint32_t* out, size_t cap);
int fri_batch_tree_level_copy(fri_ctx* ctx, uint32_t member, uint32_t layer, uint32_t level, uint8_t* out,
                              size_t cap);
int fri_batch_commit_degrees(fri_ctx* ctx, uint32_t member, int32_t* out, size_t cap, uint32_t* n_out);
int fri_batch_decommit_query(fri_ctx* ctx, uint32_t member, uint64_t index, uint32_t* values, size_t values_cap,
                             uint8_t* paths, size_t paths_cap, size_t* paths_len);

/* Batched prover: `batch` STARK-101 FibonacciSq proofs of one shape
 * (log_t, log_blowup, offset), each with its own trace and channel, in a
 * fixed number of launches per step instead of per proof.  Every member's
 * results are bit-identical to fri_trace_commit, fri_fibsq_composition_commit,
 * fri_trace_decommit and fri_decommit_query for the same inputs.
 *
 * L = log_t + log_blowup with 1 <= L <= FRI_BATCH_MAX_LOG_N (and the context's
 * log_n_max), log_t >= 2, log_blowup in 1..4, 1 <= batch <= 65535; one-device
 * contexts only (a multi-GPU context gives FRI_EINVAL, a profiling context
 * FRI_ESTATE, as fri_commit_batch).  A value that is not canonical, a shape
 * outside the limits or an offset with offset^T in <w_B> is FRI_EINVAL for the
 * whole call (the message names the member) and nothing is written.
 *
 * fri_trace_commit_batch: batch x fri_trace_commit.  traces: batch * 2^log_t
 * canonical words (host), roots32: batch * 32 bytes.  The LDEs and trees stay
 * resident in the batch's buffers (4 * 2^L + 64 * 2^L bytes per member, and
 * 8 * 2^log_t more for the input and the coefficients) through the composition
 * commit that consumes them, until the next fri_trace_commit_batch, any
 * non-batch commit, a plain fri_commit_batch or fri_ctx_destroy; the single
 * fri_trace_commit's resident trace is not touched.  FRI_ENOMEM leaves the
 * context usable and what was resident readable.
 *   How it runs: the interpolation on <w_T> in LDS up to 2^12 (one workgroup
 * per member), above that the batched transform; the LDE of fri_commit_batch;
 * then ONE launch hashes every member's tree, one 512-thread workgroup each.
 *
 * fri_fibsq_composition_commit_batch: batch x fri_fibsq_composition_commit on
 * the resident trace batch (same log_t, log_blowup, offset and batch, else
 * FRI_ESTATE).  a_last[b], alphas[3*b .. 3*b+2], chan_in[b] (required),
 * out[b], status[b].  flags: FRI_FLAG_NO_GRAPH is accepted without effect,
 * anything else is FRI_EINVAL.  The composition's coefficients are committed
 * as fri_commit_batch_device commits them (the commit generation moves, the
 * fri_batch_* read-backs serve the members).  A member whose composition
 * polynomial has degree above 2^log_t (its trace violates the constraints)
 * gets status[b] = FRI_EDEGREE and serves no read-backs; every other member
 * is served, and the call returns the first failing member's code.
 *
 * fri_batch_query_round: one query of every member of the resident batch in
 * ONE launch and ONE read-back (per chunk of fri_batch_query_phase's staging
 * budget: one chunk below 256 MiB of records).  indices[b]: member b's query index (taken
 * mod each layer's size, as fri_decommit_query; < 2^L when trace_count > 0).
 * skip (may be NULL): skip[b] != 0 leaves member b out; so is a member whose
 * commit failed.  trace_count = 0: the FRI openings only (serves a plain
 * fri_commit_batch); trace_count 1..8 needs the resident trace batch behind
 * the batch (else FRI_ESTATE) and opens LDE[(index + j*trace_stride) mod 2^L],
 * j < trace_count, with their paths.  Member b's record:
 *   values + b*values_stride (words): trace_count trace values, then
 *     2 * n_layers(b) FRI values in fri_decommit_query's order;
 *   paths + b*paths_stride (bytes): trace_count paths of 32*L bytes, then the
 *     FRI paths in fri_decommit_query's layout;
 *   paths_len[b]: the bytes written (0 for a member left out, whose record is
 *     not touched).
 * Strides too small for the served member with the most layers give
 * FRI_EINVAL with the needed paths_stride in paths_len[0]; the needed
 * values_stride is trace_count + 2 * n_layers words.
 *
 * Measured against a loop of prove_fibsq through the Python mirror
 * (tools/batch_probe.py --prove, profiles/prove_batch.txt, DESIGN.md section
 * 4f; us per proof inside the device calls, blowup 8, B = 256): 8.8 against
 * 827 at log_t 7 with 8 queries, 22.7 against 1788 with 32; 76.1 against 1320
 * and 96.9 against 2428 at log_t 13.  The batch is faster from the smallest
 * size measured, B = 16, at every measured shape (1.4x at log_t 13, 8 queries). */
int fri_trace_commit_batch(fri_ctx* ctx, const uint32_t* traces, uint32_t log_t, uint32_t log_blowup,
                           uint32_t offset, uint32_t batch, uint8_t* roots32);
int fri_fibsq_composition_commit_batch(fri_ctx* ctx, uint32_t log_t, uint32_t log_blowup, uint32_t offset,
                                       uint32_t batch, const uint32_t* a_last, const uint32_t* alphas,
                                       const fri_channel_state* chan_in, uint32_t flags, fri_commit_result* out,
                                       int* status);
int fri_batch_query_round(fri_ctx* ctx, const uint64_t* indices, const uint8_t* skip, uint32_t trace_count,
                          uint64_t trace_stride, uint32_t* values, size_t values_stride, uint8_t* paths,
                          size_t paths_stride, size_t* paths_len);

/* fri_batch_query_phase: the WHOLE query phase of every member of the resident
 * batch in one call, the members' channels included.
 * For every served member b it is num_queries x { receive_random_int(0,
 * max_index, true); the sends of prove_fibsq's query round } on chan[b]; with
 * trace_count = 0 the sends are decommit_fri_layers' alone.  The message order
 * is the one fri_verify_batch replays, the doubled value of a one-element
 * layer included.
 *   chan[b]: in, the channel before the first draw; out, after the last send.
 *   indices[b*num_queries + q]: the index drawn for member b's query q.
 *   values + (b*num_queries + q)*values_stride, paths + (b*num_queries +
 *     q)*paths_stride: fri_batch_query_round's record for that index, in the
 *     layout fri_verify_batch takes (the outputs feed it without repacking).
 *   paths_len[b]: the bytes of ONE query's paths of member b; 0 for a member
 *     left out (skip[b] != 0, or its commit failed), whose chan[b], indices
 *     and records are not touched.
 * skip, trace_count and trace_stride are fri_batch_query_round's.
 * num_queries = 0 returns FRI_OK with nothing written.
 *
 * With nothing written: FRI_ESTATE without a resident batch, or without the
 * resident trace batch behind it when trace_count > 0, and on a profiling
 * context; FRI_EINVAL for trace_count > 8, max_index >= 2^32, max_index >=
 * 2^L with trace_count > 0, num_queries above FRI_VERIFY_MAX_QUERIES, a served
 * member with has_state = 0 (the reference panics there, channel.rs:65), a
 * multi-GPU context, and strides too small (the needed paths_stride in
 * paths_len[0], as the round).
 *
 * How it runs: one lane per member draws each index, rehashes, and absorbs the
 * openings in the transcript's order, reading values and sibling digests
 * where they live, in the resident LDEs, layers and trees; a second kernel
 * then gathers the records of the drawn indices, and one read-back brings
 * indices, records and final states to the host.  The members go through
 * device and pinned staging in chunks of a 256 MiB budget
 * (fri_debug_set_query_chunk: members per chunk, 0 = by the budget; the hook
 * governs fri_batch_query_round too, which stages through the same chunks, a
 * batch under the budget in one launch and one read-back).  The call
 * reads and changes nothing of the resident batch: the commit generation does
 * not move and fri_batch_query_round serves the same batch afterwards.
 * FRI_ENOMEM leaves the context usable and what was resident readable.
 *
 * Measured (tools/batch_probe.py --prove, profiles/prove_batch_device_queries.txt,
 * DESIGN.md section 4f; us per proof, blowup 8, the whole call of the Python
 * mirror, round route -> this route): at log_t 7 with 32 queries 1338 -> 2638 at
 * B = 16, 1213 -> 856 at 64, 1180 -> 478 at 256 and 1270 -> 423 at 4096; at
 * log_t 13 with 32 queries 3009 -> 5512, 2317 -> 1861, 2121 -> 931 and 2212 ->
 * 867.  One lane hashes a member's whole phase, so the chain kernel runs for
 * milliseconds whatever the batch: at every measured shape (log_t 7, 10, 13 with
 * 8 and 32 queries) the whole call is slower than the round route at B = 16
 * (0.47x to 0.71x) and faster from B = 64, the smallest measured size where it
 * wins, in both runs (1.1x to 1.5x at 64, 1.9x to 2.5x at 256, 2.4x to 3.0x at
 * 4096).  The route is opt-in: no default uses it. */
int fri_batch_query_phase(fri_ctx* ctx, uint32_t num_queries, uint64_t max_index,
                          fri_channel_state* chan,          /* [batch] in: before the first draw; out: after the last send */
                          const uint8_t* skip,              /* may be NULL, as fri_batch_query_round */
                          uint32_t trace_count, uint64_t trace_stride,
                          uint64_t* indices,                /* [batch][num_queries] out */
                          uint32_t* values, size_t values_stride,   /* words per (member, query) */
                          uint8_t* paths, size_t paths_stride,      /* bytes per (member, query) */
                          size_t* paths_len);               /* [batch]: bytes per query of member b, 0 = left out */
int fri_debug_set_query_chunk(fri_ctx* ctx, uint32_t members);     /* 0 = automatic */

/* Proof-of-work grinding before the query phase (the
 * reference has none: its prover files are empty).  A prover that grinds
 * `bits` bits sends, after the FRI commit's final value and before the first
 * query index is drawn, the smallest 8-byte nonce that leaves the channel with
 * `bits` leading zero bits:
 *   grind(channel, bits, first = 0):
 *     v = the smallest integer in [first, last] such that
 *         D = SHA256(ascii(channel.state) || ascii(hex(be64(v))))
 *         has its `bits` most significant bits zero
 *     channel.send(be64(v))                  (channel.rs:35-44: the state becomes D)
 * with lowercase hex, an empty state for has_state = 0, and 0 <= bits <= 32.
 * bits = 0 accepts v = first and still sends it.  A verifier checks the zero
 * bits of the state after the send, not that v is the smallest; the prover
 * returns the smallest so that transcripts are deterministic.
 *
 * fri_grind: chan_in the channel before the send (NULL: Channel::new()).
 * *found = 1 with *nonce = v and, when chan_out is not NULL, *chan_out the
 * channel after the send; *found = 0, with *nonce and *chan_out untouched,
 * when [first, last] holds no such nonce (FRI_OK either way).
 * fri_grind_batch: fri_grind from first = 0 for every member of chan[batch]:
 * nonces[b], found[b], and chan[b] replaced by the member's channel after the
 * send when found[b] (untouched otherwise).
 *
 * How it runs.  The state's 64 hex characters are the first block of every
 * candidate's message, so a candidate costs ONE compression, from the member's
 * midstate, of a block in which only the nonce's four words vary: one lane per
 * candidate, on the rate-ordered rounds of the leaf kernels, and only digest
 * word 0 is formed.  The host walks the range in windows of consecutive
 * nonces, in rising order; inside a window the hits go through a wave
 * reduction and a 64-bit atomic minimum per member, and the first window with
 * a hit ends the member's search, so the answer is the smallest whatever order
 * the workgroups run in.  (A wave leaves once its next nonces lie above the
 * current minimum; that only saves work.)  One launch covers every unfinished
 * member's window and is followed by one read-back of the members' words
 * through pinned memory.  The automatic window is 8 * 2^bits nonces, from 2^12
 * up to 2^30 (one launch of 35 ms at the measured rate);
 * fri_debug_set_grind_window sets log2 of the nonces per launch for the
 * context's later calls (1..32; 0 = automatic).
 *
 * Measured on one MI355X (tools/grind_probe.py, profiles/grind.txt, DESIGN.md
 * section 4h).  The kernel alone searches 31.0 G nonces/s (2^28 in 8.7 ms, device
 * events): 1300 VALU instructions = 2038 issue units per nonce, 63.2 T units/s,
 * 99% of the measured 64 T VALU ceiling (the layer-0 leaf kernel: 94%).  One
 * whole fri_grind from nonce 0, median over 16 states: 0.049 ms at 16 bits,
 * 0.109 at 20, 1.25 at 24 and 5.0 at 28 (26.4 G nonces/s of the nonces it had
 * to look at).  fri_grind_batch at B = 4096: 0.61 us per member at 8 bits, 0.81
 * at 12, 4.4 at 16 and 51.9 at 20 (20.4 G nonces/s).  Against that the C++
 * mirror's host loop does 17.7 M nonces/s on one core with the SHA extensions
 * and 283 M over 16 threads, hashlib 2.7 M.  A call costs about 32 us whatever
 * the bits up to 12, so the mirrors grind on the host below
 * GRIND_DEVICE_MIN_BITS, the smallest measured size from which the device call
 * with its copies wins: 10 bits in the C++ mirror (51.5 us on the host against
 * 32.4) and 8 in the Python one (78.6 against 32.4).
 *
 * FRI_EINVAL, with nothing written: bits > 32, first > last, batch outside
 * 1..65535, a null nonce / found / chan array.  fri_grind_batch on a multi-GPU
 * context is FRI_EINVAL and on a profiling context FRI_ESTATE, as
 * fri_commit_batch; fri_grind runs on rank 0 of a team and, while profiling,
 * is timed as class "grind" (one span per launch).  The calls read and change
 * nothing of the resident commit, batch or trace batch: the commit generation
 * does not move.  The staging (84 bytes per member) belongs to the context and
 * stays until fri_ctx_destroy. */
int fri_grind(fri_ctx* ctx, const fri_channel_state* chan_in, uint32_t bits,
              uint64_t first, uint64_t last,            /* inclusive range, first <= last */
              uint64_t* nonce, uint32_t* found,
              fri_channel_state* chan_out);             /* may be NULL; written only when found */
int fri_grind_batch(fri_ctx* ctx, uint32_t batch, fri_channel_state* chan,   /* [batch] in/out */
                    uint32_t bits, uint64_t last, uint64_t* nonces, uint32_t* found);
int fri_debug_set_grind_window(fri_ctx* ctx, uint32_t log_window);   /* nonces per launch; 0 = automatic */

/* Batched verifier: `batch` transcripts of one shape checked in one call, the
 * counterpart of the batched prover.  verify_fri / verify_fibsq of the host
 * mirrors (one transcript, SHA-256 on one CPU core) stay the yardstick: for
 * every transcript the verdict here is 0 exactly when they return true.
 *
 * How it runs.  A transcript carries the challenges and
 * query indices it claims, so two independent kernels decide it: one lane per
 * member replays the Fiat-Shamir channel (channel.rs:35-84) over the whole
 * transcript and checks that every claimed alpha, beta and index is the one the
 * replay draws; one lane per opening checks every authentication path, fold,
 * final value and composition against the claimed values.  A member is
 * accepted when neither finds anything.  Every check runs for every member:
 * verdict[b] is the OR of the failed classes below, 0 = accepted.
 *
 * Record layout (host pointers).  Member b's head at head + b*head_stride
 * (words): with trace_count = 3 the trace root (8 big-endian digest words) and
 * the 3 claimed alphas; then max_layers roots of 8 words; max_layers - 1
 * claimed betas; the final value.  A member with fewer layers fills a prefix
 * of the roots and of the betas (the rest is not read).  A root is its 32 raw
 * bytes: the message on the wire is their 64-character lowercase hex.  Member
 * b's query q: the claimed index at indices[b*num_queries + q] and the record
 * fri_batch_query_round writes, at values + (b*num_queries + q)*values_stride
 * (words: trace_count trace values, then 2 * n_layers(b) FRI values in
 * fri_decommit_query's order) and paths + (b*num_queries + q)*paths_stride
 * (bytes: trace_count paths of 32*log_n bytes, then the FRI paths in
 * fri_decommit_query's layout).  chan_in[b]: the channel before the member's
 * first message.
 *
 * Grinding (fri_verify_batch_pow).  With grinding_bits > 0 every transcript
 * carries the 8-byte nonce a prover route sends after the final value and
 * before the first query index (fri_grind above); member b's is nonces[b], a
 * plain host uint64_t: the array fri_grind_batch writes feeds this call
 * without repacking, like the query records.  The channel kernel sends it
 * after the final value, and the state after that send must have grinding_bits
 * leading zero bits, else FRI_VERIFY_POW.  The replay goes on from that state
 * whether it has them or not, so a transcript that only lacks bits gets
 * FRI_VERIFY_POW and nothing else.  The nonce need not be the smallest.  With
 * grinding_bits = 0 there is no such message, nonces is not read and may be
 * NULL: fri_verify_batch is fri_verify_batch_pow(..., 0, NULL, verdict).
 *
 * Numbers taken from a transcript only choose left/right in a path climb and
 * exponents of domain points (indices are taken mod the layer size, trace
 * positions mod 2^log_n); they never form an address.
 *
 * FRI_EINVAL, with nothing written: a shape outside the limits in
 * fri_verify_shape, strides below the record's size, batch outside 1..65535,
 * n_layers[b] outside 1..max_layers, offset or a_last[b] >= p, a multi-GPU
 * context, grinding_bits > 32, grinding_bits > 0 with nonces = NULL.
 * FRI_ENOMEM (one member's staging does not fit) leaves the context usable.  Otherwise FRI_OK, whatever the verdicts.  The members are uploaded
 * and checked in chunks of a 2 GiB staging budget, one launch pair each
 * (fri_debug_set_verify_chunk: members per chunk, 0 = by the budget); the
 * staging belongs to the context and stays until fri_ctx_destroy.  The two
 * kernels run on two streams joined by events; FRI_VERIFY_SERIAL=1
 * (environment, a measurement hook) runs them one after the other, as a
 * profiling context does (classes "verify_chain" and "verify_open").  The
 * call reads and changes nothing of the resident commit, batch or trace
 * batch: the commit generation does not move.
 *
 * Measured (tools/batch_probe.py --verify, profiles/verify_batch.txt, DESIGN.md
 * section 4g; us per proof, blowup 8, the device call with its copies against a
 * loop of the C++ verify_fibsq on one core / over 16 threads): at log_t 7 with 8
 * queries 591 at B = 16, 31.2 at 256 and 2.6 at 4096 against 308 / 22.0; at log_t 13
 * with 32 queries 5162, 244 and 21.1 against 2367 / 152.  One lane hashes a whole
 * transcript, so the channel kernel runs for milliseconds whatever the batch: the
 * call loses to one core below B = 64 and to 16 threads below B = 4096.
 * The nonce (profiles/verify_batch_pow.txt): fri_verify_batch is as fast as
 * before it existed (the kernel without bits is the same instructions), and
 * fri_verify_batch_pow with 8 bits costs 0.32 us per proof more at log_t 7,
 * 8 queries, B = 256 (1.0%), 0.019 at B = 4096, 1.85 at log_t 13, 32 queries,
 * B = 256 and 0.12 at B = 4096 (0.6%). */
#define FRI_VERIFY_MAX_QUERIES 1024
#define FRI_VERIFY_CHANNEL      1u   /* a claimed alpha, beta or query index is not what the replayed channel draws */
#define FRI_VERIFY_TRACE_PATH   2u   /* a trace opening does not reach the trace root                               */
#define FRI_VERIFY_COMPOSITION  4u   /* layer 0 at the query is not the composition of the opened f(x), f(gx), f(g^2 x) */
#define FRI_VERIFY_FRI_PATH     8u   /* a layer opening does not reach its layer root                              */
#define FRI_VERIFY_FOLD        16u   /* a layer-k value is not the fold of its layer-(k-1) pair                    */
#define FRI_VERIFY_FINAL       32u   /* the last layer's pair is not the final value                               */
#define FRI_VERIFY_MALFORMED   64u   /* a packed word >= p, or (set by the host mirrors) a transcript that cannot be packed */
#define FRI_VERIFY_POW        128u   /* the state after the nonce's send lacks grinding_bits leading zero bits     */
typedef struct {
    uint32_t log_n;        /* layer 0 has 2^log_n values; 1..min(30, ctx log_n_max) */
    uint32_t max_layers;   /* record stride in layers, 1..log_n+1                   */
    uint32_t num_queries;  /* 0..FRI_VERIFY_MAX_QUERIES                             */
    uint32_t trace_count;  /* 0: FRI only (verify_fri); 3: STARK-101 FibonacciSq    */
    uint32_t log_t, log_blowup;   /* trace_count = 3: log_n = log_t + log_blowup,
                                     log_t >= 2, log_blowup 1..4                    */
    uint32_t offset;       /* coset offset, canonical                               */
    uint64_t max_index;    /* the query draw's upper bound (verify_fri's max_index,
                              below 2^32; 2^log_n - 2*2^log_blowup - 1 when
                              trace_count = 3)                                      */
} fri_verify_shape;
int fri_verify_batch(fri_ctx* ctx, const fri_verify_shape* shape, uint32_t batch,
                     const fri_channel_state* chan_in,   /* [batch] */
                     const uint32_t* n_layers,           /* [batch], 1..max_layers */
                     const uint32_t* a_last,             /* [batch] when trace_count = 3, else NULL */
                     const uint32_t* head, size_t head_stride,      /* words  */
                     const uint64_t* indices,                        /* [batch][num_queries] claimed */
                     const uint32_t* values, size_t values_stride,  /* words per (member, query) */
                     const uint8_t* paths, size_t paths_stride,     /* bytes per (member, query) */
                     uint32_t* verdict);                             /* [batch] mask, 0 = accepted */
int fri_verify_batch_pow(fri_ctx* ctx, const fri_verify_shape* shape, uint32_t batch,
                         const fri_channel_state* chan_in, const uint32_t* n_layers, const uint32_t* a_last,
                         const uint32_t* head, size_t head_stride, const uint64_t* indices,
                         const uint32_t* values, size_t values_stride, const uint8_t* paths, size_t paths_stride,
                         uint32_t grinding_bits,            /* 0..32; 0: no nonce message */
                         const uint64_t* nonces,            /* [batch] when grinding_bits > 0, else ignored */
                         uint32_t* verdict);
int fri_debug_set_verify_chunk(fri_ctx* ctx, uint32_t members);    /* 0 = automatic */

/* Which commit the read-backs below serve: `generation` grows with every
 * commit call on the context (successful or not), log_n / n_layers describe
 * the resident commit (n_layers = 0 when the last commit failed).  A binding
 * that hands out FRIProof objects records the generation at commit time and
 * refuses read-backs once it has moved on (the reference's FRIProof owns its
 * layers, src/fri/fri_commit.rs:9-13; here they live in the context). */
int fri_commit_info(fri_ctx* ctx, uint64_t* generation, uint32_t* log_n, uint32_t* n_layers);

/* Read-back of the last commit (FRIProof::fri_layers / fri_merkles). */
int fri_layer_copy(fri_ctx* ctx, uint32_t layer, uint32_t* out, size_t cap);
/* Merkle level `level` (0 = leaf hashes) of layer `layer`, as 32-byte digests. */
int fri_tree_level_copy(fri_ctx* ctx, uint32_t layer, uint32_t level, uint8_t* out, size_t cap);

/* Decommitment helper (src/fri/fri_commit.rs:137-165): value and the
 * rs_merkle authentication path (sibling hashes leaf->root) of `index` in
 * committed layer `layer`.  path must hold 32*depth bytes; *depth_out set. */
int fri_auth_path(fri_ctx* ctx, uint32_t layer, uint64_t index, uint32_t* value_out,
                  uint8_t* path, uint32_t* depth_out);

/* Decommitment of one FRI query (decommit_fri_layers, src/fri/fri_commit.rs:
 * 137-163) from the layers and trees of the last fri_commit, still in HBM.
 * For every committed layer k (m_k = 2^(log_n-k) elements): idx = index % m_k,
 * sib = (idx + m_k/2) % m_k; values[2k] = layer_k[idx], values[2k+1] =
 * layer_k[sib]; paths = for each k, the authentication path of idx then of
 * sib (rs_merkle single-leaf proof: sibling digests leaf -> root, 32 bytes
 * each, (log_n-k) per path) — the byte strings the reference sends.
 * *paths_len = total path bytes (also set when paths_cap is too small). */
int fri_decommit_query(fri_ctx* ctx, uint64_t index, uint32_t* values, size_t values_cap,
                       uint8_t* paths, size_t paths_cap, size_t* paths_len);

/* ------------------------------------------- single-process multi-GPU team */
/* One context over n_devices GPUs, driven by ONE call from ONE host thread:
 * the reference's fri_commit(poly, domain, &mut channel)
 * (src/fri/fri_commit.rs:72-76) spread over 1-8 GPUs ("the library drives
 * 1-8 GPUs from one host thread").  devices: the HIP
 * ordinals of ranks 0..n-1 (NULL: 0..n-1); an ordinal may repeat (several
 * ranks on one GPU; peer transport only).  n_devices: a power of two <= 64;
 * 1 gives an ordinary context.  log_n_max: the largest codeword, and the
 * bound of every other call on the context.  The contexts of ranks 1..n-1
 * are shard-sized (2^(log_n_max - log2 n), and at least 2^min(log_n_max,
 * 19)); rank 0's, which also runs the commits below the sharding threshold
 * and the kernel-level calls alone, holds twiddles and scratch for
 * 2^log_n_max (20 bytes per element on devices[0]).  transport:
 *   FRI_TRANSPORT_PEER  device copies between the ranks' buffers: one pull
 *                       kernel per collective reading the other ranks'
 *                       memory over xGMI peer access (hipMemcpyPeerAsync per
 *                       source where peer access is unavailable), ordered by
 *                       events;
 *   FRI_TRANSPORT_NONE  the default: the peer transport;
 *   FRI_TRANSPORT_RCCL  opt-in: communicators from ncclCommInitAll (xGMI),
 *                       distinct devices only (FRI_EINVAL otherwise).  A rank
 *                       that fails aborts its communicators at once and the
 *                       others theirs when they see it (FRI_ERCCL); the
 *                       team's later sharded calls then return FRI_ESTATE.
 * Inside, rank 0 runs on the calling thread and ranks 1..n-1 on worker
 * threads of the context (one per rank), each issuing the sharded protocol
 * of fri_commit_sharded on its device.  The returned context is rank 0's:
 *   fri_commit / fri_commit_device / fri_commit_sharded*: a codeword of
 *     >= 2^20 elements (and >= 2^(12 + log2 n)) is committed coset-sharded
 *     over the ranks in this one call, with the same result and transcript
 *     as a 1-GPU commit; smaller codewords run on rank 0 alone.
 *     fri_commit_device reads a buffer on rank 0's device (the other ranks
 *     copy it over xGMI);
 *   fri_layer_copy / fri_tree_level_copy / fri_auth_path / fri_decommit_query
 *     (and _sharded) serve every layer: the sharded ones are assembled from
 *     the ranks' blocks and the replicated top trees;
 *   fri_ctx_device_bytes: the sum over the ranks;
 *   the kernel-level calls (fri_lde, fri_interpolate, fri_fold,
 *     fri_merkle_root, fri_batch_inverse, fri_evaluate*,
 *     fri_interpolate_points*, fri_poly_*, fri_poly_from_roots,
 *     fri_lagrange_basis, fri_trace_commit, fri_fibsq_composition_commit)
 *     run on rank 0 alone, up to the sizes a one-device context of
 *     log_n_max takes, and leave a resident sharded commit readable;
 *   fri_commit_*async and fri_dist_attach_* / fri_dist_detach: FRI_EINVAL.
 * Not re-entrant (one host thread at a time), like every context.
 * fri_ctx_destroy(ctx) releases every rank. */
int fri_ctx_create_multi(const int* devices, uint32_t n_devices, uint32_t log_n_max, int transport, fri_ctx** out);
/* The context a caller gets without naming devices -- what a binding that
 * keeps the reference's signatures (fri_commit(poly, domain, &mut channel),
 * decommit_fri(num_queries, max_index, &layers, &merkles, &mut channel);
 * src/fri/fri_commit.rs:72-76,168-174) opens behind them: the devices are
 *   FRI_DEVICES  (environment) comma-separated HIP ordinals, a power-of-two
 *                count <= 64, ordinals may repeat (e.g. "0,0,0,0": four
 *                ranks on one GPU);
 *   otherwise    0..k-1, k the largest power of two <= the visible devices;
 * one device gives fri_ctx_create, several fri_ctx_create_multi with the
 * transport FRI_TRANSPORT (environment: "peer", the default, or "rccl").
 * *n_ranks (may be NULL) = the number of ranks.  FRI_EINVAL for a malformed
 * FRI_DEVICES or FRI_TRANSPORT. */
int fri_ctx_create_default(uint32_t log_n_max, fri_ctx** out, uint32_t* n_ranks);
/* Diagnostic: rank `rank`'s context of a team (rank 0: ctx itself), e.g. for
 * its fri_debug_transport_log; owned by the team, never destroyed by the
 * caller (FRI_EINVAL). */
int fri_debug_team_rank(fri_ctx* ctx, uint32_t rank, fri_ctx** out);
/* Test hook (peer transport): the next team call makes rank `rank` fail
 * with FRI_ERCCL at its op_index-th collective (0-based), as a rank whose
 * transfer broke would; the other ranks must return instead of waiting for
 * it.  Applies to the next team call only (cleared at its end, fired or
 * not); op_index < 0 clears it. */
int fri_debug_team_inject_failure(fri_ctx* ctx, uint32_t rank, int64_t op_index);
/* Test hook (peer transport): enable != 0 makes every collective copy with
 * hipMemcpyPeerAsync per source, the path a team takes when peer access is
 * unavailable, instead of the pull kernel; 0 restores the pull kernel where
 * peer access allows it. */
int fri_debug_team_force_copy(fri_ctx* ctx, int enable);

/* -------------------------------------------------------------- multi-GPU */
/* One process per GPU.  A codeword of 2^log_n is committed by G ranks
 * (G a power of two): rank r computes the coset slice evals[r + G*m] of the
 * LDE (size n/G NTT), an all-to-all turns it into the contiguous block
 * [r*n/G, (r+1)*n/G), every layer is hashed block-locally, the G block roots
 * are all-gathered and the tree top + Fiat-Shamir step run redundantly on
 * every rank (identical transcript everywhere), and each fold pairs rank
 * blocks b and b + G/2 (one half-block exchange per layer).  Layers below
 * 2^20 elements are gathered and finished on every rank. */
typedef struct {
    void* user;
    /* host-staged collectives; buffers are host memory; return 0 on success */
    int (*allgather)(void* user, const void* send, void* recv, size_t bytes_per_rank);
    int (*alltoall)(void* user, const void* send, void* recv, size_t bytes_per_peer);
    int (*sendrecv)(void* user, const void* send, void* recv, size_t bytes, int peer);
} fri_collectives;

/* RCCL transport (xGMI): rank 0 creates the id, the caller distributes it.
 * A rendezvous that does not complete within FRI_RCCL_TIMEOUT_S seconds
 * (environment, default 120) returns FRI_ERCCL instead of blocking; a sharded
 * commit whose collectives make no progress for that long aborts the
 * communicators and returns FRI_ERCCL (the context then needs a new attach). */
int fri_dist_unique_id(uint8_t uid[128]);
int fri_dist_attach_rccl(fri_ctx* ctx, int rank, int world, const uint8_t uid[128]);
/* Host-callback transport (e.g. torch.distributed gloo; used by tests). */
int fri_dist_attach_host(fri_ctx* ctx, int rank, int world, const fri_collectives* ops);
int fri_dist_detach(fri_ctx* ctx);
/* The attached transport: FRI_TRANSPORT_NONE / _RCCL / _HOST, and for RCCL
 * the rank and world size the communicator itself reports
 * (ncclCommUserRank / ncclCommCount). */
#define FRI_TRANSPORT_NONE 0
#define FRI_TRANSPORT_RCCL 1
#define FRI_TRANSPORT_HOST 2
#define FRI_TRANSPORT_LOOPBACK 3   /* fri_debug_attach_loopback (timing rehearsal only) */
#define FRI_TRANSPORT_PEER     4   /* in-process team (fri_ctx_create_multi): device copies between ranks */
int fri_dist_info(fri_ctx* ctx, int* rank, int* world, int* transport);
/* Diagnostic: run the transport's all-to-all, all-gather and pair exchange
 * (both streams) on a known pattern and check the result; FRI_ERCCL with a
 * message on mismatch.  Collective: every rank must call it.  world == 1
 * exercises the same calls as self-communication. */
int fri_dist_selftest(fri_ctx* ctx, size_t words_per_peer);

/* Sharded fri_commit: every rank passes the same full coefficient vector and
 * channel state and gets the same result.  world == 1 is fri_commit.
 * Each rank's plan is shard-sized: it allocates only its block of every
 * sharded layer and tree and the x^-1 slices its folds read (plus the full
 * coefficient vector, which the coset LDE reads, and the < 2^20 local tail),
 * so a context created with log_n_max = log_n - log2(world) suffices (2^28
 * over 8 ranks: ~6 GiB each).  The coefficient fold that tracks the degree
 * (next_fri_polynomial, fri_commit.rs:32-50,89) is sharded too: rank r folds
 * coefficients [r*S_k, (r+1)*S_k) of poly_k, and the maxima that give the
 * degree travel with the block roots in the per-layer all-gather.
 * Afterwards fri_layer_copy / fri_tree_level_copy / fri_auth_path serve the
 * layers finished on every rank (the < 2^20 tail); the sharded layers return
 * FRI_ESTATE (each rank holds only its block). */
int fri_commit_sharded(fri_ctx* ctx, const uint32_t* coeffs, size_t d, uint32_t log_n,
                       uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
                       const uint32_t* forced_betas, fri_commit_result* out);
int fri_commit_sharded_device(fri_ctx* ctx, const uint32_t* d_coeffs, size_t d, uint32_t log_n,
                              uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
                              const uint32_t* forced_betas, fri_commit_result* out);

/* Decommitment of one query after fri_commit_sharded (decommit_fri_layers,
 * src/fri/fri_commit.rs:137-163), same layout and bytes as fri_decommit_query
 * on a 1-GPU commit of the same codeword.  Collective: every rank calls it
 * with the same index (the reference draws it from the transcript, identical
 * on every rank) and receives the whole decommitment; each rank contributes
 * the openings that lie in the blocks it holds. */
int fri_decommit_query_sharded(fri_ctx* ctx, uint64_t index, uint32_t* values, size_t values_cap,
                               uint8_t* paths, size_t paths_cap, size_t* paths_len);

/* ------------------------------------------------------------ diagnostics */
/* Per-span device time (ms) accumulated while profiling is enabled (hipEvents
 * recorded on the context's stream; profiling commits run eagerly, no graph).
 * Classes: "lde" (LDE NTT), "merkle_layer0_leaf" (layer-0 leaf kernel: leaves
 * + levels 1-4, with its algorithmic bytes), "layer0" (all of layer 0's tree +
 * channel step), "layers" (layers >= 1), and for sharded commits "alltoall"
 * and "gather"; fri_verify_batch adds "verify_chain" and "verify_open",
 * fri_grind "grind" (one span per window's launches).  bytes = algorithmic
 * bytes of the span where defined. */
int fri_set_profiling(fri_ctx* ctx, int enabled);
int fri_get_profile(fri_ctx* ctx, const char* kernel_class, double* total_ms, uint64_t* launches,
                    uint64_t* bytes);
int fri_reset_profile(fri_ctx* ctx);
/* Device memory (HBM) the context holds now and at most so far, in bytes:
 * twiddles, scratch, the commit plan (layers, trees, x^-1 tables), multi-GPU
 * buffers and any grown scratch.  (Diagnostic; no reference counterpart.) */
int fri_ctx_device_bytes(fri_ctx* ctx, uint64_t* current, uint64_t* peak);
/* Test hook: the context's device allocations fail (FRI_ENOMEM paths) once
 * they would take it past cap_bytes of HBM (0: no cap). */
int fri_debug_set_device_cap(fri_ctx* ctx, uint64_t cap_bytes);
/* Diagnostic build only (-DFRI_STAMPS): top-kernel phase timestamps of the
 * last commit, (FRI_MAX_LAYERS x 24) u64 ticks of the 100 MHz clock.
 * Returns FRI_ESTATE in the product build. */
int fri_debug_stamps(fri_ctx* ctx, uint64_t* out, size_t cap);
/* Host-only diagnostic (no context, no device): the commit plan's layout for
 * rank `rank` of `world` (world 1: the 1-GPU plan) of a codeword 2^log_n with
 * d coefficients.  out[0] = rounds bound R, out[1] = last sharded layer k_sw
 * (-1 for world 1), out[2] = bytes of layers + trees + x^-1 tables, out[3] =
 * log2 of the coefficient chunk S_0 a rank folds (world > 1; rank r holds
 * coefficients [r*S_k, (r+1)*S_k) of poly_k, S_k = S_0 / 2^k); then per
 * layer k <= R five words: layer-slot words, tree-slot words, x^-1 entries of
 * fold k, the domain index of the first of them, the block held of sharded
 * layer k.  cap >= 4 + 5 * FRI_MAX_LAYERS. */
int fri_debug_plan_layout(size_t d, uint32_t log_n, uint32_t world, uint32_t rank, uint64_t* out, size_t cap);
/* Test hook for the collective deadline (fri_dist_attach_rccl): with enable
 * != 0 the next RCCL all-to-all on the context is replaced by a kernel that
 * waits like a collective whose peer never arrives, until the deadline's
 * abort releases it.  The call then returns FRI_ERCCL and later sharded calls
 * FRI_ESTATE, exactly as for a real stall. */
int fri_debug_inject_stall(fri_ctx* ctx, int enable);

/* Timing rehearsal of one rank of a sharded commit on one device: attaches a
 * transport whose collectives return this rank's own bytes, as device-to-
 * device copies on the streams RCCL would use.  Every kernel of the rank runs
 * on data of the right shape with no host round trip, but the transcript is
 * not the real one (tools/shard_projection.py). */
int fri_debug_attach_loopback(fri_ctx* ctx, int rank, int world);
/* The degree schedule of the loopback rehearsal: deg[k] for every layer k of
 * a 1-GPU commit of the same polynomial (fri_commit_degrees).  The sharded
 * coefficient fold gives each rank only its slice of the degree maxima, and
 * the loopback all-gather returns this rank's own slice G times, so without
 * the recorded schedule the rehearsal would run fewer rounds than the real
 * commit.  deg = NULL or n = 0 clears it. */
int fri_debug_loopback_degrees(fri_ctx* ctx, const int32_t* deg, uint32_t n);

/* Degree of poly_k for every layer k of the resident commit (the
 * reference's Polynomial degree field, src/polynomial/ops.rs:47-60, as the
 * loop of fri_commit.rs:89 sees it): out[k], k < *n_out = n_layers. */
int fri_commit_degrees(fri_ctx* ctx, int32_t* out, size_t cap, uint32_t* n_out);

/* Transport schedule of the last sharded call on the context
 * (fri_commit_sharded*, fri_decommit_query_sharded, fri_dist_selftest): one
 * entry per collective in issue order.  chan 0 = the main communicator on the
 * context stream, 1 = the exchange communicator on the exchange stream (the
 * logical channel; the host transport runs both on the context stream).  An
 * RCCL run is deadlock-free when, per channel, every rank issues the same
 * sequence of (op, bytes) and each SENDRECV at position i with peer q is
 * matched by q's SENDRECV at position i with peer = this rank;
 * the multi-rank tests check exactly that on every rank's log. */
#define FRI_OP_ALLGATHER 1
#define FRI_OP_ALLTOALL  2
#define FRI_OP_SENDRECV  3
typedef struct {
    uint32_t chan;      /* 0: main, 1: exchange                                   */
    uint32_t op;        /* FRI_OP_*                                                */
    int32_t  peer;      /* SENDRECV partner; -1 for collectives                    */
    uint32_t reserved;
    uint64_t bytes;     /* ALLGATHER: per rank; ALLTOALL: per peer; SENDRECV: each way */
} fri_transport_op;
int fri_debug_transport_log(fri_ctx* ctx, fri_transport_op* out, size_t cap, size_t* count);

#ifdef __cplusplus
}
#endif
#endif /* FRI_AMD_H */
