// fri_kernels.hip — gfx950 kernels of the FRI commit path.
//
//   NTT (coset LDE / interpolation)  replaces Horner evaluate at every domain
//                                     point (src/fri/fri_commit.rs:78,
//                                     src/polynomial/ops.rs:76-83) and Lagrange
//                                     interpolation (interpolation.rs:121-152)
//   Merkle subtree                    replaces MerkleTree::new (src/merkle/mod.rs:10-22)
//   fold (evaluation form)            replaces next_fri_layer (src/fri/fri_commit.rs:53-65)
//   coefficient fold                  next_fri_polynomial (fri_commit.rs:32-50), O(d),
//                                     kept for the exact degree / loop condition (:89)
//   channel step (single lane)        Channel::send / receive_random_field_element
//                                     (src/channel/channel.rs:35-55) on the device
//   batch inverse                     FieldElement::inverse (element.rs:54-57), 0 -> 0
//
// Data in HBM is canonical u32 (value < p); constants are Montgomery (field.hpp).
#include "fri_internal.hpp"
#include "sha256.hpp"

namespace fri {

// ============================================================== NTT ======
// Natural order in -> natural order out, DIT after a bit-reversal gather.
// Passes of NS <= 8 stages over 4096-element tiles (256 threads x 16
// elements in registers): the first min(4, NS) stages run in registers on 16
// consecutive tile elements, one LDS exchange, the remaining <= 4 stages run
// in registers on stride-2^A groups, one LDS exchange back for coalesced
// stores.  Pass 1 gathers input[bitrev(i)] (zero beyond d) scaled by pre(j)
// = s^j (coset shift of the LDE); the last pass applies post(i) (n^-1 and
// offset^-i for interpolation).  Later passes see the transform as columns
// of 2^NS points at stride 2^s0; a workgroup takes 4096/2^NS consecutive
// columns, so its loads/stores are contiguous runs across columns.
// Twiddles: stage-packed table tw[2^s + j] = w_{2^(s+1)}^j (Montgomery).

__device__ __forceinline__ uint32_t pow2lvl(const uint32_t* lo, const uint32_t* hi, size_t j, uint32_t v) {
    return mmul(mmul(v, hi[j >> POW_LO_LOG]), lo[j & ((1u << POW_LO_LOG) - 1)]);
}
// LDS word of tile element x.  One pad word per 16 keeps a thread's 16
// consecutive elements (phase A) and the stride-16 groups (phase B) on 64
// distinct banks; two more per 1024 spread the 32 columns of the load and
// store phases (column stride 256 + 16 = 16 mod 64 banks alone: 8-way
// conflicts, SQ_LDS_BANK_CONFLICT) over distinct banks.
#ifndef NTT_PAD10
#define NTT_PAD10 1
#endif
__device__ __forceinline__ uint32_t ntt_laddr(uint32_t x) { return x + (x >> 4) + (NTT_PAD10 ? (x >> 10) << 1 : 0u); }

#ifndef NTT_VEC
#define NTT_VEC 1            // 16-byte load/store phases where the tile allows (launch_pass)
#endif
#ifndef NTT_TWS
#define NTT_TWS 1            // small twiddle table staged in LDS (phase B reads it per lane)
#endif
#ifndef NTT_TPB
#define NTT_TPB 512          // threads per NTT tile (16 elements each; 512: 128-byte row runs)
#endif
#ifndef NTT_WIDE
#define NTT_WIDE 1           // first pass of 9..12 stages instead of a 1..4-stage pass (k_ntt_first_wide)
#endif

// Z (FIRST only): the input has d <= n / 2^Z coefficients, so after the
// bit-reversal gather every row q with q mod 2^Z != 0 is zero and DIT stages
// 0..Z-1 only copy a row into its zero partners (u + w*0 = u - w*0 = u):
// they become register copies (an LDE of blowup 8 skips 3 of its log_n stages).
// VEC: full tiles of 32 contiguous columns (NS = 8, n >= TILE, 16-byte
// aligned buffers, s0 >= 2): the load and store phases move 4 consecutive
// words per lane as one 16-byte access, all four of a lane's accesses issued
// before the first LDS write (or HBM store), instead of 16 4-byte accesses
// issued four at a time.
template <int A, int B, bool FIRST, int TPB, int Z = 0, bool VEC = false>
__global__ __launch_bounds__(TPB) void k_ntt_pass(const uint32_t* src, size_t d, uint32_t* dst,
                                                  uint32_t log_n, uint32_t s0, const uint32_t* __restrict__ tw,
                                                  const uint32_t* __restrict__ pre_lo, const uint32_t* __restrict__ pre_hi,
                                                  const uint32_t* __restrict__ post_lo,
                                                  const uint32_t* __restrict__ post_hi, size_t sstride,
                                                  size_t dstride) {
    // batch (NttPlan::batch): transform blockIdx.y of a launch; a single transform has gridDim.y == 1
    src += (size_t)blockIdx.y * sstride;
    dst += (size_t)blockIdx.y * dstride;
    // tile: 16 elements per thread; C columns (C consecutive words per row)
    constexpr uint32_t NS = A + B, P = 1u << NS, TILE = 16u * TPB, C = TILE / P;
    __shared__ uint32_t lds[TILE + TILE / 16 + 2 * (TILE >> 10)];
    __shared__ uint32_t tws[NTT_TWS ? P : 1];   // the pass's small twiddle table tw[0 .. 2^NS), read per lane in phase B
    const uint32_t tid = threadIdx.x;
    if (NTT_TWS && tid < P) tws[tid] = tw[tid];
    const size_t ncols = ((size_t)1 << log_n) >> NS;
    const size_t col0 = (size_t)blockIdx.x * C;
    const size_t lomask = ((size_t)1 << s0) - 1;
    // FIRST (bit-reversed input): tile column c is output column
    // bitrev(col0 + c) over the log_n - NS column bits, so its row q reads
    // input bitrev_NS(q) * 2^(log_n-NS) + col0 + c: contiguous across c.
    const uint32_t cbits = log_n - NS;
    auto gidx = [&](uint32_t c, uint32_t q) -> size_t {
        const size_t col = col0 + c;
        if (FIRST) return (size_t)(cbits ? (__brev((uint32_t)col) >> (32 - cbits)) : 0u) * P + q;
        return ((col >> s0) << (s0 + NS)) + ((size_t)q << s0) + (col & lomask);
    };
    // ---- load (contiguous runs across the tile's columns) -----------------
    if (VEC) {
        static_assert(!VEC || C % 4 == 0, "vector phases need whole 4-column groups");
        constexpr uint32_t VPR = C / 4;          // 16-byte vectors per tile row
        uint4 v4[4];
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint32_t y = r * TPB + tid;
            const uint32_t c = (y % VPR) * 4, q = y / VPR;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (FIRST) {
                const size_t si = ((size_t)(__brev(q) >> (32 - NS)) << cbits) + col0 + c;
                if (si + 3 < d) {
                    v = *reinterpret_cast<const uint4*>(src + si);
                } else if (si < d) {   // the vector straddling d: zeros beyond it
                    v.x = src[si];
                    if (si + 1 < d) v.y = src[si + 1];
                    if (si + 2 < d) v.z = src[si + 2];
                }
                if (pre_lo && si < d) {
                    v.x = pow2lvl(pre_lo, pre_hi, si, v.x);
                    v.y = pow2lvl(pre_lo, pre_hi, si + 1, v.y);
                    v.z = pow2lvl(pre_lo, pre_hi, si + 2, v.z);
                    v.w = pow2lvl(pre_lo, pre_hi, si + 3, v.w);
                }
            } else {
                v = *reinterpret_cast<const uint4*>(src + gidx(c, q));
            }
            v4[r] = v;
        }
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint32_t y = r * TPB + tid;
            const uint32_t c = (y % VPR) * 4, q = y / VPR;
            lds[ntt_laddr(c * P + q)] = v4[r].x;
            lds[ntt_laddr((c + 1) * P + q)] = v4[r].y;
            lds[ntt_laddr((c + 2) * P + q)] = v4[r].z;
            lds[ntt_laddr((c + 3) * P + q)] = v4[r].w;
        }
    } else
#pragma unroll 4
    for (uint32_t r = 0; r < 16; r++) {
        const uint32_t y = r * TPB + tid;
        const uint32_t c = y % C, q = y / C;
        uint32_t v = 0;
        if (col0 + c < ncols) {
            if (FIRST) {
                const size_t si = ((size_t)(__brev(q) >> (32 - NS)) << cbits) + col0 + c;
                if (si < d) {
                    v = src[si];
                    if (pre_lo) v = pow2lvl(pre_lo, pre_hi, si, v);
                }
            } else {
                v = src[gidx(c, q)];
            }
        }
        lds[ntt_laddr(c * P + q)] = v;
    }
    __syncthreads();
    uint32_t r[16];
    // Twiddles.  Stage s = s0 + t of element (column lo, row q) uses
    // w_{2^(s+1)}^((q mod 2^t) * 2^s0 + lo) = w_{2^(t+1)}^(q mod 2^t) * w_{2^(s+1)}^lo:
    // a small-table entry (< 2^NS, cached) times a per-column factor.  All 16
    // elements of a thread share one column in both phases, so the factors
    // cost one table load per pass (top stage) and squarings below it
    // (w_{2^s}^lo = (w_{2^(s+1)}^lo)^2) instead of a load of the 2^s-entry
    // stage table per butterfly.
    uint32_t wl[NS];
    if (!FIRST) {
        const size_t lo = (col0 + ((tid * 16) >> NS)) & lomask;
        wl[NS - 1] = tw[((size_t)1 << (s0 + NS - 1)) + lo];
#pragma unroll
        for (int t = (int)NS - 2; t >= 0; t--) wl[t] = mmul(wl[t + 1], wl[t + 1]);
    }
    auto twid = [&](int t, uint32_t q0) -> uint32_t {
        const uint32_t j = q0 & ((1u << t) - 1);
        const uint32_t w = NTT_TWS ? tws[(1u << t) + j] : tw[(1u << t) + j];
        return FIRST ? w : mmul(w, wl[t]);
    };
    // ---- phase A: stages 0..A-1 on 16 consecutive elements ----------------
    static_assert(Z == 0 || (FIRST && Z <= A), "trivial stages only in the first pass, inside phase A");
#pragma unroll
    for (int e = 0; e < 16; e++) r[e] = (e & ((1 << Z) - 1)) ? 0u : lds[ntt_laddr(tid * 16 + e)];
#pragma unroll
    for (int e = 0; e < 16; e++) r[e] = r[e & ~((1 << Z) - 1)];       // stages 0..Z-1
    {
        const uint32_t x0 = tid * 16;
#pragma unroll
        for (int t = Z; t < A; t++) {
#pragma unroll
            for (int e = 0; e < 16; e++) {
                if (e & (1 << t)) continue;
                const uint32_t q0 = (x0 + e) & (P - 1);
                // row q0 = x0 + e with x0 a multiple of 16, so the small-table
                // twiddle w_{2^(t+1)}^(e mod 2^t) is 1 at e mod 2^t == 0: no
                // multiply in the first pass, the column factor alone in later ones
                const bool j0 = (e & ((1 << t) - 1)) == 0;
                const uint32_t u = r[e];
                const uint32_t v = (FIRST && j0) ? r[e + (1 << t)]
                                                 : mmul(r[e + (1 << t)], (!FIRST && j0) ? wl[t < NS ? t : 0] : twid(t, q0));
                r[e] = add(u, v);
                r[e + (1 << t)] = sub(u, v);
            }
        }
    }
    if (B > 0) {
#pragma unroll
        for (int e = 0; e < 16; e++) lds[ntt_laddr(tid * 16 + e)] = r[e];
        __syncthreads();
        // ---- phase B: stages A..NS-1 on groups of 2^B at stride 2^A ---------
        constexpr uint32_t GPT = 16u >> B;        // groups per thread
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const uint32_t G = tid * GPT + (e >> B), m = e & ((1u << B) - 1);
            const uint32_t c = G >> A, ql = G & ((1u << A) - 1);
            r[e] = lds[ntt_laddr(c * P + ql + (m << A))];
        }
#pragma unroll
        for (int t = A; t < (int)NS; t++) {
            const uint32_t tb = t - A;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                if (e & (1 << tb)) continue;
                const uint32_t G = tid * GPT + (e >> B), m = e & ((1u << B) - 1);
                const uint32_t ql = G & ((1u << A) - 1);
                const uint32_t q0 = ql + (m << A);
                const uint32_t w = twid(t, q0);
                const uint32_t u = r[e], v = mmul(r[e + (1 << tb)], w);
                r[e] = add(u, v);
                r[e + (1 << tb)] = sub(u, v);
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const uint32_t G = tid * GPT + (e >> B), m = e & ((1u << B) - 1);
            const uint32_t c = G >> A, ql = G & ((1u << A) - 1);
            lds[ntt_laddr(c * P + ql + (m << A))] = r[e];
        }
    } else {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; e++) lds[ntt_laddr(tid * 16 + e)] = r[e];
    }
    __syncthreads();
    // ---- store (contiguous runs) ------------------------------------------
    if (VEC) {
#pragma unroll
        for (uint32_t rr = 0; rr < 4; rr++) {
            const uint32_t y = rr * TPB + tid;
            uint32_t c, q, w[4];     // first element of the vector: 4 rows (FIRST) or 4 columns
            if (FIRST) { c = y / (P / 4); q = (y % (P / 4)) * 4; } else { c = (y % (C / 4)) * 4; q = y / (C / 4); }
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) w[j] = lds[ntt_laddr(FIRST ? c * P + q + j : (c + j) * P + q)];
            const size_t g = gidx(c, q);
            if (post_lo) {
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) w[j] = pow2lvl(post_lo, post_hi, g + j, w[j]);
            }
            *reinterpret_cast<uint4*>(dst + g) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        return;
    }
#pragma unroll 4
    for (uint32_t rr = 0; rr < 16; rr++) {
        const uint32_t y = rr * TPB + tid;
        uint32_t c, q;
        if (FIRST) { c = y / P; q = y % P; } else { c = y % C; q = y / C; }
        if (col0 + c >= ncols) continue;
        const size_t g = gidx(c, q);
        uint32_t v = lds[ntt_laddr(c * P + q)];
        if (post_lo) v = pow2lvl(post_lo, post_hi, g, v);
        dst[g] = v;
    }
}

// First pass with NS = 9..12 stages (k_ntt_first_wide).  A transform of
// 2^log_n with log_n mod 8 in 1..4 would otherwise start with a 1..4-stage
// pass that reads and writes the whole codeword for a few stages (2^25: 1 of
// 4 passes, 2^28: 4): this pass takes those stages together with the next 8.
// Same tile as k_ntt_pass (512 threads x 16 elements), now P = 2^NS rows x
// C = 8192 / P columns, in three register phases of 4, 4 and NS - 8 stages
// with two LDS exchanges between them.  The loads are the bit-reversed input
// rows (C consecutive words each, only the rows that are nonzero for d <=
// n / 2^Z), the stores whole contiguous columns of P words (16-byte vectors).
template <int NS, int TPB, int Z>
__global__ __launch_bounds__(TPB) void k_ntt_first_wide(const uint32_t* src, size_t d, uint32_t* dst, uint32_t log_n,
                                                        const uint32_t* __restrict__ tw,
                                                        const uint32_t* __restrict__ pre_lo,
                                                        const uint32_t* __restrict__ pre_hi,
                                                        const uint32_t* __restrict__ post_lo,
                                                        const uint32_t* __restrict__ post_hi, size_t sstride,
                                                        size_t dstride) {
    static_assert(NS >= 9 && NS <= 12 && Z <= 3, "wide first pass: 9..12 stages");
    src += (size_t)blockIdx.y * sstride;           // batch (NttPlan::batch): transform blockIdx.y
    dst += (size_t)blockIdx.y * dstride;
    constexpr uint32_t P = 1u << NS, TILE = 16u * TPB, C = TILE / P;
    constexpr uint32_t VW = C < 4 ? C : 4;         // words per input vector (C consecutive words per row)
    constexpr uint32_t VPR = C / VW;               // input vectors per row
    constexpr uint32_t B2 = NS - 8;                // stages of phase 2
    __shared__ uint32_t lds[TILE + TILE / 16 + 2 * (TILE >> 10)];
    __shared__ uint32_t tws[P];                    // tw[0 .. 2^NS): w_{2^(t+1)}^j at 2^t + j
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < P; i += TPB) tws[i] = tw[i];
    // Neighbouring tiles read neighbouring C-word pieces of the same input
    // lines (8..64 bytes of each 128-byte line).  Blocks are dealt round-robin
    // over the 8 XCDs (MI355X_MICROARCH.md "Workgroup dispatch"), each with its
    // own L2: consecutive tiles go to blocks b, b + 8, b + 16, ... so that the
    // tiles sharing a line run on one XCD, close in time, and the line is
    // fetched from HBM once instead of once per XCD.
    const uint32_t nb = gridDim.x;
    const uint32_t tile = (nb & 7u) ? blockIdx.x : (blockIdx.x & 7u) * (nb >> 3) + (blockIdx.x >> 3);
    const size_t col0 = (size_t)tile * C;
    const uint32_t cbits = log_n - NS;
    // ---- load: rows q = q' 2^Z (the others are zero), VW words per lane ----
    constexpr uint32_t NV = (P >> Z) * VPR;
    for (uint32_t v = tid; v < NV; v += TPB) {
        const uint32_t c = (v % VPR) * VW, q = (v / VPR) << Z;
        const size_t si = ((size_t)(__brev(q) >> (32 - NS)) << cbits) + col0 + c;
        uint32_t w[VW];
#pragma unroll
        for (uint32_t i = 0; i < VW; i++) w[i] = 0u;
        if (si + VW <= d) {
            if (VW == 4) {
                const uint4 x = *reinterpret_cast<const uint4*>(src + si);
                w[0] = x.x; w[1 % VW] = x.y; w[2 % VW] = x.z; w[3 % VW] = x.w;
            } else if (VW == 2) {
                const uint2 x = *reinterpret_cast<const uint2*>(src + si);
                w[0] = x.x; w[1 % VW] = x.y;
            } else {
                w[0] = src[si];
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < VW; i++) w[i] = si + i < d ? src[si + i] : 0u;
        }
        if (pre_lo) {
#pragma unroll
            for (uint32_t i = 0; i < VW; i++)
                if (si + i < d) w[i] = pow2lvl(pre_lo, pre_hi, si + i, w[i]);
        }
#pragma unroll
        for (uint32_t i = 0; i < VW; i++) lds[ntt_laddr((c + i) * P + q)] = w[i];
    }
    __syncthreads();
    uint32_t r[16];
    auto twid = [&](int t, uint32_t q0) -> uint32_t { return tws[(1u << t) + (q0 & ((1u << t) - 1))]; };
    // ---- phase 0: stages 0..3 on 16 consecutive rows (0..Z-1 are copies) ----
#pragma unroll
    for (int e = 0; e < 16; e++) r[e] = (e & ((1 << Z) - 1)) ? 0u : lds[ntt_laddr(tid * 16 + e)];
#pragma unroll
    for (int e = 0; e < 16; e++) r[e] = r[e & ~((1 << Z) - 1)];
    {
        const uint32_t x0 = tid * 16;
#pragma unroll
        for (int t = Z; t < 4; t++) {
#pragma unroll
            for (int e = 0; e < 16; e++) {
                if (e & (1 << t)) continue;
                const uint32_t u = r[e];
                // x0 is a multiple of 16: the twiddle of e mod 2^t == 0 is 1
                const uint32_t v = (e & ((1 << t) - 1)) == 0 ? r[e + (1 << t)]
                                                              : mmul(r[e + (1 << t)], twid(t, (x0 + e) & (P - 1)));
                r[e] = add(u, v);
                r[e + (1 << t)] = sub(u, v);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 16; e++) lds[ntt_laddr(tid * 16 + e)] = r[e];
    __syncthreads();
    // ---- phase 1: stages 4..7, one group of 16 rows at stride 16 per thread --
    {
        const uint32_t ql = tid & 15, qh = (tid >> 4) & ((1u << (NS - 8)) - 1), c = tid >> (NS - 4);
        const uint32_t base = c * P + ql + qh * 256;
#pragma unroll
        for (int m = 0; m < 16; m++) r[m] = lds[ntt_laddr(base + m * 16)];
#pragma unroll
        for (int t = 4; t < 8; t++) {
            const int tb = t - 4;
#pragma unroll
            for (int m = 0; m < 16; m++) {
                if (m & (1 << tb)) continue;
                const uint32_t u = r[m], v = mmul(r[m + (1 << tb)], twid(t, ql + ((uint32_t)m << 4)));
                r[m] = add(u, v);
                r[m + (1 << tb)] = sub(u, v);
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; m++) lds[ntt_laddr(base + m * 16)] = r[m];
    }
    __syncthreads();
    // ---- phase 2: stages 8..NS-1, groups of 2^B2 rows at stride 256; group
    // g * TPB + tid, so the lanes of a wave read consecutive rows ----------
    {
        constexpr uint32_t GPT = 16u >> B2;
#pragma unroll
        for (uint32_t g = 0; g < GPT; g++) {
            const uint32_t G = g * TPB + tid, c = G >> 8, ql = G & 255;
#pragma unroll
            for (uint32_t m = 0; m < (1u << B2); m++) r[g * (1u << B2) + m] = lds[ntt_laddr(c * P + ql + m * 256)];
        }
#pragma unroll
        for (int t = 8; t < NS; t++) {
            const int tb = t - 8;
#pragma unroll
            for (uint32_t g = 0; g < GPT; g++) {
                const uint32_t ql = (g * TPB + tid) & 255;
#pragma unroll
                for (int m = 0; m < (1 << B2); m++) {
                    if (m & (1 << tb)) continue;
                    const int e = (int)g * (1 << B2) + m;
                    const uint32_t u = r[e], v = mmul(r[e + (1 << tb)], twid(t, ql + ((uint32_t)m << 8)));
                    r[e] = add(u, v);
                    r[e + (1 << tb)] = sub(u, v);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t g = 0; g < GPT; g++) {
            const uint32_t G = g * TPB + tid, c = G >> 8, ql = G & 255;
#pragma unroll
            for (uint32_t m = 0; m < (1u << B2); m++) lds[ntt_laddr(c * P + ql + m * 256)] = r[g * (1u << B2) + m];
        }
    }
    __syncthreads();
    // ---- store: tile column c is output column bitrev(col0 + c), P contiguous words
#pragma unroll
    for (uint32_t rr = 0; rr < 4; rr++) {
        const uint32_t y = rr * TPB + tid;
        const uint32_t c = y / (P / 4), q = (y % (P / 4)) * 4;
        uint32_t w[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) w[j] = lds[ntt_laddr(c * P + q + j)];
        const size_t col = col0 + c;
        const size_t g = (size_t)(cbits ? (__brev((uint32_t)col) >> (32 - cbits)) : 0u) * P + q;
        if (post_lo) {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) w[j] = pow2lvl(post_lo, post_hi, g + j, w[j]);
        }
        *reinterpret_cast<uint4*>(dst + g) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

static unsigned ntt_batch(const NttPlan& p) { return p.batch ? p.batch : 1u; }

template <int NS>
static void launch_first_wide(const uint32_t* src, size_t d, uint32_t* dst, uint32_t log_n, const NttPlan& p,
                              bool last, uint32_t z, hipStream_t s) {
    constexpr int TPB = 512;
    const unsigned blocks = (unsigned)(((size_t)1 << log_n) / (16 * TPB));
    const uint32_t* qlo = last ? p.post_lo : nullptr;
    const uint32_t* qhi = last ? p.post_hi : nullptr;
    switch (z) {
#define WIDE_CASE(ZV)                                                                                        \
    case ZV:                                                                                                 \
        hipLaunchKernelGGL((k_ntt_first_wide<NS, TPB, ZV>), dim3(blocks, ntt_batch(p)), dim3(TPB), 0, s, src, d, \
                           dst, log_n, p.tw, p.pre_lo, p.pre_hi, qlo, qhi, p.src_stride, p.dst_stride);     \
        break;
        WIDE_CASE(0) WIDE_CASE(1) WIDE_CASE(2) default: WIDE_CASE(3)
#undef WIDE_CASE
    }
}

__global__ void k_ntt_one(const uint32_t* src, size_t d, uint32_t* dst, const uint32_t* pre_lo,
                          const uint32_t* pre_hi, const uint32_t* post_lo, const uint32_t* post_hi) {
    if (threadIdx.x) return;
    uint32_t v = d ? src[0] : 0u;
    if (d && pre_lo) v = pow2lvl(pre_lo, pre_hi, 0, v);
    if (post_lo) v = pow2lvl(post_lo, post_hi, 0, v);
    dst[0] = v;
}

template <bool FIRST, int Z = 0>
static void launch_pass(uint32_t ns, const uint32_t* src, size_t d, uint32_t* dst, uint32_t log_n, uint32_t s0,
                        const NttPlan& p, bool last, hipStream_t s) {
    const size_t n = (size_t)1 << log_n;
    constexpr int TPB = NTT_TPB;
    const unsigned blocks = (unsigned)((n + 16 * TPB - 1) / (16 * TPB));
    const uint32_t* plo = FIRST ? p.pre_lo : nullptr;
    const uint32_t* phi = FIRST ? p.pre_hi : nullptr;
    const uint32_t* qlo = last ? p.post_lo : nullptr;
    const uint32_t* qhi = last ? p.post_hi : nullptr;
    const size_t sst = FIRST ? p.src_stride : p.dst_stride;   // later passes run in place on dst
#define NTT_CASE(NSV, AV, BV)                                                                                   \
    case NSV:                                                                                                   \
        hipLaunchKernelGGL((k_ntt_pass<AV, BV, FIRST, TPB, (Z < AV ? Z : AV)>), dim3(blocks, ntt_batch(p)), dim3(TPB), \
                           0, s, src, d, dst, log_n, s0, p.tw, plo, phi, qlo, qhi, sst, p.dst_stride);          \
        break;
    // vector load/store phases: whole tiles of 32 contiguous columns, 16-byte aligned buffers
    const bool vec = NTT_VEC && ns == 8 && n >= 16u * TPB && (FIRST || s0 >= 2) &&
                     ((((uintptr_t)src) | ((uintptr_t)dst)) & 15u) == 0;
    if (vec) {
        hipLaunchKernelGGL((k_ntt_pass<4, 4, FIRST, TPB, (Z < 4 ? Z : 4), true>), dim3(blocks, ntt_batch(p)), dim3(TPB),
                           0, s, src, d, dst, log_n, s0, p.tw, plo, phi, qlo, qhi, sst, p.dst_stride);
        return;
    }
    switch (ns) {
        NTT_CASE(1, 1, 0) NTT_CASE(2, 2, 0) NTT_CASE(3, 3, 0) NTT_CASE(4, 4, 0)
        NTT_CASE(5, 4, 1) NTT_CASE(6, 4, 2) NTT_CASE(7, 4, 3) NTT_CASE(8, 4, 4)
        default: break;
    }
#undef NTT_CASE
}

// First pass with the zero rows of a padded input skipped: z trivial stages
// when d <= n / 2^z (z <= 3, and at most the pass's phase-A stages).
static void launch_first(uint32_t ns, const uint32_t* src, size_t d, uint32_t* dst, uint32_t log_n, const NttPlan& p,
                         bool last, hipStream_t s) {
    uint32_t z = 0;
    while (z < 3 && z < ns && ((size_t)d << (z + 1)) <= ((size_t)1 << log_n)) z++;
    switch (z) {
        case 0: launch_pass<true, 0>(ns, src, d, dst, log_n, 0, p, last, s); break;
        case 1: launch_pass<true, 1>(ns, src, d, dst, log_n, 0, p, last, s); break;
        case 2: launch_pass<true, 2>(ns, src, d, dst, log_n, 0, p, last, s); break;
        default: launch_pass<true, 3>(ns, src, d, dst, log_n, 0, p, last, s); break;
    }
}

void launch_ntt(const NttPlan& p, const uint32_t* src, size_t d, uint32_t* dst, hipStream_t s) {
    const uint32_t log_n = p.log_n;
    if (log_n == 0) {   // one point: dst[0] = post(0) * pre(0) * src[0]
        hipLaunchKernelGGL(k_ntt_one, dim3(1), dim3(64), 0, s, src, d, dst, p.pre_lo, p.pre_hi, p.post_lo, p.post_hi);
        return;
    }
    uint32_t first = log_n % 8;
    if (first == 0) first = 8;
#if NTT_WIDE
    // a short first pass (1..4 stages) merged with the next 8: one pass fewer
    if (first <= 4 && log_n >= 13 && log_n - first >= 8 &&
        ((((uintptr_t)src) | ((uintptr_t)dst)) & 15u) == 0) {
        first += 8;
        uint32_t z = 0;
        while (z < 3 && ((size_t)d << (z + 1)) <= ((size_t)1 << log_n)) z++;
        const bool last = first == log_n;
        switch (first) {
            case 9: launch_first_wide<9>(src, d, dst, log_n, p, last, z, s); break;
            case 10: launch_first_wide<10>(src, d, dst, log_n, p, last, z, s); break;
            case 11: launch_first_wide<11>(src, d, dst, log_n, p, last, z, s); break;
            default: launch_first_wide<12>(src, d, dst, log_n, p, last, z, s); break;
        }
        for (uint32_t s0 = first; s0 < log_n; s0 += 8)
            launch_pass<false>(8, dst, 0, dst, log_n, s0, p, s0 + 8 == log_n, s);
        return;
    }
#endif
    launch_first(first, src, d, dst, log_n, p, first == log_n, s);
    for (uint32_t s0 = first; s0 < log_n; s0 += 8)
        launch_pass<false>(8, dst, 0, dst, log_n, s0, p, s0 + 8 == log_n, s);
}

// Stage-packed twiddles: tw[2^s + j] = Montgomery(w_{2^(s+1)}^j), so every
// DIT stage s reads a contiguous run (independent of the transform size).
struct StageBases { uint32_t b[32]; };
__global__ void k_twiddles(uint32_t* tw, size_t count, StageBases sb) {
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    if (e == 0) { tw[0] = R_MOD_P; return; }
    uint32_t s = 63u - (uint32_t)__clzll((unsigned long long)e);
    tw[e] = mpow(sb.b[s], e - ((size_t)1 << s));
}
void launch_twiddles(uint32_t* tw, uint32_t log_max, bool inverse, hipStream_t s) {
    StageBases sb{};
    for (uint32_t st = 0; st < log_max && st < 31; st++) {
        uint32_t w = root_of_unity(st + 1);
        sb.b[st] = to_mont(inverse ? inv_std(w) : w);
    }
    size_t count = (size_t)1 << log_max;
    hipLaunchKernelGGL(k_twiddles, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, tw, count, sb);
}

// Two-level power table of base^j scaled by `scale`: lo[t] = base^t,
// hi[t] = scale * base^(4096 t)  (Montgomery).
__global__ void k_pow_table(uint32_t* lo, uint32_t* hi, uint32_t nhi, uint32_t base_m, uint32_t scale_m) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nlo = 1u << POW_LO_LOG;
    if (t < nlo) lo[t] = mpow(base_m, t);
    else if (t < nlo + nhi) {
        uint32_t q = t - nlo;
        hi[q] = mmul(scale_m, mpow(base_m, (uint64_t)q << POW_LO_LOG));
    }
}
void launch_pow_table(uint32_t* lo, uint32_t* hi, uint32_t log_n, uint32_t base_std, uint32_t scale_std,
                      hipStream_t s) {
    uint32_t nhi = log_n > POW_LO_LOG ? (1u << (log_n - POW_LO_LOG)) : 1u;
    uint32_t tot = (1u << POW_LO_LOG) + nhi;
    hipLaunchKernelGGL(k_pow_table, dim3((tot + 255) / 256), dim3(256), 0, s, lo, hi, nhi, to_mont(base_std),
                       to_mont(scale_std));
}

// ========================================================= batch inverse ==
// Montgomery's trick per thread over BI_K strided elements (coalesced), one
// Fermat inversion per thread; zeros are skipped and map to 0 exactly like
// FieldElement::inverse (0^(p-2) = 0).
constexpr uint32_t BI_K = 16;
__global__ __launch_bounds__(256) void k_batch_inverse(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                       size_t n, size_t stride, int out_mont) {
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= stride) return;
    uint32_t a[BI_K], pre[BI_K];
    uint32_t acc = R_MOD_P;
#pragma unroll
    for (uint32_t k = 0; k < BI_K; k++) {
        size_t i = g + k * stride;
        uint32_t x = i < n ? in[i] : 0u;
        a[k] = x ? to_mont(x) : 0u;
        pre[k] = acc;
        if (x) acc = mmul(acc, a[k]);
    }
    uint32_t inv = mpow(acc, P - 2);
#pragma unroll
    for (int k = BI_K - 1; k >= 0; k--) {
        size_t i = g + (size_t)k * stride;
        uint32_t r = 0;
        if (a[k]) { r = mmul(inv, pre[k]); inv = mmul(inv, a[k]); }
        if (i < n) out[i] = out_mont ? r : from_mont(r);
    }
}
void launch_batch_inverse(const uint32_t* in, uint32_t* out, size_t n, int out_mont, hipStream_t s) {
    size_t stride = (n + BI_K - 1) / BI_K;
    if (!stride) return;
    hipLaunchKernelGGL(k_batch_inverse, dim3((unsigned)((stride + 255) / 256)), dim3(256), 0, s, in, out, n, stride,
                       out_mont);
}

// out[i] = offset * w_n^i (canonical)
__global__ void k_coset_points(uint32_t* out, size_t count, uint32_t off, uint32_t w_m) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = mmul(off, mpow(w_m, i));
}
void launch_coset_points(uint32_t* out, size_t count, uint32_t offset, uint32_t log_n, hipStream_t s) {
    hipLaunchKernelGGL(k_coset_points, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, out, count, offset,
                       to_mont(root_of_unity(log_n)));
}

__global__ void k_square_mont(const uint32_t* in, uint32_t* out, size_t count) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) { uint32_t x = in[i]; out[i] = mmul(x, x); }
}
void launch_square_mont(const uint32_t* in, uint32_t* out, size_t count, hipStream_t s) {
    if (!count) return;
    hipLaunchKernelGGL(k_square_mont, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, in, out, count);
}

// Horner at arbitrary points (ops.rs:76-83): one lane per point.
__global__ void k_evaluate(const uint32_t* __restrict__ c, size_t d, const uint32_t* __restrict__ xs, size_t count,
                           uint32_t* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t xm = to_mont(xs[i]), r = 0;
    for (size_t k = d; k-- > 0;) r = add(mmul(r, xm), c[k]);
    out[i] = r;
}
// Few points, many coefficients: lane l of the S lanes of a point takes the
// coefficients j = k S + l (coalesced across lanes) and evaluates
// H_l = sum_k c[kS + l] (x^S)^k by Horner in y = x^S; then
// p(x) = sum_l x^l H_l, summed per workgroup here and over the B workgroups
// of the point by k_evaluate_join.  Exact field arithmetic: the same value as
// Horner's rule in any order.
__global__ __launch_bounds__(256) void k_evaluate_strided(const uint32_t* __restrict__ c, size_t d,
                                                          const uint32_t* __restrict__ xs, uint32_t S,
                                                          uint32_t* __restrict__ part) {
    __shared__ uint32_t red[4];
    const uint32_t p = blockIdx.y, l = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t xm = to_mont(xs[p]);
    const uint32_t ym = mpow(xm, S);                               // x^S, Montgomery
    const size_t K = (d + S - 1) / S;
    uint32_t h = 0;
    for (size_t k = K; k-- > 0;) {
        const size_t j = k * S + l;
        h = add(mmul(h, ym), j < d ? c[j] : 0u);
    }
    uint32_t v = mmul(h, mpow(xm, l));                             // x^l H_l, canonical
    for (int o = 32; o >= 1; o >>= 1) v = add(v, (uint32_t)__shfl_xor((int)v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)p * gridDim.x + blockIdx.x] = add(add(red[0], red[1]), add(red[2], red[3]));
}
__global__ void k_evaluate_join(const uint32_t* __restrict__ part, uint32_t B, size_t count, uint32_t* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= count) return;
    uint32_t v = 0;
    for (uint32_t b = 0; b < B; b++) v = add(v, part[p * B + b]);
    out[p] = v;
}
size_t evaluate_tmp_words(size_t d, size_t count) {
    if (count >= ((size_t)1 << 16) || d < 4096) return 0;          // one lane per point is enough
    size_t S = 256;                                                // >= 2^18 lanes, >= 16 coefficients each
    while (S < 8192 && count * S < ((size_t)1 << 18) && d / (2 * S) >= 16) S *= 2;
    return count * (S / 256);
}
void launch_evaluate(const uint32_t* coeffs, size_t d, const uint32_t* xs, size_t count, uint32_t* out,
                     uint32_t* tmp, hipStream_t s) {
    if (!count) return;
    const size_t tw = evaluate_tmp_words(d, count);
    if (!tw) {
        hipLaunchKernelGGL(k_evaluate, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, coeffs, d, xs, count,
                           out);
        return;
    }
    const uint32_t B = (uint32_t)(tw / count), S = 256 * B;
    hipLaunchKernelGGL(k_evaluate_strided, dim3(B, (unsigned)count), dim3(256), 0, s, coeffs, d, xs, S, tmp);
    hipLaunchKernelGGL(k_evaluate_join, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, tmp, B, count, out);
}

// ============================================ arbitrary-point interpolate ==
// Polynomial::interpolate on points that are not a coset (interpolation.rs:
// 121-152): f = sum_j y_j w_j Z(x)/(x - x_j), w_j = 1/prod_{i!=j}(x_j - x_i).
// Products run in the "R^-1 per step" form: mmul(acc, t) = acc*t*R^-1 with
// both operands canonical, so a chain of m products carries R^-m, fixed by one
// product with R^(m+1) at the end.  x and c tiles are staged in LDS.  One
// lane per output point leaves a wave per SIMD at n = 2^16, so the point range
// is cut into S segments (blockIdx.y) whose partial results are combined by a
// second kernel.
constexpr uint32_t INTERP_TILE = 1024;

// segment s of prod_{i!=j}(x_j - x_i): part[s*n + j], exponent (segment
// length - [j in segment]) of R^-1
__global__ __launch_bounds__(256) void k_interp_weights(const uint32_t* __restrict__ xs, size_t n, size_t seg,
                                                        uint32_t* __restrict__ part) {
    __shared__ uint32_t xt[INTERP_TILE];
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t lo = (size_t)blockIdx.y * seg, hi = lo + seg < n ? lo + seg : n;
    const uint32_t xj = j < n ? xs[j] : 0u;
    uint32_t a = 1u;
    for (size_t base = lo; base < hi; base += INTERP_TILE) {
        const uint32_t m = (uint32_t)(hi - base < INTERP_TILE ? hi - base : INTERP_TILE);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) xt[i] = xs[base + i];
        __syncthreads();
        const uint32_t self = (j >= base && j < base + m) ? (uint32_t)(j - base) : INTERP_TILE;
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t t = i == self ? R_MOD_P : sub(xj, xt[i]);   // skip i == j: a Montgomery 1
            a = mmul(a, t);
        }
    }
    if (j < n) part[blockIdx.y * n + j] = a;
}
// prod over the S segments (S - 1 more R^-1), times the fix-up: the exact
// prod_{i!=j}(x_j - x_i), canonical
__global__ void k_interp_weights_join(const uint32_t* __restrict__ part, size_t n, uint32_t S, uint32_t fix,
                                      uint32_t* __restrict__ acc) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    uint32_t a = part[j];
    for (uint32_t s = 1; s < S; s++) a = mmul(a, part[s * n + j]);
    acc[j] = mmul(a, fix);
}
static uint32_t interp_segments(size_t n, size_t lanes) {
    uint32_t S = 1;                          // >= 2^20 lanes in flight, segments of >= 256 points
    while (S < 64 && lanes * S < ((size_t)1 << 20) && n / (2 * S) >= 256) S *= 2;
    return S;
}
size_t interp_tmp_words(size_t n, uint32_t log_N) {
    const size_t N = (size_t)1 << log_N;
    const size_t a = interp_segments(n, n) * n, b = 2 * (size_t)interp_segments(n, N) * N;
    return a > b ? a : b;
}
void launch_interp_weights(const uint32_t* xs, size_t n, uint32_t* acc, uint32_t* tmp, hipStream_t s) {
    const uint32_t S = interp_segments(n, n);
    const size_t seg = (n + S - 1) / S;
    // n - 1 factors carry R^-1 (the skipped i == j does not), plus S - 1 joins
    const uint32_t fix = pow_std(R_MOD_P, (uint64_t)n + S - 1);
    hipLaunchKernelGGL(k_interp_weights, dim3((unsigned)((n + 255) / 256), S), dim3(256), 0, s, xs, n, seg, tmp);
    hipLaunchKernelGGL(k_interp_weights_join, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tmp, n, S, fix,
                       acc);
}

__global__ void k_interp_coeffs(const uint32_t* __restrict__ ys, uint32_t* __restrict__ w, size_t n) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) w[j] = mmul(ys[j], w[j]);        // w Montgomery -> c_j = y_j w_j canonical
}
void launch_interp_coeffs(const uint32_t* ys, uint32_t* w_to_c, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_interp_coeffs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ys, w_to_c, n);
}

// f(u), u = w_N^k: num/den = sum_j c_j/(u - x_j) as one running fraction over
// the segment's points, num <- num (u - x_j) + c_j den, den <- den (u - x_j).
// Over all n points den = Z(u) and num = Z(u) * sum_j c_j/(u - x_j) = f(u): a
// polynomial identity in u, so it holds at u = x_j too (no inverse, no
// special case).  Segments are fractions over disjoint point sets and join as
// num = num_a den_b + num_b den_a, den = den_a den_b.
__global__ __launch_bounds__(256) void k_interp_eval(const uint32_t* __restrict__ xs, const uint32_t* __restrict__ c,
                                                     size_t n, size_t seg, uint32_t w_m, size_t N,
                                                     uint32_t* __restrict__ part) {
    __shared__ uint2 tile[INTERP_TILE];
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t lo = (size_t)blockIdx.y * seg, hi = lo + seg < n ? lo + seg : n;
    const uint32_t u = from_mont(mpow(w_m, k));
    uint32_t num = 0u, den = 1u;
    for (size_t base = lo; base < hi; base += INTERP_TILE) {
        const uint32_t m = (uint32_t)(hi - base < INTERP_TILE ? hi - base : INTERP_TILE);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) tile[i] = make_uint2(xs[base + i], c[base + i]);
        __syncthreads();
#pragma unroll 4
        for (uint32_t i = 0; i < m; i++) {
            const uint2 xc = tile[i];
            const uint32_t t = sub(u, xc.x);
            num = add(mmul(num, t), mmul(xc.y, den));
            den = mmul(den, t);
        }
    }
    if (k < N) {
        part[(2 * (size_t)blockIdx.y) * N + k] = num;
        part[(2 * (size_t)blockIdx.y + 1) * N + k] = den;
    }
}
__global__ void k_interp_eval_join(const uint32_t* __restrict__ part, size_t N, uint32_t S, uint32_t fix,
                                   uint32_t* __restrict__ f) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    uint32_t num = part[k], den = part[N + k];
    for (uint32_t s = 1; s < S; s++) {
        const uint32_t nb = part[2 * s * N + k], db = part[(2 * s + 1) * N + k];
        num = add(mmul(num, db), mmul(nb, den));
        den = mmul(den, db);
    }
    f[k] = mmul(num, fix);
}
void launch_interp_eval(const uint32_t* xs, const uint32_t* c, size_t n, uint32_t log_N, uint32_t* f, uint32_t* tmp,
                        hipStream_t s) {
    const size_t N = (size_t)1 << log_N;
    const uint32_t S = interp_segments(n, N);
    const size_t seg = (n + S - 1) / S;
    // n steps and S - 1 joins of R^-1: mmul(num, R^(n+S)) = num R^(n+S-1)
    const uint32_t fix = pow_std(R_MOD_P, (uint64_t)n + S);
    hipLaunchKernelGGL(k_interp_eval, dim3((unsigned)((N + 255) / 256), S), dim3(256), 0, s, xs, c, n, seg,
                       to_mont(root_of_unity(log_N)), N, tmp);
    hipLaunchKernelGGL(k_interp_eval_join, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, tmp, N, S, fix, f);
}

// ================================================================== fold ==
// One layer by fold_one (field.hpp); xinv_m[i] = Montgomery(x_i^-1) for the layer's domain.
__global__ __launch_bounds__(256) void k_fold(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                              size_t half, const uint32_t* __restrict__ xinv_m, uint32_t beta_m,
                                              const DevState* __restrict__ st, int r) {
    if (st && !st->active[r]) return;
    if (st) beta_m = st->beta_mont[r];
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < half) out[i] = fold_one(in[i], in[i + half], xinv_m[i], beta_m);
}
void launch_fold_plain(const uint32_t* in, uint32_t* out, uint32_t log_m, const uint32_t* xinv_m, uint32_t beta,
                       hipStream_t s) {
    size_t half = ((size_t)1 << log_m) / 2;
    hipLaunchKernelGGL(k_fold, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, s, in, out, half, xinv_m,
                       to_mont(beta), (const DevState*)nullptr, 0);
}

// Decommitment gather for one query (fri_commit.rs:137-163): block k reads
// layer k's value at idx = index % m_k and at its sibling (idx + m_k/2) % m_k,
// and the two authentication paths (sibling digest per level, leaf -> root),
// as raw big-endian bytes.  One launch + one copy per query.
__global__ void k_decommit_gather(const uint32_t* __restrict__ layers, const uint32_t* __restrict__ trees,
                                  const uint32_t* __restrict__ top, DecommitPlan dp, uint32_t* __restrict__ out) {
    const uint32_t k = blockIdx.x;
    const uint32_t L = dp.log_n - k;
    const uint64_t m = (uint64_t)1 << L;
    const uint64_t idx = dp.index % m;
    const uint64_t sib = (idx + m / 2) % m;
    const bool sharded = dp.shard_lb1[k] != 0;
    const uint32_t lb = sharded ? dp.shard_lb1[k] - 1u : 0u;
    const uint64_t bmask = sharded ? ((uint64_t)1 << lb) - 1 : ~(uint64_t)0;
    // a sharded layer: is the opened element in a block this rank holds?
    auto mine = [&](uint64_t i) -> bool { return !sharded || ((dp.owned[k] >> (i >> lb)) & 1u); };
    auto vidx = [&](uint64_t i) -> uint64_t { return (sharded && dp.val_block[k]) ? (i & bmask) : i; };
    if (threadIdx.x == 0) {
        out[2 * k] = mine(idx) ? layers[dp.layer_off[k] + vidx(idx)] : 0u;
        out[2 * k + 1] = mine(sib) ? layers[dp.layer_off[k] + vidx(sib)] : 0u;
    }
    const uint32_t l = threadIdx.x;
    if (l >= L) return;
    const uint32_t* tr = trees + dp.tree_off[k];
    uint32_t* paths = out + 2 * dp.n_layers + dp.path_off[k];
#pragma unroll
    for (int which = 0; which < 2; which++) {
        const uint64_t leaf = which ? sib : idx;
        uint32_t* o = paths + (size_t)which * 8 * L + 8 * l;
        if (!mine(leaf)) {
#pragma unroll
            for (int w = 0; w < 8; w++) o[w] = 0u;
            continue;
        }
        const uint32_t* d;
        if (!sharded) {
            d = tr + 8 * (level_offset(L, l) + ((leaf >> l) ^ 1u));
        } else if (l < lb) {                         // inside the block: the block-local tree
            d = tr + 8 * (level_offset(lb, l) + (((leaf & bmask) >> l) ^ 1u));
        } else {                                     // above it: the replicated top tree of block roots
            const uint32_t t = l - lb;
            d = top + dp.top_off[k] + 8 * (level_offset(dp.logG, t) + (((leaf >> lb) >> t) ^ 1u));
        }
#pragma unroll
        for (int w = 0; w < 8; w++) o[w] = __builtin_bswap32(d[w]);
    }
}
void launch_decommit_gather(const uint32_t* layers, const uint32_t* trees, const DecommitPlan& dp, uint32_t* out,
                            hipStream_t s, const uint32_t* top) {
    hipLaunchKernelGGL(k_decommit_gather, dim3(dp.n_layers), dim3(64), 0, s, layers, trees, top, dp, out);
}

// ================================================= polynomial arithmetic ==
// fri_poly_mul / fri_poly_div_rem (fri_poly.hip; ops.rs:114-191).
//
// Pointwise kernels on NTT outputs.  The transforms leave canonical values,
// so every mmul of two of them carries one R^-1: the product kernel leaves
// A*B*R^-1, the Newton kernel G*(2 - F*G)*R^-2 (2*R^-1 - F*G*R^-1 is
// (2 - F*G)*R^-1).  The caller folds R (R^2) and N^-1 into the inverse
// transform's post-scale table, so there is no conversion pass.  16-byte
// loads and stores when the three pointers are aligned; out may alias a or b
// (each element is read, then written, by the same lane).
template <bool NEWTON>
__device__ __forceinline__ uint32_t poly_pw(uint32_t a, uint32_t b, uint32_t two_rinv) {
    const uint32_t t = mmul(a, b);
    return NEWTON ? mmul(b, sub(two_rinv, t)) : t;
}
template <bool NEWTON>
__global__ __launch_bounds__(256) void k_poly_pointwise(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n,
                                                        size_t n4, uint32_t two_rinv) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint4* a4 = reinterpret_cast<const uint4*>(a);
    const uint4* b4 = reinterpret_cast<const uint4*>(b);
    uint4* o4 = reinterpret_cast<uint4*>(out);
    for (size_t i = t0; i < n4; i += stride) {
        const uint4 x = a4[i], y = b4[i];
        uint4 r;
        r.x = poly_pw<NEWTON>(x.x, y.x, two_rinv);
        r.y = poly_pw<NEWTON>(x.y, y.y, two_rinv);
        r.z = poly_pw<NEWTON>(x.z, y.z, two_rinv);
        r.w = poly_pw<NEWTON>(x.w, y.w, two_rinv);
        o4[i] = r;
    }
    for (size_t i = 4 * n4 + t0; i < n; i += stride) out[i] = poly_pw<NEWTON>(a[i], b[i], two_rinv);
}
template <bool NEWTON>
static void launch_pointwise(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, hipStream_t s) {
    if (!n) return;
    const bool vec = ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)out)) & 15u) == 0;
    const size_t n4 = vec ? n / 4 : 0;
    const size_t work = n4 ? n4 : n;
    size_t blocks = (work + 255) / 256;
    if (blocks > 8192) blocks = 8192;                              // grid-stride beyond 2^21 lanes
    const uint32_t rinv = from_mont(1u);
    hipLaunchKernelGGL((k_poly_pointwise<NEWTON>), dim3((unsigned)blocks), dim3(256), 0, s, a, b, out, n, n4,
                       add(rinv, rinv));
}
void launch_poly_pointwise_mul(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, hipStream_t s) {
    launch_pointwise<false>(a, b, out, n, s);
}
void launch_poly_newton(const uint32_t* f, const uint32_t* g, uint32_t* out, size_t n, hipStream_t s) {
    launch_pointwise<true>(f, g, out, n, s);
}

// Direct convolution with a short operand (`* (x - c)`, the products of a
// small composition): out[i] = sum_j sht[j] * lng[i - j] for i < n_out, one
// lane per output coefficient, no transform.  The short operand is staged in
// LDS in Montgomery form (so each product comes out canonical), next to the
// window of the long operand the workgroup's 256 outputs read, zero-filled
// outside [0, ll): the inner loop has no bounds test, the short operand is an
// LDS broadcast and the window is read at consecutive addresses across lanes.
// Terms are canonical (< 2^32), at most POLY_DIRECT_LIMIT = 2^12 of them, so
// a 64-bit sum stays below 2^44 and is reduced once (two REDCs).
__global__ __launch_bounds__(256) void k_poly_conv_direct(const uint32_t* __restrict__ lng, size_t ll,
                                                          const uint32_t* __restrict__ sht, uint32_t ls,
                                                          uint32_t* __restrict__ out, size_t n_out) {
    extern __shared__ uint32_t poly_sm[];
    uint32_t* sh = poly_sm;                 // ls words
    uint32_t* win = poly_sm + ls;           // 256 + ls - 1 words: lng[i0 - (ls - 1) .. i0 + 255]
    const size_t i0 = (size_t)blockIdx.x * 256;
    for (uint32_t j = threadIdx.x; j < ls; j += 256) sh[j] = to_mont(sht[j]);
    const uint32_t wn = 256 + ls - 1;
    for (uint32_t t = threadIdx.x; t < wn; t += 256) {
        const size_t pos = i0 + t;          // index + (ls - 1)
        win[t] = (pos >= ls - 1 && pos - (ls - 1) < ll) ? lng[pos - (ls - 1)] : 0u;
    }
    __syncthreads();
    const size_t i = i0 + threadIdx.x;
    if (i >= n_out) return;
    const uint32_t* w = win + threadIdx.x + (ls - 1);   // w[-j] = lng[i - j]
    uint64_t acc = 0;
#pragma unroll 4
    for (uint32_t j = 0; j < ls; j++) acc += mmul(w[-(int)j], sh[j]);
    out[i] = mmul(redc(acc), R2_MOD_P);
}
void launch_poly_conv_direct(const uint32_t* lng, size_t ll, const uint32_t* sht, size_t ls, uint32_t* out,
                             size_t n_out, hipStream_t s) {
    if (!n_out || !ls || ls > POLY_DIRECT_LIMIT) return;
    const size_t lds = (2 * ls + 255) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_poly_conv_direct, dim3((unsigned)((n_out + 255) / 256)), dim3(256), lds, s, lng, ll, sht,
                       (uint32_t)ls, out, n_out);
}

// Division helpers.  Reverse-truncate-pad: dst[i] = src[top - i] for
// i < cnt (cnt <= top + 1), 0 for cnt <= i < n.  Remainder: r = a - t on the
// low n coefficients.
__global__ __launch_bounds__(256) void k_poly_reverse(const uint32_t* __restrict__ src, size_t top, size_t cnt,
                                                      uint32_t* __restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dst[i] = i < cnt ? src[top - i] : 0u;
}
__global__ __launch_bounds__(256) void k_poly_sub(const uint32_t* __restrict__ a, const uint32_t* __restrict__ t,
                                                  uint32_t* __restrict__ r, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) r[i] = sub(a[i], t[i]);
}
static unsigned poly_blocks(size_t n) {
    const size_t b = (n + 255) / 256;
    return (unsigned)(b > 8192 ? 8192 : b);
}
void launch_poly_reverse(const uint32_t* src, size_t top, size_t cnt, uint32_t* dst, size_t n, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_poly_reverse, dim3(poly_blocks(n)), dim3(256), 0, s, src, top, cnt, dst, n);
}
void launch_poly_sub(const uint32_t* a, const uint32_t* t, uint32_t* r, size_t n, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_poly_sub, dim3(poly_blocks(n)), dim3(256), 0, s, a, t, r, n);
}

// ===================================== product tree and the Lagrange basis ==
// fri_poly_from_roots / fri_lagrange_basis (fri_roots.hip; interpolation.rs:
// 9-23, 46-115).  Z = prod (x - r_i) over 2^log_np roots (the list padded
// with zero roots) as a binary product tree.  Every node is monic with the
// leading 1 implicit: a node of degree m is its m low coefficients, in
// Montgomery form, and a level is the 2^log_np words of its nodes side by side.
//   (x^m + a)(x^m + b) = x^2m + (a + b) x^m + a b.
//
// Leaf kernel: one workgroup builds the subtree over 2^log_leaf consecutive
// roots in LDS, level by level between two buffers.  A work item owns the
// output coefficients k and m + k of one node: for i = 0..m-1 the term
// a_i * b_((k - i) mod m) belongs to coefficient k when i <= k and to m + k
// otherwise, so every item runs exactly m products; m + k also takes
// a_k + b_k.  A level keeps its even nodes (the a's of the next level) in the
// buffer's first half and the odd nodes in the second: consecutive lanes then
// read one a word (a broadcast) or, below m = 64, words of neighbouring nodes
// that lie side by side, and consecutive b words (mod m): no two lanes of a
// wave meet in a bank at different addresses.  Sums of <= 2^10 Montgomery
// products (< 2^32 each) stay below 2^42 in 64 bits and are reduced once.
// LDS: two buffers of the 2048-word limit, 16 KiB: ten workgroups per CU.
__global__ __launch_bounds__(256) void k_roots_leaf(const uint32_t* __restrict__ roots, size_t n, uint32_t log_leaf,
                                                    uint32_t canon, uint32_t* __restrict__ out) {
    __shared__ uint32_t buf[2][1u << ROOTS_LEAF_LOG_MAX];
    const uint32_t L = 1u << log_leaf, H = L >> 1, tid = threadIdx.x;
    const size_t r0 = (size_t)blockIdx.x << log_leaf;
    // level 0: node i is the constant -r_i; even nodes first
    for (uint32_t i = tid; i < L; i += blockDim.x) {
        const uint32_t r = r0 + i < n ? roots[r0 + i] : 0u;
        buf[0][log_leaf ? (i & 1u) * H + (i >> 1) : 0u] = to_mont(neg(r));
    }
    uint32_t cur = 0;
    for (uint32_t lm = 0; lm < log_leaf; lm++, cur ^= 1u) {
        const uint32_t m = 1u << lm;
        const uint32_t* a = buf[cur];          // node j of the even half, m words at j*m
        const uint32_t* b = buf[cur] + H;
        uint32_t* dst = buf[cur ^ 1u];
        __syncthreads();
        for (uint32_t t = tid; t < H; t += blockDim.x) {
            const uint32_t node = t >> lm, k = t & (m - 1);
            const uint32_t* an = a + node * m;
            const uint32_t* bn = b + node * m;
            uint64_t lo = 0, hi = 0;
            for (uint32_t i = 0; i < m; i++) {
                const uint64_t p = mmul(an[i], bn[(k - i) & (m - 1)]);
                lo += i <= k ? p : 0;
                hi += i <= k ? 0 : p;
            }
            const uint32_t clo = mmul(redc(lo), R2_MOD_P);
            const uint32_t chi = add(mmul(redc(hi), R2_MOD_P), add(an[k], bn[k]));
            // output node `node` (2m words): even nodes in the first half; the
            // last level's single node fills the whole buffer
            uint32_t* o = dst + (lm + 1 < log_leaf ? (node & 1u) * H + (node >> 1) * 2 * m : 0u);
            o[k] = clo;
            o[m + k] = chi;
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < L; i += blockDim.x) out[r0 + i] = canon ? from_mont(buf[cur][i]) : buf[cur][i];
}
void launch_roots_leaf(const uint32_t* roots, size_t n, uint32_t log_np, uint32_t log_leaf, bool canon, uint32_t* out,
                       hipStream_t s) {
    const uint32_t half = log_leaf ? 1u << (log_leaf - 1) : 1u;
    const uint32_t tpb = half < 64 ? 64 : half > 256 ? 256 : half;
    hipLaunchKernelGGL(k_roots_leaf, dim3(1u << (log_np - log_leaf)), dim3(tpb), 0, s, roots, n, log_leaf,
                       canon ? 1u : 0u, out);
}

// One level above the leaves whose products (2m = 2^lg words) fit LDS: a
// workgroup takes a tile of `tile` consecutive words of the level (tile / 2m
// pairs of nodes), and the whole tile runs as one batched transform, because
// the stages s < lg of a DIT over the tile are independent transforms of its
// aligned 2^lg blocks (the twiddles are stage-packed, size-independent).
// a and b of a pair are gathered bit-reversed into two arrays, zero-padded to
// 2m (the odd positions: stage 0 is then a copy), transformed, multiplied as
// (A + s)(B + s) - 1 with s = x^m at w_2m^k = (-1)^k (the monic factors; the
// product's x^2m wraps to the constant 1), scaled by (2m)^-1, scattered
// bit-reversed, transformed back and stored: one launch per level, no
// intermediate in HBM.  `scale` is Montgomery((2m)^-1), or the canonical
// value when the level is the top and leaves canonical coefficients.
__device__ __forceinline__ void roots_stage(uint32_t* v, uint32_t tile, uint32_t s, const uint32_t* __restrict__ tw) {
    const uint32_t h = 1u << s;
    for (uint32_t e = threadIdx.x; e < tile / 2; e += blockDim.x) {
        const uint32_t lo = e & (h - 1), i = ((e >> s) << (s + 1)) | lo;
        const uint32_t u = v[i], t = mmul(v[i + h], tw[h + lo]);
        v[i] = add(u, t);
        v[i + h] = sub(u, t);
    }
}
__global__ __launch_bounds__(256) void k_roots_level(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                     uint32_t tile, uint32_t lg, const uint32_t* __restrict__ tw_f,
                                                     const uint32_t* __restrict__ tw_i, uint32_t scale) {
    __shared__ uint32_t A[1u << ROOTS_LDS_LOG_MAX], B[1u << ROOTS_LDS_LOG_MAX];
    const uint32_t tid = threadIdx.x, m = 1u << (lg - 1), mask = 2 * m - 1;
    const size_t base = (size_t)blockIdx.x * tile;
    for (uint32_t e = tid; e < tile; e += 256) {
        const uint32_t r = e & mask, i = r & (m - 1);
        const uint32_t pos = (e & ~mask) + (__brev(i) >> (32 - lg));   // even: i < m
        const uint32_t v = in[base + e];
        uint32_t* dstv = r < m ? A : B;
        dstv[pos] = v;
        dstv[pos + 1] = v;                                          // stage 0 against the zero padding
    }
    for (uint32_t s = 1; s < lg; s++) {
        __syncthreads();
        roots_stage(A, tile, s, tw_f);
        roots_stage(B, tile, s, tw_f);
    }
    __syncthreads();
    uint32_t r[(1u << ROOTS_LDS_LOG_MAX) / 256];
#pragma unroll
    for (uint32_t k = 0; k < (1u << ROOTS_LDS_LOG_MAX) / 256; k++) {
        const uint32_t e = k * 256 + tid;
        if (e >= tile) continue;
        const uint32_t sg = (e & 1u) ? P - R_MOD_P : R_MOD_P;
        r[k] = mmul(sub(mmul(add(A[e], sg), add(B[e], sg)), R_MOD_P), scale);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < (1u << ROOTS_LDS_LOG_MAX) / 256; k++) {
        const uint32_t e = k * 256 + tid;
        if (e < tile) A[(e & ~mask) + (__brev(e & mask) >> (32 - lg))] = r[k];
    }
    for (uint32_t s = 0; s < lg; s++) {
        __syncthreads();
        roots_stage(A, tile, s, tw_i);
    }
    __syncthreads();
    for (uint32_t e = tid; e < tile; e += 256) out[base + e] = A[e];
}
void launch_roots_level_lds(const uint32_t* in, uint32_t* out, uint32_t log_np, uint32_t lg, bool canon,
                            const uint32_t* tw_fwd, const uint32_t* tw_inv, hipStream_t s) {
    const uint32_t tile = log_np < ROOTS_LDS_LOG_MAX ? 1u << log_np : 1u << ROOTS_LDS_LOG_MAX;
    const uint32_t ninv = inv_std(1u << lg);
    hipLaunchKernelGGL(k_roots_level, dim3((unsigned)(((size_t)1 << log_np) / tile)), dim3(256), 0, s, in, out, tile, lg,
                       tw_fwd, tw_inv, canon ? ninv : to_mont(ninv));
}

// Larger levels: the transforms are batched launches of the NTT passes
// (NttPlan::batch), and this is the pointwise step between them, elementwise
// over the level because k mod 2 is the word index mod 2: out = ((A + s)(B + s)
// - 1) * scale, A and B the transforms of the even and the odd nodes.
__global__ __launch_bounds__(256) void k_roots_pointwise(const uint4* __restrict__ a, const uint4* __restrict__ b,
                                                         uint4* __restrict__ out, size_t n4, uint32_t scale) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    auto pw = [&](uint32_t x, uint32_t y, uint32_t sg) {
        return mmul(sub(mmul(add(x, sg), add(y, sg)), R_MOD_P), scale);
    };
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const uint4 x = a[i], y = b[i];
        uint4 r;
        r.x = pw(x.x, y.x, R_MOD_P);
        r.y = pw(x.y, y.y, P - R_MOD_P);
        r.z = pw(x.z, y.z, R_MOD_P);
        r.w = pw(x.w, y.w, P - R_MOD_P);
        out[i] = r;
    }
}
void launch_roots_pointwise(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t words, uint32_t lg, bool canon,
                            hipStream_t s) {
    const uint32_t ninv = inv_std((uint32_t)(((size_t)1 << lg) % P));
    hipLaunchKernelGGL(k_roots_pointwise, dim3(poly_blocks(words / 4)), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(a), reinterpret_cast<const uint4*>(b),
                       reinterpret_cast<uint4*>(out), words / 4, canon ? ninv : to_mont(ninv));
}

// Lagrange rows: L_i = w_i * Z / (x - x_i), the quotient by synthetic
// division, q_i[n-1] = 1, q_i[j-1] = z_j + x_i q_i[j].  A wave takes 64 rows
// (one lane each) and a segment of LAGRANGE_SEG columns, 64 columns at a
// time: the lanes run the chain downwards and put w_i q_i[j] into an LDS tile
// (row stride 65 words: 64 banks, no conflict), then the tile goes out row by
// row, 64 consecutive words (256 bytes) per store instruction, instead of 64
// stores at stride n.  The chain of segment [c0, c1) starts from
//   q_i[c1 - 1] = T(c1),  T(c) = sum_{k >= c} z_k x_i^(k - c)  (z_n = 1),
// which the lane folds together from the segment values P_s(x_i) of a first
// kernel (P_s the slice of Z on segment s): T(s SEG) = P_s + x^len_s T(end_s).
constexpr uint32_t LAGRANGE_SEG = 256;
static uint32_t lagrange_segments(size_t n) {
    return n >= 1024 ? (uint32_t)((n + LAGRANGE_SEG - 1) / LAGRANGE_SEG) : 1u;
}
size_t lagrange_tmp_words(size_t n) { return (size_t)(lagrange_segments(n) - 1) * n; }
__global__ __launch_bounds__(256) void k_lagrange_parts(const uint32_t* __restrict__ xs, const uint32_t* __restrict__ z,
                                                        uint32_t n, uint32_t* __restrict__ part) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, sgm = blockIdx.y + 1;
    if (i >= n) return;
    const uint32_t lo = sgm * LAGRANGE_SEG, hi = lo + LAGRANGE_SEG < n ? lo + LAGRANGE_SEG : n;
    const uint32_t xm = to_mont(xs[i]);
    uint32_t h = 0;
    for (uint32_t k = hi; k-- > lo;) h = add(mmul(h, xm), z[k]);
    part[(size_t)(sgm - 1) * n + i] = h;
}
__global__ __launch_bounds__(64) void k_lagrange_rows(const uint32_t* __restrict__ xs, const uint32_t* __restrict__ z,
                                                      const uint32_t* __restrict__ w, uint32_t n,
                                                      const uint32_t* __restrict__ part, uint32_t* __restrict__ out) {
    __shared__ uint32_t tile[64 * 65];
    __shared__ uint32_t zs[64];
    const uint32_t lane = threadIdx.x, row0 = blockIdx.x * 64, i = row0 + lane;
    const uint32_t sgm = blockIdx.y, S = gridDim.y;
    const uint32_t c0 = S > 1 ? sgm * LAGRANGE_SEG : 0u;
    const uint32_t c1 = S > 1 && c0 + LAGRANGE_SEG < n ? c0 + LAGRANGE_SEG : n;
    const uint32_t xm = i < n ? to_mont(xs[i]) : 0u, wm = i < n ? w[i] : 0u;
    uint32_t q = 1u;                                                // T(n) = z_n
    if (i < n && c1 < n) {
        const uint32_t xseg = mpow(xm, LAGRANGE_SEG);
        for (uint32_t sp = S - 1; sp > sgm; sp--) {
            const uint32_t len = n - sp * LAGRANGE_SEG < LAGRANGE_SEG ? n - sp * LAGRANGE_SEG : LAGRANGE_SEG;
            q = add(part[(size_t)(sp - 1) * n + i], mmul(q, len == LAGRANGE_SEG ? xseg : mpow(xm, len)));
        }
    }
    for (int cb = (int)((c1 - 1) & ~63u); cb >= (int)c0; cb -= 64) {
        const uint32_t ce = (uint32_t)cb + 64 < c1 ? (uint32_t)cb + 64 : c1;
        zs[lane] = (uint32_t)cb + lane < ce ? z[cb + lane] : 0u;
        __syncthreads();
        for (int j = (int)ce - 1; j >= cb; j--) {
            tile[lane * 65 + (j - cb)] = mmul(q, wm);               // w_i q_i[j], canonical
            q = add(zs[j - cb], mmul(q, xm));                       // q_i[j - 1]
        }
        __syncthreads();
        if ((uint32_t)cb + lane < ce) {
            const uint32_t rows = n - row0 < 64 ? n - row0 : 64;
            for (uint32_t r = 0; r < rows; r++) out[(size_t)(row0 + r) * n + cb + lane] = tile[r * 65 + lane];
        }
        __syncthreads();
    }
}
void launch_lagrange_rows(const uint32_t* xs, const uint32_t* z, const uint32_t* w, size_t n, uint32_t* out,
                          uint32_t* tmp, hipStream_t s) {
    if (!n) return;
    const uint32_t S = lagrange_segments(n);
    if (S > 1)
        hipLaunchKernelGGL(k_lagrange_parts, dim3((unsigned)((n + 255) / 256), S - 1), dim3(256), 0, s, xs, z,
                           (uint32_t)n, tmp);
    hipLaunchKernelGGL(k_lagrange_rows, dim3((unsigned)((n + 63) / 64), S), dim3(64), 0, s, xs, z, w, (uint32_t)n, tmp,
                       out);
}

// ============================ multipoint evaluation and interpolation ==
// fri_evaluate_ex / fri_interpolate_points_ex on the retained product tree
// (fri_multipoint.hip).  Evaluation goes down the tree with
// the vector a_S of a node S (|S| = m words; the coefficients of x^-m..x^-1
// of f / M_S, lowest power first), interpolation comes up with F_S =
// sum_{i in S} c_i M_S / (x - x_i).  Both are cyclic products of size m with
// the children's nodes, whose leading 1 is x^(m/2) = (-1)^k in the transform
// domain, as in k_roots_pointwise:
//   down   a_L = (M_R * a_S)[m/2..m),  a_R = (M_L * a_S)[m/2..m)
//   up     F_S = F_L M_R + F_R M_L
// a and F are canonical, the tree's nodes Montgomery, so each product of one
// of each comes out canonical; `scale` is Montgomery(m^-1).

// g = F^-1 mod x^cnt for a series with F[0] = 1 (cnt <= 64, F of lf words):
// the recurrence g_i = -sum_{j=1..i} F_j g_(i-j) on one lane, the seed of the
// Newton steps (which would each be four launches on a handful of words).
__global__ void k_mp_series_seed(const uint32_t* __restrict__ F, uint32_t lf, uint32_t cnt, uint32_t* __restrict__ g) {
    __shared__ uint32_t gm[64];
    if (threadIdx.x) return;
    gm[0] = R_MOD_P;
    g[0] = 1u;
    for (uint32_t i = 1; i < cnt; i++) {
        uint32_t acc = 0;
        for (uint32_t j = 1; j <= i && j < lf; j++) acc = add(acc, mmul(F[j], gm[i - j]));
        g[i] = neg(acc);
        gm[i] = to_mont(neg(acc));
    }
}
void launch_mp_series_seed(const uint32_t* F, size_t lf, uint32_t cnt, uint32_t* g, hipStream_t s) {
    hipLaunchKernelGGL(k_mp_series_seed, dim3(1), dim3(64), 0, s, F, (uint32_t)(lf < 64 ? lf : 64), cnt, g);
}

// out[j] = (j + 1) z[j + 1], j < n: the derivative of the monic Z of degree n
// given by its n low coefficients (z[n] = 1 implied).
__global__ __launch_bounds__(256) void k_mp_derivative(const uint32_t* __restrict__ z, size_t n,
                                                       uint32_t* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride)
        out[j] = mmul(to_mont((uint32_t)(j + 1)), j + 1 < n ? z[j + 1] : 1u);
}
void launch_mp_derivative(const uint32_t* z, size_t n, uint32_t* out, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_mp_derivative, dim3(poly_blocks(n)), dim3(256), 0, s, z, n, out);
}

// Leaf subtrees, evaluation: node S of the leaf level (m = 2^log_leaf points)
// and its a_S give f(x_i) = sum_u q_i[u] a_S[m-1-u], q_i = M_S / (x - x_i) by
// the synthetic-division chain of k_lagrange_rows (q[m-1] = 1, q[u-1] =
// M_S[u] + x_i q[u]).  One lane per point; M_S and a_S are staged in LDS and
// every lane of a wave reads the same word of each per step (broadcasts).
// `canon`: the level is the tree's top (one leaf subtree) and holds canonical
// coefficients.
__global__ __launch_bounds__(256) void k_mp_leaf_eval(const uint32_t* __restrict__ xs, size_t count,
                                                      const uint32_t* __restrict__ node, uint32_t canon,
                                                      const uint32_t* __restrict__ a, uint32_t log_leaf,
                                                      uint32_t* __restrict__ out) {
    __shared__ uint32_t Ms[1u << ROOTS_LEAF_LOG_MAX], As[1u << ROOTS_LEAF_LOG_MAX];
    const uint32_t m = 1u << log_leaf, tid = threadIdx.x;
    const size_t p0 = (size_t)blockIdx.x * blockDim.x, n0 = (p0 >> log_leaf) << log_leaf;
    for (uint32_t u = tid; u < m; u += blockDim.x) {
        const uint32_t v = node[n0 + u];
        Ms[u] = canon ? to_mont(v) : v;
        As[u] = a[n0 + u];
    }
    __syncthreads();
    const size_t i = p0 + tid;
    if (i >= count || i >= n0 + m) return;
    const uint32_t xm = to_mont(xs[i]);
    uint32_t q = R_MOD_P, acc = 0;
    for (uint32_t u = m; u-- > 0;) {
        acc = add(acc, mmul(q, As[m - 1 - u]));
        q = add(Ms[u], mmul(q, xm));
    }
    out[i] = acc;
}
void launch_mp_leaf_eval(const uint32_t* xs, size_t count, const uint32_t* node, bool canon, const uint32_t* a,
                         uint32_t log_np, uint32_t log_leaf, uint32_t* out, hipStream_t s) {
    const uint32_t L = 1u << log_leaf, tpb = L < 64 ? 64 : L > 256 ? 256 : L;
    const size_t np = (size_t)1 << log_np;
    hipLaunchKernelGGL(k_mp_leaf_eval, dim3((unsigned)((np + tpb - 1) / tpb)), dim3(tpb), 0, s, xs, count, node,
                       canon ? 1u : 0u, a, log_leaf, out);
}

// Leaf subtrees, interpolation: k_roots_leaf's scheme with F carried along.
// Level 0 is M_i = x - x_i, F_i = c_i; a work item owning coefficients k and
// m + k of a node adds, to the m products of the node itself, the 2m of
// F_L b + F_R a (M_L = x^m + a, M_R = x^m + b), and m + k also takes
// F_L[k] + F_R[k].  F uses the layout of the nodes (even nodes in a buffer's
// first half), so the bank behaviour is the leaf kernel's.  The last level's
// node is not needed (the tree is retained) and is skipped.  Sums of <= 2^11
// products stay below 2^43.  LDS: four buffers of 2048 words, 32 KiB.
__global__ __launch_bounds__(256) void k_mp_leaf_up(const uint32_t* __restrict__ xs, const uint32_t* __restrict__ c,
                                                    size_t n, uint32_t log_leaf, uint32_t* __restrict__ out) {
    __shared__ uint32_t buf[2][1u << ROOTS_LEAF_LOG_MAX], fbuf[2][1u << ROOTS_LEAF_LOG_MAX];
    const uint32_t L = 1u << log_leaf, H = L >> 1, tid = threadIdx.x;
    const size_t r0 = (size_t)blockIdx.x << log_leaf;
    for (uint32_t i = tid; i < L; i += blockDim.x) {
        const bool in = r0 + i < n;
        const uint32_t pos = log_leaf ? (i & 1u) * H + (i >> 1) : 0u;
        buf[0][pos] = to_mont(neg(in ? xs[r0 + i] : 0u));
        fbuf[0][pos] = in ? c[r0 + i] : 0u;
    }
    uint32_t cur = 0;
    for (uint32_t lm = 0; lm < log_leaf; lm++, cur ^= 1u) {
        const uint32_t m = 1u << lm;
        const bool last = lm + 1 == log_leaf;
        const uint32_t* a = buf[cur];
        const uint32_t* b = buf[cur] + H;
        const uint32_t* fa = fbuf[cur];
        const uint32_t* fb = fbuf[cur] + H;
        __syncthreads();
        for (uint32_t t = tid; t < H; t += blockDim.x) {
            const uint32_t nd = t >> lm, k = t & (m - 1);
            const uint32_t* an = a + nd * m;
            const uint32_t* bn = b + nd * m;
            const uint32_t* fan = fa + nd * m;
            const uint32_t* fbn = fb + nd * m;
            uint64_t lo = 0, hi = 0, flo = 0, fhi = 0;
            for (uint32_t i = 0; i < m; i++) {
                const uint32_t av = an[(k - i) & (m - 1)], bv = bn[(k - i) & (m - 1)];
                const uint64_t fp = (uint64_t)mmul(fan[i], bv) + mmul(fbn[i], av);
                flo += i <= k ? fp : 0;
                fhi += i <= k ? 0 : fp;
                if (!last) {
                    const uint64_t p = mmul(an[i], bv);
                    lo += i <= k ? p : 0;
                    hi += i <= k ? 0 : p;
                }
            }
            const uint32_t o = last ? 0u : (nd & 1u) * H + (nd >> 1) * 2 * m;
            fbuf[cur ^ 1u][o + k] = mmul(redc(flo), R2_MOD_P);
            fbuf[cur ^ 1u][o + m + k] = add(mmul(redc(fhi), R2_MOD_P), add(fan[k], fbn[k]));
            if (!last) {
                buf[cur ^ 1u][o + k] = mmul(redc(lo), R2_MOD_P);
                buf[cur ^ 1u][o + m + k] = add(mmul(redc(hi), R2_MOD_P), add(an[k], bn[k]));
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < L; i += blockDim.x) out[r0 + i] = fbuf[cur][i];
}
void launch_mp_leaf_up(const uint32_t* xs, const uint32_t* c, size_t n, uint32_t log_np, uint32_t log_leaf,
                       uint32_t* out, hipStream_t s) {
    const uint32_t half = log_leaf ? 1u << (log_leaf - 1) : 1u;
    const uint32_t tpb = half < 64 ? 64 : half > 256 ? 256 : half;
    hipLaunchKernelGGL(k_mp_leaf_up, dim3(1u << (log_np - log_leaf)), dim3(tpb), 0, s, xs, c, n, log_leaf, out);
}

// One level in LDS, products of 2^lg <= 2^ROOTS_LDS_LOG_MAX words, on
// k_roots_level's tile scheme (a tile of the level is one batched transform).
// mp_load_child gathers one child (side 0: left) of every node pair of the
// tile bit-reversed and zero-padded to 2^lg (stage 0 is then the copy).
__device__ __forceinline__ void mp_load_child(uint32_t* dst, const uint32_t* __restrict__ src, uint32_t tile,
                                              uint32_t lg, uint32_t side) {
    const uint32_t h = 1u << (lg - 1);
    for (uint32_t e = threadIdx.x; e < tile / 2; e += 256) {
        const uint32_t nb = (e >> (lg - 1)) << lg, i = e & (h - 1);
        const uint32_t pos = nb + (__brev(i) >> (32 - lg));
        const uint32_t v = src[nb + side * h + i];
        dst[pos] = v;
        dst[pos + 1] = v;
    }
}
constexpr uint32_t MP_TILE_REGS = (1u << ROOTS_LDS_LOG_MAX) / 256;
// Down: the transform of a_S (all 2^lg words), the two children's, the two
// middle products, two inverse transforms of which the upper halves are
// kept: a_L beside a_R, the layout of the tree's level below.
__global__ __launch_bounds__(256) void k_mp_down_level(const uint32_t* __restrict__ a_in,
                                                       const uint32_t* __restrict__ nodes, uint32_t* __restrict__ a_out,
                                                       uint32_t tile, uint32_t lg, const uint32_t* __restrict__ tw_f,
                                                       const uint32_t* __restrict__ tw_i, uint32_t scale) {
    __shared__ uint32_t A[1u << ROOTS_LDS_LOG_MAX], B[1u << ROOTS_LDS_LOG_MAX];
    const uint32_t tid = threadIdx.x, h = 1u << (lg - 1), mask = 2 * h - 1;
    const size_t base = (size_t)blockIdx.x * tile;
    for (uint32_t e = tid; e < tile; e += 256) A[(e & ~mask) + (__brev(e & mask) >> (32 - lg))] = a_in[base + e];
    mp_load_child(B, nodes + base, tile, lg, 1);
    __syncthreads();
    roots_stage(A, tile, 0, tw_f);
    for (uint32_t s = 1; s < lg; s++) {
        __syncthreads();
        roots_stage(A, tile, s, tw_f);
        roots_stage(B, tile, s, tw_f);
    }
    __syncthreads();
    uint32_t pl[MP_TILE_REGS], pr[MP_TILE_REGS];
#pragma unroll
    for (uint32_t k = 0; k < MP_TILE_REGS; k++) {
        const uint32_t e = k * 256 + tid;
        if (e >= tile) continue;
        pl[k] = mmul(mmul(A[e], add(B[e], (e & 1u) ? P - R_MOD_P : R_MOD_P)), scale);   // a_S (M_R)
    }
    __syncthreads();
    mp_load_child(B, nodes + base, tile, lg, 0);
    for (uint32_t s = 1; s < lg; s++) {
        __syncthreads();
        roots_stage(B, tile, s, tw_f);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < MP_TILE_REGS; k++) {
        const uint32_t e = k * 256 + tid;
        if (e >= tile) continue;
        pr[k] = mmul(mmul(A[e], add(B[e], (e & 1u) ? P - R_MOD_P : R_MOD_P)), scale);   // a_S (M_L)
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < MP_TILE_REGS; k++) {
        const uint32_t e = k * 256 + tid;
        if (e >= tile) continue;
        const uint32_t pos = (e & ~mask) + (__brev(e & mask) >> (32 - lg));
        A[pos] = pl[k];
        B[pos] = pr[k];
    }
    for (uint32_t s = 0; s < lg; s++) {
        __syncthreads();
        roots_stage(A, tile, s, tw_i);
        roots_stage(B, tile, s, tw_i);
    }
    __syncthreads();
    for (uint32_t e = tid; e < tile; e += 256) {
        const uint32_t r = e & mask;
        a_out[base + e] = r < h ? A[e + h] : B[e];
    }
}
void launch_mp_down_level_lds(const uint32_t* a_in, const uint32_t* nodes, uint32_t* a_out, uint32_t log_np,
                              uint32_t lg, const uint32_t* tw_fwd, const uint32_t* tw_inv, hipStream_t s) {
    const uint32_t tile = log_np < ROOTS_LDS_LOG_MAX ? 1u << log_np : 1u << ROOTS_LDS_LOG_MAX;
    hipLaunchKernelGGL(k_mp_down_level, dim3((unsigned)(((size_t)1 << log_np) / tile)), dim3(256), 0, s, a_in, nodes,
                       a_out, tile, lg, tw_fwd, tw_inv, to_mont(inv_std(1u << lg)));
}
// Up: F_L with M_R, then F_R with M_L through the same two arrays, the sum
// held in registers between them; one inverse transform.
__global__ __launch_bounds__(256) void k_mp_up_level(const uint32_t* __restrict__ f_in,
                                                     const uint32_t* __restrict__ nodes, uint32_t* __restrict__ f_out,
                                                     uint32_t tile, uint32_t lg, const uint32_t* __restrict__ tw_f,
                                                     const uint32_t* __restrict__ tw_i, uint32_t scale) {
    __shared__ uint32_t A[1u << ROOTS_LDS_LOG_MAX], B[1u << ROOTS_LDS_LOG_MAX];
    const uint32_t tid = threadIdx.x, mask = (1u << lg) - 1;
    const size_t base = (size_t)blockIdx.x * tile;
    uint32_t r[MP_TILE_REGS];
    for (uint32_t side = 0; side < 2; side++) {
        if (side) __syncthreads();
        mp_load_child(A, f_in + base, tile, lg, side);
        mp_load_child(B, nodes + base, tile, lg, side ^ 1u);
        for (uint32_t s = 1; s < lg; s++) {
            __syncthreads();
            roots_stage(A, tile, s, tw_f);
            roots_stage(B, tile, s, tw_f);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < MP_TILE_REGS; k++) {
            const uint32_t e = k * 256 + tid;
            if (e >= tile) continue;
            const uint32_t t = mmul(A[e], add(B[e], (e & 1u) ? P - R_MOD_P : R_MOD_P));
            r[k] = side ? mmul(add(r[k], t), scale) : t;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < MP_TILE_REGS; k++) {
        const uint32_t e = k * 256 + tid;
        if (e < tile) A[(e & ~mask) + (__brev(e & mask) >> (32 - lg))] = r[k];
    }
    for (uint32_t s = 0; s < lg; s++) {
        __syncthreads();
        roots_stage(A, tile, s, tw_i);
    }
    __syncthreads();
    for (uint32_t e = tid; e < tile; e += 256) f_out[base + e] = A[e];
}
void launch_mp_up_level_lds(const uint32_t* f_in, const uint32_t* nodes, uint32_t* f_out, uint32_t log_np, uint32_t lg,
                            const uint32_t* tw_fwd, const uint32_t* tw_inv, hipStream_t s) {
    const uint32_t tile = log_np < ROOTS_LDS_LOG_MAX ? 1u << log_np : 1u << ROOTS_LDS_LOG_MAX;
    hipLaunchKernelGGL(k_mp_up_level, dim3((unsigned)(((size_t)1 << log_np) / tile)), dim3(256), 0, s, f_in, nodes,
                       f_out, tile, lg, tw_fwd, tw_inv, to_mont(inv_std(1u << lg)));
}

// Larger levels: batched NTT passes around these pointwise kernels
// (elementwise over the level, k mod 2 = word index mod 2).  Down reads the
// parents' transform ta and the children's tl, tr and leaves ta (M_R) over tr
// and ta (M_L) over tl; the upper halves of their inverse transforms are the
// children's vectors, and k_mp_take_high moves a_L's to its place beside a_R.
__global__ __launch_bounds__(256) void k_mp_down_pointwise(const uint4* __restrict__ ta, uint4* tl, uint4* tr,
                                                           size_t n4, uint32_t scale) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    auto pw = [&](uint32_t a, uint32_t b, uint32_t sg) { return mmul(mmul(a, add(b, sg)), scale); };
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const uint4 a = ta[i], l = tl[i], r = tr[i];
        uint4 x, y;
        x.x = pw(a.x, r.x, R_MOD_P);
        x.y = pw(a.y, r.y, P - R_MOD_P);
        x.z = pw(a.z, r.z, R_MOD_P);
        x.w = pw(a.w, r.w, P - R_MOD_P);
        y.x = pw(a.x, l.x, R_MOD_P);
        y.y = pw(a.y, l.y, P - R_MOD_P);
        y.z = pw(a.z, l.z, R_MOD_P);
        y.w = pw(a.w, l.w, P - R_MOD_P);
        tr[i] = x;
        tl[i] = y;
    }
}
void launch_mp_down_pointwise(const uint32_t* ta, uint32_t* tl, uint32_t* tr, size_t words, uint32_t lg,
                              hipStream_t s) {
    const uint32_t ninv = inv_std((uint32_t)(((size_t)1 << lg) % P));
    hipLaunchKernelGGL(k_mp_down_pointwise, dim3(poly_blocks(words / 4)), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(ta), reinterpret_cast<uint4*>(tl), reinterpret_cast<uint4*>(tr),
                       words / 4, to_mont(ninv));
}
__global__ __launch_bounds__(256) void k_mp_take_high(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n4,
                                                      uint32_t lg4) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, h4 = (size_t)1 << (lg4 - 1);
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4 / 2; e += stride) {
        const size_t o = ((e >> (lg4 - 1)) << lg4) + (e & (h4 - 1));
        dst[o] = src[o + h4];
    }
}
void launch_mp_take_high(const uint32_t* src, uint32_t* dst, size_t words, uint32_t lg, hipStream_t s) {
    hipLaunchKernelGGL(k_mp_take_high, dim3(poly_blocks(words / 8)), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), words / 4, lg - 2);
}
// Up: out = (fl (br + s) + fr (bl + s)) / 2^lg; out may be fl.
__global__ __launch_bounds__(256) void k_mp_up_pointwise(const uint4* fl, const uint4* __restrict__ fr,
                                                         const uint4* __restrict__ bl, const uint4* __restrict__ br,
                                                         uint4* out, size_t n4, uint32_t scale) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    auto pw = [&](uint32_t l, uint32_t r, uint32_t ml, uint32_t mr, uint32_t sg) {
        return mmul(add(mmul(l, add(mr, sg)), mmul(r, add(ml, sg))), scale);
    };
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const uint4 l = fl[i], r = fr[i], ml = bl[i], mr = br[i];
        uint4 o;
        o.x = pw(l.x, r.x, ml.x, mr.x, R_MOD_P);
        o.y = pw(l.y, r.y, ml.y, mr.y, P - R_MOD_P);
        o.z = pw(l.z, r.z, ml.z, mr.z, R_MOD_P);
        o.w = pw(l.w, r.w, ml.w, mr.w, P - R_MOD_P);
        out[i] = o;
    }
}
void launch_mp_up_pointwise(const uint32_t* fl, const uint32_t* fr, const uint32_t* bl, const uint32_t* br,
                            uint32_t* out, size_t words, uint32_t lg, hipStream_t s) {
    const uint32_t ninv = inv_std((uint32_t)(((size_t)1 << lg) % P));
    hipLaunchKernelGGL(k_mp_up_pointwise, dim3(poly_blocks(words / 4)), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(fl), reinterpret_cast<const uint4*>(fr),
                       reinterpret_cast<const uint4*>(bl), reinterpret_cast<const uint4*>(br),
                       reinterpret_cast<uint4*>(out), words / 4, to_mont(ninv));
}

}  // namespace fri
