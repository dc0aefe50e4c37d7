// fri_tree_device.hpp — device helpers of the tree and commit kernels that
// fri_layer.hip and fri_batch_kernels.hip share: digests and tree levels
// (lane-pair nodes, the schedule producer), coefficient maxima and the degree
// rule, the channel jobs, and the per-layer pieces of the kernels that run
// whole layers in one workgroup.  Everything is inlined: each kernel keeps its
// own LDS footprint and register budget.
#pragma once
#include "fri_internal.hpp"
#include "chan_words.hpp"
#include "sha256_fast.hpp"
#include "sha256_quad.hpp"

namespace fri {

// Diagnostic build (-DFRI_STAMPS, lib/libfri_amd_stamps.so): where `on`
// holds, a lane records s_memrealtime (STAMP) or s_memtime (STAMP_CLK) into
// slot i of its layer's row (t: the layer's LayerTask, commit mode).  The
// kernels differ only in `on`: lane 0 (or lane 448, the channel wave) of a
// commit's top or tail, lane 0 of workgroup 0 of a wide leaf kernel (slots
// 60..62: start, leaves done, levels done).  Never in the product.
#ifdef FRI_STAMPS
#define STAMP_WITH(on, i, fn)                                  \
    do {                                                       \
        if (on) t.st->stamps[t.k][(i)] = fn();                 \
    } while (0)
#else
#define STAMP_WITH(on, i, fn) do {} while (0)
#endif
#define STAMP(on, i) STAMP_WITH(on, i, __builtin_amdgcn_s_memrealtime)
#define STAMP_CLK(on, i) STAMP_WITH(on, i, __builtin_amdgcn_s_memtime)

struct Dg { uint32_t w[8]; };

__device__ __forceinline__ void dg_load(const uint32_t* p, Dg& d) {
    uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
    d.w[0] = a.x; d.w[1] = a.y; d.w[2] = a.z; d.w[3] = a.w; d.w[4] = b.x; d.w[5] = b.y; d.w[6] = b.z; d.w[7] = b.w;
}
__device__ __forceinline__ void dg_store(uint32_t* p, const Dg& d) {
    reinterpret_cast<uint4*>(p)[0] = make_uint4(d.w[0], d.w[1], d.w[2], d.w[3]);
    reinterpret_cast<uint4*>(p)[1] = make_uint4(d.w[4], d.w[5], d.w[6], d.w[7]);
}
__device__ __forceinline__ void dg_lds_load(const uint4* p, Dg& d) {
    uint4 a = p[0], b = p[1];
    d.w[0] = a.x; d.w[1] = a.y; d.w[2] = a.z; d.w[3] = a.w; d.w[4] = b.x; d.w[5] = b.y; d.w[6] = b.z; d.w[7] = b.w;
}
__device__ __forceinline__ void dg_lds_store(uint4* p, const Dg& d) {
    p[0] = make_uint4(d.w[0], d.w[1], d.w[2], d.w[3]);
    p[1] = make_uint4(d.w[4], d.w[5], d.w[6], d.w[7]);
}
__device__ __forceinline__ void hnode(const Dg& l, const Dg& r, Dg& o) { shaf::node(l.w, r.w, o.w); }
__device__ __forceinline__ void hleaf(uint32_t v, Dg& o) { shaf::leaf(v, o.w); }
// compact (looped) forms for the latency-bound mid / top kernels
__device__ __forceinline__ void cnode(const Dg& l, const Dg& r, Dg& o) { shaf::node_compact(l.w, r.w, o.w); }
__device__ __forceinline__ void cleaf(uint32_t v, Dg& o) { shaf::leaf_compact(v, o.w); }

// One node per pair of lanes (sha256_quad.hpp) for the narrow, latency-bound
// levels: thread `tid` < 2*cnt hashes node tid/2; the even lane writes
// digest words 4..7, the odd lane words 0..3 (LDS for the next level, HBM).
__device__ __forceinline__ void pair_level(const uint4* A, uint4* B, uint32_t* out, uint32_t tid, uint32_t cnt,
                                           const shaq::Role& R) {
    // Below 32 nodes the whole of wave 0 still runs: the spare lane pairs
    // recompute node (q mod cnt) and store nothing. A partly masked wave runs
    // the node 0.7-2.7 K cycles slower than a full one (8.4 K), by an amount
    // that changes from launch to launch (bench/plateau_micro.hip mode 10,
    // profiles/r01_plateau_micro_masked.txt). cnt is a power of two.
    if (tid >= max(2 * cnt, 64u)) return;
    const uint32_t q = (tid >> 1) & (cnt - 1), half = (tid & 1u) ^ 1u;
    const bool real = tid < 2 * cnt;
    Dg a, b;
    dg_lds_load(A + 4 * q, a);
    dg_lds_load(A + 4 * q + 2, b);
    uint32_t o[4];
    shaq::node(a.w, b.w, o, R);
    if (!real) return;
    const uint4 v = make_uint4(o[0], o[1], o[2], o[3]);
    B[2 * q + half] = v;
    reinterpret_cast<uint4*>(out + 8 * q)[half] = v;
}

// Narrow levels (<= 32 nodes, one round wave) with the message schedule made
// by wave 1 of the workgroup (sha256_quad.hpp produce / node_ext): the round
// wave, wave 0, issues 48 x 7 fewer instructions per node.  Wave 1 sits on
// another SIMD (waves are dealt to the SIMDs in turn), and at these levels it
// is otherwise idle.  `ord`: the level's ordinal within the launch, strictly
// increasing (the flag counts 3 per level).  0 = off (A/B builds).
#ifndef FRI_SCHED_PRODUCER
#define FRI_SCHED_PRODUCER 1
#endif
struct SchedLds {
    uint32_t wk[32 * 48];       // per node W16..W63 + K (16-byte aligned rows of 48 words)
    uint32_t flag;
};
__device__ __forceinline__ void sched_init(SchedLds* sl) {
    if (FRI_SCHED_PRODUCER && threadIdx.x == 0) sl->flag = 0u;    // (before the launch's first barrier)
}
__device__ __forceinline__ void pair_level_s(const uint4* A, uint4* B, uint32_t* out, uint32_t tid, uint32_t cnt,
                                             const shaq::Role& R, SchedLds* sl, uint32_t ord) {
    if (!FRI_SCHED_PRODUCER || cnt > 32) {
        pair_level(A, B, out, tid, cnt, R);
        return;
    }
    const uint32_t wv = tid >> 6;
    if (wv > 1) return;
    const uint32_t lane = tid & 63u;
    const uint32_t q = (lane >> 1) & (cnt - 1), half = (lane & 1u) ^ 1u;
    const bool real = lane < 2 * cnt;            // spare lanes redo node q mod cnt and store nothing (see pair_level)
    Dg a, b;
    dg_lds_load(A + 4 * q, a);
    dg_lds_load(A + 4 * q + 2, b);
    if (wv == 1) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 8; i++) { w[i] = a.w[i]; w[8 + i] = b.w[i]; }
        shaq::produce(w, sl->wk + 48 * q, &sl->flag, 3u * ord, real && (lane & 1u) == 0u, lane == 0u, R);
        return;
    }
    uint32_t o[4];
    shaq::node_ext(a.w, b.w, o, R, sl->wk + 48 * q, &sl->flag, 3u * ord);
    if (!real) return;
    const uint4 v = make_uint4(o[0], o[1], o[2], o[3]);
    B[2 * q + half] = v;
    reinterpret_cast<uint4*>(out + 8 * q)[half] = v;
}

// Barrier that waits only for this wave's LDS traffic: HIP's __syncthreads()
// also drains vmcnt, i.e. waits ~1 us for the level's global digest stores,
// which no other wave of the workgroup reads.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}

// The three maxima of a coefficient task, -1 where there is none.  Round
// k >= 1: the largest j with c'_j != 0, with c_2j != 0, with c_2j+1 != 0.
// k == 0: m0 = the largest index of a nonzero input coefficient, m1 >= 0
// flags a coefficient >= p, m2 unused.
struct Mx3 {
    int m0 = -1, m1 = -1, m2 = -1;
    // triple i of an array of triples
    __device__ __forceinline__ void load(const int32_t* p, uint32_t i) { m0 = p[3 * i]; m1 = p[3 * i + 1]; m2 = p[3 * i + 2]; }
    __device__ __forceinline__ void take(const int32_t* p, uint32_t i) {
        m0 = max(m0, p[3 * i]); m1 = max(m1, p[3 * i + 1]); m2 = max(m2, p[3 * i + 2]);
    }
    __device__ __forceinline__ void store(int32_t* p, uint32_t i) const { p[3 * i] = m0; p[3 * i + 1] = m1; p[3 * i + 2] = m2; }
    __device__ __forceinline__ void wave_max() { m0 = wave_max_i(m0); m1 = wave_max_i(m1); m2 = wave_max_i(m2); }
};
// The wave's maxima into red[3 * wave ..] (tx: the thread's index among the
// whole waves that take part); then, after a barrier, the nw waves' triples.
__device__ __forceinline__ void mx3_wave_to_red(Mx3 m, int32_t* red, uint32_t tx) {
    m.wave_max();
    if ((tx & 63) == 0) m.store(red, tx >> 6);
}
__device__ __forceinline__ Mx3 mx3_from_red(const int32_t* red, uint32_t nw) {
    Mx3 m;
    for (uint32_t i = 0; i < nw; i++) m.take(red, i);
    return m;
}
// Degree of poly_k (reference degree field; see DevState) from the layer's
// maxima; noncanon: an input coefficient >= p (layer 0 only, FRI_EINVAL).
struct Degree { int deg; bool noncanon; };
__device__ __forceinline__ Degree degree_of(int k, const Mx3& m) {
    return {k == 0 ? m.m0 : (m.m1 < 0 ? m.m2 : m.m0), k == 0 && m.m1 >= 0};
}

// One scalar load per 64-byte line of every __constant__ table the compact
// SHA forms read (KTAB, PAD_KW_C, PAD_KW_1024, PAD_KW_1536, 256 B each):
// fills the CU's scalar cache while the inputs load, instead of cold misses
// inside level 1 and inside the channel send.  Loads land in clobbered SGPRs
// and are drained inside the statement.
__device__ __forceinline__ void ktouch(const void* sym) {
    uint32_t a, b, c, d;
    asm volatile("s_nop 4\n\t"
                 "s_load_dword %0, %4, 0x0\n\ts_load_dword %1, %4, 0x40\n\t"
                 "s_load_dword %2, %4, 0x80\n\ts_load_dword %3, %4, 0xc0\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b), "=&s"(c), "=&s"(d)
                 : "s"(sym)
                 : "memory");
}
__device__ __forceinline__ void kcache_touch_sha_tables() {
    ktouch(&shaf::KTAB[0]);
    ktouch(&shaf::PAD_KW_C.kw[0]);
    ktouch(&shaf::PAD_KW_1024.kw[0]);
    ktouch(&shaf::PAD_KW_1536.kw[0]);
}

// ------------------------------------------------------------ channel ----
// Frozen spec: messages are built word by word in registers
// (hex2, hexhex and chan_beta: chan_words.hpp).

// Channel work of one top kernel as a sequence of compression jobs run by
// wave 7 (lane pairs redundant), with ONE lane-pair compress and ONE
// compress_kw call site: the jobs done during the narrow tree levels (off
// the critical path) leave exactly the code the post-root jobs need in the
// I-cache.
//   0  rehash block   X = compress(IV, hex(cs))        channel.rs:75-76, the
//   1  rehash pad     cs = X = pad(X)                  receive's deferred rehash
//   2  midstate       X = compress(IV, hex(cs))        first block of the next send
//   3  root block 1   X = compress(X | IV, hex(hex(root[0..15])))   channel.rs:35-39,
//   4  root block 2   X = compress(X, hex(hex(root[16..31])))       message = root hex
//   5  root pad       cs = X = pad_{1536|1024}(X)      -> S
//   6  final block 1  X = compress(IV, hex(cs))        fri_commit.rs:114,
//   7  final block 2  cs = X = compress(X, hex(be64(fv)) | pad)   send(final.to_bytes())
enum { CJ_REHASH = 0, CJ_MID = 2, CJ_ROOT = 3, CJ_FINAL = 6, CJ_END_ROUND = 6, CJ_END_FINAL = 8 };

// Lane-pair form (sha256_quad.hpp): X is this lane's half of the chaining
// value (even lane words 4..7, odd lane 0..3); cs stays whole on every lane.
__device__ __forceinline__ void chan_job(int j, uint32_t cs[8], uint32_t X[4], uint32_t has, const uint4* root_lds,
                                         uint32_t fv, const shaq::Role& R) {
    // the job and the channel flags are wave-uniform: in SGPRs the job's
    // branches are scalar and its padding table is read by scalar loads
    // (a per-lane table pointer costs a vector-load round trip per 16 rounds)
    j = __builtin_amdgcn_readfirstlane(j);
    has = __builtin_amdgcn_readfirstlane(has);
    uint32_t w[16];
    const bool pad = (j == 1) || (j == 5);
    if (j == 0 || j == 2 || j == 6) {
#pragma unroll
        for (int i = 0; i < 8; i++) hex2(cs[i], w[2 * i], w[2 * i + 1]);
#pragma unroll
        for (int i = 0; i < 4; i++) X[i] = R.iv[i];
    } else if (j == 3 || j == 4) {
        // one root byte per lane (lanes 0..15: this block's 16 bytes), its
        // hex(hex()) word computed once, then read out as the 16 wave-uniform
        // message words: 1 + 16 instructions instead of 16 per-word encodings
        const uint32_t b = (__lane_id() & 15u) + (j == 4 ? 16u : 0u);
        const uint32_t rw = reinterpret_cast<const uint32_t*>(root_lds)[b >> 2];
        const uint32_t hh = hexhex((rw >> (24 - 8 * (b & 3))) & 255u);
#pragma unroll
        for (int jj = 0; jj < 16; jj++) w[jj] = __builtin_amdgcn_readlane(hh, jj);
        if (j == 3 && !has) {
#pragma unroll
            for (int i = 0; i < 4; i++) X[i] = R.iv[i];
        }
    } else if (j == 7) {
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = 0u;
        w[0] = 0x30303030u; w[1] = 0x30303030u;   // "00000000": high u32 of the u64 is 0
        hex2(fv, w[2], w[3]);
        w[4] = 0x80000000u;
        w[15] = 80u * 8u;                           // hex(state) (64) + 16 chars
    }
    if (pad) shaq::compress_kw(X, j == 1 ? shaf::PAD_KW_C.kw : (has ? shaf::PAD_KW_1536.kw : shaf::PAD_KW_1024.kw), R);
    else shaq::compress(X, w, R);
    if (j == 1 || j == 5 || j == 7) {            // cs = X, both halves on every lane
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t o = shaq::swap01(X[i]);
            cs[i] = R.is_a ? X[i] : o;
            cs[4 + i] = R.is_a ? o : X[i];
        }
    }
}

// --------------------------------------------- shared by top and tail ----
// What k_tree_top and k_tree_tail (one workgroup of 512 threads each, wave 7
// the channel wave) both do, written once.  Everything here is inlined: the
// two kernels keep their own LDS footprints and register budgets.

// The leaves of a layer of N <= 512 values: value(j, real) yields layer
// value j (and stores what its kernel keeps of it); leaf digests to the
// tree's level 0 and to A.  Under 64 leaves the spare lanes of wave 0 hash
// leaf (i mod N) and store nothing: a partly masked wave is slower (see
// pair_level).
template <typename Value>
__device__ __forceinline__ void leaf_loop(uint32_t N, uint32_t* tr, uint4* A, Value&& value) {
    for (uint32_t i = threadIdx.x; i < max(N, 64u); i += blockDim.x) {
        const uint32_t j = i & (N - 1);          // N is a power of two
        const bool real = i < N;
        const uint32_t v = value(j, real);
        Dg d;
        cleaf(v, d);
        if (real) {
            dg_store(tr + 8 * j, d);
            dg_lds_store(A + 2 * j, d);
        }
    }
}

// One tree level: cnt nodes from A into B and `out`.  ord: see pair_level_s.
// (stamps, FRI_STAMPS builds: slots 24 + 2 it / 25 + 2 it around the first node)
__device__ __forceinline__ void level_step(const LayerTask& t, bool stamps, uint32_t it, const uint4* A, uint4* B,
                                           uint32_t* out, uint32_t cnt, const shaq::Role& R, SchedLds* sl,
                                           uint32_t ord) {
    const uint32_t tid = threadIdx.x;
    if (cnt <= 128) {                   // waves 0-3, one per SIMD (wave 7: channel)
        STAMP_CLK(stamps && it < 18 && tid == 0, 24 + 2 * it);
        pair_level_s(A, B, out, tid, cnt, R, sl, ord);
        STAMP_CLK(stamps && it < 18 && tid == 0, 25 + 2 * it);
        return;
    }
#pragma unroll 1
    for (uint32_t q = tid; q < cnt; q += blockDim.x) {
        Dg a, b, o;
        dg_lds_load(A + 4 * q, a);
        dg_lds_load(A + 4 * q + 2, b);
#ifdef FRI_STAMPS
        if (stamps && it < 18 && q == 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
        STAMP_CLK(stamps && it < 18 && q == 0, 24 + 2 * it);
        cnode(a, b, o);
        STAMP_CLK(stamps && it < 18 && q == 0, 25 + 2 * it);
        dg_lds_store(B + 2 * q, o);
        dg_store(out + 8 * q, o);
    }
}

// The channel wave's jobs of one iteration of the level loop: during a narrow
// level (SIMD 3 idle) one pre-root job, after the last level every job still
// left.  Its kernel's ONE chan_job call site (see chan_job).
__device__ __forceinline__ int chan_drain(const LayerTask& t, int job, int job_end, bool level, uint32_t cnt,
                                           uint32_t cs[8], uint32_t X[4], uint32_t has, const uint4* root_lds,
                                           uint32_t fv, const shaq::Role& R) {
    if (job >= job_end || (level && !(cnt <= 192 && job < CJ_ROOT))) return job;
    do {
        STAMP(threadIdx.x == 448 && job == CJ_ROOT, 14);           // job 3 / job 5 start (14, 13)
        STAMP(threadIdx.x == 448 && job == CJ_ROOT + 2, 13);
        chan_job(job, cs, X, has, root_lds, fv, R);
        STAMP(threadIdx.x == 448 && job >= CJ_ROOT && job <= CJ_ROOT + 2, 20 + job - CJ_ROOT);   // done (20..22)
        job++;
    } while (!level && job < job_end);
    return job;
}

// Results of layer t.k, by one lane of the channel wave after its last job:
// DevState's record of the layer and either the Fiat-Shamir step (round:
// beta_k, channel.rs:35-55), the final send (fri_commit.rs:114) or an error
// (FRI_EINVAL, FRI_EDEGREE).  cs: the channel state after the layer's sends;
// fbeta1: the test hook's beta + 1, or 0 when beta is not forced; root_lds:
// the tree's root.  Returns what a next layer in the same launch needs.
struct RoundOut { uint32_t active, beta_m; };
__device__ __forceinline__ RoundOut layer_results(const LayerTask& t, const Degree& dg, const uint32_t cs[8],
                                                  uint32_t fv, uint32_t fbeta1, const uint4* root_lds) {
    DevState* st = t.st;
    const int k = t.k, deg = dg.deg;
    if (dg.noncanon) {                             // FRI_EINVAL: nothing of this commit is served
        st->active[k] = 0;
        st->status = 1u;
        return {0u, 0u};
    }
    st->deg[k] = deg;
    Dg root;
    dg_lds_load(root_lds, root);
#pragma unroll
    for (int i = 0; i < 8; i++) st->roots[k][i] = root.w[i];
    st->n_layers = (uint32_t)k + 1;
    STAMP(true, 15);
    if (deg >= 1 && k < MAXR && t.L >= 1) {
        uint32_t beta = chan_beta(cs);
#pragma unroll
        for (int i = 0; i < 8; i++) st->chan[i] = cs[i];
        st->chan_has = 1;
        st->chan_pending = 1;                        // receive's rehash deferred to the next layer's jobs
        if (fbeta1) beta = fbeta1 - 1u;
        st->beta[k] = beta;
        const uint32_t bm = to_mont(beta);
        st->beta_mont[k] = bm;
        st->active[k] = 1;
        st->n_rounds = (uint32_t)k + 1;
        STAMP(true, 16);
        return {1u, bm};
    }
    st->active[k] = 0;
    if (deg >= 1) { st->status = 7u; return {0u, 0u}; }       // FRI_EDEGREE
#pragma unroll
    for (int i = 0; i < 8; i++) st->chan[i] = cs[i];          // after send(final.to_bytes())
    st->final_value = fv;
    st->final_degree = deg;
    st->chan_has = 1;
    st->chan_pending = 0;
    return {0u, 0u};
}

// ------------------------- shared by tail, batched commit, trace trees ----
// The per-layer pieces of the kernels that run whole layers in one workgroup
// of 512 threads (k_tree_tail, k_commit_batch, k_trace_trees_batch).

// The coefficient work of a layer on threads [t0, t0 + nthr) (whole waves);
// both end in mx3_wave_to_red: red[] is read after the caller's next barrier.
// Layer 0, coef_scan: the len input coefficients at `in`; m0 = the last
// nonzero index, m1 = 0 on a coefficient >= p (see Mx3).
__device__ __forceinline__ void coef_scan(const uint32_t* in, uint32_t len, int32_t* red, uint32_t t0, uint32_t nthr) {
    Mx3 m;
    const uint32_t tx = threadIdx.x - t0;
    for (uint32_t j = tx; j < len; j += nthr) {
        const uint32_t c = in[j];
        if (c) m.m0 = max(m.m0, (int)j);
        if (c >= P) m.m1 = 0;                      // not canonical
    }
    mx3_wave_to_red(m, red, tx);
}
// Layer k >= 1, coef_fold: out[j] = c[2j] + beta c[2j+1] of poly_{k-1} (len
// coefficients) with its three maxima.  c is `in`, or per element prev_c
// (LDS) where in_lds holds: the tail's form (one pointer chosen before its
// loop costs it two VGPRs).  The batch chooses its pointer before the call and
// passes in_lds = false, its form before (profiles/batch_kernels_one_body.txt).
__device__ __forceinline__ void coef_fold(bool in_lds, const uint32_t* prev_c, const uint32_t* in, uint32_t* out,
                                          uint32_t len, uint32_t beta_m, int32_t* red, uint32_t t0, uint32_t nthr) {
    Mx3 m;
    const uint32_t tx = threadIdx.x - t0, nlen = (len + 1) / 2;
    for (uint32_t j = tx; j < nlen; j += nthr) {
        const uint32_t e = in_lds ? prev_c[2 * j] : in[2 * j];
        const uint32_t o = (2 * j + 1 < len) ? (in_lds ? prev_c[2 * j + 1] : in[2 * j + 1]) : 0u;
        const uint32_t v = add(e, mmul(o, beta_m));
        out[j] = v;
        if (v) m.m0 = (int)j;
        if (e) m.m1 = (int)j;
        if (o) m.m2 = (int)j;
    }
    mx3_wave_to_red(m, red, tx);
}

// The leaves of a layer of N <= 2^TAIL_LOG values (leaf_loop, whose
// spare-lane rule for N < 64 holds here unchanged).  fold: value j is the fold
// of the previous layer's pair (j, j + N), read from LDS (prev_v) where the
// previous layer ran this path too (in_lds) and from HBM (prev) otherwise; it
// goes to values[j].  No fold (layer 0): values[j] is read.  Either way the
// value is kept in cur_v[j] (LDS) for the next layer's fold.
__device__ __forceinline__ void folded_leaves(uint32_t N, uint32_t* tr, uint4* A, bool fold, bool in_lds,
                                              const uint32_t* prev_v, const uint32_t* prev, const uint32_t* xl,
                                              uint32_t beta_m, uint32_t* values, uint32_t* cur_v) {
    leaf_loop(N, tr, A, [&](uint32_t j, bool real) {
        uint32_t v;
        if (fold) {
            const uint32_t a = in_lds ? prev_v[j] : prev[j], b = in_lds ? prev_v[j + N] : prev[j + N];
            v = fold_one(a, b, xl[j], beta_m);
            if (real) values[j] = v;
        } else {
            v = values[j];
        }
        if (real) cur_v[j] = v;
        return v;
    });
}

// Layer t.L > TAIL_LOG in tiles of 2^TAIL_LOG leaves (one per thread):
// value(i) yields leaf i (and stores what its kernel keeps of it); per tile the
// leaf hashes and a climb of TAIL_LOG levels in LDS, every digest to the tree.
// Then the 2^(L - TAIL_LOG) tile roots are reloaded into lds (the caller's A),
// after a __syncthreads() that drains vmcnt: other waves of this workgroup
// wrote them (and what value() stored) to HBM.  Returns the level now in A.
// ord (pair_level_s): one more per level, across tiles and layers.  blockDim.x
// is read once, up here: read again under the tile loop (level_step) it became
// a vector load with a vmcnt(0) that drains each tile's digest stores.
template <typename Value>
__device__ __forceinline__ uint32_t tiled_leaves(const LayerTask& t, uint32_t* tr, uint4* lds, const shaq::Role& R,
                                                 SchedLds* sl, uint32_t& ord, Value&& value) {
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, tiles = 1u << (t.L - TAIL_LOG);
#pragma unroll 1
    for (uint32_t tile = 0; tile < tiles; tile++) {
        uint4* A = lds;
        uint4* B = lds + (2u << TAIL_LOG);
        const uint32_t i = (tile << TAIL_LOG) + tid;
        Dg d;
        cleaf(value(i), d);
        dg_store(tr + 8 * (size_t)i, d);
        dg_lds_store(A + 2 * tid, d);
        lds_barrier();
        uint32_t cnt = 1u << TAIL_LOG;
#pragma unroll 1
        for (uint32_t j = 1; j <= TAIL_LOG; j++) {
            cnt >>= 1;
            level_step(t, false, 0, A, B, tr + 8 * (level_offset(t.L, j) + ((size_t)tile << (TAIL_LOG - j))), cnt, R, sl,
                       ord++);
            lds_barrier();
            uint4* tmp = A; A = B; B = tmp;
        }
    }
    __syncthreads();
    const uint32_t* in = tr + 8 * level_offset(t.L, TAIL_LOG);
    for (uint32_t i = tid; i < tiles; i += nthr) {
        Dg d;
        dg_load(in + 8 * i, d);
        dg_lds_store(lds + 2 * i, d);
    }
    return TAIL_LOG;
}

// The channel across the layers of one launch: its state in the registers of
// wave 7 (chan_wave), zero elsewhere.
struct Chan { uint32_t cs[8], X[4], has, pending; };

// Prologue: the channel fields in one round trip (see k_tree_top), the SHA
// tables into the scalar cache (wave 6), and the test hook's betas of layers
// k0 .. k0 + nf - 1 into s_fbeta (layer_results' fbeta1: beta + 1, 0 = not
// forced), off the per-layer critical path.
__device__ __forceinline__ void chan_open(Chan& c, const DevState* st, bool chan_wave, uint32_t* s_fbeta, uint32_t nf,
                                          int k0) {
    const uint32_t tid = threadIdx.x;
    c.has = 0;
    if (chan_wave) {
#pragma unroll
        for (int i = 0; i < 8; i++) c.cs[i] = st->chan[i];
        c.has = st->chan_has;
    }
    c.pending = chan_wave ? st->chan_pending : 0u;
    if (tid >= 384 && tid < 448) kcache_touch_sha_tables();
    if (tid < nf) {
        const int kk = k0 + (int)tid;
        s_fbeta[tid] = (st->forced && kk < MAXR) ? st->forced_beta[kk] + 1u : 0u;
    }
}

// red[] (after a barrier, nw waves' triples) -> degree of poly_k; is it the
// commit's last layer (job_end)?  Then c0[0] is the final value
// (fri_commit.rs:109-113): c0 = the input at k == 0, poly_k otherwise.
struct Settled { Degree dg; int job_end; uint32_t fv; };
__device__ __forceinline__ Settled settle(int k, const int32_t* red, uint32_t nw, bool chan_wave, const uint32_t* c0) {
    const Degree dg = degree_of(k, mx3_from_red(red, nw));
    return {dg, dg.deg < 1 ? CJ_END_FINAL : CJ_END_ROUND, chan_wave && dg.deg == 0 ? c0[0] : 0u};
}

// The levels above level lvl0 (its 2^(L - lvl0) digests in A) with the
// channel jobs: the levels, then one iteration in which wave 7 runs every job
// still left (their number follows the degree, settled by then).  hook(it,
// false) runs before iteration it's barrier, hook(it, true) after it: work of
// otherwise idle waves.  The hook may assign s (the tail's late settle):
// s.job_end and s.fv are read anew in every iteration.  stamps: FRI_STAMPS builds.
struct NoHook { __device__ __forceinline__ void operator()(uint32_t, bool) const {} };
template <typename Hook = NoHook>
__device__ __forceinline__ void levels_and_channel(const LayerTask& t, bool stamps, uint4*& A, uint4*& B, uint32_t* tr,
                                                   uint32_t lvl0, Chan& c, bool chan_wave, const Settled& s,
                                                   const shaq::Role& R, SchedLds* sl, uint32_t& ord,
                                                   Hook&& hook = NoHook{}) {
    int job = !chan_wave ? CJ_END_FINAL : !c.has ? CJ_ROOT : (c.pending ? CJ_REHASH : CJ_MID);   // the first job
    const uint32_t nlev = t.L - lvl0, total = nlev + 1;
    uint32_t cnt = 1u << nlev;
#pragma unroll 1
    for (uint32_t it = 0; it < total; it++) {
        const bool level = it < nlev;
        if (level) {
            cnt >>= 1;
            level_step(t, stamps, it, A, B, tr + 8 * level_offset(t.L, lvl0 + 1 + it), cnt, R, sl, ord++);
        }
        if (chan_wave) job = chan_drain(t, job, s.job_end, level, cnt, c.cs, c.X, c.has, A, s.fv, R);
        hook(it, false);
        lds_barrier();
        hook(it, true);
        if (level) {
            uint4* tmp = A; A = B; B = tmp;
            STAMP(stamps && threadIdx.x == 0 && it < 11, 2 + it);
            STAMP_CLK(stamps && threadIdx.x == 0 && it + 1 == nlev, 18);
            STAMP(stamps && threadIdx.x == 0 && it + 1 == nlev, 19);
        }
    }
}

// Results of layer t.k (one lane of wave 7) and the hand-off to the next
// layer through three LDS words of the kernel, read after the caller's
// barrier: lds_barrier() in the tail, __syncthreads() in the batch (see
// there).  The next layer's sends follow a receive: has = pending = 1.
__device__ __forceinline__ void hand_off(const LayerTask& t, const Settled& s, Chan& c, bool chan_wave,
                                         uint32_t fbeta1, const uint4* root_lds, uint32_t& s_beta_m, uint32_t& s_active,
                                         int32_t& s_deg) {
    if (threadIdx.x == 448) {
        const RoundOut r = layer_results(t, s.dg, c.cs, s.fv, fbeta1, root_lds);
        s_beta_m = r.beta_m;
        s_active = r.active;
        s_deg = s.dg.deg;
    }
    if (chan_wave) { c.has = 1; c.pending = 1; }
}

}  // namespace fri
