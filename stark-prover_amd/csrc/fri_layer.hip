// fri_layer.hip — per-layer FRI commit pipeline on gfx950.
//
// One FRI layer k (2^L evaluations, L >= 10) is committed by a leaf launch,
// mid launches and a top launch, all gated on the device state (no host round
// trip per round); the schedule is at launch_layer:
//
//   k_layer_leaf  (2^(L-11) workgroups, L >= 19), k_layer_leaf_wide (L < 19)
//       fold of layer k-1 with beta_{k-1}      (src/fri/fri_commit.rs:53-65)
//       leaf hashes SHA256(u64_be(v))           (src/merkle/mod.rs:14-15)
//       tree levels 1..4 (2048 leaves -> 128 nodes per workgroup), wide: 1..8
//       a slice of the coefficient fold of round k-1 (fri_commit.rs:32-50)
//       with per-workgroup maxima (no hot atomics) for the exact degree
//   k_tree_mid    (levels l -> l+4, 1024 nodes in / 64 out per workgroup)
//   k_tree_mid8   (levels l -> l+8, 256 nodes in / 1 out per workgroup)
//   k_tree_top    (ONE workgroup): last <= 9 levels -> root, degree of
//       poly_k, Fiat-Shamir step (channel.rs:35-55): send(root_hex),
//       beta_k = U256(state) mod p or the final send (fri_commit.rs:114).
//   k_tree_tail   (ONE workgroup, ONE launch): all of a commit's layers of
//       <= 2^9 elements, each one whole (fold, leaves, levels, coefficient
//       fold, channel step), from the per-layer helpers of fri_tree_device.hpp
//       that the batched commit's kernels (fri_batch_kernels.hip) use too.
//
// Each thread of k_layer_leaf takes 4 consecutive leaves and folds them to one
// level-2 node in registers (no LDS, no barrier, no idle lanes); levels 3 / 4
// pair through LDS.  Its loads / stores of values are 16 B per lane.
#include <cassert>
#include "fri_tree_device.hpp"

namespace fri {

// Wave priority of the latency-bound chain kernels (tops, tail, narrow mids):
// s_setprio raises their waves over co-resident throughput waves (another
// commit lane's leaf hashing) in the SIMD's issue arbitration.  0 = off.
// Three commit lanes: 3.50 -> 3.42 ms per 2^24 commit, synchronous commits
// unchanged (3 interleaved rounds, profiles/r04_prio_*.txt).
#ifndef FRI_CHAIN_PRIO
#define FRI_CHAIN_PRIO 3
#endif
__device__ __forceinline__ void chain_prio() {
    if (FRI_CHAIN_PRIO > 0) __builtin_amdgcn_s_setprio(FRI_CHAIN_PRIO);
}

// Coefficient task of one workgroup (w of G): k == 0 -> max nonzero index
// of the input (deg_0); k >= 1 -> fold slice c'_j = c_2j + beta c_2j+1 with
// maxima of c', even part, odd part.  Results: wgmax[3w .. 3w+2].
// coef_slice: the slice over threads [t0, t0 + nthr) (whole waves), per-wave
// maxima into red[3 * (wave - t0 / 64) ..]; coef_combine (one thread, after a
// barrier): red -> wgmax.
__device__ __forceinline__ void coef_slice(const LayerTask& t, uint32_t w, uint32_t G, int32_t* red, uint32_t t0,
                                           uint32_t nthr) {
    Mx3 m;
    const uint32_t tx = threadIdx.x - t0;
    // this rank's coefficient range (all of poly_k unless sharded), split
    // evenly over the G workgroups; indices j are global
    const size_t jhi_all = t.jhi ? t.jhi : ~(size_t)0;
    if (t.k == 0) {
        // (the input is validated here, on the device, instead of by a host
        // scan before the upload)
        const size_t a = t.jlo, b = min(t.d0, jhi_all), n = b > a ? b - a : 0;
        const size_t cs = (n + G - 1) / G, lo = a + (size_t)w * cs, hi = min(b, lo + cs);
        const uint32_t* in = t.coef_in - t.ibase;
        for (size_t j = lo + tx; j < hi; j += nthr) {
            const uint32_t c = in[j];
            if (c) m.m0 = max(m.m0, (int)j);
            if (c >= P) m.m1 = 0;
        }
    } else {
        const DevState* st = t.st;
        const size_t len = (size_t)(st->deg[t.k - 1] + 1), nlen = (len + 1) / 2;
        const uint32_t beta_m = st->beta_mont[t.k - 1];
        const size_t a = t.jlo, b = min(nlen, jhi_all), n = b > a ? b - a : 0;
        const size_t cs = (n + G - 1) / G, lo = a + (size_t)w * cs, hi = min(b, lo + cs);
        const uint32_t* in = t.coef_in - t.ibase;
        uint32_t* outp = t.coef_out - t.obase;
        for (size_t j = lo + tx; j < hi; j += nthr) {
            uint32_t e = in[2 * j];
            uint32_t o = (2 * j + 1 < len) ? in[2 * j + 1] : 0u;
            uint32_t v = add(e, mmul(o, beta_m));
            outp[j] = v;
            if (v) m.m0 = (int)j;
            if (e) m.m1 = (int)j;
            if (o) m.m2 = (int)j;
        }
    }
    mx3_wave_to_red(m, red, tx);
}
__device__ __forceinline__ void coef_combine(const LayerTask& t, uint32_t w, const int32_t* red, uint32_t nw) {
    mx3_from_red(red, nw).store(t.wgmax, w);
}
__device__ __forceinline__ void coef_task(const LayerTask& t, uint32_t w, uint32_t G, int32_t* red /*LDS [3*waves]*/) {
    coef_slice(t, w, G, red, 0, blockDim.x);
    lds_barrier();          // red[] only: the leaf digest stores need not drain here
    if (threadIdx.x == 0) coef_combine(t, w, red, blockDim.x / 64);
}

// Four consecutive leaves per thread -> level 2 node; lv0 / lv1 are the
// layer's level 0 / 1 arrays.  All four leaves first: the thread's 128
// contiguous level-0 bytes are written together (no partly written line waits
// in L2 for its other half), and so are its two level-1 digests.
__device__ __forceinline__ void quad(const uint4& vals, uint32_t* lv0, uint32_t* lv1, size_t q /*quad index*/,
                                     Dg& out) {
    Dg a, b, c, d, n0, n1;
    hleaf(vals.x, a); hleaf(vals.y, b); hleaf(vals.z, c); hleaf(vals.w, d);
    dg_store(lv0 + 8 * (4 * q), a); dg_store(lv0 + 8 * (4 * q + 1), b);
    dg_store(lv0 + 8 * (4 * q + 2), c); dg_store(lv0 + 8 * (4 * q + 3), d);
    hnode(a, b, n0);
    hnode(c, d, n1);
    dg_store(lv1 + 8 * (2 * q), n0);
    dg_store(lv1 + 8 * (2 * q + 1), n1);
    hnode(n0, n1, out);
}

// Levels l+3, l+4 through LDS: TPB level-(l+2) nodes -> TPB/2 -> TPB/4.
template <uint32_t TPB>
__device__ __forceinline__ void lds_two_levels(uint4* lds, const Dg& mine, uint32_t* lv2, uint32_t* lv3, uint32_t* lv4,
                                               size_t g2 /*first level-(l+2) index of this WG*/) {
    uint4* A = lds;             // TPB digests
    uint4* B = lds + 2 * TPB;   // TPB/2 digests
    const uint32_t t = threadIdx.x;
    dg_store(lv2 + 8 * (g2 + t), mine);
    dg_lds_store(A + 2 * t, mine);
    lds_barrier();
    if (t < TPB / 2) {
        Dg l, r, o;
        dg_lds_load(A + 4 * t, l); dg_lds_load(A + 4 * t + 2, r);
        hnode(l, r, o);
        dg_lds_store(B + 2 * t, o);
        dg_store(lv3 + 8 * (g2 / 2 + t), o);
    }
    lds_barrier();
    if (t < TPB / 4) {
        Dg l, r, o;
        dg_lds_load(B + 4 * t, l); dg_lds_load(B + 4 * t + 2, r);
        hnode(l, r, o);
        dg_store(lv4 + 8 * (g2 / 4 + t), o);
    }
}

__device__ __forceinline__ bool gated_off(const LayerTask& t) {
    return t.gst && t.gidx >= 0 && !t.gst->active[t.gidx];
}

// PAIR: a sharded block tree with the pair fold fused in (LayerTask::prev2),
// launched as a part of the layer's workgroups (wg_base).
__device__ __forceinline__ uint32_t pair_beta(const LayerTask& t) { return t.gst->beta_mont[t.gidx]; }

// TPB threads, 4 leaves each: 4*TPB leaves -> TPB/4 level-4 nodes per WG.
template <bool FOLD, bool COMMIT, uint32_t TPB, bool PAIR = false>
__global__ __launch_bounds__(TPB) void k_layer_leaf(LayerTask t) {
    if (gated_off(t)) return;
    __shared__ uint4 lds[3 * TPB];
    __shared__ int32_t red[3 * (TPB / 64)];
    const uint32_t L = t.L;
    const size_t wg = PAIR ? (size_t)blockIdx.x + t.wg_base : (size_t)blockIdx.x;
    const size_t q = wg * TPB + threadIdx.x;   // quad index: leaves 4q..4q+3
    uint4 v;
    if (FOLD) {
        const size_t half = (size_t)1 << L;
        const uint32_t beta_m = COMMIT ? t.st->beta_mont[t.k - 1] : (PAIR ? pair_beta(t) : t.beta_m);
        uint4 a = reinterpret_cast<const uint4*>(t.prev)[q];
        uint4 b = reinterpret_cast<const uint4*>(PAIR ? t.prev2 : t.prev + half)[q];
        uint4 x = reinterpret_cast<const uint4*>(t.xinv)[q];
        v.x = fold_one(a.x, b.x, x.x, beta_m); v.y = fold_one(a.y, b.y, x.y, beta_m);
        v.z = fold_one(a.z, b.z, x.z, beta_m); v.w = fold_one(a.w, b.w, x.w, beta_m);
        reinterpret_cast<uint4*>(t.values)[q] = v;
    } else {
        v = reinterpret_cast<const uint4*>(t.values)[q];
    }
    uint32_t* tr = t.tree;
    Dg top;
    quad(v, tr + 8 * level_offset(L, 0), tr + 8 * level_offset(L, 1), q, top);
    if (COMMIT) coef_task(t, blockIdx.x, gridDim.x, red);
    lds_two_levels<TPB>(lds, top, tr + 8 * level_offset(L, 2), tr + 8 * level_offset(L, 3),
                        tr + 8 * level_offset(L, 4), wg * TPB);
}

// Levels of the wide leaf kernel with fewer than WIDE_PAIR_MAX nodes in the
// whole layer are latency-bound: they use the lane-pair node.
#ifndef WIDE_PAIR_MAX
#define WIDE_PAIR_MAX (1u << 16)
#endif

// Tree levels the wide leaf kernel builds: all 8 of its 256-leaf subtree when
// the rest of the layer then fits the single-workgroup top (no mid launch).
__host__ __device__ __forceinline__ uint32_t wide_levels(uint32_t L) { return L <= 8 + TOP_LOG ? 8u : 4u; }

// Wide leaf kernel for narrow layers (2^10 .. 2^18 elements): one leaf per
// lane, 256 leaves per workgroup, levels 1..4 through LDS (one node per lane
// per level): latency 1 leaf + 4 nodes instead of the quad form's 4 + 5.
template <bool FOLD, bool COMMIT, bool PAIR = false>
__global__ __launch_bounds__(256) void k_layer_leaf_wide(LayerTask t) {
    if (gated_off(t)) return;
    STAMP(COMMIT && blockIdx.x == 0 && threadIdx.x == 0, 60);
    __shared__ uint4 lds[2 * 256 + 2 * 128];
    __shared__ int32_t red[12];
    __shared__ SchedLds sl;
    sched_init(&sl);
    const uint32_t L = t.L;
    const size_t wg = PAIR ? (size_t)blockIdx.x + t.wg_base : (size_t)blockIdx.x;
    const size_t grid = PAIR ? (size_t)t.wg_total : (size_t)gridDim.x;   // the whole layer's workgroups
    const size_t i = wg * 256 + threadIdx.x;
    uint32_t v;
    if (FOLD) {
        const size_t half = (size_t)1 << L;
        const uint32_t beta_m = COMMIT ? t.st->beta_mont[t.k - 1] : (PAIR ? pair_beta(t) : t.beta_m);
        v = fold_one(t.prev[i], PAIR ? t.prev2[i] : t.prev[i + half], t.xinv[i], beta_m);
        t.values[i] = v;
    } else {
        v = t.values[i];
    }
    uint32_t* tr = t.tree;
    Dg d;
    cleaf(v, d);       // looped form: its ~2 KB of code costs less cold than the unrolled leaf saves (A/B -0.6%)
    dg_store(tr + 8 * i, d);
    uint4* A = lds;
    uint4* B = lds + 2 * 256;
    dg_lds_store(A + 2 * threadIdx.x, d);
    lds_barrier();
    STAMP(COMMIT && blockIdx.x == 0 && threadIdx.x == 0, 61);
    uint32_t cnt = 256;
    const shaq::Role qr = shaq::role_of(threadIdx.x);
    if (grid * 128 < WIDE_PAIR_MAX) chain_prio();   // from level 1 on, all on lane pairs
    const uint32_t nlev = wide_levels(L);
#pragma unroll 1
    for (uint32_t j = 1; j <= nlev; j++) {
        cnt >>= 1;
        uint32_t* out = tr + 8 * (level_offset(L, j) + (wg << (8 - j)));
        if ((size_t)cnt * grid < WIDE_PAIR_MAX) {
            pair_level_s(A, B, out, threadIdx.x, cnt, qr, &sl, j);   // latency-bound level: node per lane pair
        } else if (threadIdx.x < cnt) {
            Dg a, b, o;
            dg_lds_load(A + 4 * threadIdx.x, a);
            dg_lds_load(A + 4 * threadIdx.x + 2, b);
            hnode(a, b, o);
            dg_lds_store(B + 2 * threadIdx.x, o);
            dg_store(out + 8 * threadIdx.x, o);
        }
        // the coefficient slice (needed only by the layer's top kernel) on
        // waves 2-3, idle from level 2 on: off the tree's critical path
        if (COMMIT && j == 2 && threadIdx.x >= 128) coef_slice(t, blockIdx.x, gridDim.x, red, 128, 128);
        lds_barrier();
        uint4* tmp = A; A = B; B = tmp;
    }
    if (COMMIT && threadIdx.x == 128) coef_combine(t, blockIdx.x, red, 2);   // nlev >= 4: red[] settled
    STAMP(COMMIT && blockIdx.x == 0 && threadIdx.x == 0, 62);
}

// Reduce the coefficient-maxima triples of the R producer workgroups of this
// workgroup's inputs (R <= 64) into one triple (wave 0).
__device__ __forceinline__ void reduce_mx(const int32_t* in, int32_t* out, uint32_t w, uint32_t R) {
    if (threadIdx.x >= 64) return;
    Mx3 m;
    if (threadIdx.x < R) m.load(in, R * w + threadIdx.x);
    m.wave_max();
    if (threadIdx.x == 0) m.store(out, w);
}

// Mid tree of the wide levels: NIN = 1024 level-l nodes per workgroup (512
// threads) -> 64 level-(l+4) nodes, one node per lane per level.
__global__ __launch_bounds__(512) void k_tree_mid(uint32_t* tree, uint32_t L, uint32_t l, const DevState* st,
                                                  int gate, const int32_t* mx_in, int32_t* mx_out, uint32_t R) {
    if (st && gate >= 0 && !st->active[gate]) return;
    constexpr uint32_t NIN = 1024;
    // level 1 reads its two inputs straight from HBM (64 contiguous bytes per
    // thread), so LDS holds only levels 1.. (NIN/2 + NIN/4 digests): more
    // workgroups per CU
    __shared__ uint4 lds[NIN + NIN / 2];
    __shared__ SchedLds sl;
    sched_init(&sl);
    uint4* A = lds;
    uint4* B = lds + NIN;
    const uint32_t t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * NIN;
    const uint32_t* in = tree + 8 * level_offset(L, l);
    {
        Dg a, b, o;
        dg_load(in + 8 * (base + 2 * t), a);
        dg_load(in + 8 * (base + 2 * t + 1), b);
        if (mx_in) reduce_mx(mx_in, mx_out, blockIdx.x, R);
        hnode(a, b, o);
        dg_lds_store(A + 2 * t, o);
        dg_store(tree + 8 * (level_offset(L, l + 1) + (base >> 1) + t), o);
    }
    lds_barrier();
    const shaq::Role qr = shaq::role_of(t);
    uint32_t cnt = NIN / 2;
#pragma unroll 1
    for (uint32_t j = 2; j <= 4; j++) {
        cnt >>= 1;
        uint32_t* out = tree + 8 * (level_offset(L, l + j) + (base >> j));
        // lane pairs only where the whole level is narrow: a lane-pair node
        // issues 1744 instructions on two lanes, a per-lane node 2290 on one,
        // and levels of >= 2^16 nodes are issue-bound
        const bool narrow = (size_t)cnt * gridDim.x < WIDE_PAIR_MAX;
        if (narrow) {
            pair_level_s(A, B, out, t, cnt, qr, &sl, j);   // narrow: latency-bound
        } else if (t < cnt) {
            Dg a, b, o;
            dg_lds_load(A + 4 * t, a);
            dg_lds_load(A + 4 * t + 2, b);
            hnode(a, b, o);
            dg_lds_store(B + 2 * t, o);
            dg_store(out + 8 * t, o);
        }
        lds_barrier();
        uint4* tmp = A; A = B; B = tmp;
    }
}

// Eight tree levels in one launch for the narrow part of a large layer:
// 256 level-l digests per workgroup -> 1 level-(l+8) digest, every level on
// lane pairs (level 1 reads its children straight from HBM).  Against two
// four-level launches: one kernel boundary, one HBM round trip of the
// level-(l+4) digests and one cold start less per layer.
__global__ __launch_bounds__(256) void k_tree_mid8(uint32_t* tree, uint32_t L, uint32_t l, const DevState* st,
                                                   int gate, const int32_t* mx_in, int32_t* mx_out, uint32_t R) {
    if (st && gate >= 0 && !st->active[gate]) return;
    chain_prio();
    __shared__ uint4 lds[256 + 128];
    __shared__ SchedLds sl;
    sched_init(&sl);
    uint4* A = lds;
    uint4* B = lds + 256;
    const uint32_t t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * 256;
    const uint32_t* in = tree + 8 * level_offset(L, l);
    const shaq::Role qr = shaq::role_of(t);
    {
        const uint32_t q = t >> 1, half = (t & 1u) ^ 1u;
        Dg a, b;
        dg_load(in + 8 * (base + 2 * q), a);
        dg_load(in + 8 * (base + 2 * q + 1), b);
        if (mx_in) reduce_mx(mx_in, mx_out, blockIdx.x, R);
        uint32_t o[4];
        shaq::node(a.w, b.w, o, qr);
        const uint4 v = make_uint4(o[0], o[1], o[2], o[3]);
        A[2 * q + half] = v;
        reinterpret_cast<uint4*>(tree + 8 * (level_offset(L, l + 1) + (base >> 1) + q))[half] = v;
    }
    lds_barrier();
    uint32_t cnt = 128;
#pragma unroll 1
    for (uint32_t j = 2; j <= 8; j++) {
        cnt >>= 1;
        pair_level_s(A, B, tree + 8 * (level_offset(L, l + j) + (base >> j)), t, cnt, qr, &sl, j);
        lds_barrier();
        uint4* tmp = A; A = B; B = tmp;
    }
}

// ---------------------------------------------------------------- top ----
// One workgroup.  FROM_LEAVES (a standalone tree of N = 2^L <= 2^TOP_LOG
// values, never COMMIT: a commit's small layers run in k_tree_tail): leaves
// and all levels here.  Otherwise: N = 2^(L-l) <= 1024 level-l digests -> root.
// COMMIT: the degree of poly_k is reduced up front (its inputs are complete
// at launch); wave 7 runs the channel jobs (chan_job) during the levels whose
// nodes fit waves 0-2, then after the root, in an extra iteration of the
// level loop (uniform barrier count).
// SHARD (coset-sharded layers, run_commit_sharded; never FROM_LEAVES):
//   !COMMIT: the top of this rank's block tree; it also writes the rank's
//            per-layer record (t.shard->rec_out: block root, the maxima of
//            its coefficient slice reduced from rec_R workgroup triples, its
//            first coefficient), which the ranks then all-gather;
//   COMMIT:  the replicated top of the layer: its N = G inputs are the block
//            roots in the all-gathered records (rank order, permuted to block
//            order and stored as the top tree's level 0), the maxima and the
//            final-value candidate (rank 0's first coefficient) too.
template <bool FROM_LEAVES, bool COMMIT, bool SHARD = false>
__global__ __launch_bounds__(512) void k_tree_top(LayerTask t, uint32_t l, const int32_t* mx, uint32_t G) {
    static_assert(!(FROM_LEAVES && (COMMIT || SHARD)), "from the leaves: standalone trees only");
    if (gated_off(t)) return;
    chain_prio();
    __shared__ uint4 lds[2 * 1024 + 2 * 512];
    __shared__ int32_t red[24];
    __shared__ SchedLds sl;
    sched_init(&sl);
    const uint32_t L = t.L;
    const uint32_t N = 1u << (L - l);
    const uint32_t tid = threadIdx.x;

    const bool chan_wave = COMMIT && tid >= 448;
    DevState* st = t.st;
    uint32_t cs[8], X[4];
    uint32_t has = 0, fbeta1 = 0;
    int job = CJ_END_FINAL;
    if (chan_wave) {
        // every channel field in one round trip: no load waits on another's
        // value (the wave reaches the inputs' barrier after this, so a chain
        // of dependent loads here delays every wave of the launch)
#pragma unroll
        for (int i = 0; i < 8; i++) cs[i] = st->chan[i];
        const uint32_t h = st->chan_has, pend = st->chan_pending;
        // the test hook's beta, loaded now rather than after the root
        const uint32_t fo = COMMIT ? st->forced : 0u, fb = st->forced_beta[t.k < MAXR ? t.k : 0];
        has = h;
        job = !h ? CJ_ROOT : (pend ? CJ_REHASH : CJ_MID);
        if (fo && t.k < MAXR) fbeta1 = fb + 1u;
    }
    // wave 6 pulls the compact-SHA constant tables into the scalar cache
    // while the inputs load (cold misses inside level 1 and the channel otherwise)
    if (tid >= 384 && tid < 448) kcache_touch_sha_tables();
    uint4* A = lds;
    uint4* B = lds + 2 * 1024;
    uint32_t* tr = t.tree;
    STAMP(COMMIT && tid == 0, 0);
    if (FROM_LEAVES) {
        leaf_loop(N, tr, A, [&](uint32_t j, bool) { return t.values[j]; });
    } else if (SHARD && COMMIT) {
        const ShardTop& sh = *t.shard;
        for (uint32_t i = tid; i < N; i += blockDim.x) {
            Dg d;
            dg_load(sh.recs_in + REC_WORDS * sh.rank_of_block[i], d);
            dg_lds_store(A + 2 * i, d);
            dg_store(tr + 8 * i, d);               // level 0 of the top tree (decommitment paths)
        }
        Mx3 m;
        if (tid < sh.G) {
            m.load(reinterpret_cast<const int32_t*>(sh.recs_in + REC_WORDS * tid + 8), 0);
            if (sh.sched_on) { m.m0 = sh.sched_deg; m.m1 = t.k == 0 ? -1 : 0; m.m2 = -1; }   // loopback rehearsal
        }
        mx3_wave_to_red(m, red, tid);
    } else {
        const uint32_t* in = tr + 8 * level_offset(L, l);
        // the producers' maxima are loaded before the digests are waited
        // for: both round trips overlap (G <= 512 triples, one per thread)
        Mx3 m;
        if (COMMIT && tid < G) m.load(mx, tid);
        for (uint32_t i = tid; i < N; i += blockDim.x) {
            Dg d;
            dg_load(in + 8 * i, d);
            dg_lds_store(A + 2 * i, d);
        }
        if (SHARD && !COMMIT) {                    // this rank's coefficient-slice maxima
            const ShardTop& sh = *t.shard;
            for (uint32_t i = tid; i < sh.rec_R; i += blockDim.x) m.take(sh.rec_mx, i);
            mx3_wave_to_red(m, red, tid);
        }
        if (COMMIT) {                              // producer maxima -> per-wave triples
            for (uint32_t i = tid + blockDim.x; i < G; i += blockDim.x) m.take(mx, i);
            mx3_wave_to_red(m, red, tid);
        }
    }
    lds_barrier();
    // ---- degree of poly_k, uniform ----
    const Degree dg = COMMIT ? degree_of(t.k, mx3_from_red(red, 8)) : Degree{-1, false};
    const bool is_final = COMMIT && dg.deg < 1;
    const int job_end = is_final ? CJ_END_FINAL : CJ_END_ROUND;
    uint32_t fv = 0;                               // fri_commit.rs:109-113
    if (chan_wave && is_final && dg.deg == 0)
        fv = SHARD ? t.shard->recs_in[11] : (t.k == 0 ? t.coef_in : t.coef_out)[0];
    STAMP(COMMIT && tid == 0, 1);
    STAMP_CLK(COMMIT && tid == 0, 17);
    // iterations: the levels, then one in which wave 7 runs every channel
    // job still left (no barrier between the post-root jobs)
    const uint32_t nlev = L - l;
    const uint32_t total = nlev + (COMMIT ? 1u : 0u);
    const shaq::Role R = shaq::role_of(tid);
    uint32_t cnt = N;
#pragma unroll 1
    for (uint32_t it = 0; it < total; it++) {
        const bool level = it < nlev;
        if (level) {
            cnt >>= 1;
            level_step(t, COMMIT, it, A, B, tr + 8 * level_offset(L, l + 1 + it), cnt, R, &sl, it);
        }
        if (chan_wave) job = chan_drain(t, job, job_end, level, cnt, cs, X, has, A, fv, R);
        lds_barrier();
        if (level) {
            uint4* tmp = A; A = B; B = tmp;
            STAMP(COMMIT && tid == 0 && it < 11, 2 + it);
            STAMP_CLK(COMMIT && tid == 0 && it + 1 == nlev, 18);
            STAMP(COMMIT && tid == 0 && it + 1 == nlev, 19);
        }
    }
    if (SHARD && !COMMIT && tid == 448) {          // this rank's record
        const ShardTop& sh = *t.shard;
        const Mx3 m = mx3_from_red(red, 8);
        Dg root;
        dg_lds_load(A, root);
        uint32_t* rec = sh.rec_out;
        dg_store(rec, root);
        reinterpret_cast<uint4*>(rec)[2] = make_uint4((uint32_t)m.m0, (uint32_t)m.m1, (uint32_t)m.m2, sh.rec_c0[0]);
        reinterpret_cast<uint4*>(rec)[3] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (COMMIT && tid == 448) layer_results(t, dg, cs, fv, fbeta1, A);
}

// ------------------------------------------------------------- tail ----
// The last layers of a commit (2^L <= 2^TAIL_LOG elements each) in ONE
// workgroup and ONE launch: per layer the fold, the leaves, the coefficient
// fold, the degree, the tree levels and the channel step (the helpers above),
// with the layer values, the coefficients, beta, the degree and the gate
// handed to the next layer through LDS.  Saves per layer a kernel boundary,
// the HBM round trip of the folded values and coefficients, and the cold first
// level of a fresh workgroup.  The channel state stays in wave 7's registers.
struct TailTask {
    LayerTask t[TAIL_LOG + 1];  // consecutive layers k0 .. k0 + n - 1 (commit mode)
    uint32_t n;
};

template <bool FOLD0>
__global__ __launch_bounds__(512) void k_tree_tail(TailTask tt) {
    const LayerTask& t0 = tt.t[0];
    if (gated_off(t0)) return;
    chain_prio();
    constexpr uint32_t NMAX = 1u << TAIL_LOG;
    __shared__ uint4 lds[2 * NMAX + NMAX];
    __shared__ uint32_t vals[2][NMAX];         // this / previous layer's values
    __shared__ uint32_t coefs[2][NMAX];        // this / previous round's polynomial
    __shared__ int32_t red[24];
    __shared__ uint32_t s_beta_m, s_active;      // hand_off
    __shared__ int32_t s_deg;
    __shared__ uint32_t s_fbeta[TAIL_LOG + 2];   // the test hook's betas of these layers (chan_open)
    __shared__ uint32_t xv[2 * NMAX];            // every layer's x^-1 table (prefetched)
    __shared__ SchedLds sl;
    sched_init(&sl);
    uint32_t ord = 0;                            // levels so far (schedule producer flag)
    const uint32_t tid = threadIdx.x;
    const bool chan_wave = tid >= 448;
    DevState* st = t0.st;
    // The x^-1 tables of layers 1.. are loaded into LDS by wave 6 during the
    // first layer's levels (one HBM latency for the launch, off the chain,
    // instead of one per layer fold); layer 0 folds from HBM.
    auto prefetch_x = [&](uint32_t t0p, uint32_t nthr) {
        uint32_t off = 1u << tt.t[0].L;
        for (uint32_t li = 1; li < tt.n; li++) {
            const uint32_t N = 1u << tt.t[li].L;
            for (uint32_t j = tid - t0p; j < N; j += nthr) xv[off + j] = tt.t[li].xinv[j];
            off += N;
        }
    };
    Chan ch;
    chan_open(ch, st, chan_wave, s_fbeta, tt.n + 1, t0.k);
    uint32_t beta_m = FOLD0 ? st->beta_mont[t0.k - 1] : 0u;
    int prev_deg = FOLD0 ? st->deg[t0.k - 1] : -1;
    const shaq::Role R = shaq::role_of(tid);
    uint32_t xoff = 0;
#pragma unroll 1
    for (uint32_t li = 0; li < tt.n; li++) {
        const LayerTask& t = tt.t[li];
        const int k = t.k;
        const uint32_t L = t.L, N = 1u << L;
        const uint32_t* xl = li ? xv + xoff : t.xinv;
        xoff += N;
        uint32_t* cur_c = coefs[li & 1];
        uint4* A = lds;
        uint4* B = lds + 2 * NMAX;
        STAMP(tid == 0, 0);
        // ---- fold + leaves: layer li >= 1 folds the values kept in LDS ----
        folded_leaves(N, t.tree, A, FOLD0 || li > 0, li > 0, vals[(li & 1) ^ 1], t.prev, xl, beta_m, t.values,
                      vals[li & 1]);
        // ---- coefficient fold of round k-1 (or the input scan at k == 0) ----
        // Needed only for the degree, i.e. from the root on: it runs on waves
        // 4-5 (threads [256, 384)) during the first level iteration that
        // leaves them idle (coef_it), unless the layer has no such level.
        const uint32_t coef_it = N > 256 ? 1u : 0u;   // iteration 0 of a 512-leaf layer uses all waves
        const bool coef_late = L > coef_it;
        const uint32_t* c0 = k == 0 ? t.coef_in : cur_c;
        auto coef = [&](uint32_t t0c, uint32_t nthr) {   // poly_{k-1} is in LDS where this kernel folded it
            if (k == 0) coef_scan(t.coef_in, (uint32_t)t.d0, red, t0c, nthr);
            else coef_fold(li > 0 && k >= 2, coefs[(li & 1) ^ 1], t.coef_in, cur_c, (uint32_t)(prev_deg + 1), beta_m,
                           red, t0c, nthr);
        };
        if (!coef_late) coef(0, blockDim.x);
        if (li == 0 && !coef_late) prefetch_x(0, blockDim.x);
        lds_barrier();
        STAMP(tid == 0, 1);
        STAMP_CLK(tid == 0, 17);
        Settled s{{1, false}, CJ_END_ROUND, 0u};      // provisional while the degree is pending
        if (!coef_late) s = settle(k, red, 8, chan_wave, c0);
        levels_and_channel(t, true, A, B, t.tree, 0, ch, chan_wave, s, R, &sl, ord, [&](uint32_t it, bool after) {
            if (!coef_late || it != coef_it) return;
            if (after) {
                s = settle(k, red, 2, chan_wave, c0);
            } else if (tid >= 256 && tid < 384) {
                coef(256, 128);
            } else if (li == 0 && tid >= 384 && tid < 448) {
                prefetch_x(384, 64);
            }
        });
        hand_off(t, s, ch, chan_wave, s_fbeta[li], A, s_beta_m, s_active, s_deg);
        lds_barrier();                                   // the tail's layers hand over through LDS alone
        if (!s_active) break;                            // uniform
        beta_m = s_beta_m;
        prev_deg = s_deg;
    }
}

// ------------------------------------------------------------ launcher ----
// Layer schedule of launch_layer (D = L - l: log2 of the nodes still to climb):
//   L <= 9 : one k_tree_top from the leaves (standalone trees only; a commit
//            sends these layers to launch_tail).
//   L >= 19: k_layer_leaf (2048 leaves/WG, levels 1..4);  10..18:
//            k_layer_leaf_wide (256 leaves/WG, levels 1..8, or 1..4 at L == 18)
//   then k_tree_mid (4 levels) while D >= 18, one k_tree_mid8 (8 levels) if
//   D > 9 is left, and k_tree_top on the last <= 512 nodes.
// After the leaf kernel D is <= 9 (L <= 17), 14 (L == 18) or L - 4 >= 15, and
// k_tree_mid takes D from >= 18 to >= 14: the loop never sees 10 <= D <= 13,
// so one k_tree_mid8 always leaves 6 <= D <= 9 for the top.
//
// k_tree_top instantiations <FROM_LEAVES, COMMIT, SHARD> and who reaches them:
//   <true,  false>        fri_merkle_root, fri_trace_commit with L <= 9 (no prev, no st)
//   <false, false>        the same two callers with L >= 10
//   <false, false, true>  run_commit_sharded's block trees (st null, shard set): L = log2 block >= 10
//   <false, true>         enqueue_commit and the sharded local tail, layers of L >= 10
//   <false, true,  true>  launch_top: the replicated top of a sharded layer
// Not built: from the leaves in commit mode (both commit drivers send every
// layer of L <= TAIL_LOG == TOP_LOG to launch_tail) and from the leaves with
// a fold outside a commit (only the sharded block trees fold without st, and
// next_layer_sharded keeps their blocks at >= 2^10 elements).
static LayerTask with_gate(const LayerTask& in) {
    LayerTask t = in;
    if (t.st) { t.gst = t.st; t.gidx = t.k > 0 ? t.k - 1 : -1; }
    return t;
}

#ifndef QUAD_TPB
#define QUAD_TPB 512         // quad leaf kernel: threads per WG (2048 leaves per WG; A/B: 512 beats 256 by ~0.5-1%, 128 and 1024 slower)
#endif
#ifndef QUAD_MIN_LOG
#define QUAD_MIN_LOG 19      // smaller layers: one leaf per lane (A/B: 19 beats 20 and 21)
#endif

// A fused sharded block tree's leaf kernel (PAIR): the layer's G workgroups
// as two launches of G/2, the half-block the next exchange sends first, with
// after_part1 in between (a single launch without it).
template <typename KernelLaunch>
static void pair_parts(LayerTask t, uint32_t G, hipStream_t s, const std::function<void()>& after_part1,
                       KernelLaunch&& go) {
    t.wg_total = G;
    if (!after_part1) {
        t.wg_base = 0;
        go(t, G);
        return;
    }
    const uint32_t h = G / 2;
    t.wg_base = t.send_half ? h : 0u;
    go(t, h);
    after_part1();
    t.wg_base = t.send_half ? 0u : h;
    go(t, h);
}

void launch_layer(const LayerTask& tin, hipStream_t s, hipEvent_t ev_leaf_end, const std::function<void()>& after_leaf,
                  hipEvent_t ev_before_top, const std::function<void()>& after_part1) {
    const LayerTask t = with_gate(tin);
    const uint32_t L = t.L;
    const bool fold = t.prev != nullptr;
    const bool commit = t.st != nullptr;
    const bool pair = t.prev2 != nullptr;          // sharded block tree, pair fold fused (never commit mode)
    const int32_t* nomx = nullptr;
    static_assert(TAIL_LOG == TOP_LOG, "every commit layer the top could take from its leaves goes to launch_tail");
    if (L <= TOP_LOG) {
        assert(!fold && !commit);                  // see the reachability table above
        hipLaunchKernelGGL((k_tree_top<true, false>), dim3(1), dim3(512), 0, s, t, 0u, nomx, 1u);
        if (ev_leaf_end) hipEventRecord(ev_leaf_end, s);
        return;
    }
    uint32_t G, out_per_wg;
    if (L >= QUAD_MIN_LOG) {
        constexpr uint32_t TPB = QUAD_TPB;
        G = (uint32_t)(((size_t)1 << L) / (4 * TPB));
        out_per_wg = TPB / 4;
        if (pair) {
            pair_parts(t, G, s, after_part1, [&](const LayerTask& tp, uint32_t g) {
                hipLaunchKernelGGL((k_layer_leaf<true, false, TPB, true>), dim3(g), dim3(TPB), 0, s, tp);
            });
        } else if (fold) {
            if (commit) hipLaunchKernelGGL((k_layer_leaf<true, true, TPB>), dim3(G), dim3(TPB), 0, s, t);
            else hipLaunchKernelGGL((k_layer_leaf<true, false, TPB>), dim3(G), dim3(TPB), 0, s, t);
        } else {
            if (commit) hipLaunchKernelGGL((k_layer_leaf<false, true, TPB>), dim3(G), dim3(TPB), 0, s, t);
            else hipLaunchKernelGGL((k_layer_leaf<false, false, TPB>), dim3(G), dim3(TPB), 0, s, t);
        }
    } else {
        G = 1u << (L - 8);
        out_per_wg = 256u >> wide_levels(L);
        if (pair) {
            pair_parts(t, G, s, after_part1, [&](const LayerTask& tp, uint32_t g) {
                hipLaunchKernelGGL((k_layer_leaf_wide<true, false, true>), dim3(g), dim3(256), 0, s, tp);
            });
        } else if (fold) {
            if (commit) hipLaunchKernelGGL((k_layer_leaf_wide<true, true>), dim3(G), dim3(256), 0, s, t);
            else hipLaunchKernelGGL((k_layer_leaf_wide<true, false>), dim3(G), dim3(256), 0, s, t);
        } else {
            if (commit) hipLaunchKernelGGL((k_layer_leaf_wide<false, true>), dim3(G), dim3(256), 0, s, t);
            else hipLaunchKernelGGL((k_layer_leaf_wide<false, false>), dim3(G), dim3(256), 0, s, t);
        }
    }
    if (ev_leaf_end) hipEventRecord(ev_leaf_end, s);
    if (after_leaf) after_leaf();
    const int gate = t.gidx;
    // coefficient maxima: level 0 at wgmax[0 .. 3G); each mid reduces R producers per WG
    const int32_t* mx = commit ? t.wgmax : nullptr;
    size_t mx_off = 3 * (size_t)G;
    uint32_t l = L >= QUAD_MIN_LOG ? 4u : wide_levels(L);
    while (L - l > TOP_LOG) {
        const size_t nodes = (size_t)1 << (L - l);
        // eight narrow levels in one launch once the level has < 2^18 nodes
        const bool eight = nodes < ((size_t)1 << 18);
        assert(!eight || L - l >= 8 + 6);          // see the schedule above
        const uint32_t nin = eight ? 256u : 1024u;
        const uint32_t grid = (uint32_t)(nodes / nin);
        const uint32_t R = nin / out_per_wg;
        int32_t* mx_out = commit ? t.wgmax + mx_off : nullptr;
        if (eight)
            hipLaunchKernelGGL(k_tree_mid8, dim3(grid), dim3(256), 0, s, t.tree, L, l, t.gst, gate, mx, mx_out, R);
        else
            hipLaunchKernelGGL(k_tree_mid, dim3(grid), dim3(512), 0, s, t.tree, L, l, t.gst, gate, mx, mx_out, R);
        if (commit) { mx = mx_out; mx_off += 3 * (size_t)grid; }
        G = grid;
        out_per_wg = eight ? 1u : nin / 16;
        l += eight ? 8u : 4u;
    }
    if (ev_before_top) hipStreamWaitEvent(s, ev_before_top, 0);
    if (commit) hipLaunchKernelGGL((k_tree_top<false, true>), dim3(1), dim3(512), 0, s, t, l, mx, G);
    else if (t.shard) hipLaunchKernelGGL((k_tree_top<false, false, true>), dim3(1), dim3(512), 0, s, t, l, nomx, G);
    else hipLaunchKernelGGL((k_tree_top<false, false>), dim3(1), dim3(512), 0, s, t, l, nomx, G);
}

void launch_tail(const LayerTask* ts, uint32_t n, hipStream_t s) {
    TailTask tt{};
    tt.n = n;
    for (uint32_t i = 0; i < n; i++) tt.t[i] = ts[i];
    tt.t[0] = with_gate(ts[0]);
    if (ts[0].prev) hipLaunchKernelGGL((k_tree_tail<true>), dim3(1), dim3(512), 0, s, tt);
    else hipLaunchKernelGGL((k_tree_tail<false>), dim3(1), dim3(512), 0, s, tt);
}

__global__ __launch_bounds__(256) void k_coef(LayerTask t) {
    if (gated_off(t)) return;
    __shared__ int32_t red[12];
    coef_task(t, blockIdx.x, gridDim.x, red);
}

void launch_coef(const LayerTask& tin, uint32_t G, hipStream_t s) {
    const LayerTask t = with_gate(tin);
    hipLaunchKernelGGL(k_coef, dim3(G), dim3(256), 0, s, t);
}

void launch_top(const LayerTask& tin, uint32_t l, const int32_t* mx, uint32_t G, hipStream_t s) {
    const LayerTask t = with_gate(tin);
    if (t.shard) hipLaunchKernelGGL((k_tree_top<false, true, true>), dim3(1), dim3(512), 0, s, t, l, mx, G);
    else hipLaunchKernelGGL((k_tree_top<false, true>), dim3(1), dim3(512), 0, s, t, l, mx, G);
}

}  // namespace fri
