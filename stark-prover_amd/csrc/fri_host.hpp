// fri_host.hpp — host-side state of libfri_amd.so, shared by the translation
// units of the C ABI (include/fri_amd.h).  One file per concern:
//   fri_ctx.hip        context lifetime, profiling spans, diagnostics
//   fri_ops.hip        kernel-level entry points: batch inverse, LDE,
//                      interpolation, fold, Merkle root; the direct kernels of
//                      arbitrary-point interpolation and evaluation
//   fri_poly.hip       polynomial arithmetic: mul, div_rem, compose
//   fri_roots.hip      polynomial from roots (product tree), Lagrange basis
//   fri_multipoint.hip evaluation and interpolation at arbitrary points, on the tree
//   fri_commit.hip     the commit plan (layout, allocation) and the 1-GPU
//                      commit (static launch sequence, hipGraph capture/replay)
//   fri_batch.hip      the batched commit of many small codewords and the
//                      batched prover entry points (trace commit, composition
//                      commit, query round)
//   fri_verify.hip     the batched verifier: staging, chunking, the launch pair
//   fri_grind.hip      proof-of-work grinding: the walk over windows of nonces
//   fri_lanes.hip      commit lanes, pipelined commits, the input buffer and
//                      which commit the read-backs serve (residency)
//   fri_readback.hip   read-backs and decommitment of a committed proof, the
//                      single commit's and member-wise (one set of bodies)
//   fri_fibsq.hip      the single-proof prover entry points (trace commit,
//                      FibonacciSq composition commit, trace decommitment) and
//                      the FibonacciSq shape both composition commits share
//   fri_transport.hip  collective transports (RCCL, host callbacks, loopback,
//                      in-process peer) and their self-test
//   fri_sharded.hip    one rank's coset-sharded commit and decommitment
//   fri_team.hip       the single-process multi-GPU team context
// Device-side layouts and kernel launchers are in fri_internal.hpp.
// Everything declared here has hidden visibility: the library exports the C
// ABI of fri_amd.h and nothing else of its host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/fri_amd.h"
#include "fri_internal.hpp"

#pragma GCC visibility push(hidden)

namespace fri {

static_assert(MAXR == FRI_MAX_ROUNDS, "round bound");

struct ProfEntry { double ms = 0; uint64_t launches = 0; uint64_t bytes = 0; };

struct Plan {
    bool valid = false;
    uint32_t log_n = 0;
    size_t d = 0;
    uint32_t offset = 0;
    int rmax = 0;
    // Shard-sized plan (fri_commit_sharded): rank `rank` of G holds only its
    // block of layers 0..k_sw (their slots, block-local trees and x^-1 slices
    // are block-sized); layers after k_sw are full-size local layers, and
    // layer k_sw's value slot is full-size when the tail goes local.
    bool sharded = false;
    uint32_t G = 1, rank = 0;
    int k_sw = -1;
    // Sharded coefficient fold: rank r holds coefficients [r*S_k, (r+1)*S_k)
    // of poly_k, S_k = 2^(cs0 - k), for k = 1..k_sw (coefA/B hold chunks);
    // coefF receives poly_{k_sw} whole at the switch to the local tail.
    uint32_t cs0 = 0;
    uint32_t* coefF = nullptr;  size_t coefF_cap = 0;
    // The commit's input: d_in is the plan's private staging buffer (host
    // coefficients and other device pointers are copied there); src is what
    // the launch sequence of the commit being enqueued reads: d_in, or the
    // context's caller-owned input buffer (fri_ctx::user_in), read in place.
    uint32_t* d_in = nullptr;   size_t in_cap = 0;
    const uint32_t* src = nullptr;
    uint32_t* coefA = nullptr;
    uint32_t* coefB = nullptr;  size_t coef_cap = 0;
    uint32_t* layers = nullptr; size_t layer_off[MAXR + 2] = {0};
    uint32_t* trees = nullptr;  size_t tree_off[MAXR + 2] = {0};
    uint32_t* xinv = nullptr;   size_t xinv_off[MAXR + 2] = {0};
    size_t xinv_start[MAXR + 2] = {0};   // domain index of xinv slot k's first entry (sharded slices)
    uint32_t block[MAXR + 2] = {0};      // block this rank holds of sharded layer k (k <= k_sw)
    uint32_t* pre_lo = nullptr;
    uint32_t* pre_hi = nullptr;
    int32_t* wgmax = nullptr;       // per-workgroup coefficient maxima
    // Commit graphs: one per (result slot, input), the synchronous commit's
    // as slot FRI_MAX_INFLIGHT (the DevState copy-out node targets the slot);
    // input 0 reads d_in, input 1 the caller's buffer at graph_src (captured
    // again when that buffer moves).
    hipGraph_t graph[FRI_MAX_INFLIGHT + 1][2] = {};
    hipGraphExec_t exec[FRI_MAX_INFLIGHT + 1][2] = {};
    const uint32_t* graph_src[FRI_MAX_INFLIGHT + 1][2] = {};
    hipGraph_t tail_graph = nullptr;        // sharded plan: the local layers after the switch
    hipGraphExec_t tail_exec = nullptr;
    const uint32_t* tail_src = nullptr;     // the input pointer tail_exec was captured with
    bool graph_profiled = false;
};

// One commit lane: a plan (every per-commit buffer: input, coefficient
// buffers, layers, trees, x^-1 tables, graphs), the stream the lane's commits
// run on and their device state.  Pipelined commits on one context are dealt
// to lanes (result slot i -> lane i mod max_lanes, created on first use), so
// consecutive commits run on different streams and one commit's serial tree
// tops overlap the next one's leaf hashing.  The lane of the most recently
// enqueued commit is the one installed in fri_ctx::{plan, stream, d_state}
// (use_lane), so every read-back serves that commit.
struct Lane {
    Plan plan;
    hipStream_t stream = nullptr;
    DevState* d_state = nullptr;
};

// The batched commit (fri_commit_batch, fri_batch.hip): its own buffers, one
// slice per member (laid out like a one-GPU plan, Batch::lay), grown on demand
// and kept until a larger batch or fri_ctx_destroy; no lane's plan is touched.
enum {
    BB_LAYERS, BB_TREES, BB_COEFA, BB_COEFB,
    BB_IN,        // staged input (host coefficients)
    BB_SCALED,    // c_j offset^j, the batched transform's input
    BB_STATES,    // one DevState per member
    // the batched prover (fri_trace_commit_batch and what follows it)
    BB_TLDE,      // the members' trace LDEs
    BB_TTREE,     // ... and their Merkle trees, every level
    BB_TCOEF,     // trace coefficients (the LDE's input)
    BB_TROOTS,    // the trace trees' roots, 8 words per member
    BB_CP,        // composition polynomial on the coset, n words per member
    BB_FIB,       // one FibsqMember per member
    BB_QMETA,     // the query round and phase: a chunk's states, n_layers and indices
    BB_QOUT,      // ... and its records
    BB_N
};
struct BatchBufs {
    void* dev[BB_N] = {};
    size_t cap[BB_N] = {};          // bytes
    DevState* h_states = nullptr;   // pinned: the members' states in and out
    size_t h_cap = 0;               // members
    uint32_t* words(int i) const { return static_cast<uint32_t*>(dev[i]); }
};
struct Batch {
    bool resident = false;       // the last commit call on the context was a batch
    uint32_t count = 0, log_n = 0;
    Plan lay;                    // a member's layout (offsets only; no buffers, never `valid`)
    size_t lay_stride = 0, tre_stride = 0, coef_stride = 0;
    BatchBufs b;
    // shared by the members (same log_n and offset): x^-1 of every fold, the pre-scale power table
    uint32_t* xinv = nullptr;
    uint32_t* pre_lo = nullptr;
    uint32_t* pre_hi = nullptr;
    uint32_t tab_log_n = 0, tab_offset = 0;
    // The trace batch (fri_trace_commit_batch): resident through the composition
    // commit that consumes it, until the next trace batch, plain batch or
    // single commit.
    bool trace_resident = false;
    uint32_t trace_count = 0, trace_log_t = 0, trace_log_b = 0, trace_offset = 0;
    size_t tlde_stride = 0, ttree_stride = 0;    // words
    // pinned staging of the query rounds and the trace roots (grown on demand)
    uint8_t* h_q = nullptr;
    size_t h_q_cap = 0;
    uint32_t query_chunk = 0;    // fri_debug_set_query_chunk: members per chunk of the query round and phase (0: by byte budget)
};

// The batched verifier (fri_verify_batch, fri_verify.hip): one device buffer
// for a chunk of packed transcripts (grown on demand, kept until
// fri_ctx_destroy), a second stream for k_verify_open and the events that
// join it to the context stream.
struct VerifyBufs {
    uint8_t* dev = nullptr;
    size_t cap = 0;              // bytes
    hipStream_t side = nullptr;
    hipEvent_t ev_up = nullptr, ev_open = nullptr;
    uint32_t chunk = 0;          // fri_debug_set_verify_chunk: members per launch pair (0: by byte budget)
};

// Grinding (fri_grind, fri_grind_batch; fri_grind.hip): per member the
// minimum word, the channel state, the midstate record and the active list in
// one device buffer, and the pinned mirror of what travels (grown on demand,
// kept until fri_ctx_destroy).
struct GrindBufs {
    uint8_t* dev = nullptr;
    uint8_t* host = nullptr;     // pinned
    size_t cap = 0;              // members
    uint32_t log_window = 0;     // fri_debug_set_grind_window: log2 of the nonces per launch (0: chosen from bits)
};

struct Team;   // in-process team (defined below)

// Collective transport of the sharded commit: RCCL on the context stream, or
// host-staged callbacks (synchronous; used by the gloo tests), or the peer
// transport of an in-process team (fri_ctx_create_multi: device copies
// between the ranks' buffers, ordered by events, on the same streams RCCL
// would use).
struct Transport {
    int rank = 0, world = 1;
    ncclComm_t comm = nullptr;     // main stream collectives
    ncclComm_t xcomm = nullptr;    // exchange stream (separate communicator: no cross-stream ordering hazard)
    bool host = false;
    bool loop = false;          // fri_debug_attach_loopback: every exchange returns this rank's own bytes
    bool peer = false;          // in-process team, peer transport (peer_op)
    Team* team = nullptr;       // the team this rank belongs to (peer or team RCCL transport)
    int64_t fail_at = -1;       // fri_debug_team_inject_failure: peer op index (this call) that fails
    int64_t n_ops = 0;          // peer ops issued by the current team call
    fri_collectives ops{};
    uint8_t* hs = nullptr;      // pinned staging
    uint8_t* hr = nullptr;
    size_t hcap = 0;
    std::vector<fri_transport_op> log;   // schedule of the last sharded call (fri_debug_transport_log)
};

// Scratch of the sharded commit (sized on first use).
struct DistBuf {
    size_t cap = 0;             // words in cyc/recv
    uint32_t* cyc = nullptr;    // coset slice / all-to-all send
    uint32_t* recv = nullptr;   // all-to-all / gather receive
    uint32_t* half = nullptr;   // partner half-block (even layers' exchanges)
    uint32_t* half2 = nullptr;  // partner half-block (odd layers': the fused leaf kernel still reads the other)
    uint32_t* top = nullptr;    // per-layer top trees (2G digests each)
    uint32_t* pre_lo = nullptr; // coset pre-scale tables
    uint32_t* pre_hi = nullptr;
    size_t gcap = 0;            // words in gath
    uint32_t* gath = nullptr;   // all-gathered layer at the switch to local
    uint32_t* dq = nullptr;     // sharded decommitment: this rank's openings + all ranks' (G + 1 slots)
    uint32_t* rec = nullptr;    // per-layer record: this rank's (REC_WORDS) then all ranks' (64 * REC_WORDS)
    ShardTop* shtop = nullptr;  // per layer: what the sharded top kernels read (MAXR + 1)
    std::vector<ShardTop> shtop_h;  // the contents last uploaded to shtop (re-uploaded only on change)
    std::vector<int32_t> sched_h;   // loopback rehearsal: recorded degree per layer (fri_debug_loopback_degrees)
};

// In-process team (fri_ctx_create_multi; see "in-process team" below).
struct PeerSlot {
    const void* send;
    void* recv;
    size_t bytes;
    uint32_t op, chan;
    int peer;
};

struct Team {
    uint32_t G = 1, logG = 0;
    int kind = FRI_TRANSPORT_PEER;          // FRI_TRANSPORT_PEER or FRI_TRANSPORT_RCCL
    std::vector<int> dev;
    std::vector<fri_ctx*> rk;               // rk[0] = the owning context
    bool can_pull = true;                   // every device can read every other's memory (peer access)
    bool kernel_pull = true;                // peer_op pulls with k_peer_pull (else hipMemcpyPeerAsync)
    std::vector<std::pair<int, int>> peer_pairs;   // device pairs whose peer access this team holds
    // job dispatch to the worker threads (ranks 1..G-1)
    std::vector<std::thread> th;
    std::mutex jm;
    std::condition_variable jcv, dcv;
    uint64_t seq = 0;
    uint32_t left = 0;
    bool quit = false;
    std::function<int(uint32_t)> job;
    std::vector<int> rc;
    // rendezvous of the peer transport
    std::mutex bm;
    std::condition_variable bcv;
    uint64_t bgen = 0;
    uint32_t arrived = 0;
    bool aborted = false;
    std::string why;
    std::vector<PeerSlot> slot;
    std::vector<hipEvent_t> ev_ready, ev_done;   // per rank, created on its device
};

// One timed launch group: events recorded around it on the context stream.
struct TimedSpan { std::string cls; hipEvent_t b, e; uint64_t bytes; };
}  // namespace fri

using namespace fri;

struct fri_ctx {
    int device = 0;
    uint32_t log_n_max = 0;
    hipStream_t stream = nullptr;
    std::string err;
    uint32_t* tw_fwd = nullptr;     // stage-packed Montgomery twiddles, 2^log_n_max entries
    uint32_t* tw_inv = nullptr;
    uint32_t* scratch_a = nullptr;  // 2^log_n_max words each
    uint32_t* scratch_b = nullptr;
    uint32_t* scratch_c = nullptr;
    uint32_t* pow_lo = nullptr;
    uint32_t* pow_hi = nullptr;
    DevState* d_state = nullptr;
    DevState* h_state = nullptr;    // the state of the most recently enqueued commit (h_sync or a slot)
    DevState* h_sync = nullptr;     // pinned: synchronous commits
    // pipelined commits (fri_commit_device_async): pinned state per slot, an
    // event after its copy-out, the ticket it holds and whether it is unwaited
    DevState* h_slot[FRI_MAX_INFLIGHT] = {};
    hipEvent_t ev_slot[FRI_MAX_INFLIGHT] = {};
    uint64_t slot_ticket[FRI_MAX_INFLIGHT] = {};
    uint32_t slot_log_n[FRI_MAX_INFLIGHT] = {};
    bool slot_pending[FRI_MAX_INFLIGHT] = {};
    bool slot_user[FRI_MAX_INFLIGHT] = {};   // pending slot i reads user_in (fri_ctx_input_upload waits for it)
    uint32_t* h_in[FRI_MAX_INFLIGHT] = {};  // fri_commit_async: pinned copy of the slot's host coefficients,
    uint32_t* d_slot_in[FRI_MAX_INFLIGHT] = {};   // its device copy (uploaded on h2d_stream while the
    size_t h_in_cap[FRI_MAX_INFLIGHT] = {};       // previous commit runs) and the upload's event
    hipEvent_t ev_in[FRI_MAX_INFLIGHT] = {};
    hipStream_t h2d_stream = nullptr;   // the device's shared upload stream (upload_stream())
    uint64_t next_ticket = 1;
    bool async_unsettled = false;   // commits enqueued since the stream was last drained
    Plan plan;
    Lane lanes[FRI_MAX_INFLIGHT];   // lanes[cur_lane] is empty: that lane lives in plan / stream / d_state
    int cur_lane = 0;
    int res_lane = 0;               // lane of the resident commit (init_state): the read-backs serve it
    int max_lanes = FRI_DEFAULT_LANES;
    int lanes_ok = FRI_MAX_INFLIGHT;   // lanes below this got plan memory (lowered on ENOMEM, pick_lane)
    int slot_lane[FRI_MAX_INFLIGHT] = {};            // lane of pending slot i
    uint64_t lane_ticket[FRI_MAX_INFLIGHT] = {};     // last ticket dealt to lane j (0: never)
    bool profiling = false;
    std::map<std::string, ProfEntry> prof;
    std::vector<TimedSpan> spans;      // recorded spans of the current commit
    std::vector<hipEvent_t> event_pool;
    size_t event_next = 0;
    Transport tp;
    DistBuf db;
    hipStream_t xstream = nullptr;  // exchange stream (overlaps the local tree)
    hipEvent_t ev_vals = nullptr, ev_xchg = nullptr;
    hipStream_t cstream = nullptr;  // coefficient-fold stream (overlaps the local tree)
    hipEvent_t ev_pre = nullptr, ev_coef = nullptr;
    uint32_t sharded_layers = 0;    // layers of the last commit held block-wise across ranks
    uint64_t commit_gen = 0;        // bumped by every commit: read-backs of an older proof are refused
    uint32_t commit_log_n = 0;      // codeword log2 of the resident commit
    Batch batch;                    // fri_commit_batch: buffers and residency (fri_batch.hip)
    VerifyBufs verify;              // fri_verify_batch: staging (fri_verify.hip)
    GrindBufs grind;                // fri_grind, fri_grind_batch: staging (fri_grind.hip)
    uint32_t* interp_tmp = nullptr; // partials of fri_interpolate_points / fri_evaluate, fri_merkle_root's tree (grown on use)
    size_t interp_cap = 0;
    uint32_t roots_leaf = 0;        // fri_debug_set_roots_leaf: roots per leaf subtree (0: FRI_ROOTS_LEAF)
    uint32_t* dq_host = nullptr;    // decommitment gather output: 64 KiB of coherent pinned host
    uint32_t* dq_dev = nullptr;     // memory the gather kernel writes directly (its device address)
    uint32_t* trace_tree = nullptr; // Merkle tree of the last fri_trace_commit LDE
    uint32_t* trace_lde = nullptr;  // ... and the LDE itself (prover: composition, queries)
    size_t trace_tree_cap = 0;      // leaves they can hold
    bool trace_valid = false;       // a trace commit is resident
    uint32_t trace_log_t = 0, trace_log_b = 0, trace_offset = 0;
    bool stuck = false;               // a stream stayed busy after an RCCL abort (sync_sharded)
    bool inject_stall = false;        // fri_debug_inject_stall: next RCCL all-to-all never completes
    uint32_t* stall_flag = nullptr;   // pinned host word the stalled kernel polls (set by rccl_abort)
    uint32_t* stall_flag_dev = nullptr;
    std::map<const void*, size_t> allocs;   // device allocations owned by the context (fri_ctx_device_bytes)
    size_t dev_bytes = 0, dev_peak = 0;
    size_t dev_cap = 0;             // fri_debug_set_device_cap: allocations beyond it fail (0: none)
    Team* team_root = nullptr;      // fri_ctx_create_multi: this context is rank 0 and owns the team
    // The caller-owned input buffer (fri_ctx_input_buffer): written only by the
    // caller or by fri_ctx_input_upload, never by a commit; commits from it
    // read it in place, on any lane.
    uint32_t* user_in = nullptr;
    size_t user_cap = 0;
    uint64_t* d_csum = nullptr;     // input checksum (FRI_FLAG_RANK_INPUTS): device word ...
    uint64_t* h_csum = nullptr;     // ... and its pinned host copy
};

namespace fri {

// Device allocations of a context go through these, so that
// fri_ctx_device_bytes can report what one rank / one context holds in HBM.
template <class T>
inline hipError_t dalloc(fri_ctx* ctx, T** p, size_t bytes) {
    void* q = nullptr;
    if (ctx->dev_cap && ctx->dev_bytes + bytes > ctx->dev_cap) { *p = nullptr; return hipErrorOutOfMemory; }
    const hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) { *p = nullptr; return e; }
    *p = static_cast<T*>(q);
    ctx->allocs[q] = bytes;
    ctx->dev_bytes += bytes;
    if (ctx->dev_bytes > ctx->dev_peak) ctx->dev_peak = ctx->dev_bytes;
    return hipSuccess;
}
inline void dfree(fri_ctx* ctx, const void* p) {
    if (!p) return;
    auto it = ctx->allocs.find(p);
    if (it != ctx->allocs.end()) {
        ctx->dev_bytes -= it->second;
        ctx->allocs.erase(it);
    }
    hipFree(const_cast<void*>(p));
}

#define FRI_HIP(ctx, expr)                                                              \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);             \
            return FRI_EHIP;                                                            \
        }                                                                               \
    } while (0)

inline double rccl_timeout_s() {
    const char* e = getenv("FRI_RCCL_TIMEOUT_S");
    const double v = e ? atof(e) : 0.0;
    return v > 0.0 ? v : 120.0;
}
inline double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
inline int fail(fri_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    return code;
}

// Device-reported commit failures (DevState.status, set by the layer-0 top
// or tail kernel): the input coefficients are validated on the device, in
// the layer-0 coefficient scan, rather than by a host pass over them.
inline const char* status_message(uint32_t status) {
    return status == FRI_EINVAL ? "coefficient not canonical (>= p)"
                                : "degree exceeds the domain (reference would panic)";
}

// Every value < p.  A branch-free max over 64 KiB blocks (the compiler
// vectorises it), with the early exit per block: the per-element early-exit
// loop cost about 1 ms per 2^21 coefficients of fri_commit's host input.
inline bool check_canonical(const uint32_t* v, size_t n) {
    // an OR of compares vectorises on the x86-64 baseline (an unsigned max
    // needs SSE4.1): about 2x faster per 2^21 values
    for (size_t i = 0; i < n; i += 16384) {
        const size_t e = n - i < 16384 ? n : i + 16384;
        uint32_t bad = 0;
        for (size_t j = i; j < e; j++) bad |= (uint32_t)(v[j] >= P);
        if (bad) return false;
    }
    return true;
}

// ------------------------------------------------------------- commit ----
inline int rounds_bound(size_t d, uint32_t log_n) {
    if (d <= 1) return 0;
    int b = 0;
    for (size_t v = d - 1; v; v >>= 1) b++;
    return b < (int)log_n ? b : (int)log_n;
}

// ---- coset-sharded schedule (shared by the shard-sized plan and the commit) --
constexpr uint32_t SHARD_MIN_LOG = 20;   // layers of >= 2^20 elements are hashed sharded

// Layer k of a sharded commit hands a sharded layer k+1 on while that layer
// is still large (>= 2^SHARD_MIN_LOG) and its blocks hold >= 2^10 elements;
// otherwise layer k is the last sharded one (k_sw) and the tail goes local.
inline bool next_layer_sharded(uint32_t log_n, uint32_t logG, int k, int rmax) {
    const uint32_t Lk = log_n - (uint32_t)k;
    return k < rmax && (Lk - 1) >= SHARD_MIN_LOG && (Lk - 1 - logG) >= 10;
}
inline int switch_layer(uint32_t log_n, uint32_t logG, int rmax) {
    int k = 0;
    while (next_layer_sharded(log_n, logG, k, rmax)) k++;
    return k;
}
// The fold pairs block b with block b + G/2 (fold pairs (i, i + m/2)); the
// rank holding b (< G/2) keeps output block 2b, its partner 2b + 1.
inline void advance_blocks(std::vector<uint32_t>& block_of, std::vector<uint32_t>& rank_of, uint32_t G) {
    for (uint32_t r = 0; r < G; r++) {
        const uint32_t br = block_of[r];
        block_of[r] = br < G / 2 ? 2 * br : 2 * (br - G / 2) + 1;
    }
    for (uint32_t r = 0; r < G; r++) rank_of[block_of[r]] = r;
}
// Domain index of the first x^-1 a sharded fold of layer k needs on a rank
// holding block b of size B: the half-block [bb*B + (isA ? 0 : B/2), + B/2).
inline size_t fold_xinv_start(uint32_t b, uint32_t G, size_t B) {
    const bool isA = b < G / 2;
    return (size_t)(isA ? b : b - G / 2) * B + (isA ? 0 : B / 2);
}

inline NttPlan lde_plan(fri_ctx* ctx, uint32_t log_n) {
    NttPlan p{};
    p.log_n = log_n;
    p.tw = ctx->tw_fwd;
    return p;
}

// Device scratch of at least `words` words for the interpolation / evaluation
// partials (grown on demand, freed with the context).
inline int ensure_tmp(fri_ctx* ctx, size_t words) {
    if (words <= ctx->interp_cap) return FRI_OK;
    FRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->interp_tmp) dfree(ctx, ctx->interp_tmp);
    ctx->interp_tmp = nullptr;
    ctx->interp_cap = 0;
    if (dalloc(ctx, &ctx->interp_tmp, words * 4) != hipSuccess) return fail(ctx, FRI_ENOMEM, "partials scratch");
    ctx->interp_cap = words;
    return FRI_OK;
}
// Scratch grown past TMP_KEEP_WORDS is released after the call that grew it,
// so one large fri_merkle_root (the tree of 2^28 values is 16 GiB) does not
// pin HBM for the life of the context and starve a later commit plan; smaller
// scratch is kept (no hipFree, which synchronises the device, per call).
constexpr size_t TMP_KEEP_WORDS = (size_t)1 << 26;   // 256 MiB
inline void tmp_trim(fri_ctx* ctx) {
    if (ctx->interp_cap <= TMP_KEEP_WORDS) return;
    (void)hipStreamSynchronize(ctx->stream);
    dfree(ctx, ctx->interp_tmp);
    ctx->interp_tmp = nullptr;
    ctx->interp_cap = 0;
}

// ---- polynomial layer helpers (fri_poly.hip, fri_roots.hip, fri_multipoint.hip)
inline size_t trimmed(const uint32_t* v, size_t n) {              // Polynomial::new (ops.rs:19-37)
    while (n > 0 && v[n - 1] == 0) n--;
    return n;
}
inline uint32_t ceil_log2(size_t n) {
    uint32_t l = 0;
    while (((size_t)1 << l) < n) l++;
    return l;
}
inline size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }
// dst = NTT_{2^log_N}(src[0..len)), natural order, canonical.
inline void forward(fri_ctx* ctx, const uint32_t* src, size_t len, uint32_t log_N, uint32_t* dst) {
    NttPlan p = lde_plan(ctx, log_N);
    launch_ntt(p, src, len, dst, ctx->stream);
}
// Every 2^lg block of an np-word level (np >= 2^lg) in batched launches: block
// j transforms src[j * 2^lg .. + len), zero beyond len, into dst[j * 2^lg ..).
// A launch carries at most 2^15 transforms, so there is more than one chunk
// only beyond 2^28 words.  A level that transforms several operands calls
// this once per operand: with more than one chunk the launches then reach the
// stream operand after operand, not interleaved per chunk; the operands are
// independent, and with one chunk the order is the same.
inline void batched_ntt(fri_ctx* ctx, uint32_t lg, bool inv, const uint32_t* src, size_t len, uint32_t* dst,
                        size_t np) {
    NttPlan p = lde_plan(ctx, lg);
    if (inv) p.tw = ctx->tw_inv;
    p.src_stride = p.dst_stride = (size_t)1 << lg;
    const size_t count = np >> lg;
    for (size_t j0 = 0; j0 < count; j0 += 32768) {
        p.batch = (uint32_t)(count - j0 < 32768 ? count - j0 : 32768);
        launch_ntt(p, src + (j0 << lg), len, dst + (j0 << lg), ctx->stream);
    }
}
// The inverse transform's post-scale N^-1 * R^r_pow: undoes the r_pow factors
// of R^-1 a pointwise kernel left (fri_poly_kernels.hip "polynomial arithmetic").
inline uint32_t post_scale(uint32_t log_N, uint32_t r_pow) {
    uint32_t scale = inv_std((uint32_t)(((size_t)1 << log_N) % P));
    for (uint32_t i = 0; i < r_pow; i++) scale = mul_std(scale, R_MOD_P);
    return scale;
}
// batch > 1: that many transforms in the same launches, transform b from
// src + b * src_stride into dst + b * dst_stride (NttPlan, fri_internal.hpp).
inline void inverse_with(fri_ctx* ctx, const uint32_t* src, uint32_t log_N, const uint32_t* post_lo,
                         const uint32_t* post_hi, uint32_t* dst, uint32_t batch = 0, size_t src_stride = 0,
                         size_t dst_stride = 0) {
    NttPlan p = lde_plan(ctx, log_N);
    p.tw = ctx->tw_inv;
    p.post_lo = post_lo;
    p.post_hi = post_hi;
    p.batch = batch;
    p.src_stride = src_stride;
    p.dst_stride = dst_stride;
    launch_ntt(p, src, (size_t)1 << log_N, dst, ctx->stream);
}
// The coset iNTT: dst[j] = N^-1 * R^r_pow * base^j * iNTT(src)[j], the
// coefficients of the polynomial whose values on base^-1 * <w_N> are src
// (Polynomial::interpolate, ops.rs:239-241).  The post-scale table is made on
// the stream, in ctx->pow_lo / pow_hi.
inline void coset_inverse(fri_ctx* ctx, const uint32_t* src, uint32_t log_N, uint32_t base, uint32_t r_pow,
                          uint32_t* dst, uint32_t batch = 0, size_t src_stride = 0, size_t dst_stride = 0) {
    launch_pow_table(ctx->pow_lo, ctx->pow_hi, log_N, base, post_scale(log_N, r_pow), ctx->stream);
    inverse_with(ctx, src, log_N, ctx->pow_lo, ctx->pow_hi, dst, batch, src_stride, dst_stride);
}
// dst = N^-1 * R^r_pow * iNTT(src)
inline void inverse(fri_ctx* ctx, const uint32_t* src, uint32_t log_N, uint32_t r_pow, uint32_t* dst) {
    coset_inverse(ctx, src, log_N, 1u, r_pow, dst);
}
// The coset LDE: dst[i] = sum_{j<len} src[j] (offset * w_N^i)^j, the values on
// offset * <w_N> (fri_commit.rs:78); the pre-scale table as coset_inverse's.
inline void coset_forward(fri_ctx* ctx, const uint32_t* src, size_t len, uint32_t log_N, uint32_t offset,
                          uint32_t* dst) {
    NttPlan p = lde_plan(ctx, log_N);
    launch_pow_table(ctx->pow_lo, ctx->pow_hi, log_N, offset, 1u, ctx->stream);
    p.pre_lo = ctx->pow_lo;
    p.pre_hi = ctx->pow_hi;
    launch_ntt(p, src, len, dst, ctx->stream);
}
// Power-series inverse g = F^-1 mod x^K by Newton's iteration
//   g <- g (2 - F g) mod x^m2,  m -> m2 = min(2m, K),
// from a seed of m0 = min(K, 64) coefficients (below that a step would be four
// launches on a handful of words).  F mod x^m2 times g times g has
// m2 + 2m - 2 coefficients: no wrap-around at 2^log_N.
struct NewtonStep { size_t m, m2; uint32_t log_N; };
inline std::vector<NewtonStep> newton_steps(size_t K) {
    std::vector<NewtonStep> steps;
    for (size_t m = K < 64 ? K : 64; m < K;) {
        const size_t m2 = 2 * m < K ? 2 * m : K;
        steps.push_back({m, m2, ceil_log2(m2 + 2 * m - 2)});
        m = m2;
    }
    return steps;
}
// Words of the buffer g grows in: a step's inverse transform lands in it whole.
inline size_t series_words(const std::vector<NewtonStep>& steps, size_t K) {
    return steps.empty() ? round4(K) : (size_t)1 << steps.back().log_N;
}
// Runs the steps on G, which holds the seed (enqueued by the caller); F has lf
// words, both outside scratch_a / scratch_b.  inverse_step(k, src, log_N, G)
// is step k's G = N^-1 R^2 iNTT(src): it writes over g, whose low m
// coefficients come back unchanged; m..m2 are new, and nothing reads past m2
// (the truncation).
template <class InverseStep>
inline void series_inverse(fri_ctx* ctx, const uint32_t* F, size_t lf, uint32_t* G,
                           const std::vector<NewtonStep>& steps, InverseStep inverse_step) {
    for (size_t k = 0; k < steps.size(); k++) {
        const NewtonStep& st = steps[k];
        forward(ctx, F, st.m2 < lf ? st.m2 : lf, st.log_N, ctx->scratch_a);
        forward(ctx, G, st.m, st.log_N, ctx->scratch_b);
        launch_poly_newton(ctx->scratch_a, ctx->scratch_b, ctx->scratch_a, (size_t)1 << st.log_N, ctx->stream);
        inverse_step(k, ctx->scratch_a, st.log_N, G);
    }
}

inline void digest_to_bytes(const uint32_t* w, uint8_t* out) {
    for (int i = 0; i < 8; i++) {
        out[4 * i] = (uint8_t)(w[i] >> 24); out[4 * i + 1] = (uint8_t)(w[i] >> 16);
        out[4 * i + 2] = (uint8_t)(w[i] >> 8); out[4 * i + 3] = (uint8_t)w[i];
    }
}

// The sizes of a query record in words (k_batch_query_all, fri_prover.hip, has
// the layout): what the batch's query round and phase write and the batched
// verifier reads.  A member with nl <= max_layers layers fills path_words(nl).
struct RecordShape {
    uint32_t log_n, trace_count, max_layers;
    size_t val_words() const { return trace_count + 2 * (size_t)max_layers; }
    size_t tpath_words() const { return (size_t)trace_count * 8 * log_n; }
    size_t fri_path_words(uint32_t nl) const { return 16 * ((size_t)nl * log_n - (size_t)nl * (nl ? nl - 1 : 0) / 2); }
    size_t path_words(uint32_t nl) const { return tpath_words() + fri_path_words(nl); }
    size_t rec_words() const { return val_words() + path_words(max_layers); }
};

// ---- fri_ctx.hip: timed spans of profiled commits (hipEvents on ctx->stream)
size_t span_begin(fri_ctx* ctx, const char* cls, uint64_t bytes);
void span_end(fri_ctx* ctx, size_t id);
void spans_collect(fri_ctx* ctx);

// ---- fri_lanes.hip: plans of the commit lanes and residency
void plan_release(fri_ctx* ctx, Plan& p);     // one plan (its lane's stream idle)
void plan_free(fri_ctx* ctx);                 // every lane's plan, after draining the lanes
int use_lane(fri_ctx* ctx, int j);            // install lane j in ctx->{plan, stream, d_state}
void settle(fri_ctx* ctx);                    // before a read-back: the resident commit's lane, drained

// ---- fri_commit.hip: plan and 1-GPU commit
void plan_layout(Plan& p, size_t d, uint32_t log_n, uint32_t G, uint32_t rank, size_t& lay, size_t& tre,
                 size_t& xin);
int plan_build(fri_ctx* ctx, size_t d, uint32_t log_n, uint32_t offset, uint32_t G = 1, uint32_t rank = 0);
uint32_t* coef_buf(Plan& p, int r);
LayerTask commit_task(fri_ctx* ctx, int k);
void state_reset(DevState* h, const fri_channel_state* chan_in, uint32_t flags, const uint32_t* forced_betas);
void init_state(fri_ctx* ctx, DevState* h, const fri_channel_state* chan_in, uint32_t flags,
                const uint32_t* forced_betas);
int commit_validate(fri_ctx* ctx, size_t d, uint32_t log_n, uint32_t offset, uint32_t flags,
                    const uint32_t* forced_betas);
int commit_enqueue(fri_ctx* ctx, const uint32_t* host_coeffs, const uint32_t* dev_coeffs, size_t d,
                   uint32_t log_n, uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
                   const uint32_t* forced_betas, int slot);
int commit_finish(fri_ctx* ctx, DevState* h, uint32_t log_n, fri_commit_result* out);
int run_commit(fri_ctx* ctx, const uint32_t* host_coeffs, const uint32_t* dev_coeffs, size_t d, uint32_t log_n,
               uint32_t offset, const fri_channel_state* chan_in, uint32_t flags, const uint32_t* forced_betas,
               fri_commit_result* out);

// ---- fri_roots.hip: the product tree (also under fri_multipoint.hip)
uint32_t roots_leaf_log(const fri_ctx* ctx, bool small_leaf);   // log2 of the roots per leaf subtree
const uint32_t* product_tree(fri_ctx* ctx, const uint32_t* d_roots, size_t n, uint32_t lf_log,
                             uint32_t* keep = nullptr);

// ---- fri_ops.hip: the direct kernels behind fri_evaluate_ex / fri_interpolate_points_ex
// (arguments validated by the caller)
int evaluate_direct(fri_ctx* ctx, const uint32_t* coeffs, size_t d, const uint32_t* xs, size_t count, uint32_t* out);
int interpolate_points_direct(fri_ctx* ctx, const uint32_t* xs, const uint32_t* ys, size_t n, uint32_t log_N,
                              uint32_t* coeffs_out, size_t* len_out);

// ---- fri_readback.hip
// One committed proof as the read-backs see it: the single commit (its lane's
// plan) or one member of the resident batch (its slices of Batch's buffers).
struct ProofView {
    const uint32_t* layers = nullptr;     // base of its layer slices
    const uint32_t* trees = nullptr;      // ... and of its tree slices
    const size_t* layer_off = nullptr;    // the layout's offsets (Plan::layer_off / tree_off)
    const size_t* tree_off = nullptr;
    uint32_t log_n = 0;
    uint32_t n_layers = 0;                // layers it serves: none without a valid plan, or of a failed member
    const DevState* st = nullptr;         // its copied-out state
    bool member = false;                  // refusals say "... of this member"
};
ProofView single_view(fri_ctx* ctx);          // the resident single commit, its lane drained (settle)
// The DecommitPlan of a whole query of v (index, shape, layer / tree / path
// offsets) and *words, the path words it writes after its 2 values per layer;
// *paths_len is set, then the buffers' capacities and the 64 KiB of the gather
// output are checked.
int decommit_plan(fri_ctx* ctx, const ProofView& v, uint64_t index, size_t values_cap, const uint8_t* paths,
                  size_t paths_cap, size_t* paths_len, DecommitPlan* dp, uint32_t* words);
int dq_alloc(fri_ctx* ctx);                   // pinned host buffer the gather kernels write
// FRI_ESTATE of a single-commit read-back that finds no such layer
int no_layer(fri_ctx* ctx, const char* what);

// ---- fri_fibsq.hip
// The FibonacciSq shape's checks and, in *q, the composition kernel's
// constants of it (a_last and alpha_m are the caller's to fill).  batch_caps:
// the batched prover's limits on top (FRI_BATCH_MAX_LOG_N, the context's size).
int fibsq_shape(fri_ctx* ctx, uint32_t log_t, uint32_t log_blowup, uint32_t offset, bool batch_caps, FibsqParams* q);

// ---- fri_batch.hip
void batch_free(fri_ctx* ctx);                // fri_ctx_destroy

// ---- fri_verify.hip
void verify_free(fri_ctx* ctx);               // fri_ctx_destroy

// ---- fri_grind.hip
void grind_free(fri_ctx* ctx);                // fri_ctx_destroy

int input_checksum(fri_ctx* ctx, const uint32_t* d_src, size_t d, uint64_t* out);   // (synchronous)

// ---- fri_transport.hip
int tp_host_stage(fri_ctx* ctx, size_t bytes);
void rccl_abort(fri_ctx* ctx);
int sync_sharded(fri_ctx* ctx, hipStream_t s);
int tp_allgather(fri_ctx* ctx, const void* dsend, void* drecv, size_t bytes, hipStream_t s);
int tp_alltoall(fri_ctx* ctx, const void* dsend, void* drecv, size_t bytes_per_peer, hipStream_t s);
int tp_sendrecv(fri_ctx* ctx, const void* dsend, void* drecv, size_t bytes, int peer, hipStream_t s, uint32_t chan);
int dist_buffers(fri_ctx* ctx, size_t M, uint32_t G, size_t gwords);

// ---- fri_sharded.hip
int run_commit_sharded(fri_ctx* ctx, const uint32_t* host_coeffs, const uint32_t* dev_coeffs, size_t d,
                       uint32_t log_n, uint32_t offset, const fri_channel_state* chan_in, uint32_t flags,
                       const uint32_t* forced_betas, fri_commit_result* out);
int decommit_sharded(fri_ctx* ctx, uint64_t index, uint32_t* values, size_t values_cap, uint8_t* paths,
                     size_t paths_cap, size_t* paths_len);

// ---- fri_team.hip
void team_abort(Team* T, const std::string& why);
bool team_barrier(Team* T);
int team_run(fri_ctx* root, const std::function<int(uint32_t)>& fn);
void team_destroy(fri_ctx* root);
int team_commit(fri_ctx* ctx, const uint32_t* host_coeffs, const uint32_t* dev_coeffs, size_t d, uint32_t log_n,
                uint32_t offset, const fri_channel_state* chan_in, uint32_t flags, const uint32_t* forced_betas,
                fri_commit_result* out);
int team_layer_copy(fri_ctx* ctx, uint32_t layer, uint32_t* out);
int team_tree_level_copy(fri_ctx* ctx, uint32_t layer, uint32_t level, uint32_t* w);
int team_decommit(fri_ctx* ctx, uint64_t index, uint32_t* values, size_t values_cap, uint8_t* paths,
                  size_t paths_cap, size_t* paths_len);

}  // namespace fri

#pragma GCC visibility pop
