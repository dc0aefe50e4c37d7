// fri_verify_kernels.hip — the batched verifier's two kernels (fri_verify_batch,
// include/fri_amd.h).
//
// A transcript carries the challenges and query indices it claims, so the two
// halves of verify_transcript (host/stark101.cpp) need nothing from each other:
//   k_verify_chain  replays the Fiat-Shamir channel (channel.rs:35-84) over
//                   the member's whole transcript, one lane per member, and
//                   checks that every claimed alpha, beta and query index is
//                   the one the replay draws;
//   k_verify_open   checks every authentication path, fold, final value and
//                   composition against the CLAIMED challenges and indices,
//                   one lane per check, members fastest.
// A member is accepted when neither finds anything: then the claimed values are
// the replayed ones, and every check ran on exactly the values the host
// verifier would have used.
//
// Numbers taken from a transcript only choose left/right in a path climb and
// exponents of domain points; every address is formed from the member, query
// and layer numbers alone.
#include "fri_internal.hpp"
#include "chan_send.hpp"

namespace fri {
namespace {

// Words before layer k's two paths in a (member, query) path record
__device__ __forceinline__ uint32_t fri_path_off(const VerifyTask& t, uint32_t k) {
    return t.trace_count * 8u * t.log_n + 16u * (k * t.log_n - k * (k - 1u) / 2u);
}

}  // namespace

// One lane per member, workgroups of one wave.  The lane walks its transcript
// in verify_transcript's order as a sequence of units, each a few sends:
//   q = -1: [trace root, 3 alphas], per layer (root, beta), the final value,
//           with pow_bits > 0 the grinding nonce: after its
//           send the state's top pow_bits bits must be zero (VB_POW), and the
//           replay goes on whether they are or not;
//   q >= 0: the query index, trace_count (value, path), per layer
//           (value, path, sibling value, sibling path), a one-element layer's
//           value once more first (fri_commit.rs:147-149).
// A draw compares what the channel gives with the claimed word and rehashes.
// Lanes past their member's last layer sit the unit out.
// Two instantiations, each with its ONE call site of chan_send: without
// grinding bits the kernel is the one it was before the nonce existed (163
// VGPRs, 93 SGPRs spilled); as a run-time case in one kernel the nonce cost
// that path 3 VGPRs, 13 more spilled SGPRs and 0.7-0.9% of its time
// (profiles/verify_batch_pow.txt).
template <bool POW>
__global__ __launch_bounds__(64) void k_verify_chain(VerifyTask t) {
    const uint32_t b = blockIdx.x * 64u + threadIdx.x;
    if (b >= t.members) return;
    const uint32_t L = t.log_n, ML = t.max_layers, tc = t.trace_count, Q = t.num_queries;
    const uint32_t nl = min(max(t.n_layers[b], 1u), ML);
    const uint32_t* head = t.head + (size_t)b * t.head_words;
    const uint32_t hb = tc ? 11u : 0u;              // words before the layer roots
    uint32_t cs[8], has, bad = 0u;
    {
        const uint32_t* c = t.chan + (size_t)b * 9u;
#pragma unroll
        for (int j = 0; j < 8; j++) cs[j] = __builtin_bswap32(c[j]);
        has = c[8] ? 1u : 0u;
    }
    // the head's field elements must be canonical (the values: k_verify_open)
    for (uint32_t j = 0; j < (tc ? 3u : 0u); j++)
        if (head[8 + j] >= P) bad |= VB_MALFORMED;
    for (uint32_t k = 0; k + 1 < nl; k++)
        if (head[hb + 8 * ML + k] >= P) bad |= VB_MALFORMED;
    if (head[hb + 9 * ML - 1] >= P) bad |= VB_MALFORMED;

    enum : uint32_t { DRAW_NONE = 0, DRAW_FIELD = 1, DRAW_INDEX = 2 };
#pragma unroll 1
    for (int q = -1; q < (int)Q; q++) {
        const uint32_t* vals = t.values + ((size_t)b * Q + (q < 0 ? 0 : q)) * t.val_words;
        const uint32_t* pth = t.paths + ((size_t)b * Q + (q < 0 ? 0 : q)) * t.path_words;
        // units: q < 0: [0, tcu) the trace root, [tcu, tcu + ML) the layers, then the final value,
        //               then the nonce (pow_bits > 0)
        //        q >= 0: 0 the index, [1, 1 + tc) the trace openings, then the layers
        const uint32_t tcu = tc ? 1u : 0u;
        const uint32_t units = q < 0 ? tcu + ML + 1u + (POW ? 1u : 0u) : 1u + tc + ML;
#pragma unroll 1
        for (uint32_t u = 0; u < units; u++) {
            uint32_t nsub;
            if (q < 0) nsub = u < tcu ? 4u : (u < tcu + ML ? 2u : 1u);
            else nsub = u == 0 ? 1u : (u < 1u + tc ? 2u : (L - (u - 1u - tc) == 0u ? 5u : 4u));
#pragma unroll 1
            for (uint32_t s = 0; s < nsub; s++) {
                uint32_t kind = MSG_PATH, nd = 0u, v = 0u, vhi = 0u, draw = DRAW_NONE;
                uint64_t claim = 0;
                const uint32_t* p = head;
                bool act = true;
                if (q < 0) {
                    if (u < tcu) {                       // trace root, then the alphas
                        if (s == 0) { kind = MSG_ROOT; nd = 2u; }
                        else { draw = DRAW_FIELD; claim = head[8 + (s - 1u)]; }
                    } else if (u < tcu + ML) {           // layer k: root, then beta_k unless it is the last
                        const uint32_t k = u - tcu;
                        if (s == 0) { kind = MSG_ROOT; nd = 2u; p = head + hb + 8 * k; act = k < nl; }
                        // (k = ML - 1 reads the final value's word, inside the head, and sits out)
                        else { draw = DRAW_FIELD; claim = head[hb + 8 * ML + k]; act = k + 1 < nl; }
                    } else if (!POW || u == tcu + ML) {
                        kind = MSG_VALUE; v = head[hb + 9 * ML - 1];
                    } else {                             // the nonce: every lane, a full 64-bit number
                        const uint64_t n = t.nonces[b];
                        kind = MSG_VALUE; v = (uint32_t)n; vhi = (uint32_t)(n >> 32);
                    }
                } else if (u == 0) {
                    draw = DRAW_INDEX; claim = t.indices[(size_t)b * Q + q];
                } else if (u < 1u + tc) {
                    const uint32_t j = u - 1u;
                    if (s == 0) { kind = MSG_VALUE; v = vals[j]; }
                    else { p = pth + (size_t)j * 8u * L; nd = L; }
                } else {
                    const uint32_t k = u - 1u - tc, depth = L - k;
                    const uint32_t s4 = depth ? s : s - 1u;      // depth 0: sub 0 is the doubled value
                    act = k < nl;
                    if (s4 == 0u || s4 == 2u || s4 == ~0u) { kind = MSG_VALUE; v = vals[tc + 2 * k + (s4 == 2u ? 1u : 0u)]; }
                    else { p = pth + fri_path_off(t, k) + (s4 == 3u ? 8u * depth : 0u); nd = depth; }
                }
                if (!act) continue;
                if (draw != DRAW_NONE) {
                    const uint64_t got = draw == DRAW_FIELD ? (uint64_t)chan_beta(cs) : chan_int(cs, t.range);
                    if (!has || got != claim) bad |= VB_CHANNEL;
                }
                chan_send(cs, has, kind, RecordNodes{p}, nd, v, POW ? vhi : 0u);
            }
        }
        // the nonce's send ends the q = -1 pass: the top pow_bits (1..32) bits of the state are those of cs[0]
        if (POW && q < 0 && (cs[0] >> (32u - t.pow_bits))) bad |= VB_POW;
    }
    if (bad) atomicOr(&t.verdict[b], bad);
}

void launch_verify_chain(const VerifyTask& t, hipStream_t s) {
    if (t.pow_bits) hipLaunchKernelGGL(k_verify_chain<true>, dim3((t.members + 63u) / 64u), dim3(64), 0, s, t);
    else hipLaunchKernelGGL(k_verify_chain<false>, dim3((t.members + 63u) / 64u), dim3(64), 0, s, t);
}

// --------------------------------------------------------------- openings ---
namespace {
// leaf = SHA256(be64(value)) (merkle/mod.rs:14-15), then `depth` nodes with the
// siblings at p, left/right by the bits of pos; true when it ends at root.
__device__ __forceinline__ bool climb(uint32_t value, uint64_t pos, const uint32_t* p, uint32_t depth,
                                      const uint32_t* root) {
    uint32_t h[8], sib[8];
    {
        uint32_t w[16] = {0u, value, 0x80000000u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 64u};
        sha::init(h);
        compress_c(h, w);
    }
    if (depth) load_node(p, sib);
#pragma unroll 1
    for (uint32_t lvl = 0; lvl < depth; lvl++) {
        const bool right = (pos >> lvl) & 1u;       // this node is the right child
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            w[j] = right ? sib[j] : h[j];
            w[8 + j] = right ? h[j] : sib[j];
        }
        if (lvl + 1 < depth) load_node(p + 8 * (lvl + 1), sib);
        sha::init(h);
        // the data block, then the constant padding block of a 64-byte message
#pragma unroll 1
        for (int blk = 0; blk < 2; blk++) {
            if (blk) {
#pragma unroll
                for (int j = 0; j < 16; j++) w[j] = 0u;
                w[0] = 0x80000000u;
                w[15] = 512u;
            }
            compress_c(h, w);
        }
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; j++) ok = ok && h[j] == root[j];
    return ok;
}

// Montgomery(x^-1), inverse(0) = 0 (element.rs:54-57)
__device__ __forceinline__ uint32_t minv(uint32_t x_m) { return mpow(x_m, P - 2); }
}  // namespace

// One lane per (job, member) of every query, member fastest, so a wave climbs
// paths of one depth.  Jobs of a (member, query):
//   [0, tc)             trace path j at (index + j 2^log_blowup) mod 2^L
//   [tc, tc + 2 ML)     layer k's path of idx = index mod m_k, then of its sibling
//   [.., + ML)          layer k: both values canonical, the fold from layer k - 1
//                       (stark101.cpp verify_transcript; x = offset^(2^(k-1)) w^j,
//                       the claimed beta, the pair in the order the index dictates),
//                       the final value at the last layer
//   [.., + 1 if tc)     layer 0 = the composition of the opened f(x), f(gx), f(g^2 x)
__global__ __launch_bounds__(64) void k_verify_open(VerifyTask t) {
    const uint32_t L = t.log_n, ML = t.max_layers, tc = t.trace_count, Q = t.num_queries;
    const uint32_t jobs = tc + 3u * ML + (tc ? 1u : 0u);
    const uint64_t tid = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    const uint32_t b = (uint32_t)(tid % t.members);
    const uint64_t r = tid / t.members;
    const uint32_t job = (uint32_t)(r % jobs);
    const uint64_t q = r / jobs;
    if (q >= Q) return;
    const uint32_t nl = min(max(t.n_layers[b], 1u), ML);
    const uint32_t* head = t.head + (size_t)b * t.head_words;
    const uint32_t hb = tc ? 11u : 0u;
    const uint32_t* vals = t.values + ((size_t)b * Q + q) * t.val_words;
    const uint32_t* pth = t.paths + ((size_t)b * Q + q) * t.path_words;
    const uint64_t index = t.indices[(size_t)b * Q + q];
    uint32_t bad = 0u;
    if (job < tc + 2u * ML) {
        // a path climb (the ONE call site of climb): what is opened, where, against which root
        uint32_t value, depth, fails;
        uint64_t pos;
        const uint32_t *p, *root;
        bool act = true;
        if (job < tc) {
            value = vals[job];
            depth = L;
            pos = (index + ((uint64_t)job << t.log_blowup)) & (((uint64_t)1 << L) - 1u);
            p = pth + (size_t)job * 8u * L;
            root = head;
            fails = VB_TRACE_PATH;
        } else {
            const uint32_t k = (job - tc) >> 1, which = (job - tc) & 1u;
            depth = L - k;
            const uint64_t mk = (uint64_t)1 << depth;
            const uint64_t i = index & (mk - 1u);
            act = k < nl;
            value = vals[tc + 2 * k + which];
            pos = which ? ((i + mk / 2u) & (mk - 1u)) : i;
            p = pth + fri_path_off(t, k) + (which ? 8u * depth : 0u);
            root = head + hb + 8 * k;
            fails = VB_FRI_PATH;
        }
        if (act && !climb(value, pos, p, depth, root)) bad = fails;
    } else if (job < tc + 3u * ML) {
        const uint32_t k = job - tc - 2u * ML;
        if (k < nl) {
            const uint32_t v = vals[tc + 2 * k], sv = vals[tc + 2 * k + 1];
            if (v >= P || sv >= P) bad |= VB_MALFORMED;
            if (k + 1 == nl) {
                const uint32_t fin = head[hb + 9 * ML - 1];
                if (v != fin || sv != fin) bad |= VB_FINAL;
            }
            if (k >= 1) {
                const uint32_t pv = vals[tc + 2 * k - 2], psv = vals[tc + 2 * k - 1], beta = head[hb + 8 * ML + k - 1];
                if (v < P && pv < P && psv < P && beta < P) {
                    const uint32_t pdepth = L - k + 1u;                    // layer k - 1: m = 2^pdepth >= 2
                    const uint64_t pm = (uint64_t)1 << pdepth;
                    const uint64_t pi = index & (pm - 1u), pj = pi & (pm / 2u - 1u);
                    const bool low = pi < pm / 2u;
                    const uint32_t pa = low ? pv : psv, pb = low ? psv : pv;
                    const uint32_t x_m = mmul(t.off_m[k - 1], mpow(t.w_m[k - 1], pj));
                    if (fold_one(pa, pb, minv(x_m), to_mont(beta)) != v) bad |= VB_FOLD;
                }
            }
        }
    } else {
        const uint32_t f0 = vals[0], f1 = vals[1], f2 = vals[2];
        if (f0 >= P || f1 >= P || f2 >= P) {
            bad = VB_MALFORMED;
        } else {
            // fibsq_composition_at (stark101.cpp), x = offset w_n^index
            const uint64_t pos = index & (((uint64_t)1 << L) - 1u);
            const uint32_t one_m = R_MOD_P;
            const uint32_t x_m = mmul(t.off_m[0], mpow(t.w_m[0], pos));
            const uint32_t a_last = t.a_last[b];
            const uint32_t d1 = sub(x_m, t.glast_m);
            const uint32_t p0 = mmul(sub(f0, 1u), minv(sub(x_m, one_m)));
            const uint32_t p1 = mmul(sub(f0, a_last), minv(d1));
            const uint32_t num = sub(f2, add(mmul(f1, to_mont(f1)), mmul(f0, to_mont(f0))));
            const uint32_t zf = mmul(mmul(sub(x_m, t.gprev_m), d1), minv(sub(mpow(x_m, (uint64_t)1 << t.log_t), one_m)));
            const uint32_t p2 = mmul(num, zf);
            const uint32_t cp = add(add(mmul(p0, to_mont(head[8])), mmul(p1, to_mont(head[9]))),
                                    mmul(p2, to_mont(head[10])));
            if (cp != vals[tc]) bad = VB_COMPOSITION;
        }
    }
    if (bad) atomicOr(&t.verdict[b], bad);
}

void launch_verify_open(const VerifyTask& t, hipStream_t s) {
    const uint64_t jobs = t.trace_count + 3ull * t.max_layers + (t.trace_count ? 1u : 0u);
    const uint64_t lanes = jobs * t.num_queries * t.members;
    if (!lanes) return;
    hipLaunchKernelGGL(k_verify_open, dim3((unsigned)((lanes + 63u) / 64u)), dim3(64), 0, s, t);
}

}  // namespace fri
