"""Test helper: a model of the batched prover that takes what the library
takes: any canonical trace, any a_last, any three alphas, any coset offset and
any incoming channel state.  Nothing here needs a GPU, and nothing here
imports fri_amd.

commit() is assembled from the C oracle's exported functions
(orc_interpolate_coset, orc_lde, orc_merkle_build, orc_fibsq_cp_evals,
orc_fri_commit_fast), record() and phase() from the Python twin's Channel and
merkle_proof over thin index views of the oracle's flat arrays
(oracle_flat._Values, prover_check._levels).  tests/test_prover_model_host.py
anchors all of it: against orc_fibsq_prove_commit, against the faithful twin
fibsq_prove message for message, against the golden transcripts and, term by
term, against the reference's own polynomial division.

The second half builds the inputs the GPU tests use (isolated alphas, violated
traces, the offsets), so that the host file pins exactly what the device sees.
"""
import ctypes
from collections import namedtuple

import numpy as np

import fri_oracle as fo
from oracle_flat import _Values
from prover_check import _levels

P = fo.P
GEN = fo.GEN
_PU = ctypes.POINTER(ctypes.c_uint64)


def _p(a):
    return a.ctypes.data_as(_PU)


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


TracePart = namedtuple("TracePart", "log_t lb offset coeffs lde tree levels root")


def trace_part(corc, trace, log_t, lb, offset):
    """The trace side: trimmed coefficients (interpolation on <g>, offset 1),
    the LDE on offset * <w_n>, its tree (orc_merkle_build layout) and root."""
    L = log_t + lb
    n, T = 1 << L, 1 << log_t
    tr = _u64(trace)
    assert tr.size == T and int(tr.max()) < P
    fc = np.zeros(T, dtype=np.uint64)
    fl = corc.orc_interpolate_coset(_p(tr), log_t, 1, GEN, P, _p(fc))
    lde = np.zeros(n, dtype=np.uint64)
    assert corc.orc_lde(_p(fc), fl, L, offset, GEN, P, _p(lde)) == 0
    tree = ctypes.create_string_buffer(32 * (2 * n - 1))
    assert corc.orc_merkle_build(_p(lde), n, tree) == 2 * n - 1
    levels = _levels(tree, 0, n)
    return TracePart(log_t, lb, offset, fc[:fl].copy(), lde, tree, levels, levels[-1][0])


def _fri_commit(corc, oracle, coeffs, count, log_n, offset, state):
    """orc_fri_commit_fast continued from `state` (hex, "" = fresh): (result,
    the layers' values, their trees as lists of levels, the state after)."""
    n = 1 << log_n
    och = oracle.OrcChannel()
    corc.orc_channel_init(ctypes.byref(och))
    if state:
        och.state = state.encode()
        och.state_len = 64
    res = oracle.OrcFriResult()
    lay = np.zeros(2 * n, dtype=np.uint64)
    trees = ctypes.create_string_buffer(32 * sum(2 * (n >> k) - 1 for k in range(log_n + 1)))
    assert corc.orc_fri_commit_fast(_p(coeffs), count, log_n, offset, GEN, P, ctypes.byref(och), None,
                                    ctypes.byref(res), _p(lay), trees) == 0
    layers, tlev, lo, to = [], [], 0, 0
    for k in range(res.n_layers):
        m = n >> k
        layers.append(lay[lo:lo + m])
        tlev.append(_levels(trees, to, m))
        lo += m
        to += 2 * m - 1
    return res, layers, tlev, och.state.decode()


Plain = namedtuple("Plain", "log_n offset res layers trees state_in state")


def plain_commit(corc, oracle, coeffs, log_n, offset, state=""):
    """fri_commit of `coeffs` on offset * <w_n>: what a member of a plain
    fri_commit_batch must equal."""
    c = _u64(coeffs)
    res, layers, tlev, out = _fri_commit(corc, oracle, c, c.size, log_n, offset, state)
    return Plain(log_n, offset, res, layers, tlev, state, out)


def result_bytes(model, result_type):
    """The model's commit as the library's fri_commit_result (`result_type`:
    the ctypes mirror of it), every unused root and beta zero."""
    r = result_type()
    res = model.res
    r.n_layers, r.n_rounds = res.n_layers, res.n_rounds
    r.log_n = model.log_n if hasattr(model, "log_n") else model.log_t + model.lb
    r.final_value, r.final_degree = res.final_value, res.final_degree
    for k in range(res.n_layers):
        ctypes.memmove(r.roots[k], bytes(res.roots[k]), 32)
    for k in range(res.n_rounds):
        r.betas[k] = res.betas[k]
    ctypes.memmove(r.channel_out.digest, bytes.fromhex(model.state), 32)
    r.channel_out.has_state = 1
    return bytes(r)


def assert_result(r, layer, model, result_type, what=""):
    """A device commit against the model: `r` the library's result, `layer(k)`
    its read-back of layer k.  The fields one by one (for the message), then
    every byte of the result, then every value of every layer."""
    res = model.res
    same((r.n_layers, r.n_rounds), (res.n_layers, res.n_rounds), (what, "layers, rounds"))
    same([bytes(r.roots[k]).hex()[:16] for k in range(r.n_layers)], [x.hex()[:16] for x in roots(model)],
         (what, "roots"))
    same([int(r.betas[k]) for k in range(r.n_rounds)], betas(model), (what, "betas"))
    same((r.final_value, r.final_degree), (res.final_value, res.final_degree), (what, "final value, degree"))
    same(bytes(r.channel_out.digest).hex(), model.state, (what, "state"))
    assert bytes(r) == result_bytes(model, result_type), what
    for k in range(res.n_layers):
        same(layer(k), model.layers[k], (what, "layer", k))


def same(got, want, what=""):
    """Equality with the first difference in the message: (what, position,
    observed, model)."""
    if isinstance(got, np.ndarray) or isinstance(want, np.ndarray):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, (what, "shape", got.shape, want.shape)
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, (what, "at", int(diff[0]), "observed", int(got.flat[diff[0]]), "model",
                                int(want.flat[diff[0]]), "differing", int(diff.size))
        return
    if isinstance(got, (list, tuple)) and isinstance(want, (list, tuple)) and len(got) == len(want):
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (what, "at", i, "observed", g, "model", w)
        return
    assert got == want, (what, "observed", got, "model", want)


def interpolate_coset(corc, ys, log_n, offset):
    """The trimmed coefficients of the interpolant on offset * <w_n>."""
    y = _u64(ys)
    out = np.zeros(1 << log_n, dtype=np.uint64)
    return out[:corc.orc_interpolate_coset(_p(y), log_n, offset, GEN, P, _p(out))].copy()


Model = namedtuple("Model", "log_t lb offset trace a_last alphas tr cp_evals cp_coeffs cp_degree res layers trees "
                            "state_in state")


def commit(corc, oracle, trace, log_t, lb, offset, a_last, alphas, state, tr=None):
    """Trace commit, composition and FRI commit of one member.  `state`: the
    channel's hex state before the first FRI root ("" = fresh); `tr`: the
    member's trace_part when the caller already has it (it drew the alphas
    after sending its root)."""
    L = log_t + lb
    n = 1 << L
    tr = tr or trace_part(corc, trace, log_t, lb, offset)
    assert (tr.log_t, tr.lb, tr.offset) == (log_t, lb, offset)
    al = (ctypes.c_uint64 * 3)(*[int(a) for a in alphas])
    cp = np.zeros(n, dtype=np.uint64)
    assert corc.orc_fibsq_cp_evals(_p(tr.lde), log_t, lb, offset, GEN, P, int(a_last), al, _p(cp)) == 0
    cc = np.zeros(n, dtype=np.uint64)
    cl = corc.orc_interpolate_coset(_p(cp), L, offset, GEN, P, _p(cc))
    res, layers, tlev, out = _fri_commit(corc, oracle, cc, cl, L, offset, state)
    return Model(log_t, lb, offset, _u64(trace), int(a_last), [int(a) for a in alphas], tr, cp, cc[:cl].copy(),
                 int(cl) - 1, res, layers, tlev, state, out)


def n_layers(model):
    return int(model.res.n_layers)


def roots(model):
    return [bytes(model.res.roots[k]) for k in range(model.res.n_layers)]


def betas(model):
    return [int(model.res.betas[k]) for k in range(model.res.n_rounds)]


def commit_messages(model):
    """The FRI commit's messages: per layer the root's hex, the round's beta
    after it, then the final value."""
    msgs = []
    for k, root in enumerate(roots(model)):
        msgs.append(root.hex().encode())
        if k < model.res.n_rounds:
            msgs.append(int(model.res.betas[k]).to_bytes(8, "big"))
    msgs.append(int(model.res.final_value).to_bytes(8, "big"))
    return msgs


def paths_len(model, trace_count, layers=None):
    L = model.log_t + model.lb
    nl = n_layers(model) if layers is None else layers
    return 32 * L * trace_count + sum(64 * (L - k) for k in range(nl))


def record(model, index, trace_count, trace_stride, max_layers, val_fill=0, path_fill=0):
    """One query's record in fri_batch_query_round's layout: (values, paths),
    a uint32 row of trace_count + 2 * max_layers words and a uint8 row of
    paths_len(model, trace_count, max_layers) bytes.  The trace values
    LDE[(index + j * stride) mod n] and their paths come first, then per layer
    value, sibling and the two paths; what a member with fewer than max_layers
    layers leaves untouched keeps the fill."""
    L = model.log_t + model.lb
    n, nl = 1 << L, n_layers(model)
    assert nl <= max_layers
    values = np.full(trace_count + 2 * max_layers, val_fill, dtype=np.uint32)
    raw = b""
    for j in range(trace_count):
        leaf = (index + j * trace_stride) % n
        values[j] = model.tr.lde[leaf]
        raw += fo.merkle_proof(model.tr.levels, leaf)
    for k in range(nl):
        vals = _Values(model.layers[k])
        m = len(vals)
        idx = index % m
        sib = (idx + m // 2) % m
        values[trace_count + 2 * k] = vals[idx]
        values[trace_count + 2 * k + 1] = vals[sib]
        raw += fo.merkle_proof(model.trees[k], idx) + fo.merkle_proof(model.trees[k], sib)
    assert len(raw) == paths_len(model, trace_count)
    paths = np.full(paths_len(model, trace_count, max_layers), path_fill, dtype=np.uint8)
    paths[:len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return values, paths


def record_messages(model, values, paths, trace_count):
    """The messages one record sends, in prove_fibsq's order; a one-element
    layer's value goes out once more first (fri_commit.rs:137-163)."""
    L = model.log_t + model.lb
    raw = bytes(paths)
    out, off = [], 0
    for j in range(trace_count):
        out += [int(values[j]).to_bytes(8, "big"), raw[off:off + 32 * L]]
        off += 32 * L
    for k in range(n_layers(model)):
        pl = 32 * (L - k)
        v, s = int(values[trace_count + 2 * k]), int(values[trace_count + 2 * k + 1])
        if pl == 0:
            out.append(v.to_bytes(8, "big"))
        out += [v.to_bytes(8, "big"), raw[off:off + pl], s.to_bytes(8, "big"), raw[off + pl:off + 2 * pl]]
        off += 2 * pl
    return out


Phase = namedtuple("Phase", "indices records state messages")


def phase(model, state, num_queries, max_index, trace_count, trace_stride, max_layers=None, val_fill=0, path_fill=0):
    """The query phase replayed with the twin's Channel from `state` (hex):
    per query receive_random_int(0, max_index, True), then the record's
    messages.  Returns the indices, the records (as record() gives them), the
    final state and every message, the drawn indices included."""
    ml = n_layers(model) if max_layers is None else max_layers
    ch = fo.Channel(state=state)
    indices, records = [], []
    for _ in range(num_queries):
        idx = ch.receive_random_int(0, max_index, True)
        indices.append(idx)
        values, paths = record(model, idx, trace_count, trace_stride, ml, val_fill, path_fill)
        records.append((values, paths))
        for m in record_messages(model, values, paths, trace_count):
            ch.send(m)
    return Phase(indices, records, ch.state, ch.proof)


Proof = namedtuple("Proof", "model alphas messages state queries")


def prove(corc, oracle, trace, log_t, lb, offset, num_queries, state="", a_last=None):
    """prove_fibsq's whole transcript for `trace`: the trace root, three
    alphas drawn from the channel, the FRI commit, then num_queries queries
    drawn from 0..n - 2B - 1 opening f(x), f(gx), f(g^2 x)."""
    L = log_t + lb
    n, B = 1 << L, 1 << lb
    tr = trace_part(corc, trace, log_t, lb, offset)
    ch = fo.Channel(state=state)
    ch.send(tr.root.hex().encode())
    alphas = [ch.receive_random_field_element() for _ in range(3)]
    m = commit(corc, oracle, trace, log_t, lb, offset, int(trace[-1]) if a_last is None else a_last, alphas, ch.state,
               tr=tr)
    ph = phase(m, m.state, num_queries, n - 2 * B - 1, 3, B)
    return Proof(m, alphas, ch.proof + commit_messages(m) + ph.messages, ph.state, ph.indices)


# ---- the inputs of the GPU tests ---------------------------------------------------
def root_of_unity(log_n):
    return pow(GEN, (P - 1) >> log_n, P)


# one seeded offset above 2^31: the first such value of the stream
BIG_OFFSET = next(int(v) for v in fo.splitmix64_field(20261021, 64) if v > 1 << 31)


def accepted_offsets(log_t, lb):
    """Offsets off the default coset that fibsq_shape accepts: 7, p - 2, one
    seeded value above 2^31, and w_2n, a primitive 2n-th root, whose T-th power
    w_2B lies outside <w_B>."""
    return [7, P - 2, BIG_OFFSET, root_of_unity(log_t + lb + 1)]


def refused_offsets(log_t, lb):
    """Offsets whose T-th power lies in <w_B>: the coset meets the trace domain."""
    return [root_of_unity(log_t + lb), root_of_unity(log_t), P - 1, 1]


def offset_is_accepted(offset, log_t, lb):
    """fibsq_shape's check: offset^T * w_B^j != 1 for every j < B."""
    ot, wb = pow(offset, 1 << log_t, P), root_of_unity(lb)
    return all(ot * pow(wb, j, P) % P != 1 for j in range(1 << lb))


def random_trace(seed, T):
    return fo.splitmix64_np(seed, T)


def recurrence_trace(a0, a1, T):
    """The FibonacciSq recurrence from arbitrary (a_0, a_1)."""
    a = [a0 % P, a1 % P]
    while len(a) < T:
        a.append((a[-1] * a[-1] + a[-2] * a[-2]) % P)
    return _u64(a[:T])


Member = namedtuple("Member", "name trace a_last alphas degree")


def isolated_members(log_t, seed=1):
    """One member per isolated term, then all alphas zero.  `degree`: the
    composition's, as the host file pins it (T - 2, T - 2, T, -1; at T = 4 the
    third term's leading coefficients cancel, g^2 = -1, and it is 3)."""
    T = 1 << log_t
    a = [int(x) for x in fo.splitmix64_field(seed + 100, 3)]
    t0 = random_trace(seed, T).copy()
    t0[0] = 1
    t1 = random_trace(seed + 1, T)
    t2 = recurrence_trace(int(fo.splitmix64_field(seed + 2, 1)[0]), int(fo.splitmix64_field(seed + 3, 1)[0]), T)
    t3 = random_trace(seed + 4, T)
    return [Member("first_row", t0, int(fo.splitmix64_field(seed + 5, 1)[0]), [a[0], 0, 0], T - 2),
            Member("last_row", t1, int(t1[-1]), [0, a[1], 0], T - 2),
            Member("recurrence", t2, int(fo.splitmix64_field(seed + 6, 1)[0]), [0, 0, a[2]], T if T > 4 else 3),
            Member("no_term", t3, int(t3[-1]), [0, 0, 0], -1)]


def ordinary_member(log_t, a1=3141592, seed=7):
    """A valid FibonacciSq trace with three nonzero alphas."""
    T = 1 << log_t
    t = recurrence_trace(1, a1, T)
    return Member("ordinary", t, int(t[-1]), [int(x) for x in fo.splitmix64_field(seed + 200, 3)],
                  T if T > 4 else 3)


def violated_members(log_t, lb, a1=11, seed=9):
    """Four violations of a valid trace, three nonzero alphas each: the
    composition's degree is n - 1, above T.  recurrence_only() gives the same
    traces the alphas (0, 0, a): the members named in BOUNDARY_ONLY, whose rows
    still obey the recurrence, are then accepted; the others keep degree n - 1
    (rows 0 and T - 1 feed the recurrence too)."""
    T, n = 1 << log_t, 1 << (log_t + lb)
    base = recurrence_trace(1, a1, T)
    al = [int(x) for x in fo.splitmix64_field(seed + 300, 3)]
    first = base.copy()
    first[0] = 2
    middle = base.copy()
    middle[T // 2] = (int(middle[T // 2]) + 1) % P
    last = base.copy()
    last[-1] = (int(last[-1]) + 1) % P
    return [Member("first_row_2", first, int(base[-1]), al, n - 1),
            Member("a_last_plus_1", base, (int(base[-1]) + 1) % P, al, n - 1),
            Member("middle_row_plus_1", middle, int(base[-1]), al, n - 1),
            Member("last_row_plus_1", last, int(last[-1]), al, n - 1)]


BOUNDARY_ONLY = ("a_last_plus_1", "first_row_2_from_row_0")


def recurrence_only(log_t, lb, a1=11, seed=9):
    """violated_members' traces, and the recurrence run from (2, a1), with the
    alphas (0, 0, a): only the recurrence is asked for, so the degree (T, or 3
    at T = 4) accepts the members of BOUNDARY_ONLY and no other."""
    T, n = 1 << log_t, 1 << (log_t + lb)
    a = int(fo.splitmix64_field(seed + 400, 1)[0])
    t = recurrence_trace(2, a1, T)
    members = violated_members(log_t, lb, a1, seed) + [Member("first_row_2_from_row_0", t, int(t[-1]), None, None)]
    ok = T if T > 4 else 3
    return [m._replace(alphas=[0, 0, a], degree=ok if m.name in BOUNDARY_ONLY else n - 1) for m in members]
