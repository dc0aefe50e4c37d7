"""CPU: tests/prover_model.py anchored before a GPU test trusts it, and the
inputs of tests/test_gpu_offsets.py and tests/test_gpu_composition_terms.py
pinned: a GPU test never rests on an input that is not what it claims.

The anchors: orc_fibsq_prove_commit (the C oracle's own prover) at offsets 5
and 7, the faithful twin fibsq_prove message for message, the golden
transcripts, and the reference's polynomial division for each isolated term."""
import ctypes
import hashlib

import numpy as np
import pytest

import prover_model as pm

P = pm.P
SHAPES = [(2, 1), (4, 2), (6, 3), (7, 3), (9, 3), (10, 3), (13, 1)]      # every shape a GPU test uses


def _proof_sha(msgs):
    return hashlib.sha256(b"".join(len(m).to_bytes(4, "little") + m for m in msgs)).hexdigest()


# ---- 1. the C oracle's own prover ---------------------------------------------------
@pytest.mark.parametrize("offset", [5, 7])
@pytest.mark.parametrize("log_t,lb", [(2, 1), (4, 2), (6, 3), (10, 3), (13, 1)])
def test_equals_orc_fibsq_prove_commit(corc, oracle, log_t, lb, offset):
    a1 = 3141592
    n = 1 << (log_t + lb)
    och = oracle.OrcChannel()
    corc.orc_channel_init(ctypes.byref(och))
    root = ctypes.create_string_buffer(32)
    al = (ctypes.c_uint64 * 3)()
    res = oracle.OrcFriResult()
    fe = np.zeros(n, dtype=np.uint64)
    assert corc.orc_fibsq_prove_commit(a1, log_t, lb, offset, 5, P, ctypes.byref(och), root, al, ctypes.byref(res),
                                       fe.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None, None, None) == 0
    pr = pm.prove(corc, oracle, pm.recurrence_trace(1, a1, 1 << log_t), log_t, lb, offset, 0)
    m = pr.model
    assert m.tr.root == root.raw and pr.alphas == list(al)
    assert (m.tr.lde == fe).all()
    assert pm.roots(m) == [bytes(res.roots[k]) for k in range(res.n_layers)]
    assert pm.betas(m) == [int(res.betas[k]) for k in range(res.n_rounds)]
    assert m.res.final_value == res.final_value and m.res.final_degree == res.final_degree
    assert m.state == och.state.decode() == pr.state
    assert m.cp_degree == ((1 << log_t) if log_t > 2 else 3)


# ---- 2. the faithful twin, message for message --------------------------------------
@pytest.mark.parametrize("offset", [5, 7])
@pytest.mark.parametrize("log_t,lb", [(2, 1), (4, 2)])
@pytest.mark.parametrize("a1", [3141592, 7])
def test_equals_the_faithful_twin(corc, oracle, a1, log_t, lb, offset):
    ch = oracle.Channel()
    want = oracle.fibsq_prove(a1, log_t, lb, 2, ch, offset=offset)
    pr = pm.prove(corc, oracle, pm.recurrence_trace(1, a1, 1 << log_t), log_t, lb, offset, 2)
    assert pr.messages == ch.proof
    assert pr.state == ch.state and pr.queries == want.queries
    assert pr.model.tr.root == want.trace_root and pr.alphas == want.alphas
    for k, lay in enumerate(want.fri.layers):
        assert [int(v) for v in pr.model.layers[k]] == lay, k


# ---- 3. the golden transcripts -------------------------------------------------------
def test_reproduces_the_golden_transcripts(corc, oracle, golden):
    assert golden["fibsq"]
    for c in golden["fibsq"]:
        pr = pm.prove(corc, oracle, pm.recurrence_trace(1, c["a1"], 1 << c["log_t"]), c["log_t"], c["log_blowup"], 5,
                      c["queries"], state=c["channel_in"])
        m = pr.model
        assert m.tr.root.hex() == c["trace_root"] and pr.alphas == c["alphas"] and m.a_last == c["a_last"], c["name"]
        assert [r.hex() for r in pm.roots(m)] == c["roots"] and pm.betas(m) == c["betas"], c["name"]
        assert m.res.final_value == c["final_value"] and m.res.final_degree == c["final_degree"], c["name"]
        assert pr.queries == c["query_indices"] and pr.state == c["channel_out"], c["name"]
        assert len(pr.messages) == c["messages"] and _proof_sha(pr.messages) == c["proof_sha256"], c["name"]


# ---- 4. each isolated term against the reference's polynomial arithmetic ------------
@pytest.mark.parametrize("offset", [5, 7])
@pytest.mark.parametrize("log_t,lb", [(2, 1), (4, 2)])
def test_isolated_terms_equal_the_reference_division(corc, oracle, log_t, lb, offset):
    T = 1 << log_t
    g = pm.root_of_unity(log_t)
    first, last = pm.isolated_members(log_t)[:2]
    assert last.a_last == int(last.trace[-1])
    for mem, const, point in ((first, 1, 1), (last, last.a_last, pow(g, T - 1, P))):
        m = pm.commit(corc, oracle, mem.trace, log_t, lb, offset, mem.a_last, mem.alphas, "")
        f = [int(c) for c in m.tr.coeffs]
        alpha = max(mem.alphas)
        q, r = oracle.poly_div_rem(oracle.poly_sub(f, [const], P), [(P - point) % P, 1], P)
        assert r == []                                           # the division is exact
        term = oracle.poly_trim(oracle.poly_scalar_mul(q, alpha, P))
        want = [oracle.poly_evaluate(term, x, P) for x in oracle.coset_domain(log_t + lb, offset)]
        assert [int(v) for v in m.cp_evals] == want, mem.name
        assert [int(c) for c in m.cp_coeffs] == term and m.cp_degree == T - 2, mem.name


# ---- 5. the inputs of the GPU tests ---------------------------------------------------
@pytest.mark.parametrize("offset", [5, 7])
@pytest.mark.parametrize("log_t,lb", [(2, 1), (4, 2), (6, 3), (10, 3)])
def test_member_degrees_are_what_they_claim(corc, oracle, log_t, lb, offset):
    T, L = 1 << log_t, log_t + lb
    n = 1 << L
    iso = pm.isolated_members(log_t)
    assert [m.alphas.count(0) for m in iso] == [2, 2, 2, 3] and int(iso[0].trace[0]) == 1
    assert [m.degree for m in iso] == [T - 2, T - 2, T if T > 4 else 3, -1]
    assert iso[1].a_last == int(iso[1].trace[-1]) and iso[2].a_last != int(iso[2].trace[-1])
    assert int(iso[2].trace[0]) != 1                             # arbitrary (a_0, a_1)
    ordinary = pm.ordinary_member(log_t)
    assert all(ordinary.alphas) and int(ordinary.trace[0]) == 1
    bad = pm.violated_members(log_t, lb)
    assert [m.degree for m in bad] == [n - 1] * 4 and n - 1 > T
    base = pm.recurrence_trace(1, 11, T)
    assert int(bad[0].trace[0]) == 2 and (bad[0].trace[1:] == base[1:]).all()
    assert (bad[1].trace == base).all() and bad[1].a_last == (int(base[-1]) + 1) % P
    assert int((bad[2].trace != base).sum()) == 1 and bad[2].trace[T // 2] != base[T // 2]
    assert (bad[3].trace[:-1] == base[:-1]).all() and bad[3].a_last == int(bad[3].trace[-1]) != int(base[-1])
    rec = pm.recurrence_only(log_t, lb)
    assert [m.name for m in rec if m.degree <= T] == list(pm.BOUNDARY_ONLY)
    for mem in iso + [ordinary] + bad + rec:
        m = pm.commit(corc, oracle, mem.trace, log_t, lb, offset, mem.a_last, mem.alphas, "")
        assert m.cp_degree == mem.degree, (mem.name, m.cp_degree)
        assert m.res.final_degree == (0 if mem.degree >= 0 else -1), mem.name
    none = pm.commit(corc, oracle, iso[3].trace, log_t, lb, offset, iso[3].a_last, iso[3].alphas, "")
    assert pm.n_layers(none) == 1 and none.res.final_value == 0 and not none.cp_evals.any()
    # the members of one batch end at different layers
    assert len({pm.n_layers(pm.commit(corc, oracle, m.trace, log_t, lb, offset, m.a_last, m.alphas, ""))
                for m in iso}) > 1


def test_constant_traces_with_the_last_row_term_alone(corc, oracle):
    # (f - c) / (x - g^(T-1)) of a constant trace is the zero polynomial: such
    # members are accepted with one layer beside the random ones
    log_t, lb = 4, 2
    for c in (0, 12345, P - 1):
        m = pm.commit(corc, oracle, np.full(1 << log_t, c, dtype=np.uint64), log_t, lb, 7, c, [0, 99, 0], "")
        assert m.cp_degree == -1 and pm.n_layers(m) == 1
    t = pm.random_trace(3, 1 << log_t)
    assert pm.commit(corc, oracle, t, log_t, lb, 7, int(t[-1]), [0, 99, 0], "").cp_degree == (1 << log_t) - 2


@pytest.mark.parametrize("log_t,lb", SHAPES)
def test_offsets_are_what_they_claim(log_t, lb):
    L = log_t + lb
    acc, ref = pm.accepted_offsets(log_t, lb), pm.refused_offsets(log_t, lb)
    assert acc[:3] == [7, P - 2, pm.BIG_OFFSET] and (1 << 31) < pm.BIG_OFFSET < P
    w2n = acc[3]
    assert pow(w2n, 1 << L, P) == P - 1                          # a primitive 2n-th root
    assert pow(w2n, 1 << log_t, P) == pm.root_of_unity(lb + 1)   # offset^T = w_2B, outside <w_B>
    assert all(0 < o < P and o != 5 and pm.offset_is_accepted(o, log_t, lb) for o in acc)
    assert pm.offset_is_accepted(5, log_t, lb)
    assert ref == [pm.root_of_unity(L), pm.root_of_unity(log_t), P - 1, 1] and len(set(ref)) == 4
    assert not any(pm.offset_is_accepted(o, log_t, lb) for o in ref)


# ---- 6. the records: every path authenticates its value, the wrap included ----------
def _walk(value, leaf, path, depth):
    h = hashlib.sha256(int(value).to_bytes(8, "big")).digest()
    for lv in range(depth):
        sib = path[32 * lv:32 * lv + 32]
        h = hashlib.sha256(sib + h if (leaf >> lv) & 1 else h + sib).digest()
    return h


@pytest.mark.parametrize("count,stride", [(1, 0), (3, 4), (8, 67), (8, (1 << 63) + 5)])
def test_record_paths_authenticate(corc, oracle, count, stride):
    log_t, lb, L = 4, 2, 6
    n = 1 << L
    mem = pm.ordinary_member(log_t)
    m = pm.commit(corc, oracle, mem.trace, log_t, lb, 7, mem.a_last, mem.alphas, "")
    nl = pm.n_layers(m)
    for index in (0, n - 1):
        values, paths = pm.record(m, index, count, stride, nl + 1, val_fill=0xA5A5A5A5, path_fill=0x5A)
        raw = bytes(paths)
        assert len(raw) == pm.paths_len(m, count, nl + 1)
        for j in range(count):
            leaf = (index + j * stride) % n
            assert int(values[j]) == int(m.tr.lde[leaf])
            assert _walk(values[j], leaf, raw[32 * L * j:32 * L * (j + 1)], L) == m.tr.root
        off = 32 * L * count
        for k in range(nl):
            mk = n >> k
            idx = index % mk
            for s, leaf in enumerate((idx, (idx + mk // 2) % mk)):
                assert _walk(values[count + 2 * k + s], leaf, raw[off:off + 32 * (L - k)], L - k) == pm.roots(m)[k]
                off += 32 * (L - k)
        assert off == pm.paths_len(m, count)
        assert (values[count + 2 * nl:] == 0xA5A5A5A5).all() and (paths[off:] == 0x5A).all()
    if count == 8:
        assert n - 1 + 7 * stride >= n                            # the openings wrap
