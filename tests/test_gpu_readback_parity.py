"""GPU: the member-wise read-backs (fri_batch_*) against the single-commit
ones, byte for byte.

One polynomial of d = n/8 coefficients is committed alone (Context.commit) and
as member 1 of a 3-member batch whose neighbours differ.  Every layer, every
level of the trees of layers 0, 1 and the last, the degrees and four query
decommitments are kept as bytes from the single entry points, checked against
the C oracle's stored proof (oracle/fri_oracle.py), and then demanded of
fri_batch_* for member 1.  At 2^7 the commit is the tail kernel's alone, at
2^13 the wide leaf kernel's plus a top.  The refusals of both families are
walked through raw ctypes calls: the same code from an entry point and its
twin, and nothing written to the output buffers but *paths_len."""
import ctypes

import numpy as np
import pytest

import degree_cases as dc
import stored_proof as sp

pytestmark = pytest.mark.gpu

import fri_amd  # noqa: E402

LOGS = (7, 13)
MARK = 0xA5
E, S = fri_amd.FRI_EINVAL, fri_amd.FRI_ESTATE


def _polys(oracle, log_n):
    d = (1 << log_n) // 8
    return [oracle.splitmix64_np(4100 + 10 * log_n + b, d).astype(np.uint32) for b in range(3)]


@pytest.fixture(scope="module")
def want(corc, oracle):
    """The oracle's stored proof of the shared polynomial (member 1), once per size."""
    return {log_n: sp.oracle_commit_full(corc, oracle, _polys(oracle, log_n)[1], log_n) for log_n in LOGS}


def _indices(log_n):
    n = 1 << log_n
    return (0, n // 2 - 1, n - 1, n + 3)


def _tree_layers(n_layers):
    return sorted({0, 1, n_layers - 1})


def _paths_bytes(n_layers, log_n):
    return sum(64 * (log_n - k) for k in range(n_layers))


class Single:
    """The single entry points with the member-wise ones' argument lists."""

    def __init__(self, ctx):
        self.ctx, lib, h = ctx, ctx.lib, ctx.h
        self.layer_copy = lambda layer, out, cap: lib.fri_layer_copy(h, layer, out, cap)
        self.tree_level_copy = lambda layer, level, out, cap: lib.fri_tree_level_copy(h, layer, level, out, cap)
        self.commit_degrees = lambda out, cap, n: lib.fri_commit_degrees(h, out, cap, n)
        self.decommit_query = lambda *a: lib.fri_decommit_query(h, *a)


class Member:
    def __init__(self, ctx, member):
        self.ctx, lib, h = ctx, ctx.lib, ctx.h
        self.layer_copy = lambda layer, out, cap: lib.fri_batch_layer_copy(h, member, layer, out, cap)
        self.tree_level_copy = lambda layer, level, out, cap: lib.fri_batch_tree_level_copy(h, member, layer, level,
                                                                                            out, cap)
        self.commit_degrees = lambda out, cap, n: lib.fri_batch_commit_degrees(h, member, out, cap, n)
        self.decommit_query = lambda *a: lib.fri_batch_decommit_query(h, member, *a)


def _read_all(rb, log_n, n_layers):
    """Every read-back of the resident proof behind `rb`, as bytes."""
    ck = rb.ctx._check
    got = {}
    for k in range(n_layers):
        out = np.empty(1 << (log_n - k), dtype=np.uint32)
        ck(rb.layer_copy(k, fri_amd._ptr(out), out.size))
        got["layer", k] = out.tobytes()
    for k in _tree_layers(n_layers):
        for level in range(log_n - k + 1):
            buf = ctypes.create_string_buffer(32 << (log_n - k - level))
            ck(rb.tree_level_copy(k, level, buf, len(buf)))
            got["tree", k, level] = buf.raw
    deg, n = (ctypes.c_int32 * (fri_amd.MAX_ROUNDS + 1))(), ctypes.c_uint32()
    ck(rb.commit_degrees(deg, len(deg), ctypes.byref(n)))
    got["degrees"] = [int(deg[k]) for k in range(n.value)]
    total = _paths_bytes(n_layers, log_n)
    for index in _indices(log_n):
        vals, buf, ln = np.empty(2 * n_layers, dtype=np.uint32), ctypes.create_string_buffer(total), ctypes.c_size_t()
        ck(rb.decommit_query(index, fri_amd._ptr(vals), vals.size, buf, total, ctypes.byref(ln)))
        assert ln.value == total
        got["query", index] = (vals.tobytes(), buf.raw)
    return got


@pytest.mark.parametrize("log_n", LOGS)
def test_member_read_backs_equal_the_single_commits(ctx, oracle, want, log_n):
    polys, full = _polys(oracle, log_n), want[log_n]
    res = ctx.commit(polys[1], log_n)
    nl = full.n_layers
    assert res.n_layers == nl
    single = _read_all(Single(ctx), log_n, nl)
    # the single path against the oracle's stored proof
    for k in range(nl):
        assert single["layer", k] == full.values[k].tobytes(), k
    for k in _tree_layers(nl):
        for level in range(log_n - k + 1):
            assert single["tree", k, level] == full.levels[k][level].tobytes(), (k, level)
    assert single["degrees"] == dc.degree_schedule(polys[1], full.betas + [0] * dc.N_BETAS)
    for index in _indices(log_n):
        vals, paths = [], b""
        for k in range(nl):
            m = 1 << (log_n - k)
            idx, sib = index % m, (index % m + m // 2) % m
            vals += [int(full.values[k][idx]), int(full.values[k][sib])]
            paths += sp.expected_path(full.levels[k], idx) + sp.expected_path(full.levels[k], sib)
        assert single["query", index] == (np.array(vals, dtype=np.uint32).tobytes(), paths), index
    # member 1 of a batch with two other neighbours: the same bytes
    bres = ctx.commit_batch(polys, log_n)
    assert ctx.batch_status == [0, 0, 0] and sp.transcript_of(bres[1]) == sp.transcript_of(res)
    assert sp.transcript_of(bres[0]) != sp.transcript_of(res) != sp.transcript_of(bres[2])
    member = _read_all(Member(ctx, 1), log_n, nl)
    assert member.keys() == single.keys()
    for key in single:
        assert member[key] == single[key], key


def _refusals(rb, log_n, nl):
    """(case, code, *paths_len or *n_out, whether the marker in the output
    buffers survived) of every refusal the two families share."""
    total = _paths_bytes(nl, log_n)
    out = []

    def query(case, values_cap, paths, paths_cap):
        vals = np.full(2 * nl, MARK, dtype=np.uint32)
        buf = ctypes.create_string_buffer(bytes([MARK]) * total, total)
        ln = ctypes.c_size_t(12345)
        rc = rb.decommit_query(3, fri_amd._ptr(vals), values_cap, buf if paths else None, paths_cap, ctypes.byref(ln))
        out.append((case, rc, ln.value, bool((vals == MARK).all()) and buf.raw == bytes([MARK]) * total))

    query("paths NULL", 2 * nl, False, total)
    query("paths one byte short", 2 * nl, True, total - 1)
    query("values one word short", 2 * nl - 1, True, total)

    def layer(case, k, short):
        m = 1 << max(log_n - k, 0)
        arr = np.full(m, MARK, dtype=np.uint32)
        rc = rb.layer_copy(k, fri_amd._ptr(arr), m - short)
        out.append((case, rc, None, bool((arr == MARK).all())))

    def level(case, k, lv, cnt):
        buf = ctypes.create_string_buffer(bytes([MARK]) * (32 * cnt), 32 * cnt)
        rc = rb.tree_level_copy(k, lv, buf, len(buf))
        out.append((case, rc, None, buf.raw == bytes([MARK]) * (32 * cnt)))

    layer("layer n_layers", nl, 0)
    level("tree layer n_layers", nl, 0, 1 << (log_n - nl))
    level("level L + 1", 1, log_n - 1 + 1, 1)
    layer("layer cap one word short", 1, 1)
    deg, n = (ctypes.c_int32 * nl)(*([MARK] * nl)), ctypes.c_uint32()
    rc = rb.commit_degrees(deg, nl - 1, ctypes.byref(n))
    out.append(("degrees cap short", rc, n.value, list(deg) == [MARK] * nl))
    return out


@pytest.mark.parametrize("log_n", LOGS)
def test_refusals_agree_and_write_nothing(ctx, oracle, want, log_n):
    polys, nl = _polys(oracle, log_n), want[log_n].n_layers
    total = _paths_bytes(nl, log_n)
    expect = [("paths NULL", E, total), ("paths one byte short", E, total), ("values one word short", E, total),
              ("layer n_layers", S, None), ("tree layer n_layers", S, None), ("level L + 1", E, None),
              ("layer cap one word short", E, None), ("degrees cap short", E, nl)]
    ctx.commit(polys[1], log_n)
    single = _refusals(Single(ctx), log_n, nl)
    ctx.commit_batch(polys, log_n)
    member = _refusals(Member(ctx, 1), log_n, nl)
    for got in (single, member):
        assert [r[:3] for r in got] == expect
        assert all(r[3] for r in got), [r[0] for r in got if not r[3]]
    # member = batch: no such member, whatever else is asked
    beyond = _refusals(Member(ctx, 3), log_n, nl)
    assert [r[1] for r in beyond] == [E] * len(beyond) and all(r[3] for r in beyond)
    assert [r[2] for r in beyond[:3]] == [12345] * 3        # refused before *paths_len is known
    # the refusals left both proofs readable
    vals = ctx.batch_decommit_query(1, 3, nl, log_n)
    ctx.commit(polys[1], log_n)
    assert ctx.decommit_query(3, nl, log_n) == vals
