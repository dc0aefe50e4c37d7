"""GPU: what a commit leaves in HBM, node for node against the C oracle.

A right root does not imply right stored levels: the leaf, mid and top
kernels (k_layer_leaf, k_layer_leaf_wide, k_tree_mid, k_tree_mid8,
k_tree_top, k_tree_tail; csrc/fri_layer.hip) keep a subtree in registers, DPP
lanes or LDS, and only the last level a kernel writes is read back by the
next one.  Every other level, and every layer's values past the next fold, is
stored as a side effect that the transcript never sees, yet fri_layer_copy,
fri_tree_level_copy, fri_auth_path, fri_decommit_query and fri_trace_decommit
serve exactly those words later.  Here every stored value and every node of
every level of every layer is compared with orc_fri_commit_fast's layers_out
and trees_out (tests/stored_proof.py), bit for bit, and the gather kernels are
swept over every index.  A failure names the layer, level, node and the
leaf-kernel workgroup above it.

Sizes follow launch_layer's schedule (TOP_LOG = TAIL_LOG = 9, QUAD_MIN_LOG =
19), so that each kernel runs both on layer 0 (no fold) and behind a fused
fold on the layers below it:
  2^5, 2^9    k_tree_tail: every layer of <= 2^9 values of a commit runs there
              (k_tree_top from the leaves serves only trees built outside a
              commit: the 2^9 trace tree below)
  2^10..2^17  k_layer_leaf_wide with 8 levels, then a top over 4, 32, 512 nodes
  2^18        wide leaf with 4 levels, k_tree_mid8, top
  2^19, 2^21  quad k_layer_leaf, k_tree_mid8, a top over 128 and 512 nodes
  2^22        quad leaf, k_tree_mid, k_tree_mid8, top: the smallest size
              that reaches every kernel (larger ones add grid size and a
              second k_tree_mid, no new store path).

The mid kernels have no other size class: launch_layer's loop takes k_tree_mid
while L - l >= 18 and then k_tree_mid8 once (the argument is in its comment)."""
import ctypes

import numpy as np
import pytest

import stored_proof as sp

pytestmark = pytest.mark.gpu

BIG = 22            # the ceiling: a 256 MiB tree readback for layer 0 alone
BIG_SEED = 2200


def _commit_and_compare(ctx, corc, oracle, log_n, d, seed, offset=5, state=None, graph=True):
    coeffs = oracle.splitmix64_np(seed, d).astype(np.uint32)
    full = sp.oracle_commit_full(corc, oracle, coeffs, log_n, offset=offset, state=state)
    res = ctx.commit(coeffs, log_n, offset, channel_state=state, graph=graph)
    # the oracle run is the one the GPU mirrored
    assert res.n_layers == full.n_layers
    assert sp.transcript_of(res) == sp.transcript_want(full)
    msg = sp.stored_proof_mismatch(ctx, full, log_n)
    assert msg is None, msg
    return full, res


# ---- 1. every layer value and tree node of a single-GPU commit -------------
@pytest.mark.parametrize("log_n", [5, 9, 10, 13, 17, 18, 19, 21])
def test_stored_proof_matches_oracle(ctx, corc, oracle, log_n):
    """Blowup 8: every committed layer's values and every level of its tree."""
    full, _ = _commit_and_compare(ctx, corc, oracle, log_n, (1 << log_n) >> 3, 100 + log_n)
    assert full.n_layers == log_n - 2


@pytest.fixture(scope="module")
def big(ctx, corc, oracle):
    """The 2^22 polynomial and the oracle's whole commit of it, computed once:
    the single-GPU test, the team test and the sampled gathers share it."""
    coeffs = oracle.splitmix64_np(BIG_SEED, (1 << BIG) >> 3).astype(np.uint32)
    full = sp.oracle_commit_full(corc, oracle, coeffs, BIG)
    return {"coeffs": coeffs, "full": full, "generation": None}


def _big_resident(ctx, big):
    """The 2^22 commit resident on the shared context: committed once, and
    again only if another commit replaced it in between."""
    if big["generation"] is None or ctx.commit_info()[0] != big["generation"]:
        res = ctx.commit(big["coeffs"], BIG)
        assert sp.transcript_of(res) == sp.transcript_want(big["full"])
        big["generation"] = ctx.commit_info()[0]
    return big["full"]


def test_stored_proof_matches_oracle_2p22(ctx, big):
    """Quad leaf, k_tree_mid, k_tree_mid8 and top on layer 0, and every
    smaller schedule behind a fused fold below it: 2^23 values and 2^23 nodes."""
    full = _big_resident(ctx, big)
    assert full.n_layers == BIG - 2
    msg = sp.stored_proof_mismatch(ctx, full, BIG)
    assert msg is None, msg


SAMPLE = [0, 1, (1 << BIG) // 2 - 1, (1 << BIG) // 2, (1 << BIG) - 1] + \
    [int(v) for v in np.random.default_rng(20220).integers(0, 1 << BIG, 64)]


def _check_query(ctx, full, log_n, index, paths=None):
    """fri_decommit_query of `index` against the oracle's values and paths,
    every layer.  paths[k]: layer k's sp.path_table over all its leaves, if built."""
    got = ctx.decommit_query(index, full.n_layers, log_n)
    assert len(got) == full.n_layers
    for k, (val, sval, path, spath) in enumerate(got):
        m = (1 << log_n) >> k
        idx = index % m
        sib = (idx + m // 2) % m
        where = f"decommit_query({index}): layer {k} idx {idx} sib {sib}"
        assert (val, sval) == (int(full.values[k][idx]), int(full.values[k][sib])), where
        for name, leaf, p in (("path", idx, path), ("sibling path", sib, spath)):
            want = paths[k][leaf].tobytes() if paths else sp.expected_path(full.levels[k], leaf)
            if p != want:
                assert len(p) == len(want), where
                lvl = next(l for l in range(log_n - k) if p[32 * l:32 * l + 32] != want[32 * l:32 * l + 32])
                raise AssertionError(f"{where}: {name} of leaf {leaf} differs at level {lvl} "
                                     f"(node {(leaf >> lvl) ^ 1}): got {p[32 * lvl:32 * lvl + 32].hex()} "
                                     f"want {want[32 * lvl:32 * lvl + 32].hex()}")


def _check_auth_path(ctx, full, log_n, k, i, paths=None):
    val, path = ctx.auth_path(k, i, log_n)
    assert val == int(full.values[k][i]), f"auth_path(layer {k}, {i}): value"
    want = paths[k][i].tobytes() if paths else sp.expected_path(full.levels[k], i)
    assert b"".join(path) == want, f"auth_path(layer {k}, {i}): path"


def test_gathers_sampled_2p22(ctx, big):
    """Both gather entry points on the 2^22 commit of the test above (reused,
    not committed again): the corners, the halves and 64 seeded indices."""
    full = _big_resident(ctx, big)
    for index in SAMPLE:
        _check_query(ctx, full, BIG, index)
        for k in range(full.n_layers):
            _check_auth_path(ctx, full, BIG, k, index % ((1 << BIG) >> k))


def test_stored_proof_blowup_1(ctx, corc, oracle):
    """d = n at 2^11: log_n + 1 layers, the last of one element (a tree of one node)."""
    full, _ = _commit_and_compare(ctx, corc, oracle, 11, 1 << 11, 1111)
    assert full.n_layers == 12 and full.values[-1].size == 1 and len(full.levels[-1]) == 1


def test_stored_proof_high_blowup(ctx, corc, oracle):
    """(log_n, d) = (16, 4): the final send runs in a k_tree_top and the later
    layers are gated off; layers and trees are served for res.n_layers only."""
    import fri_amd
    full, res = _commit_and_compare(ctx, corc, oracle, 16, 4, 1604)
    assert res.n_layers == 3
    buf = np.zeros(1 << 16, dtype=np.uint32)
    assert ctx.lib.fri_layer_copy(ctx.h, res.n_layers, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                  buf.size) == fri_amd.FRI_ESTATE
    assert ctx.lib.fri_tree_level_copy(ctx.h, res.n_layers, 0, buf.ctypes.data_as(ctypes.c_char_p),
                                       buf.nbytes) == fri_amd.FRI_ESTATE


def test_stored_proof_offset_and_channel_state(ctx, corc, oracle):
    """A non-default coset offset and a pre-filled channel state at 2^19."""
    _commit_and_compare(ctx, corc, oracle, 19, 1 << 16, 1907, offset=7,
                        state=bytes.fromhex("c3" * 16 + "5a" * 16))


def test_stored_proof_eager(ctx, corc, oracle):
    """graph=False at 2^19: the same launches, issued without the captured graph."""
    _commit_and_compare(ctx, corc, oracle, 19, 1 << 16, 1908, graph=False)


# ---- 2. team (sharded) trees against the oracle ------------------------------
@pytest.fixture(scope="module")
def team4():
    import fri_amd
    c = fri_amd.Context.multi([0, 0, 0, 0], 23, transport="peer")
    yield c
    c.close()


def test_team_stored_proof_matches_oracle(team4, big):
    """A 4-rank team commit at 2^22, read back whole, against the oracle (not
    against another GPU commit): the PAIR leaf kernels, the block-local
    levels 2..lb-1, the SHARD top, and the top tree that team_tree_level_copy
    stitches above the block roots."""
    full = big["full"]
    res = team4.commit(big["coeffs"], BIG)
    assert sp.transcript_of(res) == sp.transcript_want(full)
    msg = sp.stored_proof_mismatch(team4, full, BIG)
    assert msg is None, "team of 4: " + msg


# ---- 3. the gather kernels, swept --------------------------------------------
@pytest.mark.parametrize("log_n,d", [(11, 256), (5, 32)])
def test_gathers_exhaustive(ctx, corc, oracle, log_n, d):
    """fri_decommit_query at every index of [0, n), every layer (a one-element
    layer has empty paths), and fri_auth_path at every leaf of layers 0, 1 and
    the last."""
    n = 1 << log_n
    coeffs = oracle.splitmix64_np(300 + log_n, d).astype(np.uint32)
    full = sp.oracle_commit_full(corc, oracle, coeffs, log_n)
    res = ctx.commit(coeffs, log_n)
    assert sp.transcript_of(res) == sp.transcript_want(full)
    if d == n:
        assert full.values[-1].size == 1
        val, sval, path, spath = ctx.decommit_query(n - 1, full.n_layers, log_n)[-1]
        assert (path, spath) == (b"", b"") and val == sval == int(full.values[-1][0])
    paths = [sp.path_table(full.levels[k], np.arange(n >> k)) for k in range(full.n_layers)]
    for index in range(n):
        _check_query(ctx, full, log_n, index, paths)
    for k in (0, 1, full.n_layers - 1):
        for i in range(n >> k):
            _check_auth_path(ctx, full, log_n, k, i, paths)


def _trace_oracle(corc, oracle, trace, lb):
    """The trace LDE and its tree as test_trace_commit_vs_fast_oracle builds
    them: orc_interpolate_coset on <w_t>, orc_lde on 5 * <w_n>, orc_merkle_build."""
    nt = len(trace)
    log_t = nt.bit_length() - 1
    ys = np.ascontiguousarray(np.asarray(trace, dtype=np.uint64))
    oc = np.zeros(nt, dtype=np.uint64)
    ln = corc.orc_interpolate_coset(ys.ctypes.data_as(sp.P64), log_t, 1, 5, oracle.P, oc.ctypes.data_as(sp.P64))
    ol = np.zeros(nt << lb, dtype=np.uint64)
    c64 = np.ascontiguousarray(oc[:max(ln, 1)])
    assert corc.orc_lde(c64.ctypes.data_as(sp.P64), ln, log_t + lb, 5, 5, oracle.P, ol.ctypes.data_as(sp.P64)) == 0
    return ol.astype(np.uint32), sp.oracle_tree(corc, ol)


def _check_trace_calls(ctx, lde, levels, L, calls):
    """fri_trace_decommit for every (index, stride) of `calls`, count 8: each
    value and path against leaf (index + j * stride) mod n of the oracle's tree."""
    n = 1 << L
    for index, stride in calls:
        leaves = [(index + j * stride) % n for j in range(8)]
        want = sp.path_table(levels, leaves)
        for j, (val, path) in enumerate(ctx.trace_decommit(index, stride, 8, L)):
            leaf = leaves[j]
            where = f"trace_decommit({index}, stride {stride}) j = {j}: leaf {leaf}"
            assert val == int(lde[leaf]), where
            if path != want[j].tobytes():
                got = np.frombuffer(path, dtype=np.uint8).reshape(L, 32)
                lvl = sp.first_mismatch(got, want[j])
                raise AssertionError(f"{where}: path differs at level {lvl} (node {(leaf >> lvl) ^ 1}; leaf-kernel "
                                     f"workgroup {sp.leaf_workgroup(L, lvl, (leaf >> lvl) ^ 1)}): "
                                     f"got {got[lvl].tobytes().hex()} want {want[j][lvl].tobytes().hex()}")


@pytest.mark.parametrize("log_t,lb", [(6, 3), (8, 3), (16, 3)])
def test_trace_tree_gather(ctx, corc, oracle, log_t, lb):
    """The trace tree (launch_layer without the commit: the COMMIT=false
    kernels), whose only reader is fri_trace_decommit.

    Coverage, a condition of this test rather than a sample size:
      2^9 (k_tree_top from the leaves) and 2^11 (wide leaf, top): every
            leaf, n / 8 calls of 8 at stride 1, so every node below the root
            of every level appears as some leaf's sibling;
      2^19: every node of the levels >= 6 (2^13 leaves at stride 64: 1024
            calls of 8; the level-l sibling of leaf 64 i is node (i >> (l - 6)) ^ 1,
            and i runs over all 2^13), and every leaf, hence every node of the
            levels 0..10, under the first, a middle and the last 2048-leaf
            workgroup of the quad leaf kernel (3 x 256 calls of 8 at stride 1).
    The root itself is the value fri_trace_commit returns.  A call whose
    index + j * stride passes n wraps modulo n, as include/fri_amd.h states."""
    L = log_t + lb
    n = 1 << L
    trace = oracle.splitmix64_np(800 + log_t, 1 << log_t)
    root, _, lde = ctx.trace_commit(trace.astype(np.uint32), lb)
    want_lde, levels = _trace_oracle(corc, oracle, trace, lb)
    msg = sp.value_report(0, L, lde, want_lde, what="trace LDE")
    assert msg is None, msg
    assert root == levels[-1][0].tobytes()
    if L <= 11:
        calls = [(i, 1) for i in range(0, n, 8)]
    else:
        assert L == 19
        calls = [(i, 64) for i in range(0, n, 512)]
        for wg in (0, (n // 2048) // 2, n // 2048 - 1):
            calls += [(2048 * wg + i, 1) for i in range(0, 2048, 8)]
        assert len(calls) == 1024 + 768
    _check_trace_calls(ctx, lde, levels, L, calls)
    # past the end: leaves n-3, n-2, n-1, 0, 1, ..., and a stride that wraps on every step
    _check_trace_calls(ctx, lde, levels, L, [(n - 3, 1), (n - 1, n - 1), (5, n // 2 + 1)])
