"""Test helper: everything a commit leaves behind, from the C oracle.

orc_fri_commit_fast (oracle/fri_oracle.c, fri_commit.rs:72-122) writes every
layer's values and every level of every layer's Merkle tree (orc_merkle_build
layout: leaves first, root last) into two flat arrays.  oracle_commit_full
slices them into per-layer, per-level numpy views, so a test can compare what
the library keeps in HBM (fri_layer_copy, fri_tree_level_copy, fri_auth_path,
fri_decommit_query, fri_trace_decommit) node for node, and name the first node
that differs.  Pure numpy + ctypes: nothing here needs a GPU."""
import ctypes
from types import SimpleNamespace

import numpy as np

P64 = ctypes.POINTER(ctypes.c_uint64)


def _state_hex(state):
    """A channel state as the oracle keeps it (64 hex characters) from hex or 32 raw bytes; "" = fresh."""
    if not state:
        return ""
    if isinstance(state, (bytes, bytearray)) and len(state) == 32:
        return bytes(state).hex()
    s = state.decode() if isinstance(state, (bytes, bytearray)) else state
    assert len(s) == 64
    return s


def split_levels(nodes, m):
    """orc_merkle_build's node array (u8, shape (count, 32)) of an m-leaf
    tree, m a power of two -> [level 0 (m leaves), ..., level log2(m) (root)]."""
    out, off = [], 0
    while True:
        out.append(nodes[off:off + m])
        off += m
        if m == 1:
            assert off == nodes.shape[0]
            return out
        m >>= 1


def oracle_commit_full(corc, oracle, coeffs, log_n, offset=5, state=None, forced_betas=None):
    """The C oracle's commit of `coeffs` on offset * <w_{2^log_n}> (with
    `forced_betas` in place of the channel's, if given), with all it stores:
    .res (OrcFriResult), .n_layers, .roots (bytes), .betas, .final_value, .final_degree, .state (hex), and per layer k
    .values[k] (uint32, n >> k) and .levels[k][l] (uint8, (n >> k >> l, 32))."""
    n = 1 << log_n
    c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.uint64))
    counts = [corc.orc_merkle_nodes_count(n >> k) for k in range(log_n + 1)]
    layers_out = np.zeros(2 * n, dtype=np.uint64)
    trees_out = np.zeros((sum(counts), 32), dtype=np.uint8)
    och = oracle.OrcChannel()
    corc.orc_channel_init(ctypes.byref(och))
    st = _state_hex(state)
    if st:
        och.state = st.encode()
        och.state_len = 64
    res = oracle.OrcFriResult()
    fb = None if forced_betas is None else np.ascontiguousarray(np.asarray(forced_betas, dtype=np.uint64))
    rc = corc.orc_fri_commit_fast(c.ctypes.data_as(P64), c.size, log_n, offset, oracle.GEN, oracle.P,
                                  ctypes.byref(och), None if fb is None else fb.ctypes.data_as(P64),
                                  ctypes.byref(res), layers_out.ctypes.data_as(P64),
                                  trees_out.ctypes.data_as(ctypes.c_char_p))
    assert rc == 0
    values, levels, lo, to = [], [], 0, 0
    for k in range(res.n_layers):
        m = n >> k
        v = layers_out[lo:lo + m]
        assert m == 0 or int(v.max()) < oracle.P
        values.append(v.astype(np.uint32))
        levels.append(split_levels(trees_out[to:to + counts[k]], m))
        lo += m
        to += counts[k]
    return SimpleNamespace(res=res, n_layers=int(res.n_layers), values=values, levels=levels,
                           roots=[bytes(res.roots[k]) for k in range(res.n_layers)],
                           betas=[int(res.betas[r]) for r in range(res.n_rounds)],
                           final_value=int(res.final_value), final_degree=int(res.final_degree),
                           state=och.state.decode())


def oracle_tree(corc, values):
    """orc_merkle_build over `values` (a power-of-two count) as levels, leaves first."""
    v = np.ascontiguousarray(np.asarray(values, dtype=np.uint64))
    nodes = np.zeros((corc.orc_merkle_nodes_count(v.size), 32), dtype=np.uint8)
    assert corc.orc_merkle_build(v.ctypes.data_as(P64), v.size, nodes.ctypes.data_as(ctypes.c_char_p)) == nodes.shape[0]
    return split_levels(nodes, v.size)


def expected_path(levels_k, idx):
    """Authentication path of leaf idx: the sibling digests leaf -> root,
    levels_k[l][(idx >> l) ^ 1] for every level below the root, as bytes."""
    return b"".join(levels_k[l][(idx >> l) ^ 1].tobytes() for l in range(len(levels_k) - 1))


def path_table(levels_k, idx):
    """expected_path for an array of leaf indices at once: uint8 (len(idx), L, 32)."""
    idx = np.asarray(idx, dtype=np.int64)
    L = len(levels_k) - 1
    out = np.empty((idx.size, L, 32), dtype=np.uint8)
    for l in range(L):
        out[:, l] = levels_k[l][(idx >> l) ^ 1]
    return out


def transcript_of(res):
    """(roots, betas, final value, final degree, state hex) of a library CommitResult."""
    return ([bytes(res.roots[k]) for k in range(res.n_layers)], [int(res.betas[r]) for r in range(res.n_rounds)],
            int(res.final_value), int(res.final_degree), bytes(res.channel_out.digest).hex())


def transcript_want(full):
    return (full.roots, full.betas, full.final_value, full.final_degree, full.state)


def read_level(ctx, k, level, log_n):
    """Level `level` of layer k's stored tree through fri_tree_level_copy,
    straight into a numpy buffer: uint8 (2^(log_n - k - level), 32)."""
    cnt = 1 << (log_n - k - level)
    out = np.empty((cnt, 32), dtype=np.uint8)
    ctx._check(ctx.lib.fri_tree_level_copy(ctx.h, k, level, out.ctypes.data_as(ctypes.c_char_p), out.nbytes))
    return out


def leaf_workgroup(L, level, node):
    """The leaf-kernel workgroup whose leaves node `node` of level `level`
    covers (its first, for a node wider than one workgroup): 2048 leaves per
    workgroup for a layer of 2^L >= 2^19 values, 256 below."""
    return (node << level) // (2048 if L >= 19 else 256)


def first_mismatch(got, want):
    """Row index of the first difference between two equal-shape arrays, or None."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if np.array_equal(got, want):
        return None
    ne = got != want
    if ne.ndim > 1:
        ne = ne.reshape(ne.shape[0], -1).any(axis=1)
    return int(np.argmax(ne))


def node_report(k, log_n, level, got, want, what="tree"):
    """None if level `level` of layer k's tree equals the oracle's, else a
    message naming the first differing node and the count of them."""
    i = first_mismatch(got, want)
    if i is None:
        return None
    L = log_n - k
    bad = int((got != want).reshape(got.shape[0], -1).any(axis=1).sum())
    return (f"{what}: layer {k} (2^{L} values) level {level} node {i} differs (first of {bad} of {got.shape[0]}); "
            f"leaf-kernel workgroup {leaf_workgroup(L, level, i)}, leaves {i << level}..{((i + 1) << level) - 1}; "
            f"got {got[i].tobytes().hex()} want {want[i].tobytes().hex()}")


def value_report(k, log_n, got, want, what="layer"):
    """None if layer k's stored values equal the oracle's, else the first differing index."""
    i = first_mismatch(got, want)
    if i is None:
        return None
    L = log_n - k
    return (f"{what}: layer {k} (2^{L} values) value {i} differs (first of {int((got != want).sum())}); "
            f"leaf-kernel workgroup {leaf_workgroup(L, 0, i)}; got {int(got[i])} want {int(want[i])}")


def stored_proof_mismatch(ctx, full, log_n, n_layers=None):
    """First difference between the commit resident on `ctx` and the oracle's
    `full`: every committed layer's values and every level of its tree.
    Returns None when all are equal."""
    for k in range(full.n_layers if n_layers is None else n_layers):
        msg = value_report(k, log_n, ctx.layer(k, log_n), full.values[k])
        if msg:
            return msg
        for level in range(log_n - k + 1):
            msg = node_report(k, log_n, level, read_level(ctx, k, level, log_n), full.levels[k][level])
            if msg:
                return msg
    return None
