"""CPU tests of tests/stored_proof.py, the helper the stored-proof GPU tests
(tests/test_gpu_stored_proof.py) stand on: the C oracle's flat layer and tree
outputs, sliced per layer and level, equal the Python twin's own layers,
merkle_levels and merkle_proof; the slicing offsets reproduce every root; the
readback goes through fri_tree_level_copy's signature; and the mismatch
reporter names the layer, level, node and leaf-kernel workgroup."""
import ctypes

import numpy as np
import pytest

import stored_proof as sp

# (log_n, d, offset, channel state): n = 1, 2, 8, 2^10, and blowup 1 (d = n: the last layer has one element)
CASES = [(0, 1, 5, ""), (1, 1, 5, ""), (3, 1, 5, ""), (3, 8, 5, ""), (10, 128, 5, ""), (6, 64, 5, ""),
         (7, 16, 7, "5a" * 32)]


@pytest.mark.parametrize("log_n,d,offset,state", CASES)
def test_full_commit_equals_python_twin(corc, oracle, log_n, d, offset, state):
    coeffs = oracle.splitmix64_field(1000 + 10 * log_n + d, d)
    full = sp.oracle_commit_full(corc, oracle, coeffs, log_n, offset=offset, state=state)
    ch = oracle.Channel(state=state)
    twin = oracle.fri_commit(coeffs, log_n, ch, offset=offset)
    assert full.n_layers == len(twin.layers) == len(full.values) == len(full.levels)
    assert full.roots == twin.roots and full.betas == twin.betas
    assert full.final_value == twin.final_value and full.state == ch.state
    for k in range(full.n_layers):
        m = (1 << log_n) >> k
        assert full.values[k].dtype == np.uint32 and full.values[k].tolist() == twin.layers[k]
        want = oracle.merkle_levels(twin.layers[k])
        assert len(full.levels[k]) == len(want) == log_n - k + 1
        for l, lvl in enumerate(full.levels[k]):
            assert lvl.shape == (m >> l, 32) and lvl.dtype == np.uint8
            assert [row.tobytes() for row in lvl] == want[l], (k, l)
        # the slicing offsets: each layer's last node is the root the transcript carries
        assert full.levels[k][-1][0].tobytes() == bytes(full.res.roots[k]) == twin.roots[k]
        idxs = range(m) if m <= 64 else [0, 1, 2, m // 2 - 1, m // 2, m - 2, m - 1, 345 % m]
        for idx in idxs:
            assert sp.expected_path(full.levels[k], idx) == oracle.merkle_proof(want, idx), (k, idx)
        tab = sp.path_table(full.levels[k], list(idxs))
        assert tab.shape == (len(idxs), log_n - k, 32)
        assert [tab[i].tobytes() for i in range(len(idxs))] == [sp.expected_path(full.levels[k], j) for j in idxs]
    if d == 1 << log_n:
        assert full.values[-1].size == 1 and sp.expected_path(full.levels[-1], 0) == b""


def test_state_forms_agree(corc, oracle):
    """A pre-filled channel state as 32 raw bytes (what Context.commit takes) or as hex."""
    coeffs = oracle.splitmix64_field(9, 8)
    a = sp.oracle_commit_full(corc, oracle, coeffs, 6, state=bytes(range(32)))
    b = sp.oracle_commit_full(corc, oracle, coeffs, 6, state=bytes(range(32)).hex())
    c = sp.oracle_commit_full(corc, oracle, coeffs, 6)
    assert sp.transcript_want(a) == sp.transcript_want(b) != sp.transcript_want(c)
    assert a.roots[0] == c.roots[0] and a.betas != c.betas


def test_root_offsets_in_the_flat_buffer(corc, oracle):
    """Layer 0's root sits at node 2n - 2 of trees_out, layer 1's at
    (2n - 1) + 2 (n / 2) - 2: checked against a run that passes the raw buffer."""
    log_n, n = 8, 256
    c = np.ascontiguousarray(oracle.splitmix64_np(4, 32))
    cnt = sum(corc.orc_merkle_nodes_count(n >> k) for k in range(log_n + 1))
    trees = np.zeros((cnt, 32), dtype=np.uint8)
    lay = np.zeros(2 * n, dtype=np.uint64)
    och, res = oracle.OrcChannel(), oracle.OrcFriResult()
    corc.orc_channel_init(ctypes.byref(och))
    assert corc.orc_fri_commit_fast(c.ctypes.data_as(sp.P64), c.size, log_n, 5, 5, oracle.P, ctypes.byref(och), None,
                                    ctypes.byref(res), lay.ctypes.data_as(sp.P64),
                                    trees.ctypes.data_as(ctypes.c_char_p)) == 0
    assert trees[2 * n - 2].tobytes() == bytes(res.roots[0])
    assert trees[(2 * n - 1) + 2 * (n // 2) - 2].tobytes() == bytes(res.roots[1])
    full = sp.oracle_commit_full(corc, oracle, c, log_n)
    assert full.roots == [bytes(res.roots[k]) for k in range(res.n_layers)]
    assert np.array_equal(np.concatenate(full.levels[0] + full.levels[1]), trees[:(2 * n - 1) + (n - 1)])


def test_oracle_tree_equals_twin(corc, oracle):
    for n in (1, 2, 16, 512):
        vals = oracle.splitmix64_field(n, n)
        lv = sp.oracle_tree(corc, vals)
        assert [[r.tobytes() for r in l] for l in lv] == oracle.merkle_levels(vals)


class _FakeLib:
    """fri_tree_level_copy's signature over a dict of levels: writes through the raw pointer."""

    def __init__(self, levels):
        self.levels = levels
        self.calls = []

    def fri_tree_level_copy(self, h, k, level, out, cap):
        src = np.ascontiguousarray(self.levels[k][level])
        self.calls.append((k, level, cap))
        if cap < src.nbytes:
            return 1
        ctypes.memmove(out, src.ctypes.data, src.nbytes)
        return 0


class _FakeCtx:
    def __init__(self, values, levels):
        self.h = None
        self.values = values
        self.lib = _FakeLib(levels)

    def _check(self, rc):
        assert rc == 0

    def layer(self, k, log_n):
        return self.values[k]


def test_read_level_and_whole_comparison(corc, oracle):
    log_n = 9
    full = sp.oracle_commit_full(corc, oracle, oracle.splitmix64_field(2, 64), log_n)
    fake = _FakeCtx([v.copy() for v in full.values], [[l.copy() for l in lv] for lv in full.levels])
    got = sp.read_level(fake, 1, 3, log_n)
    assert got.shape == (32, 32) and np.array_equal(got, full.levels[1][3])
    assert fake.lib.calls == [(1, 3, 32 * 32)]
    assert sp.stored_proof_mismatch(fake, full, log_n) is None
    # every (layer, level) was read: sum_k (log_n - k + 1) calls after the first one
    assert len(fake.lib.calls) - 1 == sum(log_n - k + 1 for k in range(full.n_layers))
    # one word of one interior digest stored wrong, the root untouched: found and named
    fake.lib.levels[2][4][5, 8:12] ^= 0xFF
    msg = sp.stored_proof_mismatch(fake, full, log_n)
    assert msg.startswith("tree: layer 2 (2^7 values) level 4 node 5 differs (first of 1 of 8); "
                          "leaf-kernel workgroup 0, leaves 80..95; ")
    fake.lib.levels[2][4][5, 8:12] ^= 0xFF
    fake.values[3][17] ^= 1
    assert sp.stored_proof_mismatch(fake, full, log_n).startswith("layer: layer 3 (2^6 values) value 17 differs")


def test_reporter_names_the_workgroup():
    want = np.zeros((1 << 12, 32), dtype=np.uint8)
    got = want.copy()
    assert sp.node_report(0, 19, 7, got, want) is None
    got[[4095, 33], 31] = 1
    msg = sp.node_report(0, 19, 7, got, want)
    # node 33 of level 7 covers leaves 4224..4351: workgroup 4224 // 2048 of the quad leaf kernel (L >= 19)
    assert "layer 0 (2^19 values) level 7 node 33 differs (first of 2 of 4096)" in msg
    assert "leaf-kernel workgroup 2, leaves 4224..4351" in msg
    # the same node of layer 1 (2^18 values) falls under the wide leaf kernel: 256 leaves per workgroup
    assert "leaf-kernel workgroup 16," in sp.node_report(1, 19, 7, got[:2048], want[:2048])
    assert sp.leaf_workgroup(22, 0, 2047) == 0 and sp.leaf_workgroup(22, 0, 2048) == 1
    assert sp.leaf_workgroup(18, 4, 16) == 1 and sp.leaf_workgroup(19, 19, 0) == 0
    v = np.arange(4096, dtype=np.uint32)
    w = v.copy()
    w[300] = 0
    assert "value 300 differs (first of 1); leaf-kernel workgroup 1;" in sp.value_report(2, 14, w, v)
    assert sp.value_report(2, 14, v, v) is None
