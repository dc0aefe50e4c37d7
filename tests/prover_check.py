"""Test helper: a prove_fibsq transcript against the oracle, shared by
tests/test_gpu_prover.py (an explicit one-device context) and
tests/test_gpu_default_team.py (no context, default team).

The commit phase is the C oracle's (orc_fibsq_prove_commit: NTT, batch inverse,
fast FRI), which keeps the trace LDE, the trace tree and every FRI layer and
tree; the decommitment is the Python twin's (fri_oracle.decommit_fri_layers,
fri_commit.rs:137-163) over thin index views of those flat arrays
(tests/oracle_flat.py), continued from the oracle's channel state.  Nothing
here needs a GPU."""
import ctypes

import numpy as np

from oracle_flat import _Level, _Values

P = 3221225473


def oracle_fibsq_commit(corc, oracle, a1, log_t, lb):
    """orc_fibsq_prove_commit with everything it stores: (och, trace root
    bytes, alphas, res, fe, ftree, lay, trees); fe the trace LDE (uint64, n),
    ftree its tree (orc_merkle_build layout), lay / trees the FRI layers'
    values and trees, layer after layer."""
    L = log_t + lb
    n = 1 << L
    och = oracle.OrcChannel()
    corc.orc_channel_init(ctypes.byref(och))
    root = ctypes.create_string_buffer(32)
    al = (ctypes.c_uint64 * 3)()
    res = oracle.OrcFriResult()
    fe = np.zeros(n, dtype=np.uint64)
    ftree = ctypes.create_string_buffer(32 * (2 * n - 1))
    lay = np.zeros(2 * n, dtype=np.uint64)
    tsz = sum(2 * (n >> k) - 1 for k in range(L + 1))
    trees = ctypes.create_string_buffer(32 * tsz)
    pu = ctypes.POINTER(ctypes.c_uint64)
    assert corc.orc_fibsq_prove_commit(a1, log_t, lb, 5, 5, P, ctypes.byref(och), root, al, ctypes.byref(res),
                                       fe.ctypes.data_as(pu), ftree, lay.ctypes.data_as(pu), trees) == 0
    return och, root.raw, list(al), res, fe, ftree, lay, trees


def _levels(buf, off, m):
    """orc_merkle_build layout (leaves first, power-of-two m) at node `off` -> list of levels."""
    raw = memoryview(buf).cast("B")
    out = []
    while True:
        out.append(_Level(raw, off, m))
        off += m
        if m == 1:
            return out
        m //= 2


def oracle_fibsq_proof(corc, oracle, a1, log_t, lb, queries):
    """The oracle's whole proof: (res, trace root, alphas, ref, msgs, state).
    res: the commit phase's OrcFriResult; ref: the Python twin's channel
    continued from the oracle's state, holding the decommitment messages of
    `queries` queries; msgs: every message of the transcript (trace root,
    alphas, FRI roots / betas / final value, then ref's); state: the final
    channel state."""
    L = log_t + lb
    n, B = 1 << L, 1 << lb
    # oracle: commit phase in C, keeping trace LDE / trace tree / FRI layers / trees
    och, root, al, res, fe, ftree, lay, trees = oracle_fibsq_commit(corc, oracle, a1, log_t, lb)
    # decommitment over the oracle's data, channel continued from the oracle state
    flev = _levels(ftree, 0, n)
    layers, tlev, lo, to = [], [], 0, 0
    for k in range(res.n_layers):
        m = n >> k
        layers.append(_Values(lay[lo:lo + m]))
        tlev.append(_levels(trees, to, m))
        lo += m
        to += 2 * m - 1
    ref = oracle.Channel(state=och.state.decode())
    for _ in range(queries):
        idx = ref.receive_random_int(0, n - 2 * B - 1, True)
        for j in range(3):
            ref.send(oracle.fe_to_bytes(int(fe[idx + j * B])))
            ref.send(oracle.merkle_proof(flev, idx + j * B))
        oracle.decommit_fri_layers(idx, layers, tlev, ref)
    msgs = [root.hex().encode()] + [int(a).to_bytes(8, "big") for a in al]
    for k in range(res.n_layers):
        msgs.append(bytes(res.roots[k]).hex().encode())
        if k < res.n_rounds:
            msgs.append(int(res.betas[k]).to_bytes(8, "big"))
    msgs.append(int(res.final_value).to_bytes(8, "big"))
    return res, root, al, ref, msgs + ref.proof, ref.state


def check_proof_matches_c_oracle(fri_amd, corc, oracle, pr, ch, a1, log_t, lb, queries):
    """`pr`, `ch`: what fri_amd.prove_fibsq(a1, log_t, lb, queries, ch) returned
    and left in a fresh channel.  The whole transcript equals the oracle's, and
    verify_fibsq accepts it."""
    res, root, al, ref, msgs, _ = oracle_fibsq_proof(corc, oracle, a1, log_t, lb, queries)
    assert pr.trace_root == root and pr.alphas == al
    assert pr.fri.roots == [bytes(res.roots[k]) for k in range(res.n_layers)]
    assert pr.fri.betas == [int(res.betas[k]) for k in range(res.n_rounds)]
    assert pr.fri.final_value == res.final_value and pr.fri.final_degree == res.final_degree
    # deg CP = T: the folds end at a constant after log_t + 1 rounds.  T = 4 is
    # the exception: g^2 = -1 there, so the leading terms of f(g x)^2 and f(x)^2
    # cancel (1 + g^(2(T-1)) = 0), deg CP = 3 and two rounds reach the constant
    assert res.n_rounds == (log_t + 1 if log_t > 2 else 2)
    assert ch.state == ref.state
    assert ch.proof[-len(ref.proof):] == ref.proof
    assert ch.proof == msgs
    assert fri_amd.verify_fibsq(ch.proof, fri_amd.fibsq_trace(a1, 1 << log_t)[-1], log_t, lb, queries,
                                len(pr.fri.roots))
