"""GPU: the prover slice (BASELINE configs[3]) — fri_trace_commit +
fri_fibsq_composition_commit + fri_trace_decommit + fri_decommit_query,
driven by fri_amd.prove_fibsq — against the oracle bit for bit: the golden
transcripts (faithful restatement, small T), and at T = 2^10 and 2^16 the C
oracle's commit phase (orc_fibsq_prove_commit: NTT, batch inverse, fast FRI)
plus the Python twin's decommitment over the oracle's own layers and trees.
The composition polynomial itself is parity-unpinned against the reference
(its src/prover is empty); see tests/test_prover_oracle.py."""
import ctypes
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 3221225473


def _proof_sha(msgs):
    return hashlib.sha256(b"".join(len(m).to_bytes(4, "little") + m for m in msgs)).hexdigest()


def test_prove_matches_golden_transcripts(ctx, golden):
    import fri_amd
    for c in golden["fibsq"]:
        ch = fri_amd.Channel(state=c["channel_in"])
        pr = fri_amd.prove_fibsq(c["a1"], c["log_t"], c["log_blowup"], c["queries"], ch, ctx=ctx)
        assert pr.trace_root.hex() == c["trace_root"], c["name"]
        assert pr.alphas == c["alphas"] and pr.fri.betas == c["betas"], c["name"]
        assert [r.hex() for r in pr.fri.roots] == c["roots"], c["name"]
        assert pr.fri.final_value == c["final_value"] and pr.queries == c["query_indices"], c["name"]
        assert ch.state == c["channel_out"], c["name"]
        assert len(ch.proof) == c["messages"] and _proof_sha(ch.proof) == c["proof_sha256"], c["name"]


@pytest.mark.parametrize("log_t,lb,queries", [(10, 3, 4), (16, 3, 3), (12, 1, 2), (9, 4, 2), (2, 1, 2), (2, 2, 2)])
def test_prove_matches_c_oracle(ctx, corc, oracle, log_t, lb, queries):
    """The whole transcript at scale (configs[3] is log_t = 16, blowup 8), and
    the smallest cosets the entry point accepts: 8 points (fewer than one
    composition lane's 16) and 16."""
    import fri_amd
    from prover_check import check_proof_matches_c_oracle
    a1 = 3141592
    ch = fri_amd.Channel()
    pr = fri_amd.prove_fibsq(a1, log_t, lb, queries, ch, ctx=ctx)
    check_proof_matches_c_oracle(fri_amd, corc, oracle, pr, ch, a1, log_t, lb, queries)


def test_prove_verify_rejects_tampering(ctx):
    import fri_amd
    log_t, lb, q = 12, 3, 3
    ch = fri_amd.Channel()
    pr = fri_amd.prove_fibsq(5, log_t, lb, q, ch, ctx=ctx)
    a_last = fri_amd.fibsq_trace(5, 1 << log_t)[-1]
    args = (a_last, log_t, lb, q, len(pr.fri.roots))
    assert fri_amd.verify_fibsq(ch.proof, *args)
    first_query = 2 + 3 + 2 * len(pr.fri.roots)            # trace root, 3 alphas, roots/betas/final, index
    for i in (0, 2, first_query, first_query + 1, first_query + 2, len(ch.proof) - 1):
        b = bytearray(ch.proof[i])
        b[-1] ^= 1
        assert not fri_amd.verify_fibsq(ch.proof[:i] + [bytes(b)] + ch.proof[i + 1:], *args), i


def test_composition_detects_constraint_violation(ctx):
    """A wrong claimed output a_{T-1}: CP is no longer a polynomial of degree
    <= T and the library refuses (FRI_EDEGREE) instead of committing it."""
    import fri_amd
    log_t, lb = 10, 3
    trace = fri_amd.fibsq_trace(3141592, 1 << log_t)
    ctx.trace_commit(trace, lb, readback=False)
    with pytest.raises(fri_amd.FriError) as e:
        ctx.fibsq_composition_commit(log_t, lb, (int(trace[-1]) + 1) % P, [1, 2, 3], channel_state=bytes(32))
    assert e.value.code == fri_amd.FRI_EDEGREE
    # the refused commit's layers are not served afterwards
    assert ctx.commit_info()[1:] == (0, 0)
    buf = np.zeros(16, dtype=np.uint32)
    assert ctx.lib.fri_layer_copy(ctx.h, 0, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                  buf.size) == fri_amd.FRI_ESTATE
    res = ctx.fibsq_composition_commit(log_t, lb, int(trace[-1]), [1, 2, 3], channel_state=bytes(32))
    assert res.n_rounds == log_t + 1


def test_composition_commit_refuses_bad_shapes(ctx, golden):
    """fri_fibsq_composition_commit's shape refusals, each behind a resident
    trace commit of that very shape (so it is the shape check that refuses),
    then a golden proof on the same context."""
    import fri_amd

    def refused(log_t, lb, offset=fri_amd.GENERATOR, a_last=None, alphas=(1, 2, 3), flags=0):
        trace = fri_amd.fibsq_trace(7, 1 << log_t)
        ctx.trace_commit(trace, lb, offset=offset, readback=False)
        al = np.array(alphas, dtype=np.uint32)
        ch, res = fri_amd.ChannelState(), fri_amd.CommitResult()
        a_last = int(trace[-1]) if a_last is None else a_last
        return ctx.lib.fri_fibsq_composition_commit(ctx.h, log_t, lb, offset, a_last, fri_amd._ptr(al), ctypes.byref(ch),
                                                    flags, ctypes.byref(res))

    E = fri_amd.FRI_EINVAL
    assert refused(4, 0) == E                              # log_blowup below 1
    assert refused(4, 5) == E                              # ... above 4
    assert refused(1, 1) == E                              # fewer than 4 rows
    assert refused(4, 3, offset=1) == E                    # 1^T lies in <w_B>
    for j in range(3):
        assert refused(4, 3, alphas=[P if i == j else i + 1 for i in range(3)]) == E
    assert refused(4, 3, a_last=P) == E
    assert refused(4, 3, flags=fri_amd.FLAG_FORCE_BETAS) == E
    assert refused(4, 3) == fri_amd.FRI_OK                 # the helper's call is a good one otherwise
    c = golden["fibsq"][2]
    ch = fri_amd.Channel(state=c["channel_in"])
    pr = fri_amd.prove_fibsq(c["a1"], c["log_t"], c["log_blowup"], c["queries"], ch, ctx=ctx)
    assert pr.trace_root.hex() == c["trace_root"] and [r.hex() for r in pr.fri.roots] == c["roots"]
    assert ch.state == c["channel_out"]
    assert len(ch.proof) == c["messages"] and _proof_sha(ch.proof) == c["proof_sha256"]


def test_prover_entry_errors(ctx):
    import fri_amd
    trace = fri_amd.fibsq_trace(7, 1 << 8)
    ctx.trace_commit(trace, 3, readback=False)
    with pytest.raises(fri_amd.FriError) as e:          # other (log_t, blowup) than the resident trace
        ctx.fibsq_composition_commit(9, 3, int(trace[-1]), [1, 2, 3])
    assert e.value.code == fri_amd.FRI_ESTATE
    with pytest.raises(fri_amd.FriError) as e:
        ctx.trace_decommit(1 << 11, 8, 3, 11)             # index beyond the LDE
    assert e.value.code == fri_amd.FRI_EINVAL
    with pytest.raises(fri_amd.FriError) as e:
        ctx.trace_decommit(0, 8, 9, 11)                   # count > 8
    assert e.value.code == fri_amd.FRI_EINVAL
    vals = ctx.trace_decommit(5, 8, 3, 11)
    _, _, lde = ctx.trace_commit(trace, 3)
    assert [v for v, _ in vals] == [int(lde[5]), int(lde[13]), int(lde[21])]
