"""GPU: the Python mirror's calls that name no context, on a default team.

Every reference-shaped function of fri_amd (MerkleTree, prove_fibsq, poly_mul,
poly_div_rem, gen_polynomial_from_roots, fri_commit, fri_commit_pipelined,
fri_commit_batch) opens fri_ctx_create_default behind a call without ``ctx``:
on a node with several GPUs, or with FRI_DEVICES naming several ranks, that is
a team.  Here FRI_DEVICES=0,0 makes it a two-rank team on GPU 0, and every call
runs at the first size a shard-sized rank 0 would refuse (2^20), or on the
paths a team routes elsewhere (pipelined and batched commits run on one-device
contexts beside it).  The module fixture swaps the mirror's context caches for
empty ones, so the contexts other modules cached are neither used nor closed.

Every expected value is the oracle's (orc_merkle_build, orc_fibsq_prove_commit,
orc_poly_evaluate, orc_poly_div_rem's identity, orc_fri_commit_fast with the
Python twin's decommitment), never another GPU context's."""
import hashlib

import numpy as np
import pytest

import oracle_flat
from test_gpu_poly_arith import c_eval, check_div_rem, rnd
from test_gpu_tier_sweep import P, c_merkle_nodes, merkle_values, seeded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mirror():
    """fri_amd with FRI_DEVICES=0,0 and empty context caches; the contexts the
    module's calls create are closed and the caches put back afterwards."""
    import fri_amd
    mp = pytest.MonkeyPatch()
    mp.setenv("FRI_DEVICES", "0,0")
    fresh = {name: {} for name in ("_CTX_CACHE", "_BATCH_CTX", "_PIPE_CTX")}
    for name, cache in fresh.items():
        mp.setattr(fri_amd, name, cache)
    try:
        yield fri_amd
    finally:
        for cache in fresh.values():
            for c in cache.values():
                c.close()
        mp.undo()


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).astype(np.uint32))


def _state(i):
    """Channel i's starting state: fresh for i = 0, else 64 hex characters of its own."""
    return "" if i == 0 else hashlib.sha256(b"default team %d" % i).hexdigest()


def test_fri_commit_opens_a_team(mirror, corc, oracle):
    """fri_commit at 2^20 and decommit_fri: the default context really is the
    two-rank team, the commit runs sharded, the whole transcript is the oracle's."""
    L = 20
    coeffs = oracle.splitmix64_np(61, (1 << L) >> 3)
    ch = mirror.Channel()
    proof = mirror.fri_commit(_u32(coeffs), L, ch)
    assert proof.ctx.n_ranks == 2 and proof.ctx.dist_info() == (0, 2, "peer")
    assert proof.ctx.team_rank(1).transport_log(), "the commit did not run sharded"
    mirror.decommit_fri(2, (1 << L) - 1, proof, ch)
    msgs, state = oracle_flat.transcript(corc, coeffs, L, 2)
    assert ch.proof == msgs and ch.state == state
    assert mirror.verify_fri(ch.proof, L, proof.n_layers, 2, (1 << L) - 1)


@pytest.mark.parametrize("n", [1 << 20, (1 << 19) + 1])
def test_merkle_tree(mirror, corc, n):
    v = merkle_values(41000 + n % 1000, n)
    assert mirror.MerkleTree(_u32(v)).root() == c_merkle_nodes(corc, v)[-32:].tobytes().hex()


def test_prove_fibsq(mirror, corc, oracle):
    from prover_check import check_proof_matches_c_oracle
    a1, log_t, lb, queries = 3141592, 17, 3, 2
    ch = mirror.Channel()
    pr = mirror.prove_fibsq(a1, log_t, lb, queries, ch)
    assert pr.fri.ctx.n_ranks == 2
    check_proof_matches_c_oracle(mirror, corc, oracle, pr, ch, a1, log_t, lb, queries)


def test_poly_mul(mirror, corc):
    """la = lb = 2^18 + 1: the product has 2^19 + 1 coefficients and needs a 2^20 transform."""
    la = (1 << 18) + 1
    a, b = rnd(42001, la), rnd(42002, la)
    got = mirror.poly_mul(_u32(a), _u32(b))
    assert got.dtype == np.uint32 and got.size == 2 * la - 1
    assert int(got[0]) == int(a[0]) * int(b[0]) % P and int(got[-1]) == int(a[-1]) * int(b[-1]) % P
    for x in seeded(42003, 8):
        assert c_eval(corc, got, x) == c_eval(corc, a, x) * c_eval(corc, b, x) % P, int(x)


def test_gen_polynomial_from_roots(mirror, corc):
    n = (1 << 19) + 1
    roots = seeded(43001, n)
    z = mirror.gen_polynomial_from_roots(_u32(roots))
    assert z.dtype == np.uint32 and z.size == n + 1 and z[-1] == 1
    for i in seeded(43002, 8):
        r = int(roots[int(i) % n])
        assert c_eval(corc, z, r) == 0, r
    rs = [int(r) for r in roots]
    for x in (int(v) for v in seeded(43003, 4)):
        want = 1
        for r in rs:
            want = want * (x - r) % P
        assert c_eval(corc, z, x) == want, x


def test_poly_div_rem_on_its_margin(mirror, corc):
    """la = 2^18 asks for a 2^20 context (the documented + 2), lb = 5."""
    points = [0, 1, P - 1] + [int(v) for v in seeded(44003, 13)]
    check_div_rem(_NoCtx(mirror), corc, points, rnd(44001, 1 << 18), rnd(44002, 5))


class _NoCtx:
    """The mirror's module-level poly_div_rem behind the method check_div_rem calls."""

    def __init__(self, mirror):
        self.mirror = mirror

    def poly_div_rem(self, a, b):
        return self.mirror.poly_div_rem(_u32(a), _u32(b))


def test_fri_commit_pipelined(mirror, corc, oracle):
    """5 polynomials at 2^12, each channel with a state of its own: the team
    takes no pipelined commits, so they run on a one-device context beside it."""
    L, n = 12, 1 << 12
    polys = [oracle.splitmix64_np(45000 + i, n >> 3) for i in range(5)]
    chans = [mirror.Channel(state=_state(i)) for i in range(5)]
    proofs = mirror.fri_commit_pipelined([_u32(c) for c in polys], L, chans)
    assert mirror._CTX_CACHE and all(c.n_ranks == 2 for c in mirror._CTX_CACHE.values())
    assert len(proofs) == 5 and all(p.ctx.n_ranks == 1 for p in proofs)
    for i, (c, ch) in enumerate(zip(polys, chans)):
        msgs, state = oracle_flat.transcript(corc, c, L, 0, state=_state(i))
        assert ch.proof == msgs and ch.state == state, i
    mirror.decommit_fri(2, n - 1, proofs[-1], chans[-1])
    msgs, state = oracle_flat.transcript(corc, polys[-1], L, 2, state=_state(4))
    assert chans[-1].proof == msgs and chans[-1].state == state
    assert mirror.verify_fri(chans[-1].proof, L, proofs[-1].n_layers, 2, n - 1, channel_state=_state(4))


def test_fri_commit_batch_beside_the_team(mirror, corc, oracle, oracle_commit):
    """16 members at 2^10 run on the batch's own one-device context; the team
    behind the other calls is untouched: a later fri_commit at 2^20 is right."""
    L, n = 10, 1 << 10
    polys = [oracle.splitmix64_np(46000 + i, n >> 3) for i in range(16)]
    chans = [mirror.Channel(state=_state(i)) for i in range(16)]
    proofs = mirror.fri_commit_batch([_u32(c) for c in polys], L, chans)
    assert mirror._BATCH_CTX and all(c.n_ranks == 1 for c in mirror._BATCH_CTX.values())
    assert len(proofs) == 16
    for i, (c, ch) in enumerate(zip(polys, chans)):
        msgs, state = oracle_flat.transcript(corc, c, L, 0, state=_state(i))
        assert ch.proof == msgs and ch.state == state, i
    m = 11
    mirror.decommit_fri(2, n - 1, proofs[m], chans[m])
    msgs, state = oracle_flat.transcript(corc, polys[m], L, 2, state=_state(m))
    assert chans[m].proof == msgs and chans[m].state == state
    assert mirror.verify_fri(chans[m].proof, L, proofs[m].n_layers, 2, n - 1, channel_state=_state(m))
    ch = mirror.Channel()
    big = mirror.fri_commit(_u32(oracle.splitmix64_np(47, (1 << 20) >> 3)), 20, ch)
    want = oracle_commit(20, 47)
    assert big.ctx.n_ranks == 2
    assert [r.hex() for r in big.roots] == want["roots"] and big.betas == want["betas"]
    assert (big.final_value, big.final_degree, ch.state) == (want["final_value"], want["final_degree"], want["state"])
