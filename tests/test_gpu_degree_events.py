"""GPU: the commit's degree bookkeeping at every kernel tier.

fri_commit ends when the folded polynomial's degree falls below 1.  On the
device that degree is a max-reduction of three values per fold (m0, m1, m2:
the last non-zero index of the folded coefficients, of the even and of the odd
part) through coef_slice / coef_combine in the leaf-kernel workgroups, the
mx -> mx_out pass of every k_tree_mid / k_tree_mid8 launch, the per-wave
triples of k_tree_top, the LDS copy inside k_tree_tail and, sharded, the rank
records.  A dense polynomial under a channel-drawn beta keeps m0 = m1 = m2 =
nlen - 1 in the last workgroup with work, whatever those stages do with the
other triples.  The inputs of tests/degree_cases.py put the three maxima in
different workgroups, mid groups, waves and ranks, and make the commit end
while most of the planned layers are still enqueued behind the gate.

Every case: roots, betas, final value, final degree and channel state equal
orc_fri_commit_fast's under the same forced betas; fri_commit_degrees equals
degree_schedule (numpy, pinned against both oracles in
tests/test_degree_cases_host.py); n_layers == len(schedule); up to 2^16 every
stored value and tree node too.  Each runs as a graph replay and eagerly, and
a collapse is followed by a dense commit of the same shape on the same
context (stale gate or degree state)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import degree_cases as dc
import stored_proof as sp

pytestmark = pytest.mark.gpu

STORED_MAX_LOG = 16


def _oracle(corc, oracle, coeffs, log_n, betas=None):
    """The C oracle's transcript; with everything it stores up to 2^16."""
    if log_n <= STORED_MAX_LOG:
        return sp.oracle_commit_full(corc, oracle, coeffs, log_n, forced_betas=betas)
    c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.uint64))
    fb = None if betas is None else np.ascontiguousarray(np.asarray(betas, dtype=np.uint64))
    och = oracle.OrcChannel()
    corc.orc_channel_init(ctypes.byref(och))
    res = oracle.OrcFriResult()
    assert corc.orc_fri_commit_fast(c.ctypes.data_as(sp.P64), c.size, log_n, 5, oracle.GEN, oracle.P, ctypes.byref(och),
                                    None if fb is None else fb.ctypes.data_as(sp.P64), ctypes.byref(res), None,
                                    None) == 0
    return SimpleNamespace(n_layers=int(res.n_layers), roots=[bytes(res.roots[k]) for k in range(res.n_layers)],
                           betas=[int(res.betas[r]) for r in range(res.n_rounds)], final_value=int(res.final_value),
                           final_degree=int(res.final_degree), state=och.state.decode())


def _dense_after(cx, oracle, oracle_commit, log_n, d, what):
    """An ordinary dense commit of the same shape on the same context."""
    bl = log_n - (d.bit_length() - 1)
    seed = 7000 + log_n
    res = cx.commit(oracle.splitmix64_np(seed, d).astype(np.uint32), log_n)
    want = oracle_commit(log_n, seed, bl)
    roots, betas, fv, fd, state = sp.transcript_of(res)
    got = {"roots": [r.hex() for r in roots], "betas": betas, "final_value": fv, "final_degree": fd, "state": state}
    assert got == want, f"dense commit after {what}"
    assert cx.commit_degrees() == [(d - 1) >> k for k in range(d.bit_length())], f"dense degrees after {what}"


def _check(cx, res, full, schedule, log_n, what, stored):
    assert sp.transcript_of(res) == sp.transcript_want(full), what
    assert cx.commit_degrees() == schedule, what
    assert res.n_layers == len(schedule) == full.n_layers, what
    assert res.final_degree == schedule[-1], what
    if stored:
        msg = sp.stored_proof_mismatch(cx, full, log_n)
        assert msg is None, f"{what}: {msg}"


def _run_case(ctx, corc, oracle, oracle_commit, case):
    betas = case.betas
    full = _oracle(corc, oracle, case.coeffs, case.log_n, betas)
    # the oracle alone satisfies the event (also checked without a GPU)
    assert full.n_layers == len(case.schedule) and full.final_degree == case.schedule[-1], case.name
    for graph in (True, False):
        what = f"{case.name} ({'graph' if graph else 'eager'})"
        res = ctx.commit(case.coeffs, case.log_n, forced_betas=betas, graph=graph)
        _check(ctx, res, full, case.schedule, case.log_n, what, case.log_n <= STORED_MAX_LOG)
        if case.collapses:
            _dense_after(ctx, oracle, oracle_commit, case.log_n, case.d, what)


@pytest.mark.parametrize("name", list(dc.GPU_SPECS))
def test_degree_events(ctx, corc, oracle, oracle_commit, name):
    """The large shapes, one tier each (see GPU_SPECS for what lies where)."""
    _run_case(ctx, corc, oracle, oracle_commit, dc.gpu_case(name))


@pytest.mark.parametrize("log_n,d", [(9, 64), (5, 4), (3, 1), (5, 32)])
def test_degree_events_one_tail_launch(ctx, corc, oracle, oracle_commit, log_n, d):
    """Every family that fits, where the whole commit is one k_tree_tail
    launch: events at layer 1 (poly_0 read from global memory), layer 2 and
    the last folds (read from LDS); blowup 8, and blowup 1 at 2^5."""
    cases = dc.family_cases(log_n, d)
    assert d <= 2 or {ev[0] for c in cases for ev in c.events.values()} == {"cancel", "beta_zero", "even_zero", "phantom"}
    for case in cases:
        _run_case(ctx, corc, oracle, oracle_commit, case)


@pytest.mark.parametrize("name", ["odd_only", "one_plus_top", "monomial", "half_minus_one"])
@pytest.mark.parametrize("log_n", [16, 22])
def test_natural_degree_events(ctx, corc, oracle, oracle_commit, log_n, name):
    """No hook, the channel's own betas: x Q(x^2) (m1 < 0 at fold 0),
    1 + x^(d-1), x^(d-1) alone (every other workgroup reports -1) and
    x^(d/2) - 1."""
    d = (1 << log_n) >> 3
    coeffs = dc.natural_inputs(d)[name]
    full = _oracle(corc, oracle, coeffs, log_n)
    schedule = dc.degree_schedule(coeffs, full.betas + [0] * dc.N_BETAS)
    assert len(schedule) == full.n_layers and schedule[-1] == full.final_degree
    for graph in (True, False):
        res = ctx.commit(coeffs, log_n, graph=graph)
        _check(ctx, res, full, schedule, log_n, f"{name}@{log_n} graph={graph}", log_n <= STORED_MAX_LOG)


# ---- team: the maxima travel in the rank records -----------------------------
@pytest.fixture(scope="module")
def team4():
    import fri_amd
    c = fri_amd.Context.multi([0, 0, 0, 0], dc.TEAM_LOG_N, transport="peer")
    yield c
    c.close()


@pytest.mark.parametrize("name", list(dc.TEAM_SPECS))
def test_team_degree_events(team4, corc, oracle, oracle_commit, name):
    """4 ranks in one process at 2^22: layers 0-2 are sharded, each rank folds
    its own coefficient chunk (k_coef), its maxima go into its 64-byte record
    (rec_mx), and k_tree_top<SHARD> reduces the gathered records.  Every rank
    takes the same early exit (check_transport_schedule on the four logs)."""
    from test_dist import check_transport_schedule
    case = dc.gpu_case(name)
    L = dc.TEAM_LOG_N
    full = _oracle(corc, oracle, case.coeffs, L, case.betas)
    assert full.n_layers == len(case.schedule), name
    res = team4.commit(case.coeffs, L, forced_betas=case.betas)
    _check(team4, res, full, case.schedule, L, name, False)
    check_transport_schedule([team4.team_rank(r).transport_log() for r in range(4)])
    _dense_after(team4, oracle, oracle_commit, L, case.d, name)
    check_transport_schedule([team4.team_rank(r).transport_log() for r in range(4)])
