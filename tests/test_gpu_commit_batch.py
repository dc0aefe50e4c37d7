"""GPU: fri_commit_batch, B independent commits of one shape in one call.

One launch commits every member, one workgroup each (k_commit_batch): layers
of more than 2^9 elements in tiles of 2^9 leaves through the member's HBM
slots, smaller ones in LDS as k_tree_tail does; the members' LDE runs in LDS
up to 2^12 and through the batched transform above.  The yardstick of every
test is the C oracle (orc_fri_commit_fast / stored_proof.oracle_commit_full)
under the member's own channel state and forced betas; a batch is never
compared with itself.  Up to 2^14 every stored value and tree node of every
member is compared too, through a view of one member behind the read-back
interface stored_proof_mismatch expects of a Context."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import degree_cases as dc
import stored_proof as sp

pytestmark = pytest.mark.gpu

import fri_amd  # noqa: E402

CAP = fri_amd.BATCH_MAX_LOG_N
LDS_LDE = fri_amd.BATCH_LDE_LDS_MAX_LOG_N       # the LDE's switch point: LDS up to here, batched transform above
STORED_MAX_LOG = 14
FRI_EINVAL, FRI_ESTATE, FRI_EDEGREE = fri_amd.FRI_EINVAL, fri_amd.FRI_ESTATE, fri_amd.FRI_EDEGREE


def test_constants_match_header():
    import re
    text = open(fri_amd.HEADER_PATH).read()
    assert int(re.search(r"#define\s+FRI_BATCH_MAX_LOG_N\s+(\d+)", text).group(1)) == CAP
    assert int(re.search(r"#define\s+FRI_BATCH_LDE_LDS_MAX_LOG_N\s+(\d+)", text).group(1)) == LDS_LDE
    assert 14 <= CAP <= 18


def _want(corc, oracle, coeffs, log_n, betas=None, state=None):
    """The C oracle's commit of one member; with everything it stores up to 2^14."""
    if log_n <= STORED_MAX_LOG:
        return sp.oracle_commit_full(corc, oracle, coeffs, log_n, state=state, forced_betas=betas)
    c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.uint64))
    fb = None if betas is None else np.ascontiguousarray(np.asarray(betas, dtype=np.uint64))
    och = oracle.OrcChannel()
    corc.orc_channel_init(ctypes.byref(och))
    if state:
        och.state = sp._state_hex(state).encode()
        och.state_len = 64
    res = oracle.OrcFriResult()
    assert corc.orc_fri_commit_fast(c.ctypes.data_as(sp.P64), c.size, log_n, 5, oracle.GEN, oracle.P, ctypes.byref(och),
                                    None if fb is None else fb.ctypes.data_as(sp.P64), ctypes.byref(res), None,
                                    None) == 0
    return SimpleNamespace(n_layers=int(res.n_layers), roots=[bytes(res.roots[k]) for k in range(res.n_layers)],
                           betas=[int(res.betas[r]) for r in range(res.n_rounds)], final_value=int(res.final_value),
                           final_degree=int(res.final_degree), state=och.state.decode())


class MemberView:
    """Member b of the resident batch as stored_proof_mismatch reads a Context."""

    def __init__(self, ctx, b):
        self.m = fri_amd.BatchMember(ctx, b)
        self.h, self._check = ctx.h, ctx._check
        self.lib = SimpleNamespace(fri_tree_level_copy=lambda h, k, level, buf, n:
                                   ctx.lib.fri_batch_tree_level_copy(h, b, k, level, buf, n))

    def layer(self, k, log_n):
        return self.m.layer(k, log_n)


def _transcript(res):
    roots, betas, fv, fd, state = sp.transcript_of(res)
    return roots, betas, fv, fd, (state if res.channel_out.has_state else "")


def _check_member(ctx, b, res, full, log_n, what, schedule=None):
    assert _transcript(res) == sp.transcript_want(full), what
    assert res.n_layers == full.n_layers and res.log_n == log_n, what
    if schedule is not None:
        assert ctx.batch_commit_degrees(b) == schedule, what
    if log_n <= STORED_MAX_LOG:
        msg = sp.stored_proof_mismatch(MemberView(ctx, b), full, log_n)
        assert msg is None, f"{what}: {msg}"


def _members(oracle, seed, count, d):
    return [oracle.splitmix64_np(seed + b, d).astype(np.uint32) for b in range(count)]


def _run_batch(ctx, corc, oracle, log_n, polys, what, betas=None, states=None):
    """One batch, every member against the oracle (transcript, degrees, stored proof)."""
    res = ctx.commit_batch(polys, log_n, forced_betas=betas, channel_states=states)
    assert ctx.batch_status == [0] * len(polys), what
    assert ctx.batch_info()[1:] == (len(polys), log_n), what
    for b, c in enumerate(polys):
        fb = None if betas is None else betas[b]
        full = _want(corc, oracle, c, log_n, betas=fb, state=None if states is None else states[b])
        sched = dc.degree_schedule(c, (full.betas if fb is None else list(fb)) + [0] * dc.N_BETAS)
        assert len(sched) == full.n_layers, what
        _check_member(ctx, b, res[b], full, log_n, f"{what} member {b}", sched)
    return res


def _sweep_logs():
    return sorted({1, 2, 3, 5, 9, 10, 11, 12, 13, 14, CAP, LDS_LDE, LDS_LDE + 1})


def _sweep_ds(log_n):
    n = 1 << log_n
    ds = []
    if n >= 8:
        ds.append(n // 8)
    ds.append(n)                                  # blowup 1
    odd = n // 8 - 1 if n // 8 - 1 >= 3 else 3    # not a power of two
    if odd <= n:
        ds.append(odd)
    return ds


# ---- 1. parity sweep ---------------------------------------------------------
@pytest.mark.parametrize("log_n", _sweep_logs())
def test_parity_sweep(ctx, corc, oracle, log_n):
    """5 distinct members at blowup 8, blowup 1 and a d that is no power of
    two; then member 0's input through ctx.commit on the same context: the
    same transcript, and the single path survived the batch."""
    for d in _sweep_ds(log_n):
        polys = _members(oracle, 9000 + 10 * log_n, 5, d)
        what = f"2^{log_n} d={d}"
        res = _run_batch(ctx, corc, oracle, log_n, polys, what)
        single = ctx.commit(polys[0], log_n)
        assert sp.transcript_of(single) == sp.transcript_of(res[0]), what
        assert ctx.batch_info()[1] == 0, what


# ---- 2. batch sizes ----------------------------------------------------------
@pytest.mark.parametrize("log_n,batch", [(10, 1), (10, 2), (10, 7), (6, 300), (CAP, 3)])
def test_batch_sizes(ctx, corc, oracle, log_n, batch):
    """Every member checked, also with more members than CUs."""
    d = (1 << log_n) // 8
    _run_batch(ctx, corc, oracle, log_n, _members(oracle, 500 + batch, batch, d), f"B={batch} 2^{log_n}")


# ---- 3. degree events in one batch -------------------------------------------
def _event_cases(log_n, d):
    if (log_n, d) == (12, 512):
        return [dc.gpu_case("12_tail_chain"), dc.gpu_case("12_tail_cancel_zero")]
    if (log_n, d) == (10, 128):
        # 127 -> cancel to 21 at fold 0, 10, 5 -> phantom 2, -1
        return [dc.chain(10, 128, {0: ("cancel", 21), 3: ("phantom", 2)}, 1001, "10_cancel0_phantom3"),
                dc.cancel(10, 128, 0, -1, 1002)]
    return dc.family_cases(log_n, d)


@pytest.mark.parametrize("log_n,d", [(9, 64), (5, 4), (5, 32), (12, 512), (10, 128)])
def test_degree_events_in_one_batch(ctx, corc, oracle, log_n, d):
    """Members with their own forced betas end at different layers of the one
    launch; one dense member runs every layer beside them."""
    cases = _event_cases(log_n, d)
    polys = [c.coeffs for c in cases] + [oracle.splitmix64_np(31, d).astype(np.uint32)]
    betas = [c.betas for c in cases] + [dc.make_betas(77)]
    scheds = [c.schedule for c in cases] + [[(d - 1) >> k for k in range(d.bit_length())]]
    for case in cases:      # the oracle alone shows the event
        full = _want(corc, oracle, case.coeffs, log_n, betas=case.betas)
        assert full.n_layers == len(case.schedule) and full.final_degree == case.schedule[-1], case.name
    res = _run_batch(ctx, corc, oracle, log_n, polys, f"events 2^{log_n}/{d}", betas=betas)
    assert [r.n_layers for r in res] == [len(s) for s in scheds]
    assert [ctx.batch_commit_degrees(b) for b in range(len(polys))] == scheds
    assert len({r.n_layers for r in res}) > 1


# ---- 4. per-member channels --------------------------------------------------
def test_per_member_channels(ctx, corc, oracle):
    log_n, d = 11, 256
    polys = _members(oracle, 40, 4, d)
    states = [bytes([17 * b + i for i in range(32)]) for b in range(3)] + [None]
    _run_batch(ctx, corc, oracle, log_n, polys, "channels", states=states)
    a = ctx.commit_batch(polys, log_n, channel_states=None)
    b = ctx.commit_batch(polys, log_n, channel_states=[None] * 4)
    assert [_transcript(r) for r in a] == [_transcript(r) for r in b]
    assert _transcript(a[0]) == sp.transcript_want(_want(corc, oracle, polys[0], log_n))


# ---- 5. zero members ---------------------------------------------------------
@pytest.mark.parametrize("log_n", [4, 10, 13])
def test_zero_members(ctx, corc, oracle, log_n):
    n = 1 << log_n
    empty = [np.zeros(0, dtype=np.uint32)] * 3
    res = ctx.commit_batch(empty, log_n)
    full = _want(corc, oracle, [], log_n)
    for b in range(3):
        _check_member(ctx, b, res[b], full, log_n, f"d = 0 member {b}", [-1])
    d = n // 8
    polys = [np.zeros(d, dtype=np.uint32), oracle.splitmix64_np(3, d).astype(np.uint32), np.zeros(d, dtype=np.uint32)]
    res = _run_batch(ctx, corc, oracle, log_n, polys, "all-zero coefficients")
    assert [r.n_layers for r in res] == [1, d.bit_length(), 1] and res[0].final_degree == -1


# ---- 6. failure isolation ----------------------------------------------------
@pytest.mark.parametrize("log_n", [8, 11, 13])
def test_failure_isolation(ctx, corc, oracle, log_n):
    d = (1 << log_n) // 8
    polys = _members(oracle, 60, 5, d)
    polys[2] = polys[2].copy()
    polys[2][d // 2] = fri_amd.P                    # not canonical
    with pytest.raises(fri_amd.FriError) as e:
        ctx.commit_batch(polys, log_n)
    assert e.value.code == FRI_EINVAL
    assert ctx.batch_status == [0, 0, FRI_EINVAL, 0, 0]
    for b in (0, 1, 3, 4):
        full = _want(corc, oracle, polys[b], log_n)
        _check_member(ctx, b, ctx.batch_results[b], full, log_n, f"beside a failed member: {b}",
                      [(d - 1) >> k for k in range(d.bit_length())])
    assert ctx.batch_results[2].n_layers == 0
    for call in (lambda: ctx.batch_layer(2, 0, log_n), lambda: ctx.batch_tree_level(2, 0, 0, log_n),
                 lambda: ctx.batch_commit_degrees(2), lambda: ctx.batch_decommit_query(2, 1, 1, log_n)):
        with pytest.raises(fri_amd.FriError) as e:
            call()
        assert e.value.code == FRI_ESTATE


# ---- 7. decommitment ---------------------------------------------------------
def _oracle_decommit(corc, oracle, coeffs, log_n, queries):
    """The oracle's whole transcript: the C oracle's commit (every value and
    node kept), then decommit_fri (fri_commit.rs:137-179) over what it stored,
    on the Python oracle's channel."""
    full = sp.oracle_commit_full(corc, oracle, coeffs, log_n)
    och = oracle.Channel()
    for k, root in enumerate(full.roots):
        och.proof.append(root.hex().encode())
        if k < len(full.betas):
            och.proof.append(full.betas[k].to_bytes(8, "big"))
    och.proof.append(full.final_value.to_bytes(8, "big"))
    och.state = full.state
    for _ in range(queries):
        index = och.receive_random_int(0, (1 << log_n) - 1, True)
        for k in range(full.n_layers):
            m = (1 << log_n) >> k
            idx = index % m
            sib = (idx + m // 2) % m
            if m == 1:
                och.send(int(full.values[k][0]).to_bytes(8, "big"))
            for i in (idx, sib):
                och.send(int(full.values[k][i]).to_bytes(8, "big"))
                och.send(sp.expected_path(full.levels[k], i))
    return och


@pytest.mark.parametrize("log_n", [10, CAP])
def test_decommitment(ctx, corc, oracle, log_n):
    d = (1 << log_n) // 8
    polys = _members(oracle, 70, 3, d)
    chans = [fri_amd.Channel() for _ in polys]
    proofs = fri_amd.fri_commit_batch(polys, log_n, chans, ctx=ctx)
    assert [p.member for p in proofs] == [0, 1, 2]
    for b in (2, 0):
        fri_amd.decommit_fri(3, (1 << log_n) - 1, proofs[b], chans[b])
        want = _oracle_decommit(corc, oracle, polys[b], log_n, 3)
        assert chans[b].proof == want.proof and chans[b].state == want.state, f"member {b}"
        msgs = list(chans[b].proof)
        assert fri_amd.verify_fri(msgs, log_n, proofs[b].n_layers, 3, (1 << log_n) - 1)
        bad = list(msgs)
        flip = bytearray(bad[len(bad) // 2])
        flip[0] ^= 1
        bad[len(bad) // 2] = bytes(flip)
        assert not fri_amd.verify_fri(bad, log_n, proofs[b].n_layers, 3, (1 << log_n) - 1)
    # the reference's own form, through the proof's layers and device-backed trees
    ch2 = fri_amd.Channel()
    ch2.state, ch2.proof = chans[1].state, list(chans[1].proof)
    fri_amd.decommit_fri(1, (1 << log_n) - 1, proofs[1].fri_layers, proofs[1].fri_merkles, ch2)
    fri_amd.decommit_fri(1, (1 << log_n) - 1, proofs[1], chans[1])
    assert ch2.proof == chans[1].proof
    v = proofs[1].layer(1)
    path = proofs[1].fri_merkles[1].get_authentication_path(5)
    assert fri_amd._merkle_path_ok(int(v[5]), 5, path, log_n - 1, proofs[1].roots[1])


# ---- 8. residency ------------------------------------------------------------
def test_residency(ctx, corc, oracle):
    polys = _members(oracle, 80, 3, 128)
    res = ctx.commit_batch(polys, 10)
    g, log_n, n_layers = ctx.commit_info()
    assert n_layers == 0 and g == ctx.batch_info()[0]
    for call in (lambda: ctx.layer(0, 10), lambda: ctx.decommit_query(1, res[0].n_layers, 10)):
        with pytest.raises(fri_amd.FriError) as e:
            call()
        assert e.value.code == FRI_ESTATE
    ctx.lib.fri_layer_copy(ctx.h, 0, fri_amd._ptr(np.empty(1024, dtype=np.uint32)), 1024)
    assert b"fri_batch_" in ctx.lib.fri_last_error(ctx.h)
    single = ctx.commit(polys[1], 10)
    assert sp.transcript_of(single) == sp.transcript_of(res[1])
    assert ctx.commit_info()[1:] == (10, single.n_layers)
    with pytest.raises(fri_amd.FriError) as e:
        ctx.batch_layer(0, 0, 10)
    assert e.value.code == FRI_ESTATE
    # another shape, then the first again: both correct
    _run_batch(ctx, corc, oracle, 13, _members(oracle, 81, 4, 1024), "second shape")
    _run_batch(ctx, corc, oracle, 10, polys, "first shape again")


# ---- 9. refusals -------------------------------------------------------------
def _raw_batch(cx, d, batch, log_n, flags=0):
    c = np.zeros(max(d * max(batch, 1), 1), dtype=np.uint32)
    res = (fri_amd.CommitResult * max(batch, 1))()
    status = (ctypes.c_int * max(batch, 1))(*([-1] * max(batch, 1)))
    rc = cx.lib.fri_commit_batch(cx.h, fri_amd._ptr(c), d, batch, log_n, 5, None, flags, None, res, status)
    if rc:
        assert list(status) == [-1] * max(batch, 1)     # a refused call writes nothing
    else:
        assert list(status) == [0] * batch and all(r.n_layers == 1 and r.final_degree == -1 for r in res)
    return rc


def test_refusals(ctx):
    gen = ctx.batch_info()[0]
    assert _raw_batch(ctx, 16, 2, CAP + 1) == FRI_EINVAL
    assert _raw_batch(ctx, 1025, 2, 10) == FRI_EDEGREE
    assert _raw_batch(ctx, 16, 0, 10) == FRI_EINVAL
    assert _raw_batch(ctx, 16, 65536, 10) == FRI_EINVAL
    assert _raw_batch(ctx, 16, 2, 0) == FRI_EINVAL
    assert _raw_batch(ctx, 16, 2, 10, fri_amd.FLAG_RANK_INPUTS) == FRI_EINVAL
    assert _raw_batch(ctx, 16, 2, 10, fri_amd.FLAG_FORCE_BETAS) == FRI_EINVAL      # no betas given
    assert ctx.batch_info()[0] == gen                # none of them counted as a commit
    assert _raw_batch(ctx, 16, 2, 10, fri_amd.FLAG_NO_GRAPH) == fri_amd.FRI_OK


def test_team_context_refused():
    team = fri_amd.Context.multi([0, 0], 20, transport="peer")
    try:
        assert _raw_batch(team, 16, 2, 10) == FRI_EINVAL
    finally:
        team.close()


def test_profiling_context_refused(oracle):
    cx = fri_amd.Context(0, 12)
    try:
        cx.set_profiling(True)
        assert _raw_batch(cx, 16, 2, 10) == FRI_ESTATE
        cx.set_profiling(False)
        assert _raw_batch(cx, 16, 2, 10) == fri_amd.FRI_OK
    finally:
        cx.close()


# ---- 10. device input --------------------------------------------------------
@pytest.mark.parametrize("log_n", [10, 13])
def test_device_input(ctx, corc, oracle, log_n):
    """fri_commit_batch_device reads batch*d words in place from a device
    buffer (fri_amd.DeviceBuffer, what this suite's device-input tests use
    for a data_ptr()): the host-input call's results, and the oracle's."""
    d, batch = (1 << log_n) // 8, 6
    polys = _members(oracle, 90, batch, d)
    host = [_transcript(r) for r in ctx.commit_batch(polys, log_n)]
    dev = fri_amd.DeviceBuffer(np.concatenate(polys))
    got = ctx.commit_batch(None, log_n, d_coeffs=dev.data_ptr(), d=d, batch=batch)
    assert [_transcript(r) for r in got] == host
    assert host[-1] == sp.transcript_want(_want(corc, oracle, polys[-1], log_n))
    assert (ctx.batch_layer(batch - 1, 0, log_n) == ctx.lde(polys[-1], log_n)).all()


# ---- memory: FRI_ENOMEM leaves what was resident readable --------------------
def test_enomem_keeps_the_resident_commit(corc, oracle):
    cx = fri_amd.Context(0, 14)
    try:
        log_n, d = 12, 512
        polys = _members(oracle, 95, 40, d)
        single = cx.commit(polys[0], log_n)
        layer1 = cx.layer(1, log_n)
        cx.set_device_cap(cx.device_bytes()[0] + (1 << 20))          # a member takes 0.53 MiB
        with pytest.raises(fri_amd.FriError) as e:
            cx.commit_batch(polys, log_n)
        assert e.value.code == fri_amd.FRI_ENOMEM
        assert cx.commit_info()[1:] == (log_n, single.n_layers) and (cx.layer(1, log_n) == layer1).all()
        # a resident batch survives a larger batch that gets no memory
        cx.set_device_cap(0)
        _run_batch(cx, corc, oracle, log_n, polys[:2], "small batch")
        cx.set_device_cap(cx.device_bytes()[0] + (1 << 20))
        gen = cx.batch_info()[0]
        with pytest.raises(fri_amd.FriError) as e:
            cx.commit_batch(polys, log_n)
        assert e.value.code == fri_amd.FRI_ENOMEM and cx.batch_info() == (gen, 2, log_n)
        full = _want(corc, oracle, polys[1], log_n)
        assert sp.stored_proof_mismatch(MemberView(cx, 1), full, log_n) is None
        cx.set_device_cap(0)
        _run_batch(cx, corc, oracle, log_n, polys, "after the cap is lifted")
    finally:
        cx.close()


def test_batch_settles_pending_pipelined_commits(corc, oracle):
    """Two pipelined commits are pending when the batch is called: the batch
    is correct, and the tickets still deliver their own results afterwards."""
    cx = fri_amd.Context(0, 14)
    try:
        log_n, d = 13, 1024
        polys = _members(oracle, 97, 4, d)
        tickets = [cx.commit_async(polys[i], log_n) for i in (0, 1)]
        _run_batch(cx, corc, oracle, log_n, polys[2:], "batch behind pending commits")
        for i, t in zip((0, 1), tickets):
            assert sp.transcript_of(cx.commit_wait(t)) == sp.transcript_want(_want(corc, oracle, polys[i], log_n))
        assert cx.batch_info()[1] == 2      # waiting is no commit: the batch stays resident
        full = _want(corc, oracle, polys[3], log_n)
        assert sp.stored_proof_mismatch(MemberView(cx, 1), full, log_n) is None
    finally:
        cx.close()
