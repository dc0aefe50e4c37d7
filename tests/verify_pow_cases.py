"""Ground transcripts for the tests of the batched verifier's nonce check
(test_verify_pow_host.py on the CPU, test_gpu_verify_pow.py on the device),
made on the CPU: the oracle's commit, a nonce from grind_model sent on the
oracle's channel, then the oracle's query phase on the ground channel (the
recipe of test_grind_host.py).  Tamperings of them, and the batches both tests
hand to verify_pow_model.  Built once per process."""
import copy
import dataclasses
import functools

import fri_amd
import fri_oracle as fo
import grind_model as gm
import verify_batch_cases as vc
from verify_mask_corpus import MIXED, S1, S2

P = fo.P

# how a member's nonce is chosen: ("grind", bits, first) is grind_model.grind's
# answer (the verifiers do not check minimality, so any `first` is honest);
# ("weak", bits) the smallest nonce whose state has FEWER than `bits` zero bits
GRIND8 = ("grind", 8, 0)
HIGH32 = ("grind", 4, 2 ** 32 - 3)        # crosses into the high word
HIGH63 = ("grind", 4, 2 ** 63)            # the high word's top bit


def pick_nonce(state, rule):
    if rule[0] == "grind":
        return gm.grind(state, rule[1], rule[2])[0]
    v = 0
    while gm.zero_bits(gm.grind(state, 0, v)[1]) >= rule[1]:
        v += 1
    return v


@dataclasses.dataclass
class Ground:
    msgs: list          # the transcript with its nonce
    plain: list         # the same commit's transcript without one (other indices follow)
    pos: int            # the nonce's position in msgs
    after: str          # the state after the nonce's send
    nonce: int
    nl: int
    a_last: int = 0


def _send_nonce(ch, rule):
    nonce = pick_nonce(ch.state, rule)
    want = gm.grind(ch.state, 0, nonce)[1]
    ch.send(nonce.to_bytes(8, "big"))
    assert ch.state == want
    return nonce


@functools.lru_cache(maxsize=None)
def _fri_commit(seed, coeffs, log_n, state):
    ch = fo.Channel(state=state)
    return ch, fo.fri_commit(fo.splitmix64_field(seed, coeffs), log_n, ch)


@functools.lru_cache(maxsize=None)
def fri_ground(seed, coeffs, log_n, queries, max_index, state="", rule=GRIND8):
    ch0, r = _fri_commit(seed, coeffs, log_n, state)
    ch, plain = copy.deepcopy(ch0), copy.deepcopy(ch0)
    pos = len(ch.proof)
    nonce = _send_nonce(ch, rule)
    after = ch.state
    fo.decommit_fri(queries, max_index, r.layers, r.trees, ch)
    fo.decommit_fri(queries, max_index, r.layers, r.trees, plain)
    return Ground(list(ch.proof), list(plain.proof), pos, after, nonce, len(r.roots))


@functools.lru_cache(maxsize=None)
def _fibsq_commit(a1, log_t, lb, state):
    ch = fo.Channel(state=state)
    pr = fo.fibsq_prove(a1, log_t, lb, 0, ch)
    trace = fo.fibsq_trace(a1, 1 << log_t)
    f = fo.interpolate_lagrange_polynomials(fo.coset_domain(log_t, offset=1), trace, P)
    f_eval = [fo.poly_evaluate(f, x, P) for x in fo.coset_domain(log_t + lb)]
    return ch, pr, f_eval, fo.merkle_levels(f_eval), trace[-1]


@functools.lru_cache(maxsize=None)
def fibsq_ground(a1, log_t, lb, queries, state="", rule=GRIND8):
    ch0, pr, f_eval, f_levels, a_last = _fibsq_commit(a1, log_t, lb, state)
    L, B = log_t + lb, 1 << lb

    def query_phase(ch):                               # fibsq_prove's (fri_oracle.py)
        for _ in range(queries):
            idx = ch.receive_random_int(0, (1 << L) - 2 * B - 1, True)
            for j in range(3):
                ch.send(fo.fe_to_bytes(f_eval[idx + j * B]))
                ch.send(fo.merkle_proof(f_levels, idx + j * B))
            fo.decommit_fri_layers(idx, pr.fri.layers, pr.fri.trees, ch)
    ch, plain = copy.deepcopy(ch0), copy.deepcopy(ch0)
    pos = len(ch.proof)
    nonce = _send_nonce(ch, rule)
    after = ch.state
    query_phase(ch)
    query_phase(plain)
    return Ground(list(ch.proof), list(plain.proof), pos, after, nonce, len(pr.fri.roots), a_last)


# ---- tamperings: Ground -> messages -----------------------------------------
def honest(g):
    return list(g.msgs)


def nonce_plus_one(g):
    """Another nonce with the rest honest: other indices would follow."""
    other = ((g.nonce + 1) % 2 ** 64).to_bytes(8, "big")
    return g.msgs[:g.pos] + [other] + g.msgs[g.pos + 1:]


def behind_nonce(g):
    """The openings of the transcript without a nonce, behind the nonce."""
    return g.plain[:g.pos] + [g.msgs[g.pos]] + g.plain[g.pos:]


def flipped_index(g):
    """The first claimed index + 2^24: the same openings, another draw."""
    return vc.flip(g.msgs, g.pos + 1)


def flipped_last_path(g):
    """A byte of the last path that is not empty, behind every draw."""
    return vc.flip(g.msgs, max(i for i, m in enumerate(g.msgs) if len(m) >= 32 and i > g.pos))


TAMPERINGS = [honest, nonce_plus_one, behind_nonce, flipped_index, flipped_last_path]


# ---- batches ----------------------------------------------------------------
@dataclasses.dataclass
class Batch:
    pk: "fri_amd.PackedTranscripts"
    names: list
    msgs: list
    nls: list
    bits: int
    states: list
    grounds: list                  # the Ground every member was made from
    a_last: list = None

    def verify(self, b, bits=None, msgs=None):
        """The host verifier on member b (or on other messages in its place)."""
        sh, bits = self.pk.shape, self.bits if bits is None else bits
        msgs = self.msgs[b] if msgs is None else msgs
        if sh.trace_count:
            return fri_amd.verify_fibsq(msgs, self.a_last[b], sh.log_t, sh.log_blowup, sh.num_queries, self.nls[b],
                                        sh.offset, self.states[b], grinding_bits=bits)
        return fri_amd.verify_fri(msgs, sh.log_n, self.nls[b], sh.num_queries, sh.max_index, sh.offset,
                                  self.states[b], grinding_bits=bits)

    def repack(self, b, bits, msgs=None):
        """Member b alone (or other messages in its place) packed under `bits`."""
        return _pack([self.msgs[b] if msgs is None else msgs], [self.nls[b]], [self.states[b]], bits, self.pk.shape,
                     [self.a_last[b]] if self.a_last else None)


def _pack(msgs, nls, states, bits, sh, a_last):
    return fri_amd.pack_transcripts(msgs, sh.log_n, nls, sh.num_queries, sh.max_index, sh.trace_count, sh.log_t,
                                    sh.log_blowup, a_last, offset=sh.offset, channel_states=states,
                                    grinding_bits=bits)


def _batch(members, bits, log_n, queries, max_index, tc=0, log_t=0, lb=0):
    """members: (name, Ground, tampering, state)."""
    sh = fri_amd.VerifyShape(log_n, 1, queries, tc, log_t, lb, fo.GEN, max_index)
    msgs = [t(g) for _, g, t, _ in members]
    nls, states = [g.nl for _, g, _, _ in members], [s for _, _, _, s in members]
    a_last = [g.a_last for _, g, _, _ in members] if tc else None
    pk = _pack(msgs, nls, states, bits, sh, a_last)
    assert not pk.host.any() and not pk.reasons.any()          # every member goes to the device
    return Batch(pk, [n for n, _, _, _ in members], msgs, nls, bits, states, [g for _, g, _, _ in members], a_last)


RULES = [("grind8", GRIND8), ("high32", HIGH32), ("high63", HIGH63)]


@functools.lru_cache(maxsize=None)
def fibsq_batch():
    """(3, 2) with 2 queries under 8 bits: honest members from an empty and
    from a non-empty channel, every tampering, and nonces that lack the bits."""
    members = []
    for a1, st in ((3141592, ""), (99, S1)):
        g = fibsq_ground(a1, 3, 2, 2, st)
        members += [("%s a1=%d" % (t.__name__, a1), g, t, st) for t in TAMPERINGS]
        members.append(("weak a1=%d" % a1, fibsq_ground(a1, 3, 2, 2, st, ("weak", 8)), honest, st))
    return _batch(members, 8, 5, 2, 32 - 8 - 1, 3, 3, 2)


@functools.lru_cache(maxsize=None)
def fibsq_high_batch():
    """(3, 2) with 3 queries under 4 bits: the nonces with a high word."""
    members = []
    for a1, st in ((7, ""), (12345, S2)):
        for rn, rule in RULES:
            g = fibsq_ground(a1, 3, 2, 3, st, rule)
            members.append(("%s a1=%d" % (rn, a1), g, honest, st))
        members.append(("weak a1=%d" % a1, fibsq_ground(a1, 3, 2, 3, st, ("weak", 4)), honest, st))
        members.append(("high32+1 a1=%d" % a1, fibsq_ground(a1, 3, 2, 3, st, HIGH32), nonce_plus_one, st))
    return _batch(members, 4, 5, 3, 32 - 8 - 1, 3, 3, 2)


RAGGED_MEMBERS = 67


@functools.lru_cache(maxsize=None)
def fri_ragged_batch():
    """FRI-only at log_n = 6 under 4 bits, 67 members (a wave and a ragged
    one): the layer counts of MIXED, three channel states, the three nonce
    rules, accepted and rejected members interleaved."""
    kinds = [("grind8", GRIND8, honest), ("weak", ("weak", 4), honest), ("high32", HIGH32, honest),
             ("high32+1", HIGH32, nonce_plus_one), ("high63", HIGH63, honest), ("index", HIGH63, flipped_index),
             ("behind", GRIND8, behind_nonce), ("path", HIGH32, flipped_last_path)]
    members = []
    for b in range(RAGGED_MEMBERS):
        d, st = MIXED[b % len(MIXED)], ("", S1, S2)[b % 3]
        name, rule, t = kinds[b % len(kinds)]
        g = fri_ground(500 + b, d, 6, 2, 63, st, rule)
        members.append(("%s nl=%d #%d" % (name, g.nl, b), g, t, st))
    return _batch(members, 4, 6, 2, 63)


@functools.lru_cache(maxsize=None)
def one_element_batch():
    """FRI-only at blowup 1 (8 coefficients at log_n = 3) under 8 bits: the
    last layer has one element, whose value is sent twice, before the nonce's
    draws and after."""
    members = []
    for seed, st in ((15, ""), (16, S1)):
        g = fri_ground(seed, 8, 3, 2, 7, st)
        assert g.nl == 4
        members += [("%s seed=%d" % (t.__name__, seed), g, t, st) for t in TAMPERINGS]
        members.append(("weak seed=%d" % seed, fri_ground(seed, 8, 3, 2, 7, st, ("weak", 8)), honest, st))
    return _batch(members, 8, 3, 2, 7)


def batches():
    """(name, Batch) of every batch the tests hand to the model."""
    yield "fibsq (3,2,2) 8 bits", fibsq_batch()
    yield "fibsq (3,2,3) 4 bits, high words", fibsq_high_batch()
    yield "FRI ragged 4 bits", fri_ragged_batch()
    yield "FRI one-element layer 8 bits", one_element_batch()
