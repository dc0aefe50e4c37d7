"""Test helper: polynomials whose degree does something other than halve.

A dense polynomial folded with a channel-drawn beta loses exactly half its
degree each round, so the three maxima fri_commit reduces per fold (m0: last
non-zero index of c_2j + beta c_2j+1, m1: of the even part, m2: of the odd
part; csrc/fri_layer.hip coef_slice) all equal nlen - 1 and sit in the last
workgroup that has work.  The builders here work backwards from a terminal
polynomial to poly_0 under a fixed list of forced betas (FRI_FLAG_FORCE_BETAS;
the oracles take the same list), so that chosen folds separate the three:

  cancel(r, a)       dense odd part, poly_{r+1} of degree a far below
                     deg(poly_r) // 2: m0 = a, m1 = m2 = nlen - 1.  a = 0
                     collapses to a constant, a = -1 to the zero polynomial.
  beta_zero(r, b, c) betas[r] = 0, even top b, odd top c: m0 = m1 = b, m2 = c.
  even_zero(r)       poly_r = x Q(x^2) / beta_r: m1 = -1, m0 = m2.
  phantom(r, c)      even part zero and betas[r] = 0: poly_{r+1} is all zeros,
                     but the reference keeps degree c for one more round
                     (scalar_mul keeps the degree field, add_assign of a zero
                     right-hand side leaves the left unchanged), then -1:
                     m0 = m1 = -1, m2 = c.
  chain              several of them at different folds of one commit.

"Fold r" takes poly_r to poly_{r+1} with betas[r]; its maxima are settled by
layer r + 1's kernels.  Every builder asserts that degree_schedule of what it
built is exactly the schedule it planned and contains the event it was asked
for, so a case cannot quietly degrade to the dense one.  Plain numpy: nothing
here needs a GPU, and nothing here is collected by pytest."""
from types import SimpleNamespace

import numpy as np

P = 3 * 2**30 + 1
N_BETAS = 32          # FRI_MAX_ROUNDS: the forced-beta list is always whole
_P = np.uint64(P)


def top(c):
    """Last non-zero index of c, -1 if there is none."""
    nz = np.flatnonzero(np.asarray(c))
    return int(nz[-1]) if nz.size else -1


def _pad(c, m):
    out = np.zeros(m, dtype=np.uint64)
    out[:len(c)] = c
    return out


def fold(c, beta):
    """c_2j + beta c_2j+1 (untrimmed; (p-1)^2 + p - 1 < 2^64)."""
    c = _pad(c, len(c) + (len(c) & 1))
    return (c[0::2] + np.uint64(beta) * c[1::2] % _P) % _P


def unfold(q, beta, odd):
    """The coefficient vector with even part q - beta * odd and odd part `odd`,
    interleaved: folding it with `beta` gives exactly q."""
    m = max(len(q), len(odd))
    q, odd = _pad(q, m), _pad(odd, m)
    out = np.empty(2 * m, dtype=np.uint64)
    out[0::2] = (q + _P - np.uint64(beta) * odd % _P) % _P
    out[1::2] = odd
    return out


def fold_maxima(c, beta):
    """(m0, m1, m2) of folding c with beta, and the folded coefficients."""
    c = _pad(c, len(c) + (len(c) & 1))
    q = fold(c, beta)
    return (top(q), top(c[0::2]), top(c[1::2])), q


def degree_schedule(coeffs, betas):
    """The reference's degree field of every layer's polynomial
    (fri_commit.rs:32-50, 89): deg_0 is the trimmed degree; a fold gives the
    trimmed degree of the sum (m0) unless the even part is zero, where the
    scaled odd part is returned with the degree it had before scaling (m2).
    The commit ends at the first degree below 1."""
    c = np.asarray(coeffs, dtype=np.uint64)
    sched = [top(c)]
    r = 0
    while sched[-1] >= 1:
        (m0, m1, m2), c = fold_maxima(c[:sched[-1] + 1], betas[r])
        sched.append(m2 if m1 < 0 else m0)
        r += 1
    return sched


def fold_chain(case):
    """The coefficients left after the last fold of case.schedule (the final value is the first)."""
    c = case.coeffs.astype(np.uint64)
    for r in range(len(case.schedule) - 1):
        c = fold(c[:case.schedule[r] + 1], case.betas[r])
    return c


def make_betas(seed, zero_at=()):
    """32 canonical non-zero betas from `seed`, zero at the folds of zero_at."""
    b = np.random.default_rng(seed).integers(1, P, N_BETAS, dtype=np.uint64)
    for r in zero_at:
        b[r] = 0
    return [int(x) for x in b]


def _plan(deg0, betas, events):
    """Forward: the degree schedule that `events` ask for, checking each
    event's preconditions.  Returns (schedule, all-zero flags per layer)."""
    D, zero = [deg0], [deg0 < 0]
    r = 0
    while D[-1] >= 1:
        ev = events.get(r, ("dense",))
        d, kind = D[-1], ev[0]
        if zero[-1]:                       # the round after a phantom
            assert kind == "dense", (r, ev)
            D.append(-1)
            zero.append(True)
        elif kind == "dense":
            D.append(d // 2)
            zero.append(False)
        elif kind == "cancel":
            a = ev[1]
            assert d & 1 and betas[r] != 0 and -1 <= a < d // 2, (r, ev, d)
            D.append(a)
            zero.append(a < 0)
        elif kind == "beta_zero":
            _, b, c = ev
            assert betas[r] == 0 and b != c and b >= 0 and c >= 0 and max(2 * b, 2 * c + 1) == d, (r, ev, d)
            D.append(b)
            zero.append(False)
        elif kind == "even_zero":
            assert d & 1 and betas[r] != 0, (r, ev, d)
            D.append(d // 2)
            zero.append(False)
        elif kind == "phantom":
            c = ev[1]
            assert betas[r] == 0 and d == 2 * c + 1, (r, ev, d)
            D.append(c)
            zero.append(True)
        else:
            raise ValueError(ev)
        r += 1
    assert all(e < r for e in events), (events, D)
    return D, zero


def build(name, log_n, d, events, seed, deg0=None):
    """poly_0 (d coefficients, degree deg0, default d - 1) and its 32 forced
    betas such that fold r behaves as events[r] says and every other fold is
    dense.  events: {r: ("cancel", a) | ("beta_zero", b, c) | ("even_zero",) |
    ("phantom", c)}."""
    rng = np.random.default_rng(seed)
    deg0 = d - 1 if deg0 is None else deg0
    assert deg0 < d <= 1 << log_n
    betas = make_betas(seed + 1, [r for r, ev in events.items() if ev[0] in ("beta_zero", "phantom")])
    D, zero = _plan(deg0, betas, events)

    def dense(n):
        return rng.integers(1, P, max(n, 0), dtype=np.uint64)

    T = len(D) - 1
    q = np.zeros(0, dtype=np.uint64) if zero[T] else dense(1)           # D[T] is 0 or -1
    for r in range(T - 1, -1, -1):
        kind = events.get(r, ("dense",))[0]
        if zero[r]:
            q = np.zeros(0, dtype=np.uint64)
        elif kind in ("dense", "cancel"):
            q = unfold(q, betas[r], dense((D[r] + 1) // 2))               # odd D[r]: the odd part carries the top
        elif kind == "beta_zero":
            q = unfold(q, 0, dense(events[r][2] + 1))
        elif kind == "even_zero":
            inv = pow(betas[r], P - 2, P)
            q = unfold(np.zeros(0, dtype=np.uint64), 0, q * np.uint64(inv) % _P)
        elif kind == "phantom":
            q = unfold(np.zeros(0, dtype=np.uint64), 0, dense(events[r][1] + 1))
    coeffs = _pad(q[:deg0 + 1], d)
    assert top(q) == deg0 and int(coeffs.max(initial=0)) < P
    case = SimpleNamespace(name=name, log_n=log_n, d=d, coeffs=coeffs.astype(np.uint32), betas=betas,
                           schedule=D, events=dict(events), collapses=_collapses(D))
    check_events(case)
    return case


def _collapses(D):
    """A commit that ends while dense halving would still have rounds left."""
    return len(D) < max(D[0], 0).bit_length() + 1


def check_events(case):
    """The event assertions: the schedule of what was built is the planned
    one, and each fold's maxima are the ones its family is there to produce."""
    sched = degree_schedule(case.coeffs, case.betas)
    assert sched == case.schedule, (case.name, sched, case.schedule)
    c = case.coeffs.astype(np.uint64)
    for r in range(len(sched) - 1):
        (m0, m1, m2), c = fold_maxima(c[:sched[r] + 1], case.betas[r])
        ev = case.events.get(r)
        if ev is None:
            continue
        nlen = (sched[r] + 2) // 2
        if ev[0] == "cancel":
            assert sched[r + 1] < sched[r] // 2 and (m0, m1, m2) == (ev[1], nlen - 1, nlen - 1), (case.name, r, m0, m1, m2)
        elif ev[0] == "beta_zero":
            assert (m0, m1, m2) == (ev[1], ev[1], ev[2]) and sched[r + 1] == ev[1], (case.name, r, m0, m1, m2)
        elif ev[0] == "even_zero":
            assert m1 == -1 and m0 == m2 == nlen - 1 == sched[r + 1], (case.name, r, m0, m1, m2)
        elif ev[0] == "phantom":
            assert (m0, m1, m2) == (-1, -1, ev[1]) and sched[r + 1] == ev[1], (case.name, r, m0, m1, m2)
            assert ev[1] < 1 or sched[r + 2] == -1, (case.name, sched)


# ---- the families, one event each -------------------------------------------
def cancel(log_n, d, r, a, seed=1, name=None):
    return build(name or f"cancel({r},{a})@{log_n}", log_n, d, {r: ("cancel", a)}, seed)


def beta_zero(log_n, d, r, b, c, seed=2, name=None):
    """At fold 0 poly_0's degree is max(2b, 2c+1), whatever d is; at a later
    fold that must be the dense degree (d >> r) - 1."""
    return build(name or f"beta_zero({r},{b},{c})@{log_n}", log_n, d, {r: ("beta_zero", b, c)}, seed,
                 deg0=max(2 * b, 2 * c + 1) if r == 0 else None)


def even_zero(log_n, d, r, seed=3, name=None):
    return build(name or f"even_zero({r})@{log_n}", log_n, d, {r: ("even_zero",)}, seed)


def phantom(log_n, d, r, c, seed=4, name=None):
    return build(name or f"phantom({r},{c})@{log_n}", log_n, d, {r: ("phantom", c)}, seed,
                 deg0=2 * c + 1 if r == 0 else None)


def chain(log_n, d, events, seed=5, name=None, deg0=None):
    return build(name or f"chain{sorted(events)}@{log_n}", log_n, d, events, seed, deg0=deg0)


def family_cases(log_n, d):
    """Every family that fits d coefficients (a power of two), at the first
    fold (poly_0 is what the caller uploaded), at fold 1 and at the fold that
    leaves degree 3: for a commit of one tail launch and for the oracles'
    cross-check.  d = 1 and 2 have no fold to bend: the constant, the zero
    polynomial and the dense line stand in."""
    if d <= 2:
        return [build(f"dense@{log_n}/{d}", log_n, d, {}, 10),
                build(f"constant@{log_n}/{d}", log_n, d, {}, 11, deg0=0),
                build(f"zero@{log_n}/{d}", log_n, d, {}, 12, deg0=-1)]
    ld = d.bit_length() - 1
    out, seed = [], 100 * log_n + ld
    for r in sorted({0, 1, ld - 2} & set(range(ld - 1))):
        Dr = (d >> r) - 1                       # >= 3, odd
        h = Dr // 2
        tag = f"@{log_n}/{d}"
        for a in sorted({h - 2, h // 2, 0, -1} & set(range(-1, h))):
            seed += 1
            out.append(cancel(log_n, d, r, a, seed, f"cancel({r},{a}){tag}"))
        seed += 4
        out.append(even_zero(log_n, d, r, seed - 3, f"even_zero({r}){tag}"))
        out.append(phantom(log_n, d, r, h, seed - 2, f"phantom({r},{h}){tag}"))
        out.append(beta_zero(log_n, d, r, h // 2, h, seed - 1, f"beta_zero({r},{h // 2},{h}){tag}") if r
                   else build(f"beta_zero(0,{h // 2},{h}){tag}", log_n, d, {0: ("beta_zero", h // 2, h)}, seed - 1))
    # fold 0 alone can start below d - 1: even top above the odd top, and the
    # phantom whose kept degree is 0 (final_degree 0, final value 0)
    tag = f"@{log_n}/{d}"
    b, c = d // 2 - 1, d // 4 - 1 if d >= 8 else 0
    out.append(beta_zero(log_n, d, 0, b, c, seed + 1, f"beta_zero(0,{b},{c}){tag}"))
    out.append(phantom(log_n, d, 0, 0, seed + 2, f"phantom(0,0){tag}"))
    if d >= 16:
        out.append(chain(log_n, d, {0: ("cancel", 5), 1: ("cancel", 0)}, seed + 5, f"chain_small@{log_n}/{d}"))
    if d >= 64:
        # two cancels (d-1, d/2-1, 9, 3, 1, 0), and one of each family in one commit
        out.append(chain(log_n, d, {1: ("cancel", 9), 2: ("cancel", 3)}, seed + 3, f"chain_cancel2@{log_n}/{d}"))
        out.append(chain(log_n, d, {0: ("even_zero",), 1: ("cancel", 7), 2: ("beta_zero", 1, 3), 3: ("phantom", 0)},
                         seed + 4, f"chain_mixed@{log_n}/{d}"))
    return out


# ---- natural inputs: no hook, the channel's own betas ------------------------
def natural_inputs(d, seed=77):
    """{name: d coefficients} whose first fold leaves the dense pattern without
    any forced beta: the m1 < 0 branch, two lone coefficients at the ends, one
    lone top coefficient (every other workgroup reports -1), and x^(d/2) - 1."""
    rng = np.random.default_rng(seed)
    odd_only = np.zeros(d, dtype=np.uint64)
    odd_only[1::2] = rng.integers(1, P, d // 2, dtype=np.uint64)
    ends = np.zeros(d, dtype=np.uint64)
    ends[0] = ends[d - 1] = 1
    mono = np.zeros(d, dtype=np.uint64)
    mono[d - 1] = 1
    half = np.zeros(d, dtype=np.uint64)
    half[0], half[d // 2] = P - 1, 1
    out = {"odd_only": odd_only, "one_plus_top": ends, "monomial": mono, "half_minus_one": half}
    assert top(odd_only[0::2]) == -1 and top(odd_only) == d - 1
    return {k: v.astype(np.uint32) for k, v in out.items()}


# ---- the GPU cases (tests/test_gpu_degree_events.py), built on demand --------
# Layer k has L = log_n - k values (log2); fold k - 1's maxima are reduced by
# layer k's kernels: its G leaf-kernel workgroups take ceil(nlen / G)
# coefficients each (coef_slice), G = 2^L / 2048 for L >= 19 and 2^L / 256 below.
def leaf_grid(L):
    return (1 << L) // (2048 if L >= 19 else 256)


def coef_workgroup(case, r, j):
    """The leaf-kernel workgroup of layer r + 1 that folds coefficient j of poly_{r+1}."""
    nlen = (case.schedule[r] + 2) // 2
    G = leaf_grid(case.log_n - r - 1)
    return j // -(-nlen // G)


def _gpu_specs():
    s = {}

    def add(name, fn, *a, **kw):
        assert name not in s
        s[name] = (fn, a, dict(kw, name=name))

    # 2^23, d = 2^20: layer 1 has L = 22 (quad leaf, k_tree_mid with R = 8,
    # k_tree_mid8 with R = 4, top over 64).  nlen = 2^19 over 2048 workgroups.
    add("23_cancel_first_quarter", cancel, 23, 1 << 20, 0, 70001, 2301)
    add("23_beta_zero_two_mid_groups", beta_zero, 23, 1 << 20, 0, 300007, 131101, 2302)
    # (m1 and m2 can only be told apart where the even part is zero and m0 != m2)
    add("23_phantom(0,c)", phantom, 23, 1 << 20, 0, 250001, 2303)
    # 2^22, d = 2^19: events in layers 1 (L = 21: quad, mid8 with R = 2, top over
    # 512), 3 (L = 19: quad, mid8, top over 128) and 4 (L = 18: wide leaf with 4
    # levels, mid8 with R = 16).  2^19-1, 200003, 100001, 30001, 9001, 4500, ...
    add("22_chain", chain, 22, 1 << 19, {0: ("cancel", 200003), 2: ("cancel", 30001), 3: ("cancel", 9001)}, 2201)
    add("22_cancel(0,0)", cancel, 22, 1 << 19, 0, 0, 2202)
    add("22_cancel(1,-1)", cancel, 22, 1 << 19, 1, -1, 2203)
    add("22_phantom(0,c)", phantom, 22, 1 << 19, 0, 150000, 2204)
    # 2^18, d = 2^15: layer 1 has L = 17 (wide leaf with 8 levels, the top reads
    # all 512 producer triples; 32 coefficients per workgroup), layer 8 has
    # L = 10 (4 workgroups).  15051 >> 6 = 235 is odd, so fold 7 can cancel.
    add("18_top_last_wave", chain, 18, 1 << 15, {0: ("cancel", 15051), 7: ("cancel", 40)}, 1801)
    add("18_top_triple_0", chain, 18, 1 << 15, {0: ("cancel", 19), 2: ("cancel", 1)}, 1802)
    # 2^16 (d = 2^13) and 2^12 (d = 2^9): the tail kernel takes the layers of
    # L <= 9, k >= 7 and k >= 3; events at its first, second and a later layer
    # (folded from LDS), ending in a phantom inside the tail.
    # 8191, 4095, ..., 255, 127 | 21, 9, 4, 2, 1 -> phantom 0 (final degree 0, value 0)
    add("16_tail_chain", chain, 16, 1 << 13, {6: ("cancel", 21), 7: ("cancel", 9), 9: ("beta_zero", 2, 1),
                                             11: ("phantom", 0)}, 1601)
    add("16_tail_phantom", chain, 16, 1 << 13, {6: ("cancel", 27), 7: ("even_zero",), 8: ("phantom", 6)}, 1602)
    # 511, 255, 127 | 41, 15, 7, 3 -> phantom 1, -1
    add("12_tail_chain", chain, 12, 1 << 9, {2: ("cancel", 41), 3: ("cancel", 15), 5: ("even_zero",),
                                            6: ("phantom", 1)}, 1201)
    add("12_tail_cancel_zero", chain, 12, 1 << 9, {2: ("even_zero",), 3: ("cancel", 13), 4: ("cancel", -1)}, 1202)
    return s


GPU_SPECS = _gpu_specs()
TEAM_LOG_N = 22


def _team_specs():
    # 4 ranks at 2^22, d = 2^19: layers 0-2 are sharded, rank r folds
    # coefficients [r * 2^(17 - k), (r + 1) * 2^(17 - k)) of poly_k.
    s = {}
    d = 1 << 19
    s["team_cancel_rank0"] = (cancel, (22, d, 0, 1001, 2211), {"name": "team_cancel_rank0"})
    s["team_beta_zero_two_ranks"] = (chain, (22, d, {1: ("beta_zero", 50001, 131071)}, 2212),
                                     {"name": "team_beta_zero_two_ranks"})
    s["team_cancel(1,0)"] = (cancel, (22, d, 1, 0, 2213), {"name": "team_cancel(1,0)"})
    s["team_cancel(0,-1)"] = (cancel, (22, d, 0, -1, 2214), {"name": "team_cancel(0,-1)"})
    return s


TEAM_SPECS = _team_specs()
_built = {}


def gpu_case(name):
    """A case of GPU_SPECS / TEAM_SPECS by name, built once per process."""
    if name not in _built:
        fn, a, kw = (GPU_SPECS.get(name) or TEAM_SPECS[name])
        _built[name] = fn(*a, **kw)
    return _built[name]


def small_gpu_cases():
    """The one-tail-launch shapes: 2^9, 2^5 and 2^3 at blowup 8, 2^5 at blowup 1."""
    out = []
    for log_n, d in ((9, 64), (5, 4), (3, 1), (5, 32)):
        out += family_cases(log_n, d)
    return out
