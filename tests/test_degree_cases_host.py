"""CPU: the degree-event cases of tests/degree_cases.py against both oracles.

tests/test_gpu_degree_events.py compares the library with orc_fri_commit_fast
and with degree_schedule on inputs no random test produces (cancelled folds,
zero betas, zero even parts, the reference's phantom degree).  Here those two
references are pinned on exactly those inputs, without a GPU: degree_schedule
against the Python twin's next_fri_polynomial (the reference's degree field,
quirks included), the twin's faithful Horner commit against the C oracle, and
every GPU case's event assertion."""
import numpy as np
import pytest

import degree_cases as dc
import stored_proof as sp


def _twin_schedule(oracle, coeffs, betas):
    poly = oracle.poly_trim([int(x) for x in coeffs])
    deg = len(poly) - 1
    sched, r = [deg], 0
    while deg >= 1:
        poly, deg = oracle.next_fri_polynomial(poly, deg, betas[r], oracle.P)
        sched.append(deg)
        r += 1
    return sched


def test_helper_constants(oracle):
    import fri_amd
    assert dc.P == oracle.P and dc.N_BETAS == fri_amd.MAX_ROUNDS


def test_unfold_inverts_fold():
    rng = np.random.default_rng(5)
    for nq, no, beta in ((7, 7, 12345), (3, 9, dc.P - 1), (9, 3, 1), (5, 5, 0), (0, 4, 77), (4, 0, 77)):
        q = rng.integers(0, dc.P, nq, dtype=np.uint64)
        odd = rng.integers(0, dc.P, no, dtype=np.uint64)
        c = dc.unfold(q, beta, odd)
        assert int(c.max(initial=0)) < dc.P
        assert np.array_equal(dc.fold(c, beta)[:nq], q) and dc.top(dc.fold(c, beta)) == dc.top(q)
        assert np.array_equal(c[1::2][:no], odd)


@pytest.mark.parametrize("ld", [5, 6, 7, 8, 9])
def test_degree_schedule_matches_twin(oracle, ld):
    """degree_schedule == the schedule of next_fri_polynomial, every family at d = 2^ld."""
    cases = dc.family_cases(ld + 3, 1 << ld)
    kinds = {ev[0] for c in cases for ev in c.events.values()}
    assert kinds == {"cancel", "beta_zero", "even_zero", "phantom"}
    for c in cases:
        assert _twin_schedule(oracle, c.coeffs, c.betas) == c.schedule == dc.degree_schedule(c.coeffs, c.betas), c.name


def test_degree_schedule_dense_and_natural(oracle):
    """Without events the schedule halves; the natural inputs under arbitrary betas match the twin too."""
    betas = dc.make_betas(9)
    c = oracle.splitmix64_np(3, 100)
    assert dc.degree_schedule(c, betas) == _twin_schedule(oracle, c, betas) == [99, 49, 24, 12, 6, 3, 1, 0]
    for name, c in dc.natural_inputs(64).items():
        assert dc.degree_schedule(c, betas) == _twin_schedule(oracle, c, betas), name
    assert dc.degree_schedule(dc.natural_inputs(64)["monomial"], betas) == [63, 31, 15, 7, 3, 1, 0]


SMALL = [(9, 64), (5, 4), (3, 1), (5, 32), (8, 32), (6, 8), (7, 128)]


@pytest.mark.parametrize("log_n,d", SMALL)
def test_twin_and_c_oracle_agree_on_every_family(oracle, corc, log_n, d):
    """The twin's faithful commit (Horner on every domain point, the
    reference's own polynomial arithmetic) and orc_fri_commit_fast (NTT,
    evaluation-form folds) under the same forced betas: roots, betas, final
    value, final degree, state and layer count, which is len(schedule)."""
    for c in dc.family_cases(log_n, d):
        ch = oracle.Channel()
        tw = oracle.fri_commit([int(x) for x in c.coeffs], log_n, ch, forced_betas=c.betas, keep=False)
        full = sp.oracle_commit_full(corc, oracle, c.coeffs, log_n, forced_betas=c.betas)
        assert (tw.roots, tw.betas, tw.final_value, tw.final_degree, ch.state) == sp.transcript_want(full), c.name
        assert full.n_layers == len(tw.roots) == len(c.schedule), c.name
        assert full.final_degree == c.schedule[-1], c.name
        assert full.betas == c.betas[:len(c.schedule) - 1], c.name
        assert full.final_value == (0 if c.schedule[-1] < 0 else int(dc.fold_chain(c)[0])), c.name


def test_small_gpu_cases_are_the_pinned_ones():
    """The one-tail-launch GPU shapes are a subset of SMALL above."""
    names = [c.name for c in dc.small_gpu_cases()]
    assert len(set(names)) == len(names)
    pinned = {c.name for log_n, d in SMALL for c in dc.family_cases(log_n, d)}
    assert set(names) <= pinned


@pytest.mark.parametrize("name", list(dc.GPU_SPECS) + list(dc.TEAM_SPECS))
def test_gpu_case_events(name):
    """Every large GPU case, built once: build() asserts the planned schedule
    and each fold's (m0, m1, m2); here, where the event lies in the grid."""
    c = dc.gpu_case(name)
    assert c.coeffs.dtype == np.uint32 and c.coeffs.size == c.d and len(c.betas) == dc.N_BETAS
    assert c.events
    dc.check_events(c)


def test_gpu_case_placement():
    """The positions the GPU shapes were chosen for (launch_layer's schedule)."""
    wg = dc.coef_workgroup
    c = dc.gpu_case("23_cancel_first_quarter")          # layer 1: 2048 workgroups, mid<1024> R = 8
    assert dc.leaf_grid(22) == 2048 and wg(c, 0, c.schedule[1]) < 512 and wg(c, 0, (c.schedule[0] - 1) // 2) == 2047
    c = dc.gpu_case("23_beta_zero_two_mid_groups")
    b, cc = c.events[0][1:]
    assert wg(c, 0, b) // 8 != wg(c, 0, cc) // 8
    c = dc.gpu_case("23_phantom(0,c)")                  # m2 alone, in the last of the mid groups with work
    assert c.schedule == [500003, 250001, -1] and wg(c, 0, 250001) // 8 > 200
    c = dc.gpu_case("22_chain")                         # events in layers 1, 3, 4
    assert sorted(c.events) == [0, 2, 3]
    assert [c.log_n - r - 1 for r in sorted(c.events)] == [21, 19, 18]
    for r in c.events:
        assert wg(c, r, c.schedule[r + 1]) < wg(c, r, c.schedule[r] // 2) < dc.leaf_grid(c.log_n - r - 1)
    for name in ("22_cancel(0,0)", "22_cancel(1,-1)", "22_phantom(0,c)"):
        c = dc.gpu_case(name)                           # rounds_bound plans 20 layers for d = 2^19
        assert 20 - len(c.schedule) >= 17, name
    c = dc.gpu_case("18_top_last_wave")                 # layer 1: 512 triples; layer 8: 4
    assert dc.leaf_grid(17) == 512 and wg(c, 0, c.schedule[1]) >= 448
    assert c.log_n - 8 == 10 and dc.leaf_grid(10) == 4 and 0 < wg(c, 7, c.schedule[8]) < wg(c, 7, c.schedule[7] // 2) == 3
    c = dc.gpu_case("18_top_triple_0")
    assert wg(c, 0, c.schedule[1]) == 0
    for name, first_tail in (("16_tail_chain", 7), ("16_tail_phantom", 7), ("12_tail_chain", 3),
                             ("12_tail_cancel_zero", 3)):
        c = dc.gpu_case(name)                           # the tail takes the layers of <= 2^9 values
        assert c.log_n - first_tail == 9
        layers = sorted(r + 1 for r in c.events)
        assert layers[0] == first_tail and layers[1] == first_tail + 1 and layers[-1] >= first_tail + 2, name
    # team: rank of coefficient j of poly_k at a sharded layer k is j >> (17 - k)
    c = dc.gpu_case("team_cancel_rank0")
    assert c.schedule[1] >> 16 == 0 and ((c.schedule[0] - 1) // 2) >> 16 == 3
    c = dc.gpu_case("team_beta_zero_two_ranks")
    b, cc = c.events[1][1:]
    assert (b >> 15, cc >> 15) == (1, 3)
    assert dc.gpu_case("team_cancel(1,0)").schedule == [(1 << 19) - 1, (1 << 18) - 1, 0]
    assert dc.gpu_case("team_cancel(0,-1)").schedule == [(1 << 19) - 1, -1]
