"""Transcripts for the batched verifier's tests (test_gpu_verify_batch.py,
test_verify_batch_host.py, and through verify_mask_corpus.py the mask tests):
honest ones from the Python oracle, cached per process, forgeries built from
oracle parts, and the class of every message of a transcript.  CPU code only,
independent of the device."""
import functools

import fri_oracle as fo

P = fo.P


@functools.lru_cache(maxsize=None)
def fibsq_case(a1, log_t, lb, queries, state="", offset=fo.GEN):
    """(messages, a_last, n_layers) of oracle.fibsq_prove from channel `state`."""
    ch = fo.Channel(state=state)
    pr = fo.fibsq_prove(a1, log_t, lb, queries, ch, offset=offset)
    return tuple(ch.proof), fo.fibsq_trace(a1, 1 << log_t)[-1], len(pr.fri.roots)


@functools.lru_cache(maxsize=None)
def fri_case(seed, coeffs, log_n, queries, max_index, state="", offset=fo.GEN):
    """(messages, n_layers) of oracle.fri_commit + decommit_fri of `coeffs`
    splitmix64 coefficients."""
    ch = fo.Channel(state=state)
    r = fo.fri_commit(fo.splitmix64_field(seed, coeffs), log_n, ch, offset=offset)
    fo.decommit_fri(queries, max_index, r.layers, r.trees, ch)
    return tuple(ch.proof), len(r.roots)


def flip(msgs, i):
    """msgs with message i's middle byte XOR 1."""
    b = bytearray(msgs[i])
    b[len(b) // 2] ^= 1
    return list(msgs[:i]) + [bytes(b)] + list(msgs[i + 1:])


def message_classes(log_n, n_layers, queries, trace_count):
    """The class of every message of a transcript, in order: 'root', 'alpha',
    'beta', 'final', 'index', 'trace_value', 'trace_path', 'value', 'path'."""
    out = []
    if trace_count:
        out += ["root"] + ["alpha"] * 3
    for k in range(n_layers):
        out.append("root")
        if k < n_layers - 1:
            out.append("beta")
    out.append("final")
    for _ in range(queries):
        out.append("index")
        out += ["trace_value", "trace_path"] * trace_count
        for k in range(n_layers):
            if log_n - k == 0:
                out.append("value")
            out += ["value", "path", "value", "path"]
    return out


def _forged_commit(poly, log_n, ch, tweak, final_delta):
    """fri_commit (fri_commit.rs:72-122) with the hooks on what each layer
    commits and on the final value: (layers, trees)."""
    poly = fo.poly_trim(poly)
    deg, domain, layers, trees, k = len(poly) - 1, fo.coset_domain(log_n), [], [], 0
    while True:
        evals = [fo.poly_evaluate(poly, x, P) for x in domain]
        if tweak is not None:
            evals = tweak(k, evals, deg < 1)
        levels = fo.merkle_levels(evals)
        layers.append(evals)
        trees.append(levels)
        ch.send(levels[-1][0].hex().encode())
        if deg < 1:
            break
        beta = ch.receive_random_field_element()
        poly, deg = fo.next_fri_polynomial(poly, deg, beta, P)
        domain = [fo.fe_pow(x, 2, P) for x in domain[: len(domain) // 2]]
        k += 1
    ch.send(fo.fe_to_bytes(((0 if deg == -1 else poly[0]) + final_delta) % P))
    return layers, trees


def forged_fibsq(log_t, lb, queries, a1=99, cp_seed=None, tweak=None, final_delta=0, cp_alphas=None, layer0=None):
    """A FibonacciSq transcript whose channel runs honestly over what the
    prover chose to commit.  cp_seed: commit a low-degree polynomial unrelated
    to the trace instead of the composition.  tweak(k, evals, last) -> evals:
    what is committed as layer k instead of the honest evaluations (the
    polynomial itself folds on honestly).  cp_alphas(alphas) -> alphas: the
    three the composition polynomial is built with instead of the drawn ones.
    layer0(f_evals, alphas, a_last) -> evals: what is committed as layer 0,
    from the trace polynomial's evaluations on the coset and the drawn alphas.
    Returns (messages, a_last, n_layers)."""
    L = log_t + lb
    T, B, n = 1 << log_t, 1 << lb, 1 << L
    trace = fo.fibsq_trace(a1, T)
    f = fo.interpolate_lagrange_polynomials(fo.coset_domain(log_t, offset=1), trace, P)
    fe = [fo.poly_evaluate(f, x, P) for x in fo.coset_domain(L)]
    lv = fo.merkle_levels(fe)
    ch = fo.Channel()
    ch.send(lv[-1][0].hex().encode())
    alphas = [ch.receive_random_field_element() for _ in range(3)]
    poly = fo.splitmix64_field(cp_seed, T + 1) if cp_seed is not None else \
        fo.fibsq_cp_faithful(f, log_t, trace[-1], cp_alphas(alphas) if cp_alphas is not None else alphas)
    if layer0 is not None:
        inner = tweak
        tweak = lambda k, ev, last: layer0(fe, alphas, trace[-1]) if k == 0 else (inner(k, ev, last) if inner else ev)  # noqa: E731
    layers, trees = _forged_commit(poly, L, ch, tweak, final_delta)
    for _ in range(queries):
        idx = ch.receive_random_int(0, n - 2 * B - 1, True)
        for j in range(3):
            ch.send(fo.fe_to_bytes(fe[idx + j * B]))
            ch.send(fo.merkle_proof(lv, idx + j * B))
        fo.decommit_fri_layers(idx, layers, trees, ch)
    return list(ch.proof), trace[-1], len(layers)


def forged_fri(seed, coeffs, log_n, queries, max_index, state="", tweak=None, final_delta=0):
    """fri_case with forged_fibsq's hooks on the committed layers and the
    final value, the channel honest over them: (messages, n_layers)."""
    ch = fo.Channel(state=state)
    layers, trees = _forged_commit(fo.splitmix64_field(seed, coeffs), log_n, ch, tweak, final_delta)
    fo.decommit_fri(queries, max_index, layers, trees, ch)
    return list(ch.proof), len(layers)


def bump_layer(k, high_only=False):
    """A tweak: layer k alone + 1, everywhere or only in its high half (a
    one-element layer is its own high half)."""
    def tweak(kk, ev, last):
        if kk != k:
            return ev
        h = len(ev) // 2 if high_only else 0
        return ev[:h] + [(v + 1) % P for v in ev[h:]]
    return tweak


