"""Runs tests/cpp/test_grind.cpp: proof-of-work grinding in the C++ host mirror.
The CPU group checks the host route against the known answers up to 16 bits,
the argument errors, and the verifiers' accept / reject cases on transcripts
with a nonce that this file writes with the Python oracle; it also pins the
libraries' symbols.  The GPU group repeats the known answers on the device and
compares the provers' host and device routes byte for byte."""
import os
import re
import subprocess

import pytest

import fri_amd
import grind_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stark-prover_amd")
BIN = os.path.join(PKG, "build", "test_grind")


def _run(group, *args):
    subprocess.run(["make", "-s", "-C", PKG, "test_grind_host"], check=True, timeout=600)
    p = subprocess.run([BIN, group, *args], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert " 0 failures" in p.stdout
    return p.stdout


def _ground(och, bits):
    ch = fri_amd.Channel(state=och.state)
    nonce = ch.grind(bits)
    och.proof.append(nonce.to_bytes(8, "big"))
    och.state = ch.state
    return len(och.proof) - 1


def _messages(msgs):
    return [str(len(msgs))] + [m.hex() or "-" for m in msgs]


def _transcripts(oracle, golden):
    """Transcripts with an 8-bit nonce by the Python oracle, in the format of
    tests/cpp/test_grind.cpp."""
    lines = []
    for name in ("rand_n7_s42", "channel_prefilled", "blowup1", "offset_3"):
        c = next(x for x in golden["cases"] if x["name"] == name)
        och = oracle.Channel(state=c["channel_in"])
        r = oracle.fri_commit(c["coeffs"], c["log_n"], och, offset=c["offset"])
        pos = _ground(och, 8)
        have = gm.zero_bits(och.state)
        oracle.decommit_fri(3, (1 << c["log_n"]) - 1, r.layers, r.trees, och)
        lines.append("fri %d %d 3 %d %d %s %d %d" % (c["log_n"], len(r.roots), (1 << c["log_n"]) - 1, c["offset"],
                                                   c["channel_in"] or "-", pos, have))
        lines += _messages(och.proof)
    log_t, lb, q = 3, 2, 3
    L, B = log_t + lb, 1 << lb
    och = oracle.Channel()
    pr = oracle.fibsq_prove(3141592, log_t, lb, 0, och)
    pos = _ground(och, 8)
    have = gm.zero_bits(och.state)
    trace = oracle.fibsq_trace(3141592, 1 << log_t)
    f = oracle.interpolate_lagrange_polynomials(oracle.coset_domain(log_t, offset=1), trace, fri_amd.P)
    f_eval = [oracle.poly_evaluate(f, x, fri_amd.P) for x in oracle.coset_domain(L)]
    f_levels = oracle.merkle_levels(f_eval)
    for _ in range(q):                                                # fibsq_prove's query phase (fri_oracle.py)
        idx = och.receive_random_int(0, (1 << L) - 2 * B - 1, True)
        for j in range(3):
            och.send(oracle.fe_to_bytes(f_eval[idx + j * B]))
            och.send(oracle.merkle_proof(f_levels, idx + j * B))
        oracle.decommit_fri_layers(idx, pr.fri.layers, pr.fri.trees, och)
    lines.append("fibsq %d %d %d %d %d %d %d" % (trace[-1], log_t, lb, q, len(pr.fri.roots), pos, have))
    lines += _messages(och.proof)
    return "\n".join(lines) + "\n"


def test_cpp_grind_host_and_symbols(oracle, golden, tmp_path):
    path = tmp_path / "transcripts.txt"
    path.write_text(_transcripts(oracle, golden))
    out = _run("cpu", str(path))
    assert "ok   cpu::host_route_reproduces_the_known_answers" in out
    assert "ok   cpu::argument_errors" in out
    assert "ok   cpu::verifiers_accept_and_reject_a_nonce" in out
    # the C++ table is the model's, up to 16 bits
    src = open(os.path.join(ROOT, "tests", "cpp", "test_grind.cpp")).read()
    for state, bits, first, nonce, after in gm.KATS:
        if bits <= 16:
            assert '"%s"' % after in src and re.search(r"\b%d,\s*(0x%X|%d)(ull)?, (0x%X|%d)(ull)?,"
                                                        % (bits, first, first, nonce, nonce), src), (bits, first)
    lib = os.path.join(PKG, "lib", "libstark101.so")
    und = subprocess.run(["nm", "-DC", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ("fri_grind", "fri_grind_batch"):
        assert re.search(r"\bU %s$" % name, und, re.M), name
    abi = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", "libfri_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    for name in ("fri_grind", "fri_grind_batch", "fri_debug_set_grind_window"):
        assert re.search(r"\bT %s$" % name, abi, re.M), name


@pytest.mark.gpu
def test_cpp_grind_gpu():
    out = _run("gpu")
    assert "ok   gpu::device_route_reproduces_the_known_answers" in out
    assert "ok   gpu::provers_grind_the_same_by_both_routes" in out
    assert "ok   gpu::decommit_fri_grinds_the_same_by_both_routes" in out
