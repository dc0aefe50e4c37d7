"""Runs tests/cpp/test_prove_batch.cpp: stark101::prove_fibsq_batch and
decommit_fri_batch of the C++ host mirror (stark-prover_amd/host/stark101.hpp).
The CPU group pins the empty batch, the size mismatch and the library's
symbols; the GPU group proves 4 members at (8, 3) with 2 queries in one batch,
compares every channel with prove_fibsq run one by one, verifies each and
rejects a flipped byte, and decommits a plain batch in rounds."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stark-prover_amd")
BIN = os.path.join(PKG, "build", "test_prove_batch")


def _run(group):
    subprocess.run(["make", "-s", "-C", PKG, "test_prove_batch_host"], check=True, timeout=600)
    p = subprocess.run([BIN, group], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert " 0 failures" in p.stdout
    return p.stdout


def test_cpp_prove_batch_host_and_symbols():
    out = _run("cpu")
    assert "ok   cpu::empty_batch_and_size_mismatch" in out
    lib = os.path.join(PKG, "lib", "libstark101.so")
    syms = subprocess.run(["nm", "-DC", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "stark101::prove_fibsq_batch(" in syms and "stark101::decommit_fri_batch(" in syms
    und = subprocess.run(["nm", "-DC", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ("fri_trace_commit_batch", "fri_fibsq_composition_commit_batch", "fri_batch_query_round"):
        assert re.search(r"\bU %s$" % name, und, re.M), name


@pytest.mark.gpu
def test_cpp_prove_batch_gpu():
    out = _run("gpu")
    assert "ok   gpu::members_equal_single_proofs_and_verify" in out
    assert "ok   gpu::decommit_fri_batch_equals_member_by_member" in out
