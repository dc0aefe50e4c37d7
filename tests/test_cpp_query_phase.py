"""Runs tests/cpp/test_query_phase.cpp: the device route of the batched query
phase in the C++ host mirror (prove_fibsq_batch / decommit_fri_batch with
device_queries = true).  The CPU group pins the empty batch, the size mismatch
and the library's symbols; the GPU group proves 5 members at (6, 3) with 3
queries by the device route and compares every channel, query list and root
with the round route and with prove_fibsq run one by one, then decommits a
plain batch by both routes."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stark-prover_amd")
BIN = os.path.join(PKG, "build", "test_query_phase")


def _run(group):
    subprocess.run(["make", "-s", "-C", PKG, "test_query_phase_host"], check=True, timeout=600)
    p = subprocess.run([BIN, group], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert " 0 failures" in p.stdout
    return p.stdout


def test_cpp_query_phase_host_and_symbols():
    out = _run("cpu")
    assert "ok   cpu::empty_batch_and_size_mismatch" in out
    lib = os.path.join(PKG, "lib", "libstark101.so")
    und = subprocess.run(["nm", "-DC", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ("fri_batch_query_phase", "fri_batch_query_round"):
        assert re.search(r"\bU %s$" % name, und, re.M), name
    abi = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", "libfri_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    for name in ("fri_batch_query_phase", "fri_debug_set_query_chunk"):
        assert re.search(r"\bT %s$" % name, abi, re.M), name


@pytest.mark.gpu
def test_cpp_query_phase_gpu():
    out = _run("gpu")
    assert "ok   gpu::device_route_equals_round_route_and_single_proofs" in out
    assert "ok   gpu::decommit_fri_batch_device_route" in out
