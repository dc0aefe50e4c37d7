"""Runs tests/cpp/test_verify_batch.cpp: stark101::verify_fri_batch and
verify_fibsq_batch of the C++ host mirror (stark-prover_amd/host/stark101.hpp).
The CPU group pins the empty batch, the size mismatches, the members the packer
decides on the host and the library's symbols; the GPU group verifies 4 members
at (8, 3) with 2 queries from prove_fibsq_batch, rejects a flipped byte,
compares with a loop of verify_fibsq and sends a plain fri_commit_batch through
verify_fri_batch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stark-prover_amd")
BIN = os.path.join(PKG, "build", "test_verify_batch")


def _run(group):
    subprocess.run(["make", "-s", "-C", PKG, "test_verify_batch_host"], check=True, timeout=600)
    p = subprocess.run([BIN, group], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert " 0 failures" in p.stdout
    return p.stdout


def test_cpp_verify_batch_host_and_symbols():
    out = _run("cpu")
    assert "ok   cpu::empty_batch_and_size_mismatch" in out
    assert "ok   cpu::packer_host_rejections" in out
    lib = os.path.join(PKG, "lib", "libstark101.so")
    syms = subprocess.run(["nm", "-DC", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "stark101::verify_fri_batch(" in syms and "stark101::verify_fibsq_batch(" in syms
    und = subprocess.run(["nm", "-DC", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bU fri_verify_batch$", und, re.M)


@pytest.mark.gpu
def test_cpp_verify_batch_gpu():
    out = _run("gpu")
    assert "ok   gpu::batch_equals_a_loop_of_verify_fibsq" in out
    assert "ok   gpu::plain_batch_through_verify_fri_batch" in out
