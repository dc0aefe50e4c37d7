"""Runs tests/cpp/test_verify_pow.cpp: the grinding nonce in
stark101::verify_fri_batch and verify_fibsq_batch of the C++ host mirror
(stark-prover_amd/host/stark101.hpp; fri_verify_batch_pow).  The CPU group pins
the empty batch, grinding_bits above 32, the packer's decisions about the nonce
message and the libraries' symbols; the GPU group verifies 4 members at (3, 2)
with 2 queries from prove_fibsq_batch at 8 bits by both query routes, rejects
them without bits and member 2 after a flipped nonce byte, and compares with a
loop of verify_fibsq."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stark-prover_amd")
BIN = os.path.join(PKG, "build", "test_verify_pow")


def _run(group):
    subprocess.run(["make", "-s", "-C", PKG, "test_verify_pow_host"], check=True, timeout=600)
    p = subprocess.run([BIN, group], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert " 0 failures" in p.stdout
    return p.stdout


def test_cpp_verify_pow_host_and_symbols():
    out = _run("cpu")
    assert "ok   cpu::empty_batch_and_bits_above_32" in out
    assert "ok   cpu::packer_nonce_rejections" in out
    und = subprocess.run(["nm", "-DC", "--undefined-only", os.path.join(PKG, "lib", "libstark101.so")],
                         capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bU fri_verify_batch_pow$", und, re.M)
    assert re.search(r"\bU fri_verify_batch$", und, re.M)          # still the call without grinding bits
    exp = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(PKG, "lib", "libfri_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT fri_verify_batch_pow$", exp, re.M) and re.search(r"\bT fri_verify_batch$", exp, re.M)


@pytest.mark.gpu
def test_cpp_verify_pow_gpu():
    out = _run("gpu")
    assert "ok   gpu::ground_batch_equals_a_loop_of_verify_fibsq" in out
