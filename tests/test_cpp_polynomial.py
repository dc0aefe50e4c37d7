"""Runs tests/cpp/test_polynomial.cpp: Polynomial<M> arithmetic of the C++
host mirror (stark-prover_amd/host/stark101.hpp; ops.rs:87-342).  The CPU
group replays the reference's known answers at moduli 7, 17 and 23 on the
host's schoolbook algorithms; the GPU group drives Poly (the frozen field),
whose mul_assign / div_rem / compose always run on the device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stark-prover_amd")
BIN = os.path.join(PKG, "build", "test_polynomial")


def _run(group):
    subprocess.run(["make", "-s", "-C", PKG, "test_poly_host"], check=True, timeout=600)
    p = subprocess.run([BIN, group], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert " 0 failures" in p.stdout
    return p.stdout


def test_cpp_polynomial_cpu():
    out = _run("cpu")
    for name in ("test_poly_multiplication", "test_poly_div_rem_with_remainder", "test_poly_div_by_zero_polynomial",
                 "test_compose_edge_cases", "test_readme_examples_mod_17_and_23", "test_operator_forms",
                 "test_stale_degree_is_zero"):
        assert f"ok   cpu::{name}" in out


def test_host_library_exports_device_polynomial_arithmetic():
    """Poly's mul_assign / div_rem / compose are the specialisations compiled
    into libstark101.so (the device path), not the header's schoolbook."""
    subprocess.run(["make", "-s", "-C", PKG, "test_poly_host"], check=True, timeout=600)
    syms = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(PKG, "lib", "libstark101.so")],
                          capture_output=True, text=True, check=True).stdout
    for name in ("mul_assign", "div_rem", "compose"):
        assert f"stark101::Polynomial<3221225473ul>::{name}(" in syms, name
    und = subprocess.run(["nm", "-DC", "--undefined-only", os.path.join(PKG, "lib", "libstark101.so")],
                         capture_output=True, text=True, check=True).stdout
    for name in ("fri_poly_mul", "fri_poly_div_rem", "fri_poly_compose"):
        assert name in und, name


def test_python_constants_match_the_header():
    import re

    import fri_amd
    src = open(fri_amd.HEADER_PATH).read()
    for name in ("POLY_FORCE_NTT", "POLY_FORCE_DIRECT", "POLY_DIRECT_LIMIT", "POLY_DIRECT_MAX"):
        m = re.search(r"#define\s+FRI_%s\s+(\d+)u?\b" % name, src)
        assert m and int(m.group(1)) == getattr(fri_amd, name), name
    assert fri_amd.POLY_DIRECT_MAX & (fri_amd.POLY_DIRECT_MAX - 1) == 0
    assert fri_amd.POLY_DIRECT_MAX <= fri_amd.POLY_DIRECT_LIMIT


def test_python_host_polynomial_ops(oracle):
    """poly_add / poly_sub / poly_scalar_mul (host, O(n)) against the oracle."""
    import numpy as np

    import fri_amd
    P = fri_amd.P
    a, b = oracle.splitmix64_field(1, 37), oracle.splitmix64_field(2, 12)
    assert [int(v) for v in fri_amd.poly_add(a, b)] == oracle.poly_add(a, b, P)
    assert [int(v) for v in fri_amd.poly_sub(b, a)] == oracle.poly_sub(b, a, P)
    assert [int(v) for v in fri_amd.poly_scalar_mul(a, 12345)] == oracle.poly_scalar_mul(a, 12345, P)
    assert fri_amd.poly_sub(a, a).size == 0 and fri_amd.poly_add(a, []).size == 37
    assert fri_amd.poly_add([1, 2, 3], [5, P - 2, P - 3]).tolist() == [6]          # trims
    z = fri_amd.poly_scalar_mul(a, 0)                                              # not re-trimmed (ops.rs:194-198)
    assert z.size == 37 and not z.any() and z.dtype == np.uint32
    with pytest.raises(fri_amd.FriError):
        fri_amd.poly_scalar_mul(a, P)


@pytest.mark.gpu
def test_cpp_polynomial_gpu():
    out = _run("gpu")
    for name in ("poly_mul_identity", "poly_div_rem_identity", "poly_mul_then_div_rem_round_trip",
                 "poly_compose_identity"):
        assert f"ok   gpu::{name}" in out
