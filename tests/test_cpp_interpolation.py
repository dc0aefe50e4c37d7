"""Runs tests/cpp/test_interpolation.cpp: gen_polynomial_from_roots and
gen_lagrange_polynomials (_parallel) of the C++ host mirror
(stark-prover_amd/host/stark101.hpp; interpolation.rs:9-115).  The CPU group
replays the reference's known answers at modulus 7 on the header's
schoolbook; the GPU group drives the frozen field, whose specialisations call
fri_poly_from_roots / fri_lagrange_basis.  Also the constants of the Python
mirror against the header."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stark-prover_amd")
BIN = os.path.join(PKG, "build", "test_interpolation")


def _run(group):
    subprocess.run(["make", "-s", "-C", PKG, "test_interp_host"], check=True, timeout=600)
    p = subprocess.run([BIN, group], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert " 0 failures" in p.stdout
    return p.stdout


def test_cpp_interpolation_cpu():
    out = _run("cpu")
    for name in ("from_roots_known_answer", "empty_input", "lagrange_basis_values", "parallel_equals_serial",
                 "repeated_point_gives_zero_rows"):
        assert f"ok   cpu::{name}" in out


def test_host_library_exports_device_interpolation():
    """The frozen field's gen_polynomial_from_roots / gen_lagrange_polynomials
    are the specialisations compiled into libstark101.so (the device path),
    not the header's schoolbook."""
    subprocess.run(["make", "-s", "-C", PKG, "test_interp_host"], check=True, timeout=600)
    lib = os.path.join(PKG, "lib", "libstark101.so")
    syms = subprocess.run(["nm", "-DC", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ("gen_polynomial_from_roots", "gen_lagrange_polynomials"):
        assert f"stark101::{name}<3221225473ul>(" in syms, name
    und = subprocess.run(["nm", "-DC", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ("fri_poly_from_roots", "fri_lagrange_basis"):
        assert name in und, name


def test_python_constants_match_the_header():
    import fri_amd
    src = open(fri_amd.HEADER_PATH).read()
    for name in ("ROOTS_SMALL_LEAF", "ROOTS_LEAF", "LAGRANGE_MAX"):
        m = re.search(r"#define\s+FRI_%s\s+(\d+)u?\b" % name, src)
        assert m and int(m.group(1)) == getattr(fri_amd, name), name
    leaf = fri_amd.ROOTS_LEAF
    assert leaf & (leaf - 1) == 0 and 128 <= leaf <= 2048
    assert fri_amd.gen_lagrange_polynomials_parallel is fri_amd.gen_lagrange_polynomials


@pytest.mark.gpu
def test_cpp_interpolation_gpu():
    out = _run("gpu")
    for name in ("from_roots_round_trip", "lagrange_round_trip", "lagrange_repeated_point"):
        assert f"ok   gpu::{name}" in out
