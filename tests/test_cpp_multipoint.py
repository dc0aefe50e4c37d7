"""Runs tests/cpp/test_multipoint.cpp: arbitrary-point interpolate() and
evaluate_points() of the C++ host mirror (stark-prover_amd/host/stark101.hpp;
ops.rs:76-83, 239-241 -> interpolation.rs:121-152) on the device's product
tree.  The CPU group pins the constants and exports of fri_evaluate_ex /
fri_interpolate_points_ex in the header, the Python mirror and the two
libraries; the GPU group drives the frozen field."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stark-prover_amd")
BIN = os.path.join(PKG, "build", "test_multipoint")


def _run(group):
    subprocess.run(["make", "-s", "-C", PKG, "test_multipoint_host"], check=True, timeout=600)
    p = subprocess.run([BIN, group], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert " 0 failures" in p.stdout
    return p.stdout


def test_python_constants_match_the_header():
    import fri_amd
    src = open(fri_amd.HEADER_PATH).read()
    for name in ("MP_FORCE_TREE", "MP_FORCE_DIRECT", "MP_SMALL_LEAF", "MP_EVAL_MIN", "MP_INTERP_MIN"):
        m = re.search(r"#define\s+FRI_%s\s+(\d+)u?\b" % name, src)
        assert m and int(m.group(1)) == getattr(fri_amd, name), name
    for v in (fri_amd.MP_EVAL_MIN, fri_amd.MP_INTERP_MIN):
        assert v > 0 and v & (v - 1) == 0
    assert fri_amd.MP_INTERP_MIN <= 1 << 17          # the direct kernels stop there
    out = _run("cpu")
    assert "ok   cpu::crossovers_are_powers_of_two" in out
    assert "constants %d %d" % (fri_amd.MP_EVAL_MIN, fri_amd.MP_INTERP_MIN) in out


def test_header_declares_and_library_exports_the_ex_calls():
    import fri_amd
    src = open(fri_amd.HEADER_PATH).read()
    lib = os.path.join(PKG, "lib", "libfri_amd.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ("fri_evaluate_ex", "fri_interpolate_points_ex", "fri_evaluate", "fri_interpolate_points"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    ctypes_lib = fri_amd.load_library()
    assert ctypes_lib.fri_evaluate_ex.argtypes is not None and ctypes_lib.fri_interpolate_points_ex.argtypes is not None


def test_host_library_calls_device_evaluation():
    subprocess.run(["make", "-s", "-C", PKG, "test_multipoint_host"], check=True, timeout=600)
    lib = os.path.join(PKG, "lib", "libstark101.so")
    syms = subprocess.run(["nm", "-DC", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "stark101::evaluate_points(" in syms
    und = subprocess.run(["nm", "-DC", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ("fri_evaluate", "fri_interpolate_points"):
        assert re.search(r"\bU %s$" % name, und, re.M), name


@pytest.mark.gpu
def test_cpp_multipoint_gpu():
    out = _run("gpu")
    for name in ("interpolate_shuffled_coset_beyond_the_direct_limit", "evaluate_points_equals_host_horner",
                 "evaluate_points_on_the_tree", "interpolate_repeated_point_gives_zero_terms"):
        assert f"ok   gpu::{name}" in out
