"""The single casts' operand check on CPU (cast_check in
prophet_amd/csrc/bpsr_cast_table.cpp, compiled unchanged with g++): for every
scheme (plain, error feedback, stochastic rounding) and both wire formats,
every accepted and rejected (wide, wire) pair, nelem == 0 with null pointers,
each null operand, an element count that overflows the byte count, each
operand wrapping the address space, every pair of operands overlapping by one
byte (rejected) and exactly adjacent (accepted), and stochastic rounding's
2^34 elements (accepted) and one more (rejected) — each with its status and
message text (tests/cpp/cast_check.cpp).  Once plain and once under
AddressSanitizer + UBSan: a stand-alone program, run as a subprocess."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_cast_check(tmp_path, san):
    exe = tmp_path / "cast_check"
    flags = ["-g", f"-fsanitize={san}", "-fno-sanitize-recover=undefined"] if san else []
    csrc = os.path.join(ROOT, "prophet_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags,
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(csrc, "bpsr_cast_table.cpp"),
                    os.path.join(csrc, "bpsr_table.cpp"),     # elem_size
                    os.path.join(ROOT, "tests", "cpp", "cast_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fails=0" in r.stdout
