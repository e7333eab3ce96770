"""The stochastic-rounding cast plan's table builder on CPU
(build_cast_table_sr in prophet_amd/csrc/bpsr_cast_table.cpp, compiled
unchanged with g++): the records are the plain builder's byte for byte, every
record's parallel entry is the index in its segment of the record's first
element (64-bit: a segment of 2^34 elements is accepted, one more is EARGS)
and the segment's key, and overlap between any two of the 2 * nsegs ranges, a
null pointer and a non-f32 wide dtype are rejected with nothing written
(tests/cpp/cast_table_sr.cpp).  Once plain and once under AddressSanitizer +
UBSan: a stand-alone program, run as a subprocess."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_cast_table_sr_builder(tmp_path, san):
    exe = tmp_path / "cast_table_sr"
    flags = ["-g", f"-fsanitize={san}", "-fno-sanitize-recover=undefined"] if san else []
    csrc = os.path.join(ROOT, "prophet_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags,
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(csrc, "bpsr_cast_table.cpp"),
                    os.path.join(csrc, "bpsr_table.cpp"),     # elem_size
                    os.path.join(ROOT, "tests", "cpp", "cast_table_sr.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fails=0" in r.stdout
