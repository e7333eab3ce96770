"""The segment record lists the cast table builders make for the decompress
statistics, on CPU (CastSegList: build_cast_table / _ef / _sr with a `lists`
argument in prophet_amd/csrc/bpsr_cast_table.cpp, compiled unchanged with
g++): every record appears once, under the segment whose wide range contains
it, ascending within a segment; empty segments own nothing; the CastRec bytes
and the parallel arrays equal those of the builders without lists; an error
writes nothing (tests/cpp/cast_table_stats.cpp).  Once plain and once under
AddressSanitizer + UBSan: a stand-alone program, run as a subprocess."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_cast_table_stats_builder(tmp_path, san):
    exe = tmp_path / "cast_table_stats"
    flags = ["-g", f"-fsanitize={san}", "-fno-sanitize-recover=undefined"] if san else []
    csrc = os.path.join(ROOT, "prophet_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags,
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(csrc, "bpsr_cast_table.cpp"),
                    os.path.join(csrc, "bpsr_table.cpp"),     # elem_size
                    os.path.join(ROOT, "tests", "cpp", "cast_table_stats.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fails=0" in r.stdout
