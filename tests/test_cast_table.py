"""The cast plan's table builder on CPU (prophet_amd/csrc/bpsr_cast_table.cpp,
compiled unchanged with g++): for every wide dtype the segments that take each
branch of the cut — sizes around one unit and one tile, operands 0, 1 and 3
elements past a boundary on either side (co-aligning and never co-aligning),
element-misaligned operands, a long segment that is split into element parts,
lists long enough for tiles of 2 and of 4 — are built into a table and walked
back: every element covered exactly once by the right kind of record, no
record outside its segment, as many records as workgroups.  Every kind of
overlap, a null pointer, a bad dtype and an oversized grid are rejected with
nothing written; empty plans are accepted (tests/cpp/cast_table.cpp).  Once
plain and once under AddressSanitizer + UBSan: a stand-alone program, run as a
subprocess."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_cast_table_builder(tmp_path, san):
    exe = tmp_path / "cast_table"
    flags = ["-g", f"-fsanitize={san}", "-fno-sanitize-recover=undefined"] if san else []
    csrc = os.path.join(ROOT, "prophet_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags,
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(csrc, "bpsr_cast_table.cpp"),
                    os.path.join(csrc, "bpsr_table.cpp"),     # elem_size
                    os.path.join(ROOT, "tests", "cpp", "cast_table.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fails=0" in r.stdout
