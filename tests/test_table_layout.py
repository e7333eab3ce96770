"""The batch-table builder on CPU (prophet_amd/csrc/bpsr_table.cpp, compiled
unchanged with g++): the table every batched, planned, block-queue and keyed
launch reads is built for the smallest buckets that take each branch — full,
partial and element tiles, heads, fp16 tails, trailing bytes, 1 and kMaxSrcs
sources, blocks with empty buckets, forced tile sizes — parsed back and
compared with the layout bpsr_internal.h defines, and every bad bucket is
rejected with nothing written (tests/cpp/table_layout.cpp).  Once plain and
once under AddressSanitizer + UBSan: a stand-alone program, run as a
subprocess."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_table_builder_layout(tmp_path, san):
    exe = tmp_path / "table_layout"
    flags = ["-g", f"-fsanitize={san}", "-fno-sanitize-recover=undefined"] if san else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags,
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "prophet_amd", "csrc"),
                    os.path.join(ROOT, "prophet_amd", "csrc", "bpsr_table.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "table_layout.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fails=0" in r.stdout
