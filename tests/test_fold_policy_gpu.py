"""The two cache policies of the folds that no other GPU test runs
(bpsr_internal.h cache_pol; the kernels' NT template argument), in reference
mode, bit for bit against the oracle, NaN replay included:

  kPolPlain  plain loads and stores — a third of all fold instantiations —
             through the public knob set_tuning(nt=0) (or BPSR_NT=0);
  kPolNt     non-temporal loads and stores, which every launch takes from
             Tuning::wt_max_bytes per source on (96 MiB); there
             fold_vector_exact<Op, NT> re-reads non-temporally too.  The
             tuning's threshold is read once a process: this file, run as a
             script in one fresh child process with BPSR_WT_MAX_MIB=0, takes
             kPolNt for every launch.

Both run the same list: SMALL (VPT 1: 3 full tiles, a partial one, a tail)
for every dtype with 2, 8, 9 and 16 sources, (8 sources, V2) for fp32 and
fp16, the VPT 2 batched table, one block-queue iteration of each consumer
shape; kPolNt also (8, V4) for fp32.  tests/test_fold_shapes.py checks on the
CPU that these launches get those policies and tile sizes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import fold_shapes as fs  # noqa: E402
from prophet_amd.dtypes import ALL_DTYPES, DType  # noqa: E402
from test_fold_tiles_gpu import check_batched, check_blockq, check_sum_n  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SMALL = [(dt, n, "SMALL") for dt in ALL_DTYPES for n in fs.POLICY_SMALL_N]
# (dtype, consumer shape): dispatch-ordered and persistent
BLOCKQ = list(zip(fs.POLICY_BLOCKQ_DTYPES, (0, 1)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def red(dev):
    from prophet_amd.reducer import GpuReducer
    return GpuReducer(device=0)


@pytest.fixture
def plain(red):
    """Plain loads and stores for the launches of one test."""
    saved = red.get_tuning()
    try:
        red.set_tuning(nt=0)
        assert red.get_tuning()[1] == 0
        yield
    finally:
        red.set_tuning(*saved)
        assert red.get_tuning() == saved


# ----------------------------------------------------------------- kPolPlain ----

@pytest.mark.parametrize("case", SMALL + fs.POLICY_BIG, ids=fs.case_id)
def test_plain_sum_n(red, dev, plain, case):
    check_sum_n(red, dev, case)


@pytest.mark.parametrize("dt", fs.BATCH_DTYPES, ids=lambda d: DType(d).name)
def test_plain_batched_table_vpt2(red, dev, plain, dt):
    check_batched(red, dev, dt, 2, plan=False)


@pytest.mark.parametrize("dt,shape", BLOCKQ, ids=["FLOAT32-dispatch", "FLOAT16-persistent"])
def test_plain_blockq_one_iteration(red, dev, plain, dt, shape):
    check_blockq(red, dev, dt, shape, fs.POLICY_BLOCKQ_VPT, 1)


# -------------------------------------------------------------------- kPolNt ----

GROUPS = ["sum_n small", "sum_n big tiles", "batched table", "block queue"]


@pytest.mark.timeout(240)
def test_nt_policy_in_a_child_process():
    """One child with BPSR_WT_MAX_MIB=0 (no other environment touched): every
    group of the list prints its line."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)],
                       env=dict(os.environ, BPSR_WT_MAX_MIB="0"), cwd=ROOT,
                       capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for g in GROUPS:
        assert f"nt group passed: {g}" in r.stdout, r.stdout[-2000:]


if __name__ == "__main__":
    assert os.environ.get("BPSR_WT_MAX_MIB") == "0"
    from prophet_amd.reducer import GpuReducer
    assert torch.cuda.is_available()
    _dev, _red = torch.device("cuda:0"), GpuReducer(device=0)
    assert _red.get_tuning()[1] == 1
    for _case in SMALL:
        check_sum_n(_red, _dev, _case)
    print(f"nt group passed: {GROUPS[0]}", flush=True)
    for _case in fs.POLICY_BIG + fs.POLICY_NT_EXTRA:
        check_sum_n(_red, _dev, _case)
    print(f"nt group passed: {GROUPS[1]}", flush=True)
    for _dt in fs.BATCH_DTYPES:
        check_batched(_red, _dev, _dt, 2, plan=False)
    print(f"nt group passed: {GROUPS[2]}", flush=True)
    for _dt, _shape in BLOCKQ:
        check_blockq(_red, _dev, _dt, _shape, fs.POLICY_BLOCKQ_VPT, 1)
    print(f"nt group passed: {GROUPS[3]}", flush=True)
