"""The shapes and inputs of tests/fold_shapes.py do what the GPU tests that
use them (tests/test_fold_tiles_gpu.py, tests/test_fold_policy_gpu.py) say
they do.  No GPU.

Launch rules: tests/cpp/fold_shapes.cpp — the unchanged bpsr_internal.h and
bpsr_table.cpp under g++, plain and under ASan + UBSan, a stand-alone program
run as a subprocess — prints for every (dtype, sources, shape, offset, tuning)
and every table of the GPU tests the tile size, the cache policy and the tile
geometry; each must be what its test id names, so a later retuning fails here
and no GPU test silently drops back to VPT 1.

Discriminating power: against the oracle alone, the probed tiles hold NaN
results and finite ones in every slot, and a replay that read slot 0 for every
slot, or folded right to left, changes bytes in every probed tile."""
import os
import subprocess

import numpy as np
import pytest

import fold_shapes as fs
import order_probe as op
from prophet_amd.dtypes import ALL_DTYPES, DType, FLOAT_DTYPES, elem_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULT, PLAIN, NT = (1, -1), (0, -1), (1, 0)      # (nt, wt_max_mib; -1: the default 96)
POLICY_OF = {DEFAULT: fs.POL_WT, PLAIN: fs.POL_PLAIN, NT: fs.POL_NT}


def fold_cases():
    """(case, tuning) of every sum_n the GPU tests launch."""
    out = [(c, DEFAULT) for c in fs.SUM_N + fs.IN_PLACE + fs.OFFSET]
    for tuning in (PLAIN, NT):
        out += [((dt, n, "SMALL"), tuning) for dt in ALL_DTYPES for n in fs.POLICY_SMALL_N]
        out += [(c, tuning) for c in fs.POLICY_BIG]
    out += [(c, NT) for c in fs.POLICY_NT_EXTRA]
    # the aliased folds (tests/test_fold_alias_gpu.py): which operands are one
    # buffer does not enter the launch rules
    out += [(c[:3], DEFAULT) for c in fs.ALIAS]
    out += [(c, DEFAULT) for c in fs.SUM3_CASES + fs.DOUBLING]
    return list(dict.fromkeys(out))


SCATTER_WORLD = 3


def scatter_slices():
    """(dtype, elements, byte offset) of every owner's slice of the in-place
    reduce_scatter of test_fold_alias_gpu (fold_shapes.scatter_vectors)."""
    out = []
    for dt in dict.fromkeys(c[0] for c in fs.ALIAS_SCATTER):
        per = fs.n_elems(dt, fs.SHAPES["V4"][0])
        out += [(dt, per, (q * per * elem_size(dt)) % 16) for q in range(SCATTER_WORLD)]
    return out


def table_cases():
    """(kind, dtype, vpt of the table's ballast or forced, tuning)."""
    out = [("batched", dt, vpt, DEFAULT) for dt in fs.BATCH_DTYPES for vpt in (2, 4)]
    out += [("blockq", dt, vpt, DEFAULT) for dt in fs.BLOCKQ_DTYPES for vpt in (2, 4)]
    for tuning in (PLAIN, NT):
        out += [("batched", dt, 2, tuning) for dt in fs.BATCH_DTYPES]
        out += [("blockq", dt, 0, tuning) for dt in fs.POLICY_BLOCKQ_DTYPES]
    return out


def fold_line(case, tuning):
    dt, n, shape = case[:3]
    off = case[3] if len(case) > 3 else 0
    ne = fs.n_elems(dt, fs.SHAPES[shape][0], fs.head_elems(dt, off))
    return f"fold {int(dt)} {ne} {n} {off} {tuning[0]} {tuning[1]}"


def table_lines(kind, dt, vpt, tuning):
    es = elem_size(dt)
    rows = []
    if kind == "batched":
        for i, (ne, n, offs, _) in enumerate(fs.table_spec(dt, vpt)):
            rows.append((ne * es + (3 if i == fs.TRAILING_BUCKET else 0), n, 0,
                         fs.bucket_offsets(offs, n)))
        head = f"table {int(dt)} {tuning[0]} {tuning[1]} 0 0 {len(rows)}"
    else:
        blocks = fs.blockq_blocks()
        for b, blk in enumerate(blocks):
            for ne, n, _ in blk:
                rows.append((ne * es, n, b, fs.bucket_offsets(fs.blockq_offsets(dt, ne, n), n)))
        head = f"table {int(dt)} {tuning[0]} {tuning[1]} {vpt} {len(blocks)} {len(rows)}"
    return [head] + [f"b {L} {n} {b} " + " ".join(map(str, o)) for L, n, b, o in rows]


def parse(line):
    word, *fields = line.split()
    return word, {k: int(v) for k, v in (f.split("=") for f in fields)}


@pytest.fixture(scope="module", params=[None, "address,undefined"], ids=["plain", "asan_ubsan"])
def rules(request, tmp_path_factory):
    """The program's answers: per fold case and per table case."""
    san = request.param
    exe = tmp_path_factory.mktemp("fold_shapes") / "fold_shapes"
    flags = ["-g", f"-fsanitize={san}", "-fno-sanitize-recover=undefined"] if san else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags,
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "prophet_amd", "csrc"),
                    os.path.join(ROOT, "prophet_amd", "csrc", "bpsr_table.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "fold_shapes.cpp"), "-o", str(exe)],
                   check=True)
    folds, tables, slices = fold_cases(), table_cases(), scatter_slices()
    lines = [fold_line(*c) for c in folds]
    for t in tables:
        lines += table_lines(*t)
    lines += [f"fold {int(dt)} {ne} {SCATTER_WORLD} {off} {DEFAULT[0]} {DEFAULT[1]}"
              for dt, ne, off in slices]
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    assert out[-1] == "done" and len(out) == len(folds) + len(tables) + len(slices) + 1, out[-3:]
    got_f = {c: parse(x) for c, x in zip(folds, out)}
    got_t = {c: parse(x) for c, x in zip(tables, out[len(folds):])}
    got_s = {c: parse(x) for c, x in zip(slices, out[len(folds) + len(tables):])}
    assert all(w == "fold" for w, _ in list(got_f.values()) + list(got_s.values()))
    assert all(w == "table" for w, _ in got_t.values()), [x for x in out if "error" in x]
    return tuple({c: v for c, (_, v) in got.items()} for got in (got_f, got_t, got_s))


def test_shapes_are_what_they_say():
    """2,048 tiles, the last one partial, under the half-tile band; the slots
    of the partial tiles are valid where the GPU tests' docstrings say."""
    for name, want_partial in (("V2", 300), ("V4", 700)):
        vecs, vpt = fs.SHAPES[name]
        tile = fs.K_BLOCK * vpt
        assert -(-vecs // tile) == fs.K_MIN_TILES and vecs % tile == want_partial
        assert vecs * 16 < 64 << 20
    valid = lambda part, j: max(0, min(fs.K_BLOCK, part - j * fs.K_BLOCK))      # noqa: E731
    assert [valid(300, j) for j in range(2)] == [256, 44]
    assert [valid(700, j) for j in range(4)] == [256, 256, 188, 0]
    assert fs.SHAPES["SMALL"] == (3 * 256 + 100, 1)
    assert fs.n_elems(DType.FLOAT16, fs.SHAPES["SMALL"][0]) == 3 * 2048 + 803


def test_every_sum_n_case_gets_its_tile_size_kernel_and_policy(rules):
    folds, _, _ = rules
    seen = set()
    for (case, tuning), got in folds.items():
        dt, n, shape = case[:3]
        off = case[3] if len(case) > 3 else 0
        what = (fs.case_id(case), tuning)
        vecs, vpt = fs.SHAPES[shape]
        head = fs.head_elems(dt, off)
        ne = fs.n_elems(dt, vecs, head)
        tile = fs.K_BLOCK * vpt
        assert got["vpt"] == vpt, what
        assert got["pol"] == POLICY_OF[tuning] and got["band"] == 0, what
        assert got["aligned"] == 1 and got["nvec"] == vecs and got["head"] == head, what
        assert (got["full"], got["partial"]) == (vecs // tile, vecs % tile), what
        assert got["partial"] > 0 and got["grid"] == got["full"] + 1, what
        # the module's own geometry is make_geom's, and fp16's tail is scalar tail
        nvec, tail_begin, body = fs.geometry(dt, ne, head)
        assert (nvec, ne - tail_begin) == (got["nvec"], got["tail"]), what
        assert got["tail"] >= fs.ragged_tail(dt), what
        if DType(dt) == DType.FLOAT16:
            assert ne - body == 3 and ne % 8 == 3, what
        seen.add((int(dt), vpt, got["pol"], fs.ns_kernel(n)))
    # the instantiation axes the GPU tests name: every op family at VPT 2 and 4 ...
    for dt in (DType.FLOAT32, DType.FLOAT64, DType.FLOAT16, DType.BFLOAT16, DType.UINT8,
               DType.INT32, DType.INT64):
        for vpt in (2, 4):
            assert any(s[0] == int(dt) and s[1] == vpt for s in seen), (dt, vpt)
    # ... every compile-time source count at both, NS = 16 at VPT 4 included ...
    for vpt in (2, 4):
        for ns in (2, 8, 16, 0):
            if (vpt, ns) != (2, 2):          # two sources are tuned to VPT 4
                assert (int(DType.FLOAT32), vpt, fs.POL_WT, ns) in seen, (vpt, ns)
    # ... and the two other policies at VPT 1 (every dtype, every NS), 2 and 4
    for pol in (fs.POL_PLAIN, fs.POL_NT):
        for dt in ALL_DTYPES:
            for ns in (2, 8, 16, 0):
                assert (int(dt), 1, pol, ns) in seen
        assert (int(DType.FLOAT16), 2, pol, 8) in seen
    assert (int(DType.FLOAT32), 4, fs.POL_NT, 8) in seen


def test_every_table_gets_its_tile_size_policy_and_record_kinds(rules):
    _, tables, _ = rules
    for (kind, dt, vpt, tuning), got in tables.items():
        what = (kind, DType(dt).name, vpt, tuning)
        if vpt:
            assert got["vpt"] == vpt, what
        else:                       # the policy tests' block queue: the fold rule's choice
            assert got["vpt"] == fs.POLICY_BLOCKQ_VPT, what
        assert got["nmax"] == 32 and got["pol"] == POLICY_OF[tuning], what
        # full and partial tiles on the register path (n <= 8) and on the
        # pointer-array path (n > 8), and element tiles
        for k in ("full_reg", "full_mem", "partial_reg", "partial_mem", "elem"):
            assert got[k] > 0, what + (k,)
        if kind == "batched":
            assert got["full_reg"] >= 2047, what


# ------------------------------------------------------ discriminating power ----

FLOATS = pytest.mark.parametrize("dt", FLOAT_DTYPES, ids=lambda d: DType(d).name)
BIG = pytest.mark.parametrize("shape", ["V2", "V4"])
TILES = ("first_tile", "interior_tile", "last_full_tile", "partial_tile")


def nan_vectors(dt, raw):
    """Per 16-byte vector of whole vectors `raw`: does it hold a NaN?"""
    return op.is_nan(dt, raw).reshape(-1, fs.vec_elems(dt)).any(axis=1)


@FLOATS
@BIG
def test_tile_coverage(dt, shape):
    """8 sources: every slot of the probed full tiles holds a vector whose
    result has a NaN (replayed) and one with none (the fast path's result is
    stored), every valid slot of the partial tile a NaN vector; the second
    tile is finite throughout; every probed range holds NaN results."""
    vpt = fs.SHAPES[shape][1]
    es = elem_size(dt)
    ins, kind, want, reg = fs.fold_case(dt, 8, shape)
    for name in TILES[:3]:
        for j in range(vpt):
            lo, hi = fs.slot(dt, reg[name], j)
            nv = nan_vectors(dt, want[lo * es:hi * es])
            assert len(nv) == fs.K_BLOCK and nv.any() and not nv.all(), (name, j)
    part = (reg["partial_tile"][1] - reg["partial_tile"][0]) // fs.vec_elems(dt)
    for j in range(vpt):
        lo, hi = fs.slot(dt, reg["partial_tile"], j)
        assert (hi - lo) // fs.vec_elems(dt) == max(0, min(fs.K_BLOCK, part - j * fs.K_BLOCK))
        if hi > lo:
            assert nan_vectors(dt, want[lo * es:hi * es]).any(), j
    t = reg["first_tile"][1] - reg["first_tile"][0]
    second = want[reg["first_tile"][1] * es:(reg["first_tile"][1] + t) * es]
    assert not op.is_nan(dt, second).any() and not op.is_nan(dt, ins[0]).all()
    nan = op.is_nan(dt, want)
    for name, (lo, hi) in reg.items():
        if name != "scalar_tail":               # fp16's: every NaN there is 0x7fff
            assert nan[lo:hi].any(), name
    assert (kind[nan] >= 0).all()


def _tile_model(dt, ins, want, reg, vpt, replay):
    """The tile at `reg` as a kernel would write it whose fast path is right
    and whose NaN replay is `replay(tile sources, slot, lanes)` -> the bytes of
    those vectors (lanes: a boolean mask over the slot's vectors)."""
    es, v = elem_size(dt), fs.vec_elems(dt)
    lo0 = reg[0]
    tile = [np.ascontiguousarray(x[lo0 * es:reg[1] * es]) for x in ins]
    out = want[lo0 * es:reg[1] * es].copy()
    for j in range(vpt):
        lo, hi = fs.slot(dt, reg, j)
        if hi == lo:
            continue
        bad = nan_vectors(dt, want[lo * es:hi * es])
        sl = out[(lo - lo0) * es:(hi - lo0) * es].reshape(-1, 16)
        sl[bad] = replay(tile, j, bad)
    return out


def _fold_vectors(dt, vecs):
    """The oracle's fold of per-source (k, 16)-byte vector arrays (whole
    vectors: for fp16 whole groups of 8 elements, no scalar tail)."""
    flat = [np.ascontiguousarray(x).reshape(-1) for x in vecs]
    return fs.oracle_fold(dt, flat, len(flat[0])).reshape(-1, 16)


@FLOATS
@BIG
def test_replay_at_slot_0_changes_every_probed_tile(dt, shape):
    """The mutant fold_tile_full_buf / fold_tile_body whose replay of slot j
    re-reads the lane's slot-0 vector: right at VPT 1, and wrong bytes in each
    of the four probed tiles here."""
    vpt = fs.SHAPES[shape][1]
    es = elem_size(dt)
    ins, _, want, reg = fs.fold_case(dt, 8, shape)

    def replay(tile, j, lanes):
        return _fold_vectors(dt, [x.reshape(-1, 16)[:fs.K_BLOCK][:len(lanes)][lanes]
                                  for x in tile])

    for name in TILES:
        model = _tile_model(dt, ins, want, reg[name], vpt, replay)
        assert not np.array_equal(model, want[reg[name][0] * es:reg[name][1] * es]), name
    # the model with the right offset is the oracle: the mutation alone differs
    def right(tile, j, lanes):
        return _fold_vectors(dt, [x.reshape(-1, 16)[j * fs.K_BLOCK:][:len(lanes)][lanes]
                                  for x in tile])
    for name in TILES:
        model = _tile_model(dt, ins, want, reg[name], vpt, right)
        assert np.array_equal(model, want[reg[name][0] * es:reg[name][1] * es]), name


@FLOATS
@BIG
def test_replay_right_to_left_changes_every_probed_tile(dt, shape):
    """The mutant replay that folds the sources right to left."""
    vpt = fs.SHAPES[shape][1]
    es = elem_size(dt)
    ins, _, want, reg = fs.fold_case(dt, 8, shape)

    def replay(tile, j, lanes):
        return _fold_vectors(dt, [x.reshape(-1, 16)[j * fs.K_BLOCK:][:len(lanes)][lanes]
                                  for x in tile[::-1]])

    for name in TILES:
        model = _tile_model(dt, ins, want, reg[name], vpt, replay)
        assert not np.array_equal(model, want[reg[name][0] * es:reg[name][1] * es]), name


@pytest.mark.parametrize("dt", fs.BATCH_DTYPES, ids=lambda d: DType(d).name)
@pytest.mark.parametrize("vpt", [2, 4])
def test_table_buckets_hold_nan_results(dt, vpt):
    """The batched tables: every float bucket of two sources or more holds
    NaN results beside finite ones; integer buckets hold no probes."""
    spec = fs.table_spec(dt, vpt)
    for i, ((ne, n, _, _), (ins, kind, want)) in enumerate(
            zip(spec, fs.table_inputs(dt, spec, vpt, 300))):
        assert len(want) == ne * elem_size(dt) + (3 if i == fs.TRAILING_BUCKET else 0)
        if DType(dt) in FLOAT_DTYPES and n >= 2 and ne:
            nan = op.is_nan(dt, want[:ne * elem_size(dt)])
            assert nan.any() and not nan.all(), i
            assert (kind >= 0).any()
        else:
            assert (kind < 0).all()


# ------------------------------------------------------- aliased operands ----

def test_every_alias_case_gets_its_tile_size_kernel_and_policy(rules):
    """fold_shapes.ALIAS: the tile size its shape names, the write-through
    policy, full tiles and a partial one, and between them every kernel
    (NS 8, 16 and generic with one and with two load groups) with a
    duplicate and with dst at a later source; the owners' slices of the
    in-place reduce_scatter keep 2,047 full tiles of VPT 4 behind the heads
    their byte offsets give, and one of them at least is misaligned."""
    folds, _, slices = rules
    seen = set()
    for case in fs.ALIAS:
        dt, n, shape, alias, same = case
        got = folds[(case[:3], DEFAULT)]
        vecs, vpt = fs.SHAPES[shape]
        assert (got["vpt"], got["pol"], got["aligned"]) == (vpt, fs.POL_WT, 1), fs.alias_id(case)
        assert got["full"] == vecs // (fs.K_BLOCK * vpt) and got["partial"] > 0 and got["tail"] > 0
        assert alias is None or 0 <= alias < n
        assert all(0 <= k < n for g in same for k in g)
        assert alias is None or all(alias not in g for g in same), "dst would alias two sources"
        seen.add((vpt, fs.ns_kernel(n), n > 8, "dup" if same else "later" if alias else "first"))
    for key in ((4, 0, False, "dup"), (2, 8, False, "dup"), (2, 0, True, "dup"),
                (2, 16, True, "dup"), (4, 0, False, "later"), (2, 8, False, "later"),
                (2, 0, True, "later"), (1, 0, True, "later")):
        assert key in seen, key
    assert any(a is not None and a >= 8 for _, _, _, a, _ in fs.ALIAS)     # fold_elements' group 2
    for (dt, ne, off), got in slices.items():
        assert (got["vpt"], got["pol"], got["aligned"]) == (4, fs.POL_WT, 1), (dt, off)
        assert got["full"] == 2047 and got["partial"] > 0 and got["tail"] > 0, (dt, off)
        assert got["head"] == fs.head_elems(dt, off)
    for dt in dict.fromkeys(s[0] for s in slices):
        assert any(off for d, _, off in slices if d == dt), "no misaligned slice"
    # two sources: n <= 4 is tuned to 16 KiB tiles
    for case in fs.SUM3_CASES + fs.DOUBLING:
        assert folds[(case, DEFAULT)]["vpt"] == fs.SHAPES[case[2]][1]


@pytest.mark.parametrize("case", fs.ALIAS_SCATTER + fs.ALIAS_ROOT + fs.ALIAS_LANDED,
                         ids=fs.alias_id)
def test_aliased_source_holds_nans_a_peer_holds_too(case):
    """dst at srcs[k], k > 0: in every probed range the aliased source holds
    NaNs at elements where another source holds one too and the result is a
    NaN, so the exact replay re-reads the source that dst overwrites."""
    dt, n, shape, alias, _ = case
    ins, kind, want, reg = fs.alias_case(case)
    mine = op.is_nan(dt, ins[alias])
    peer = np.zeros_like(mine)
    for k in range(n):
        if k != alias:
            peer |= op.is_nan(dt, ins[k])
    both = mine & peer & op.is_nan(dt, want)
    for name, (lo, hi) in reg.items():
        assert both[lo:hi].any(), name


def test_scatter_vectors_hold_nans_in_every_slice_of_every_rank():
    world = SCATTER_WORLD
    for dt in dict.fromkeys(c[0] for c in fs.ALIAS_SCATTER):
        E, full, kind, offs = fs.scatter_vectors(dt, world, "V4", 77)
        es = elem_size(dt)
        assert E % world == 0 and all(len(v) == E * es for v in full) and any(offs)
        per = E // world
        nan = [op.is_nan(dt, v) for v in full]
        for q in range(world):
            sl = slice(q * per, (q + 1) * per)
            others = np.logical_or.reduce([nan[r][sl] for r in range(world) if r != q])
            assert (nan[q][sl] & others).any(), (dt, q)


@pytest.mark.parametrize("case", fs.ALIAS_DUP, ids=fs.alias_id)
def test_duplicates_share_their_input_and_change_the_fold(case):
    dt, n, shape, _, same = case
    ins, _, want, _ = fs.alias_case(case)
    for g in same:
        assert all(ins[k] is ins[g[0]] for k in g)
    assert len({id(x) for x in ins}) == n - sum(len(g) - 1 for g in same)
    assert not np.array_equal(want, fs.fold_case(dt, n, shape)[2])
