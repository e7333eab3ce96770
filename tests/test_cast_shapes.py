"""The shapes of tests/cast_shapes.py do what the GPU test that uses them
(tests/test_cast_tiles_gpu.py) says they do.  No GPU.

tests/cpp/cast_shapes.cpp — the unchanged bpsr_internal.h and
bpsr_cast_table.cpp under g++, plain and under ASan + UBSan, a stand-alone
program run as a subprocess — prints for every (process, entry, U, wide
element size, scheme) of the GPU test the tile size the table is cut for, the
store policy of every launch, and every segment's records.  Each must be what
the GPU test claims: it cannot see U or the policy, so a later retuning fails
here and the GPU test never silently runs one unit a lane again.

The one-tensor calls are checked as plans of one segment.  Their rule,
cast_rule, lives in a HIP header (bpsr_cast_single.h) that g++ cannot
compile, but it cuts its operand pair with the same cast_cut, starts from the
same Tuning::copy_vpt and halves it in the same loop while the launch has
fewer than kMinTiles tiles, as the table builder's own comment says ("the
single cast's tile-size rule (launch_cast), over the whole launch"); with one
segment the sum over segments is that one term.  Its output bytes
(launch_cast: nelem * 2 for a compress, nelem * element size for a
decompress) are the plan's.

Discriminating power, against numpy alone: the inputs differ at every
position of a tile, so a tile that re-read its j = 0 units would change
bytes."""
import os
import subprocess

import numpy as np
import pytest

import cast_shapes as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_cases():
    return [(env,) + c for env in cs.ENVS for c in cs.cases(env)]


def case_lines(env, entry, u, es, scheme):
    _, copy_vpt, wt_mib, _, _ = cs.ENVS[env]
    segs = cs.segments(u, entry)
    woffs, hoffs, _, _ = cs.layout(segs, es)
    head = f"plan {es} {copy_vpt} {wt_mib} {int(scheme == 'ef')} {len(segs)}"
    return [head] + [f"s {n} {wo} {ho}" for (_, n, _), wo, ho in zip(segs, woffs, hoffs)]


def parse(line):
    word, *fields = line.split()
    return word, {k: int(v) for k, v in (f.split("=") for f in fields)}


@pytest.fixture(scope="module", params=[None, "address,undefined"], ids=["plain", "asan_ubsan"])
def rules(request, tmp_path_factory):
    """case -> (the plan's line, its segments' lines)."""
    san = request.param
    exe = tmp_path_factory.mktemp("cast_shapes") / "cast_shapes"
    flags = ["-g", f"-fsanitize={san}", "-fno-sanitize-recover=undefined"] if san else []
    csrc = os.path.join(ROOT, "prophet_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags,
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(csrc, "bpsr_cast_table.cpp"),
                    os.path.join(csrc, "bpsr_table.cpp"),     # elem_size
                    os.path.join(ROOT, "tests", "cpp", "cast_shapes.cpp"), "-o", str(exe)],
                   check=True)
    cases = all_cases()
    lines = [x for c in cases for x in case_lines(*c)]
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    assert out[-1] == "done", out[-3:]
    got, at = {}, 0
    for c in cases:
        nsegs = len(cs.segments(c[2], c[1]))
        word, plan = parse(out[at])
        assert word == "plan", out[at]
        segs = [parse(x) for x in out[at + 1:at + 1 + nsegs]]
        assert all(w == "seg" for w, _ in segs)
        got[c] = (plan, [s for _, s in segs])
        at += 1 + nsegs
    assert at == len(out) - 1
    return got


def test_the_matrix_is_whole():
    """Every tile size under both policies, the three wide element sizes
    through both entries at each, the two f32-only schemes at U 2 and 4."""
    seen = {(cs.ENVS[env][4], entry, u, es, scheme) for env, entry, u, es, scheme in all_cases()}
    for pol in (cs.POL_WT, cs.POL_NT):
        for u in cs.UNITS:
            for es in cs.WIDE_ES.values():
                for entry in ("single", "plan"):
                    assert (pol, entry, u, es, "plain") in seen
            if u > 1:
                assert (pol, "plan", u, 4, "ef") in seen and (pol, "plan", u, 4, "sr") in seen
    assert len({tuple(sorted(e[0].items())) for e in cs.ENVS.values()}) == len(cs.ENVS) == 4
    assert cs.WT_MAX_MIB == 96 and cs.ENVS["default"][2] == -1


def test_shapes_are_what_they_say():
    assert cs.NEVER == 2 * cs.ELEM_PART + 5 and cs.NSEG == cs.K_MIN_TILES
    assert cs.K_BLOCK < cs.PARTIAL_UNITS < 2 * cs.K_BLOCK and cs.PARTIAL_UNITS % cs.K_BLOCK
    for u in cs.UNITS:
        m = cs.main_segment(u)
        assert m["n"] >= cs.ALL16 + cs.HEAD + cs.TAIL and m["head"] == cs.HEAD and m["tail"] == 5
        assert m["full"] >= 3 and m["n"] < 80_000
        if u > 1:
            assert m["partial"] == cs.PARTIAL_UNITS
            # j = 0: every lane; j = 1: 37 lanes; beyond: none
            live = [max(0, min(cs.K_BLOCK, m["partial"] - j * cs.K_BLOCK)) for j in range(u)]
            assert live[:2] == [cs.K_BLOCK, 37] and not any(live[2:])
            b = cs.main_segment(u, n=cs.big_elems(u))
            assert (b["full"], b["partial"]) == (cs.K_MIN_TILES - 1, cs.PARTIAL_UNITS)
            assert cs.big_elems(u) == cs.single_elems(u) < (4 << 20) * u + 4096
        else:
            assert m["partial"] == 37 and cs.single_elems(1) == m["n"]
    for es in cs.WIDE_ES.values():
        segs = cs.segments(4)
        woffs, hoffs, wsize, hsize = cs.layout(segs, es)
        assert (wsize + hsize) < 2 << 20                   # the whole plan is small
        ball = [i for i, s in enumerate(segs) if s[0] == "ballast"]
        assert len(ball) == cs.NSEG
        for offs, width in ((woffs, es), (hoffs, 2)):
            assert all(offs[i] % 16 == 0 for i in ball)
            assert all(offs[b] - offs[a] == 8 * width + 16 for a, b in zip(ball, ball[1:]))
            ends = [o + s[1] * width for o, s in zip(offs, segs)]
            assert all(b - a >= 16 for a, b in zip(ends, offs[1:]))   # sentinels between
        assert (woffs[0] % 16, hoffs[0] % 16) == cs.offsets(cs.HEAD, es)
        assert (woffs[1] % 16, hoffs[1] % 16) == (0, 2)


def test_every_case_gets_its_tile_size_policy_and_records(rules):
    for (env, entry, u, es, scheme), (plan, segs) in rules.items():
        what = (env, entry, u, es, scheme)
        want_pol = cs.ENVS[env][4]
        assert plan["u"] == u, what
        if scheme == "ef":
            assert plan["pol_ef"] == want_pol, what
        else:
            assert plan["pol_c"] == want_pol, what
        assert plan["pol_d"] == want_pol, what               # the plain decompress, any scheme
        spec = cs.segments(u, entry)
        assert len(segs) == len(spec)
        m = cs.main_segment(u, n=spec[0][1])
        main = segs[0]
        assert main["full"] == m["full"] >= 3 and main["partial"] == 1, what
        assert main["pcount"] == m["partial"], what
        assert (main["head"], main["tail"], main["elem"]) == (cs.HEAD, cs.TAIL, 2), what
        if entry == "single":
            assert u == 1 or main["full"] + 1 == cs.K_MIN_TILES, what
            continue
        never = segs[1]
        assert (never["full"], never["partial"], never["elem"]) == (0, 0, 3), what
        assert (never["head"], never["tail"]) == (cs.ELEM_PART, 5), what
        ball = segs[2:]
        assert len(ball) == (cs.NSEG if u > 1 else 0), what
        for b in ball:
            assert (b["full"], b["partial"], b["pcount"], b["elem"]) == (0, 1, 1, 0), what
        assert plan["records"] == sum(s["full"] + s["partial"] + s["elem"] for s in segs), what


def test_inputs_differ_at_every_position_of_a_tile():
    """A full tile whose j >= 1 units were read from j = 0, the mutant of
    cast_tile_full's 2-byte compress branch and of its decompress re-deal,
    changes bytes: unit j of every lane differs from unit 0 of that lane, in
    every full tile of every source."""
    for u in (2, 4):
        m = cs.main_segment(u)
        srcs = [cs.patterns16(m["n"])] + [cs.wide_source(es, m, m["n"]) for es in (4, 8)]
        for x in srcs:
            bits = x.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[x.itemsize])
            for t in range(m["full"]):
                tile = bits[m["head"] + t * u * cs.TILE1:][:u * cs.TILE1].reshape(u, cs.K_BLOCK, 8)
                for j in range(1, u):
                    assert (tile[j] != tile[0]).any(axis=1).all(), (u, x.itemsize, t, j)


def test_sources_hold_every_kind():
    p = cs.patterns16(cs.ALL16)
    assert len(np.unique(p)) == 65536 and p[0] % 2 == 1
    for es in (4, 8):
        for u in cs.UNITS:
            m = cs.main_segment(u)
            x = cs.wide_source(es, m, m["n"])
            e = x[cs.edge_positions(m)]
            for v in (x, e):
                assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any()
                assert ((v == 0) & np.signbit(v)).any() and ((v == 0) & ~np.signbit(v)).any()
                assert (v == 65520.0).any() and (v == 1 + 2.0 ** -11).any()
                assert ((v != 0) & (np.abs(v) < 2.0 ** -126)).any()       # f32 subnormals
                assert ((np.abs(v) > 2.0 ** -25) & (np.abs(v) < 2.0 ** -14)).any()
            if es == 8:
                assert (e == 1 + 2.0 ** -11 + 2.0 ** -30).any()
            # the positions: the head, lanes 0 and 255 at both j extremes, the tail
            pos = set(cs.edge_positions(m))
            t_last = cs.HEAD + (m["full"] - 1) * u * cs.TILE1
            for want in (0, cs.HEAD - 1, cs.HEAD, cs.HEAD + 7,
                         cs.HEAD + ((u - 1) * cs.K_BLOCK + cs.K_BLOCK - 1) * 8 + 7,
                         t_last + (u - 1) * cs.K_BLOCK * 8,
                         m["partial_at"] + (m["partial"] - 1) * 8, m["n"] - 1):
                assert want in pos, (es, u, want)
