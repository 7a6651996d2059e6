"""The edge vectors of tests/bn254_edges.py through the HOST build of csrc/bn254.h (tests/emu/bn254_host.cpp: h_raw_op, the
twin of the device probe, and h_msm_pipeline): raw, weakly reduced operands in [0, 2p) against bit-exact integer models,
the group law at every zero-difference class, the MSM's digit recoding and reductions on directed scalars.  This proves the
vectors and their expectations on the CPU before tests/test_gpu_bn254_edges.py hands the same ones to the device.  CPU only."""
import ctypes as C

import pytest

import bn254_edges as E
from test_bn254_host import H  # noqa: F401  (the fixture: builds build/libbn254_host.so)


def raw_op(H, name, a, b):
    op, wa, wb, wo = E.OPS[name]
    n = len(a)
    ba = E.pack(a)
    bb = E.pack(b) if wb else None
    assert len(ba) == 8 * wa * n and (bb is None or len(bb) == 8 * wb * n)
    out = C.create_string_buffer(8 * wo * n)
    H.h_raw_op.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    assert H.h_raw_op(op, ba, bb, out, n) == 0
    return E.unpack(out.raw, wo // 4, 32) if wo >= 4 else E.unpack(out.raw, 1, 8)


@pytest.mark.parametrize("idx", range(2 * len(E.FIELD_MODEL)), ids=[n + s for n in E.FIELD_MODEL for s in ("", "-n1")])
def test_field_raw(H, idx):
    name, a, b, want = E.field_vectors()[idx]
    got = raw_op(H, name, a, b)
    E.check_field(name, a, b, want, got)


def test_unknown_op(H):
    assert H.h_raw_op(99, None, None, None, 0) == -1


def test_op_codes_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ronkathon_amd", "csrc", "bn254_probe.h")).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bPROBE_(\w+) = (\d+)", hdr)}
    assert codes == {name: v[0] for name, v in E.OPS.items()}


def test_probe_argument_checks():
    """the device probe refuses an unknown op and a null pointer before it touches the device, and n = 0 is a no-op (no call
    here is a valid one with n > 0: this test runs without a GPU)"""
    from ronkathon_amd import _lib as L
    f = L.lib.ronk_bn254_probe_dev
    buf = (C.c_uint64 * 16)()
    for op in (-1, 10, 15, 21, 99):
        assert f(op, buf, buf, buf, 1, None) == L.ERR_INVALID
        assert f(op, buf, buf, buf, 0, None) == L.ERR_INVALID
    for name, (op, wa, wb, wo) in E.OPS.items():
        assert f(op, None, None, None, 0, None) == L.OK, name
        assert f(op, None, buf, buf, 1, None) == L.ERR_INVALID, name
        assert f(op, buf, buf, None, 1, None) == L.ERR_INVALID, name
        if wb:
            assert f(op, buf, None, buf, 1, None) == L.ERR_INVALID, name


@pytest.mark.parametrize("name", ["xyzz_add", "xyzz_dbl", "xyzz_madd", "xyzz_madd_neg"])
def test_point_raw(H, name):
    cases = E.point_vectors()[name]
    got = raw_op(H, name, [c[1] for c in cases], [c[2] for c in cases] if E.OPS[name][2] else None)
    E.check_points(name, cases, got)
    one = cases[-1:]
    E.check_points(name, one, raw_op(H, name, [one[0][1]], [one[0][2]] if E.OPS[name][2] else None))


def test_on_curve_raw(H):
    v = E.on_curve_vectors()
    got = raw_op(H, "on_curve", [q for q, _ in v], None)
    assert [g[0] for g in got] == [w for _, w in v]


def test_zero_difference_census():
    """every (X class, Y class) of the module docstring is met by a generated P + P operand pair, for add and for madd in
    both signs; the P + (-P) operands meet the three X classes; and the classes are what the NAMED cases claim"""
    found = E.equal_cases()
    for name in ("xyzz_add", "xyzz_madd", "xyzz_madd_neg"):
        for cx in E.CLASSES:
            for cy in E.CLASSES:
                a, b, _ = found[(name, cx, cy)]
                assert E.classes(name, a, b) == (cx, cy)
    census = {}
    for name, cases in E.point_vectors().items():
        if name == "xyzz_dbl":
            continue
        for label, a, b, want in cases:
            if label.startswith("P+P") and want is not None:
                cl = E.classes(name, a, b)
                census[(name,) + cl] = census.get((name,) + cl, 0) + 1
    assert set(census) == {(n, x, y) for n in ("xyzz_add", "xyzz_madd", "xyzz_madd_neg") for x in E.CLASSES for y in E.CLASSES}, census
    opp = {label for label, *_ in E.point_vectors()["xyzz_add"] if label.startswith("P+(-P) class")}
    assert opp == {"P+(-P) class X:%s" % c for c in E.CLASSES}


def test_operands_are_weak_and_cover_the_upper_half():
    """no vector is canonical by accident: the field values, and every coordinate position of the point operands, occur
    both below p and in [p, 2p)"""
    assert any(v >= E.P for v in E.VALUES) and all(v < E.P2 for v in E.VALUES + E.MORE)
    assert all(v < 3 * E.P for v in E.BELOW_3P) and max(E.WIDE) == E.RR - 1
    for name, cases in E.point_vectors().items():
        for side in (1, 2):
            rows = [c[side] for c in cases if c[side] is not None]
            for i in range(len(rows[0]) if rows else 0):
                col = [r[i] for r in rows if len(r) == len(rows[0])]
                assert all(v < E.P2 for v in col)
                assert any(v >= E.P for v in col) and any(0 < v < E.P for v in col), (name, side, i)


MSM = E.msm_cases()


@pytest.mark.parametrize("case", MSM, ids=[cs["name"] for cs in MSM])
def test_msm_pipeline(H, case):
    pw, sw = E.pack_msm(case["mult"], case["scalars"])
    n = len(case["mult"])
    out = C.create_string_buffer(64)
    H.h_msm_pipeline.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    assert H.h_msm_pipeline(pw, sw, n, case["c"], out) == 0
    x, y = E.unpack(out.raw, 2)[0]
    assert (None if x == 0 and y == 0 else (x, y)) == E.expected(case["mult"], case["scalars"])


STAGED = E.fold_cases() + E.stage_cases()


@pytest.mark.parametrize("case", STAGED, ids=[cs["name"] for cs in STAGED])
def test_msm_case_meets_its_stage(case):
    """the census of the pipeline cases: an integer model of the stages (E.stage_events: multiples of G, runs in input
    order) must meet the equal / opposite operands in the stage each case is named for, and must itself sum to the expected
    multiplier"""
    events, total = E.stage_events(case)
    assert total == sum(k * a for k, a in zip(case["scalars"], case["mult"])) % E.R
    assert set(case["meets"]) <= events, (case["name"], sorted(events))


def test_every_adding_stage_is_targeted_both_ways():
    want = {(s, k) for s in ("collect", "heavy", "sliced0", "sliced1", "bitplane", "sum", "tail") for k in ("equal", "opposite")}
    assert want <= {m for cs in E.stage_cases() for m in cs["meets"]}


def test_sort_and_scan_shapes_cross_their_bounds():
    """the large shapes of the device test really sit where they claim: one chunk | one chunk, full | two chunks, and three
    chunks with more than 256 * 4 * 1024 keys x chunks, which doubles the scan's entries per lane"""
    shapes = [E.sort_shape(n, c if c else E.default_window(n)) for n, c in E.SORT_CASES]
    assert [s[0] for s in shapes] == [1, 1, 2, 3]
    assert [s[2] for s in shapes] == [4, 4, 4, 8]
    assert shapes[3][1] > E.SCAN_LANES * E.SCAN_PER * E.SCAN_BLOCKS >= shapes[2][1]
