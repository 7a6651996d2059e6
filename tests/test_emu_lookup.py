"""The bodies of csrc/lookup_kernels.h compiled for the host (tests/emu/emu_lookup.cpp) against the Python restatement
tests/lookup_ref.py.

Multiplicities: the four launches (clear, build, count, finalise) run lane by lane with the lanes of every launch forward,
reversed and in a seeded shuffled order; the three must give identical words -- every word written is a function of the inputs
alone.  T on both sides of a capacity step (the capacity is the power of two >= 2 T), tables with repeats, F_17 with T = 40 (every
value repeated, counts above p), words >= p.

Quotient: M = 2^4, 2^11 and 2^12 (the first sizes with a second workgroup at 4 and at 8 rows per lane), B = 2 and 8, C = 1, 3
and 16, with and without the multiplicities and T_in (in place when there is one); M = 2 and 4 on the one-row lane.  The
emulator holds every row to its own `unsigned __int128` restatement; here every row is compared at M = 2^4 and the ends, the
lanes' stride boundaries and a seeded sample above.  Test infrastructure only."""
import os
import subprocess

import numpy as np
import pytest

import emu_cxx
import lookup_ref as LR
import plonk_ref as PR
import prime_classes as PC
from test_emu_plonk import words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL, MONT = 0xFFFFFFFF00000001, PC.MONT_P
SRC = os.path.join(ROOT, "tests", "emu", "emu_lookup.cpp")
DEPS = [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in ("lookup_kernels.h", "plonk_kernels.h", "deep_kernels.h", "ext2_kernels.h",
                                                                 "ext2.h", "fri_kernels.h", "field_policy.h", "gl64.h", "mont64.h")]
DEPS.append(os.path.join(ROOT, "tests", "emu", "emu_ref.h"))
FIELDS = [(GL, 7, 7, 3), (GL, 7, 11, 2), (MONT, 10, 10, 1)]       # p, g, w, policies that serve it
ORDERS = (0, 1, 20261)                                            # forward, reverse, the seed of a shuffle


@pytest.fixture(scope="module")
def emu():
    return emu_cxx.build("g++", os.path.join(ROOT, "build", "emu_lookup"), [SRC], DEPS)


def run(exe, args, tmp_path, blob):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    blob.tofile(src)
    out = subprocess.run([exe] + [str(a) for a in args] + [src, dst], capture_output=True, text=True, timeout=600)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("OK"), out.stdout[-800:] + out.stderr[-400:]
    return last, np.fromfile(dst, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ multiplicities
def table_and_lookups(rng, p, T, n, C, repeats, absent):
    """a table of T words (with `repeats`, words >= p that equal earlier entries among them) and C columns of n lookups drawn from
    it, `absent` of them replaced by words the table does not hold"""
    table = words(rng, T, p)
    if repeats and T > 1:
        k = rng.integers(0, T, size=(T + 1) // 2)
        table[k] = table[rng.integers(0, T, size=k.size)]
        j = int(rng.integers(1, T))
        if int(table[0]) % p + p < 2**64:
            table[j] = np.uint64(int(table[0]) % p + p)               # the same value as entry 0, another word
    vals = table[rng.integers(0, T, size=C * n)]
    have = {int(t) % p for t in table}
    for e in rng.choice(C * n, size=absent, replace=False) if absent else ():
        v = int(rng.integers(0, 2**62))
        while v % p in have:
            v += 1
        vals[e] = np.uint64(v)
    return table, vals


def check_mult(emu, tmp_path, p, T, n, C, negate, repeats=True, absent=0, seed=0):
    rng = np.random.default_rng(1000 * T + n + seed)
    table, vals = table_and_lookups(rng, p, T, n, C, repeats, absent)
    want_m, want_missing, want_first = LR.multiplicities(p, table.tolist(), vals.reshape(C, n).tolist(), negate=bool(negate))
    got = [run(emu, ("mult", p, T, n, C, negate, order), tmp_path, np.concatenate([table, vals]))[1] for order in ORDERS]
    for g in got:
        assert g[:T].tolist() == want_m and (int(g[T]), int(g[T + 1])) == (want_missing, want_first), (p, T, n, C)
    assert all(np.array_equal(g, got[0]) for g in got[1:])
    return want_m, want_missing


@pytest.mark.parametrize("T", [1, 2, 255, 256, 257, 2**10, 2**10 + 1])
@pytest.mark.parametrize("p", [GL, MONT, PC.P_32])
def test_multiplicities_in_three_lane_orders(emu, tmp_path, p, T):
    """both sides of a capacity step (T = 256 | 257: 512 | 1024 slots; 2^10 | 2^10 + 1: 2048 | 4096), repeats, words >= p, a few
    words the table lacks"""
    check_mult(emu, tmp_path, p, T, 3 * T + 5, 2, negate=T & 1, absent=min(3, T))
    check_mult(emu, tmp_path, p, T, 300, 1, negate=1 - (T & 1), repeats=False, seed=1)


def test_f17_every_value_repeated_and_counts_above_p(emu, tmp_path):
    for negate in (0, 1):
        m, missing = check_mult(emu, tmp_path, 17, 40, 2000, 2, negate, seed=negate)
        assert missing == 0 and sum(1 for v in m if v) <= 17


def test_a_table_of_one_value_and_lookups_of_one_value(emu, tmp_path):
    p = MONT
    table = np.full(300, 5, dtype=np.uint64)
    vals = np.full(4096, np.uint64(p + 5), dtype=np.uint64)
    for order in ORDERS:
        got = run(emu, ("mult", p, 300, 4096, 1, 0, order), tmp_path, np.concatenate([table, vals]))[1]
        assert got.tolist() == [4096] + [0] * 299 + [0, LR.NONE_MISSING]
    vals[-1] = 6                                                   # the last lane of the last column
    got = run(emu, ("mult", p, 300, 2048, 2, 1, 1), tmp_path, np.concatenate([table, vals]))[1]
    assert got.tolist() == [p - 4095] + [0] * 299 + [1, 4095]


# ------------------------------------------------------------------------------------------------ the quotient
def rows_to_compare(rng, M, B):
    if M <= 256:
        return list(range(M))
    edges = [q * (M // 8) + d for q in range(8) for d in range(-2 * B, 2 * B)]
    return sorted({r % M for r in edges} | {int(r) for r in rng.integers(0, M, size=48)})


def check_quotient(emu, tmp_path, p, g, w, policies, log2_m, log2_b, C, with_mult, with_tin):
    M = 1 << log2_m
    rng = np.random.default_rng(1000 * log2_m + 100 * log2_b + 10 * C + 2 * with_mult + with_tin)
    E = LR.Ext2(p, w)
    dom = PR.Domain(p, g, log2_m - log2_b, log2_b, g)
    vals, mult, S, T_in = (words(rng, k * M, p) for k in (C, C, 2, 2))
    ch = words(rng, 6, p)
    parts = [vals] + ([mult] if with_mult else []) + [S, ch] + ([T_in] if with_tin else [])
    last, got = run(emu, ("quot", p, g, w, log2_m - log2_b, log2_b, g, C, int(with_mult), int(with_tin)), tmp_path, np.concatenate(parts))
    got = got.reshape(-1, 2 * M)
    assert got.shape[0] == policies and ("results=%d" % policies) in last
    v, m, s, t = vals.reshape(C, M), mult.reshape(C, M) if with_mult else None, S.reshape(2, M), T_in.reshape(2, M) if with_tin else None
    for i in rows_to_compare(rng, M, 1 << log2_b):
        want = LR.quotient_row(E, dom, v, m, s, ch[0:2].tolist(), [ch[2:4].tolist(), ch[4:6].tolist()], t, i)
        for r in range(policies):
            assert (int(got[r][i]), int(got[r][M + i])) == want, (p, w, log2_m, log2_b, C, "row %d policy %d" % (i, r))


@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("log2_b", [1, 3])
@pytest.mark.parametrize("log2_m", [4, 11, 12])
@pytest.mark.parametrize("p,g,w,policies", FIELDS)
def test_quotient_bodies_against_lookup_ref(emu, tmp_path, p, g, w, policies, log2_m, log2_b, C):
    check_quotient(emu, tmp_path, p, g, w, policies, log2_m, log2_b, C, True, True)
    check_quotient(emu, tmp_path, p, g, w, policies, log2_m, log2_b, C, False, False)
    if log2_m == 4:
        check_quotient(emu, tmp_path, p, g, w, policies, log2_m, log2_b, C, True, False)
        check_quotient(emu, tmp_path, p, g, w, policies, log2_m, log2_b, C, False, True)


@pytest.mark.parametrize("p,g,w,policies", FIELDS + [(97, 5, 5, 1)])
def test_fewer_rows_than_a_lane_owns(emu, tmp_path, p, g, w, policies):
    """M = 2 (B = 1) and M = 4 (B = 2): one row per lane"""
    for log2_m, log2_b in ((1, 0), (2, 1)):
        check_quotient(emu, tmp_path, p, g, w, policies, log2_m, log2_b, 3, True, True)
        check_quotient(emu, tmp_path, p, g, w, policies, log2_m, log2_b, 2, False, False)


@pytest.mark.parametrize("p,g,w", [(GL, 7, 7), (MONT, 10, 10), (PC.P_MID, PC.GEN[PC.P_MID], PC.GEN[PC.P_MID]), (17, 3, 3)])
def test_own_battery(emu, p, g, w):
    """the emulator's random cases of both families against its own restatement (what `make sanitize` runs under UBSan)"""
    out = subprocess.run([emu, str(p), str(g), str(w)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("OK"), out.stdout[-800:] + out.stderr[-400:]
