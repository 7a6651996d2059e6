"""The Goldilocks tile kernels ON THE GPU on the directed inputs of tests/gl_branch_inputs.py.  Needs a real MI355X (-m gpu).

tests/test_emu_gl_branches.py shows on the host emulator that these arrays -- small signed integers placed at one cut of the
transform each -- make gl64::add, add_lazy and mad_eps_canon take their ">= p without a carry" outcome in every pass and phase
that calls them, and that random residues never do.  The DEVICE forms of mad_eps_canon and sub32 (hand-written carry-out blocks
no host build compiles) and the compiler's scheduling around them exist only here, so the same arrays go through every C-ABI
route that reaches a tile body: bit-exact against the oracle, every word canonical, and for `pre` equal to the small signed array
it was built from (a kernel that stores p where the oracle has 0 fails all three)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gl_branch_inputs as GB

pytestmark = pytest.mark.gpu

GP, GG = GB.P, GB.G
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# above 2^20 an array and its oracle transform cost a second or more: small / pre / colpre and these cuts (the butterfly outputs of
# the later rounds, before their twiddles; the state entering the second pass) -- on the emulator they reach every phase
BIG_CUTS = ((0, 1, True), (1, 0, False), (1, 0, True), (1, 1, True))


@pytest.fixture(scope="module")
def L():
    import ronkathon_amd as R
    assert R.device_count() >= 1
    from ronkathon_amd import _lib
    return _lib


@functools.lru_cache(maxsize=4)
def directed(k, batch, inverse, logrs, cuts=None):
    """[(name, x, want, s)] flat [batch * n] arrays: the families of one transform with the oracle's result, computed once and
    shared by every route that runs this shape"""
    n = 1 << k
    out = []
    for name, x, s in GB.families(n, batch, inverse, logrs, cuts):
        want = GB.fft(x, inverse)
        if s is not None:
            assert np.array_equal(want, s)
        for a in (x, want):
            a.setflags(write=False)
        out.append((name, x.reshape(-1), want.reshape(-1), None if s is None else s.reshape(-1)))
    return out


def check(got, want, s, what):
    assert np.array_equal(got, want), what + (int(np.flatnonzero(got != want)[0]),)
    assert bool((got < np.uint64(GP)).all()), what
    if s is not None:
        assert np.array_equal(got, s), what


def plan_from_opts(L, k, batch, **fields):
    """a Plan over ronk_plan_create_opts with ronk_plan_opts fields the Python wrapper's constructor does not take"""
    import ctypes as C
    opts = L.PlanOpts()
    for name, value in fields.items():
        setattr(opts, name, value)
    h = C.c_void_p()
    L.check(L.lib.ronk_plan_create_opts(C.byref(h), GP, GG, k, batch, -1, C.byref(opts)))
    plan = L.Plan.__new__(L.Plan)
    plan.h, plan.p, plan.g, plan.log2n, plan.n, plan.batch = h, GP, GG, k, 1 << k, batch
    return plan


def run_plan(L, k, batch, logrs, cuts=None, raw_opts=None, **opts):
    plan = plan_from_opts(L, k, batch, **raw_opts) if raw_opts else L.Plan(GP, GG, k, batch, **opts)
    try:
        assert plan.path() == 1 and plan.num_passes() == len(logrs)
        for inverse in (False, True):
            for name, x, want, s in directed(k, batch, inverse, tuple(logrs), cuts):
                got = plan.inverse(x) if inverse else plan.forward(x)
                check(got, want, s, (k, batch, inverse, name, tuple(sorted(opts.items()))))
    finally:
        plan.close()


# shape -> the body the selection rule picks for it (tests/test_emu_gl_branches.py lists and asserts them on the emulator)
@pytest.mark.parametrize("k,batch,logrs,opts", [
    (4, 3, (4,), {}),                                           # staged I/O
    (10, 64, (10,), {}),                                        # whole-polynomial pass
    (13, 1, (7, 6), {"tile_log2_columns": 4}),                  # general + generic
    (13, 2, (7, 6), {}),
    (16, 2, (8, 8), {"tile_log2_columns": 4, "twiddle_matrix_log2_max": 18}),   # column/matrix + row
    (16, 2, (8, 8), {"tile_log2_columns": 0}),
    (16, 2, (8, 8), {"tile_log2_columns": 2}),
    (16, 1, (8, 8), {}),                                        # the planner's latency form (ntt_small.h)
], ids=lambda v: str(v).replace(" ", ""))
def test_directed_inputs_small_plans(L, k, batch, logrs, opts):
    """every family and every cut, forward and inverse"""
    run_plan(L, k, batch, logrs, **opts)


def test_directed_inputs_three_pass_plan(L):
    """2^14 as three passes of 2^5, 2^5 and 2^4 rows (ronk_plan_opts::three_pass_from_log2 = 13): the generic body with the middle
    pass's own twiddle"""
    run_plan(L, 14, 1, (5, 5, 4), raw_opts={"tile_log2_columns": 2, "three_pass_from_log2": 13})


@pytest.mark.parametrize("tlc", [-1, 0, 2, 4])
def test_directed_inputs_2_20(L, tlc):
    """column/two-level + row (16-column tiles), the wave-local bodies (4 columns), the planner's own tiles"""
    run_plan(L, 20, 1, (10, 10), tile_log2_columns=tlc)


def test_directed_inputs_2_20_two_lanes_in_flight(L):
    """ronk_ntt_forward_many_dev / _inverse_many_dev: the families as unrelated device arrays on a plan with two lanes"""
    from test_gpu_parity import _DevArr
    k, n = 20, 1 << 20
    plan = L.Plan(GP, GG, k, 1, in_flight=2)
    assert plan.in_flight() == 2
    for inverse in (False, True):
        fams = directed(k, 1, inverse, (10, 10))
        din = [_DevArr(x) for _, x, _, _ in fams]
        dout = [_DevArr(n=n) for _ in fams]
        plan.forward_many_dev([d.ptr for d in din], [d.ptr for d in dout], inverse=inverse)
        for (name, _, want, s), d in zip(fams, dout):
            check(d.get(), want, s, ("many_dev", inverse, name))
        for d in din + dout:
            d.free()
    plan.close()


def test_directed_inputs_2_22_default_plan(L):
    """the headline size once, the default plan, forward and inverse"""
    run_plan(L, 22, 1, (11, 11), ((0, 1, True), (1, 1, True)))


def test_directed_inputs_fused_multiply(L):
    """ronk_poly_mul at the smallest NTT size whose middle is fused (2^21 = 2^11 x 2^10, csrc/ntt_mul.h).  The operands are zero
    padded on load, so a directed operand is a whole 2^21-word array and the other factor is the constant 1: the product must be
    the operand itself.  With a = `pre` the spectrum the inverse starts from is small signed; the inverse's own families (split
    2^10 x 2^11) arrive as b = ifft(y), whose spectrum is y.  Ragged lengths with small signed coefficients against the oracle."""
    import oracle as orc
    k, n = 21, 1 << 21

    def mul(a, b):
        out = np.empty(a.size + b.size - 1, dtype=np.uint64)
        L.check(L.lib.ronk_poly_mul(GP, GG, L.ptr(L.arr(a)), a.size, L.ptr(L.arr(b)), b.size, L.ptr(out)))
        return out

    one = np.ones(1, dtype=np.uint64)
    for name, x, _, _ in directed(k, 1, False, (11, 10), BIG_CUTS):
        for tag, got in (("a", mul(x, one)), ("b", mul(one, x))):
            check(got, x, None, ("mul", tag, name))
    for name, y, x, _ in directed(k, 1, True, (10, 11), BIG_CUTS):      # x = ifft(y)
        check(mul(one, x), x, None, ("mul", "spectrum", name))
    da, db = (n >> 1) + 5, (n >> 1) - 4
    a, b = GB.small(da, 1, seed=7)[0], GB.small(db, 1, seed=8)[0]
    z = lambda v: np.concatenate([v, np.zeros(n - v.size, dtype=np.uint64)])
    want = orc.ifft(GP, GG, orc.vec_mul(GP, orc.fft(GP, GG, z(a)), orc.fft(GP, GG, z(b))))
    check(mul(a, b), want[:da + db - 1], None, ("mul", "ragged"))


@pytest.mark.parametrize("log2n,W,chunks,inv", [(16, 4, 2, True), (20, 8, 4, False)])
def test_directed_inputs_sharded_transform(L, log2n, W, chunks, inv):
    """ronk_sharded_*: the four-step's phase pair on logical ranks of one GPU, two of the shapes
    test_sharded_transform_inside_the_library runs -- the two-pass pipeline (R, C) = (2^(k - k/2), 2^(k/2))"""
    logrs = (log2n - log2n // 2, log2n // 2)
    sp = L.ShardedPlan(log2n, [0] * W, inverse=inv, chunks=chunks)
    try:
        assert (sp.R, sp.C) == (1 << logrs[0], 1 << logrs[1])
        for name, x, want, s in directed(log2n, 1, inv, logrs):
            check(sp.transform(x), want, s, ("sharded", log2n, W, chunks, inv, name))
    finally:
        sp.close()


_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
from ronkathon_amd import _lib as L
import gl_branch_inputs as GB
k, batch, logrs, opts = %(case)r
n = 1 << k
plan = L.Plan(GB.P, GB.G, k, batch, **opts)
for inverse in (False, True):
    for name, x, s in GB.families(n, batch, inverse, logrs, %(cuts)r):
        want = GB.fft(x, inverse).reshape(-1)
        got = plan.inverse(x.reshape(-1)) if inverse else plan.forward(x.reshape(-1))
        assert np.array_equal(got, want), (name, inverse)
        assert bool((got < np.uint64(GB.P)).all()), (name, inverse)
        assert s is None or np.array_equal(got, s.reshape(-1)), (name, inverse)
plan.close()
print("DIRECTED OK")
"""


@pytest.mark.parametrize("env,case,cuts", [
    ({"RONK_HALF_LDS": "1", "RONK_WL": "0"}, (16, 3, (8, 8), {"tile_log2_columns": 4, "twiddle_matrix_log2_max": 18}), None),
    ({"RONK_R4MID": "1"}, (19, 2, (10, 9), {"tile_log2_columns": 4}), BIG_CUTS),
], ids=["half", "r4"])
def test_directed_inputs_opt_in_round_structures(env, case, cuts):
    """the half-size LDS image and the [16 . 4] . [8 | 16] round structure: switches the library reads once per process, so a
    child process each (the way test_r4_round_structure_opt_in runs R4)"""
    code = _CHILD % {"root": ROOT, "case": case, "cuts": cuts}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert out.returncode == 0 and "DIRECTED OK" in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]
