"""The Goldilocks tile kernels on DIRECTED inputs (tests/gl_branch_inputs.py), with a census of gl64.h's branches.

Uniformly random residues take the ">= p without a carry" outcome of gl64::add / add_lazy / mad_eps_canon with probability 2^-32
per call: inside a transform it never happens (asserted below: zero non-canonical add_lazy results on the emulator's random
input in every shape), so a kernel that stores a non-canonical word on that event, or a `mad_eps_canon` without its `r >= P`
term, passes every random-input run.  The families place small signed integers at one cut of the transform each; the census
emulator (tests/emu/emu_tile.cpp built with -DRONK_GL64_CENSUS: counting hooks in gl64.h that no product build compiles) reports,
per (pass, phase) -- phase = barriers / wave_syncs a work-item has passed -- how often every function took each outcome.

Asserted per shape, with no exceptions list: every input of every family comes out of the plain emulator equal to the oracle;
wherever add_lazy is called the families together make it return a non-canonical word, and wherever add / mad_eps_canon are
called they take their ">= p" outcome."""
import collections
import concurrent.futures
import os
import subprocess

import numpy as np
import pytest

import emu_cxx
import gl_branch_inputs as GB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "emu_tile.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "ronkathon_amd", "csrc", f) for f in (
    "ntt_tile.h", "ntt_small.h", "ntt_mul.h", "plan.h", "gl64.h", "tile_cfg_table.h", "field_policy.h", "mont64.h", "ntt_tile_wl.h",
    "tile_select.h")] + [os.path.join(ROOT, "oracle", "ronk_oracle.c")]


def _oracle_obj():
    obj = os.path.join(ROOT, "build", "orc_gl_branches.o")
    os.makedirs(os.path.dirname(obj), exist_ok=True)
    src = os.path.join(ROOT, "oracle", "ronk_oracle.c")
    if not os.path.exists(obj) or os.path.getmtime(src) > os.path.getmtime(obj):
        tmp = "%s.tmp.%d" % (obj, os.getpid())
        subprocess.check_call(["gcc", "-O2", "-c", "-o", tmp, src])
        os.replace(tmp, obj)
    return obj


def _build(cxx, name, census, opt):
    """emu_tile for these tests (its own binaries: the census build differs by a macro, the clang builds by the optimisation level)"""
    exe = os.path.join(ROOT, "build", name)
    obj = _oracle_obj()
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        tmp = "%s.tmp.%d" % (exe, os.getpid())
        subprocess.check_call([cxx, opt, "-std=c++17"] + (["-DRONK_GL64_CENSUS"] if census else []) + ["-o", tmp, SRC, obj])
        os.replace(tmp, exe)
    return exe


@pytest.fixture(scope="module")
def emu_plain():
    return _build("g++", "emu_tile_glb", False, "-O2")


@pytest.fixture(scope="module")
def emu_census_gxx():
    return _build("g++", "emu_tile_census", True, "-O2")


@pytest.fixture(scope="module")
def emu_census_clang():
    """the `__clang__` borrow chains of gl64::sub (what the device build compiles).  -O1: the census runs are long, and clang
    spends minutes on -O2"""
    cxx = emu_cxx.device_form_cxx()
    if cxx is None:
        pytest.skip("no clang++ beside hipcc: the device form of the carry chains cannot be built for the host")
    return _build(cxx, "emu_tile_census_clang", True, "-O1")


# ---- shapes: one per body the selection rule (tile_select.h) can pick for Goldilocks, the smallest that selects it.
# args are emu_tile's; `kernels` is what `emu_tile select` prints for them (asserted); logrs the rows (log2) of the passes.
# cuts: None = every cut of the pipeline, or the (q, j, before_twiddle) to take (the 2^22 arrays cost seconds each to build).
Shape = collections.namedtuple("Shape", "id mode args env kernels logrs inverse batch cuts")


def _s(id, args, kernels, logrs, env=None, mode="plain", cuts=None):
    return Shape(id, mode, tuple(args), env or {}, tuple(kernels), tuple(logrs), bool(args[2]), int(args[1]), cuts)


PLAIN_SHAPES = [
    _s("n4-staged-io", (4, 3, 0, 4), ["generic"], [4]),
    _s("2^10x64-whole", (10, 64, 0, 0), ["cfg:whole"], [10]),
    _s("2^13-general+generic", (13, 1, 0, 4), ["cfg:general", "generic"], [7, 6]),
    _s("2^16x2-inv-matrix+row", (16, 2, 1, 4, 18), ["cfg:column/matrix", "cfg:row"], [8, 8]),
    _s("2^20-two-level+row", (20, 1, 0, 4), ["cfg:column/two-level", "cfg:row"], [10, 10]),
    _s("2^16-planner-latency", (16, 1, 0, 4, 18, 25, 0, 0, 1), ["small", "small"], [8, 8]),
    _s("2^22-planner-wave-local", (22, 1, 0, 2, 22, 25, 0, 0, 1), ["wl:column/matrix", "wl:row"], [11, 11],
       cuts=[(0, 1, True), (1, 1, True)]),
    _s("2^14-three-pass", (14, 1, 1, 2, 0, 13), ["generic", "generic", "generic"], [5, 5, 4]),
    _s("2^16x3-half", (16, 3, 0, 4, 18), ["half:column/matrix", "half:row"], [8, 8], env={"RONK_HALF_LDS": "1", "RONK_WL": "0"}),
    _s("2^19x2-inv-r4", (19, 2, 1, 4, 18), ["r4:column/two-level", "r4:row"], [10, 9], env={"RONK_R4MID": "1"}),
]


def signed_words(a):
    return np.ascontiguousarray(a, dtype="<u8")


def run_emu(exe, shape, tmp_path, x=None, x2=None, tag="in", label=""):
    """one emulator run of `shape` on input x (None: the emulator's own random input); returns stdout, asserts OK"""
    env = dict(os.environ, **shape.env)
    for var, arr in (("RONK_EMU_INPUT", x), ("RONK_EMU_INPUT2", x2)):
        if arr is not None:
            path = os.path.join(str(tmp_path), "%s_%s.u64" % (tag, var))
            signed_words(arr).tofile(path)
            env[var] = path
    argv = [exe] + ([shape.mode] if shape.mode != "plain" else []) + [str(a) for a in shape.args]
    out = subprocess.run(argv, capture_output=True, text=True, timeout=1800, env=env)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("OK"), (shape.id, label or tag, out.stdout[-400:] + out.stderr[-400:])
    return out.stdout


def parse_census(stdout):
    """{(pass, phase): {fn: {outcome: count}}}"""
    cen = {}
    for line in stdout.splitlines():
        if not line.startswith("census "):
            continue
        f = dict(t.split("=") for t in line.split()[1:])
        cen.setdefault((int(f["pass"]), f["phase"]), {}).setdefault(f["fn"], {})[f["outcome"]] = int(f["count"])
    return cen


def merge(total, cen):
    for key, fns in cen.items():
        for fn, ocs in fns.items():
            for oc, cnt in ocs.items():
                d = total.setdefault(key, {}).setdefault(fn, {})
                d[oc] = d.get(oc, 0) + cnt
    return total


def families(shape):
    """(name, x) for every directed input of a plain shape"""
    return [(name, x) for name, x, _ in GB.families(1 << shape.args[0], shape.batch, shape.inverse, shape.logrs, shape.cuts)]


# ---- the fused multiply (ntt_mul.h) at the smallest size the emulator's `mul` mode fuses: 2^20 = 2^10 x 2^10, 4-column tiles.
# Census passes: 0 = the forward column pass of both operands, 1 = the fused middle (row pass of a, row pass of b, product,
# inverse column pass -- apart by their barrier counts), 2 = the inverse row pass.
MUL_K, MUL_LOGC, MUL_TWF = 20, 2, 18
MUL_LOGRS = (10, 10)


def _mul_shape(tag, d, d2):
    return Shape("mul-" + tag, "mul", (MUL_K, d, d2, MUL_LOGC, MUL_TWF), {}, (), MUL_LOGRS, False, 1, None)


def mul_cases():
    """(shape, name, a, b): the operands are zero padded to n on load, so a directed operand is a whole n-word array and the other
    one is the constant 1 (lengths n and 1: the padding limit of the second batch entry at its extreme); the ragged pair
    (2^19 + 5, 2^19 - 4) carries small signed coefficients.  With a = `pre` the spectrum of a, and so the product spectrum the
    inverse starts from, is small signed; the inverse's own families arrive as b = ifft(y), whose spectrum is y."""
    n = 1 << MUL_K
    one = np.ones(1, dtype=np.uint64)
    # (the `b` cuts of the later rounds: with small / pre / colpre they reach every phase, and each run transforms 2^20 points thrice)
    fwd = Shape("", "plain", (MUL_K, 1, 0), {}, (), MUL_LOGRS, False, 1, [(0, 1, True), (1, 0, True), (1, 1, True)])
    inv = Shape("", "plain", (MUL_K, 1, 1), {}, (), MUL_LOGRS, True, 1, [(0, 0, True), (0, 1, True), (1, 0, True), (1, 1, True)])
    for name, x in families(fwd):
        yield _mul_shape("a", n, 1), "a=" + name, x[0], one
        yield _mul_shape("b", 1, n), "b=" + name, one, x[0]
    for name, y in families(inv):
        yield _mul_shape("b", 1, n), "spectrum=" + name, one, GB.fft(y, inverse=True)[0]
    da, db = (n >> 1) + 5, (n >> 1) - 4
    yield _mul_shape("ragged", da, db), "ragged-small", GB.small(da, 1, seed=7)[0], GB.small(db, 1, seed=8)[0]


# ---- one phase pair of the multi-GPU four-step, all ranks in one process: 2^16 over 4 ranks = 2^8-row column transforms,
# twiddle, exchange, 2^8-point row transforms -- the two-pass pipeline (8, 8).  Census passes: phase 1 from 0, phase 2 from 8.
DIST = Shape("dist-2^16x4", "dist", (16, 4, 0), {}, (), (8, 8), False, 1, None)


# ---- the checks
DIRECTED_FNS = ("add_lazy", "add", "mad_eps_canon")
_FAMILY_CACHE = {}


def cached_families(shape):
    """the arrays of the shape the previous test used too (the two compiler legs of one shape run back to back)"""
    if shape.id not in _FAMILY_CACHE:
        _FAMILY_CACHE.clear()
        _FAMILY_CACHE[shape.id] = families(shape)
    return _FAMILY_CACHE[shape.id]


def check_census(cases, random_shapes, exe_census, exe_plain, tmp_path):
    """cases: (shape, name, x, x2).  Every case through the census emulator (and the plain one when given) against the oracle; then
    the census assertions over the passes and phases the random-input runs of `random_shapes` and the cases themselves show"""
    called, total = {}, {}
    for shape in random_shapes:
        cen = parse_census(run_emu(exe_census, shape, tmp_path))
        for key, fns in cen.items():
            assert fns.get("add_lazy", {}).get("ge_p", 0) == 0, ("random input made add_lazy return a non-canonical word", shape.id, key, fns["add_lazy"])
        merge(called, cen)
    # the emulator runs are independent single-threaded processes: a few at a time
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(4, os.cpu_count() or 1))) as pool:
        jobs = []
        for i, (shape, name, x, x2) in enumerate(cases):
            if exe_plain:
                jobs.append((False, pool.submit(run_emu, exe_plain, shape, tmp_path, x, x2, "p%d" % i, name)))
            jobs.append((True, pool.submit(run_emu, exe_census, shape, tmp_path, x, x2, "c%d" % i, name)))
        for counted, job in jobs:
            out = job.result()       # (raises the run's assertion: which shape, which input, the mismatch line)
            if counted:
                cen = parse_census(out)
                merge(called, cen)
                merge(total, cen)
    missing = []
    for key in sorted(called):
        for fn in DIRECTED_FNS:
            if sum(called[key].get(fn, {}).values()) and not total.get(key, {}).get(fn, {}).get("ge_p", 0):
                missing.append((key, fn))
    assert not missing, "(pass, phase) in which the function runs but no directed input makes it take its '>= p' outcome: %r" % missing
    return total


def _exes(request, cxx):
    if cxx == "g++":
        return request.getfixturevalue("emu_census_gxx"), request.getfixturevalue("emu_plain")
    return request.getfixturevalue("emu_census_clang"), None     # (the census emulator checks every output against the oracle too)


def test_pipeline_model_is_the_oracle_transform():
    """gl_branch_inputs.Pipeline -- every round, round twiddle and inter-pass twiddle of one-, two- and three-pass plans, forward
    and inverse -- reproduces the oracle's fft / ifft; and each family's cut really holds small signed values"""
    rng = np.random.default_rng(5)
    for n, logrs in ((1 << 4, [4]), (1 << 10, [10]), (1 << 13, [7, 6]), (1 << 14, [5, 5, 4]), (1 << 19, [10, 9])):
        for inv in (False, True):
            x = rng.integers(0, GB.P, size=(2, n), dtype=np.uint64)
            assert np.array_equal(GB.model_transform(x, logrs, inv), GB.fft(x, inv)), (n, logrs, inv)
    is_small = lambda a: bool(np.all((a <= 2) | (a >= GB.P - 2)))
    n, logrs = 1 << 13, [7, 6]
    for inv in (False, True):
        pl = GB.Pipeline(n, logrs, inv)
        state = lambda x, q, j, before: pl.apply(x.reshape([2] + pl.shape), pl.cut_steps(q, j, before))
        assert is_small(state(GB.colpre(n, 2, inv, 7), 0, 1, True))
        assert is_small(state(GB.cut(n, 2, inv, logrs, 1, 0, False), 1, 0, False))
        assert not is_small(state(GB.cut(n, 2, inv, logrs, 1, 0, False), 0, 1, True))
        x, s = GB.pre(n, 2, inv)
        assert is_small(s) and np.array_equal(GB.fft(x, inv), s)


@pytest.mark.parametrize("shape", PLAIN_SHAPES, ids=[s.id for s in PLAIN_SHAPES])
def test_shapes_select_the_bodies_they_are_listed_for(emu_plain, shape):
    out = subprocess.run([emu_plain, "select"] + [str(a) for a in shape.args], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **shape.env))
    assert out.returncode == 0, out.stderr[-400:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("pass")]
    assert tuple(l.split("kernel=")[1] for l in lines) == shape.kernels, out.stdout
    assert tuple(int(l.split("logr=")[1].split()[0]) for l in lines) == shape.logrs, out.stdout


@pytest.mark.parametrize("cxx", ["g++", "clang++"])
@pytest.mark.parametrize("shape", PLAIN_SHAPES, ids=[s.id for s in PLAIN_SHAPES])
def test_directed_inputs_reach_every_branch(request, tmp_path, shape, cxx):
    """small / pre / colpre / every cut of the shape's pipeline: equal to the oracle on the plain and on the census emulator; the
    families together take the '>= p' outcome of add_lazy, add and mad_eps_canon in every (pass, phase) that calls them; the
    emulator's random input never makes add_lazy return a non-canonical word"""
    exe_census, exe_plain = _exes(request, cxx)
    cases = [(shape, name, x, None) for name, x in cached_families(shape)]
    check_census(cases, [shape], exe_census, exe_plain, tmp_path)


@pytest.mark.parametrize("cxx", ["g++", "clang++"])
def test_directed_inputs_reach_every_branch_of_the_fused_multiply(request, tmp_path, cxx):
    """ntt_mul.h: the families on either operand, the inverse's families as the product spectrum, ragged small operands"""
    exe_census, exe_plain = _exes(request, cxx)
    n = 1 << MUL_K
    check_census(mul_cases(), [_mul_shape("ragged", (n >> 1) + 5, (n >> 1) - 4)], exe_census, exe_plain, tmp_path)


@pytest.mark.parametrize("cxx", ["g++", "clang++"])
def test_directed_inputs_reach_every_branch_of_a_dist_phase_pair(request, tmp_path, cxx):
    exe_census, exe_plain = _exes(request, cxx)
    check_census([(DIST, name, x, None) for name, x in families(DIST)], [DIST], exe_census, exe_plain, tmp_path)
