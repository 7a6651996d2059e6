"""The Goldilocks bodies outside the NTT on DIRECTED inputs (tests/gl_directed.py and the emulators' directed mode), with a census
of gl64.h's branches per body.

gl64::add and gl64::mad_eps_canon (inside every gl64::mul, and the last step of PosGl::acc_reduce) each have an outcome that needs
a 64-bit sum in [p, 2^64) without a carry.  The emulators' own inputs -- uniform words with p - 1, 0 and p .. p + 4 mixed in --
reach it where two edge words meet at the first operation of a body and nowhere after that: in nine million additions of the
Poseidon permutation, never.  A kernel that stores p for 0 there, or a mad_eps_canon without its `r >= P` term, passes all of it.

The emulators (tests/emu/*.cpp) name the body they drive with census_stage (tests/emu/emu_census.h); built with
-DRONK_GL64_CENSUS they print how often every gl64.h function took each outcome in every stage.  Their directed inputs:
  emu_poseidon   file mode (RONK_EMU_INPUT): the constants, states and words of gl_directed's Poseidon families; and the directed
                 mode of its own generator (small constants, a +-1 matrix), which `make sanitize` runs
  emu_plonk      its blob, with small signed columns and challenges
  emu_air_per    its blob, with gl_directed's program (every opcode, operand kind and constraint kind) on small signed columns
  emu_ext2       besides the directed mode, a file mode for the folds: gl_directed's `small`, `cut`, `out` and `beta` layers
  the others     RONK_EMU_SMALL=B: every input word and every challenge is t mod p, t uniform in [-B, B]
In every mode the emulator's `unsigned __int128 % p` restatement checks every output.

Asserted, on a g++ build and on a build with the clang beside hipcc (the `__builtin_addc / subc` chains the device compiles):
  1. every directed input gives the restatement's words, on the plain and on the census build;
  2. in every stage, every one of add and mad_eps_canon that the stage calls at all takes its ">= p" outcome on the directed
     inputs -- no exceptions list; what a stage CANNOT show is in NOT_SEPARABLE below, with the reason;
  3. over the `lin` family at width 12 at least 5 % of the permutation's additions and 10 % of its reductions take ">= p";
  4. the borrow counts of sub / sub32 per stage are printed (-s), and asserted > 0 where the families reach them."""
import concurrent.futures
import os
import subprocess

import numpy as np
import pytest

import emu_cxx
import gl_directed as GD
from test_emu_gl_branches import merge, parse_census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL = GD.P
CSRC = os.path.join(ROOT, "ronkathon_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
EMULATORS = ("poseidon", "fri", "ext2", "deep", "mpcs", "accum", "plonk", "air", "air_per")
DIRECTED_FNS = ("add", "mad_eps_canon")

# What the census cannot tell apart.  A stage is what an emulator can call on its own; gl64.h's hooks are the only ones, and no
# product header gains one, so a part of a body that only runs inside it has no counts of its own:
NOT_SEPARABLE = {
    "deep_combine / deep_check / mpcs_combine / mpcs_check: the quotient part":
        "deep_combine_lane runs the S-accumulation (matrix word times a power of alpha: directed) and the division by x - z_k in "
        "one body; the quotient part multiplies by the inverse of a domain point minus a random z, so its operands are uniform "
        "whatever the matrix holds.  The stage's '>= p' counts come from the accumulation.",
    "plonk: the permutation and boundary terms":
        "the gate sum is a chain of small additions and products (directed); the permutation argument multiplies beta by the "
        "domain point x, and the division by the vanishing polynomial multiplies by a table word: uniform operands.",
}


# ------------------------------------------------------------------------------------------------ builds
def _deps():
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + \
           [os.path.join(EMU, f) for f in os.listdir(EMU) if f.endswith((".h", ".cpp"))]


def _build(cxx, emulator, kind, census, opt):
    exe = os.path.join(ROOT, "build", "gld_%s_%s" % (emulator, kind))
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in _deps()):
        tmp = "%s.tmp.%d" % (exe, os.getpid())
        src = os.path.join(EMU, "emu_%s.cpp" % emulator)
        subprocess.check_call([cxx, opt, "-std=c++17"] + (["-DRONK_GL64_CENSUS"] if census else []) + ["-o", tmp, src])
        os.replace(tmp, exe)
    return exe


def _build_all(cxx, kind, census, opt):
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:
        jobs = {e: pool.submit(_build, cxx, e, kind, census, opt) for e in EMULATORS}
        return {e: j.result() for e, j in jobs.items()}


@pytest.fixture(scope="module")
def plain_gxx():
    return _build_all("g++", "plain", False, "-O2")


@pytest.fixture(scope="module")
def census_gxx():
    return _build_all("g++", "census", True, "-O1")


@pytest.fixture(scope="module")
def census_clang():
    cxx = emu_cxx.device_form_cxx()
    if cxx is None:
        pytest.skip("no clang++ beside hipcc: the device form of the carry chains cannot be built for the host")
    return _build_all(cxx, "census_clang", True, "-O1")


# ------------------------------------------------------------------------------------------------ runs
class Run:
    """one emulator run: argv, environment, and the file it reads (None: its own generator)"""

    def __init__(self, label, argv, env=None, blob=None, blob_args=False):
        self.label, self.argv, self.env, self.blob, self.blob_args = label, [str(a) for a in argv], dict(env or {}), blob, blob_args


def run_emu(exe, run, tmp_path, tag):
    env = dict(os.environ, **run.env)
    argv = [exe] + run.argv
    if run.blob is not None:
        path = os.path.join(str(tmp_path), "%s.u64" % tag)
        np.ascontiguousarray(run.blob, dtype="<u8").tofile(path)
        if run.blob_args:
            argv += [path, path + ".out"]
        else:
            env["RONK_EMU_INPUT"] = path
    out = subprocess.run(argv, capture_output=True, text=True, timeout=1800, env=env)
    lines = out.stdout.splitlines()
    ok = out.returncode == 0 and any(l.startswith("OK") for l in lines) and not any(l.startswith("FAIL") for l in lines)
    assert ok, (run.label, " ".join(run.argv), [l for l in lines if not l.startswith("census ")][-6:], out.stderr[-400:])
    return out.stdout


def poseidon_runs():
    """every family at every width: 200 states through the permutation, the family's words through the sponge and the tree; and
    one run whose sponge and leaf words are window_words (the `lin` constants)"""
    runs = []
    for family in GD.POSEIDON_FAMILIES:
        for width in GD.POSEIDON_WIDTHS:
            Pm, st, _ = GD.poseidon_states(family, width, 200)
            words = np.array(GD.limb_ints(4096, 9), dtype=np.uint64) if family == "limb" else \
                GD.small_signed((4096,), 9, GD.poseidon_state_bound(family))
            argv = (GL, width, Pm.alpha, Pm.num_p, Pm.num_f, Pm.rate, 1)
            runs.append(Run("%s-w%d" % (family, width), argv, blob=GD.poseidon_blob(Pm, st, words)))
    Pm, st, _ = GD.poseidon_states("lin", 12, 200)
    runs.append(Run("own-generator-w12", (GL, 12, 1, 22, 8, 8, 1), SMALL))       # (the line of `make sanitize`)
    runs.append(Run("lin-w12-window", (GL, 12, Pm.alpha, Pm.num_p, Pm.num_f, Pm.rate, 1),
                    blob=GD.poseidon_blob(Pm, GD.window_words(st.size, 4).reshape(st.shape), GD.window_words(4096, 5))))
    return runs


def fold_runs():
    """every fold family of every form, arity, layer size and coset shift: one file per family"""
    runs = []
    for family in GD.fold_families(3):
        runs.append(Run("fold-" + family, (GL, 7), blob=GD.fold_blob(GD.all_fold_cases(family))))
    return runs


SMALL = {"RONK_EMU_SMALL": "2"}
# per emulator: (its default runs, as in `make sanitize`; the directed runs)
RUNS = {
    "poseidon": ([Run("random", (GL, 12, 7, 22, 8, 8, 1))], poseidon_runs),
    "fri": ([Run("random", (GL, 7))], lambda: [Run("small", (GL, 7), SMALL)]),
    "ext2": ([Run("random", (GL, 7))], lambda: [Run("small", (GL, 7), {"RONK_EMU_SMALL": "8"})] + fold_runs()),
    "deep": ([Run("random-w7", (GL, 7)), Run("random-w11", (GL, 7, 11))],
             lambda: [Run("small-w7", (GL, 7), SMALL), Run("small-w11", (GL, 7, 11), SMALL)]),
    "mpcs": ([Run("random-w7", (GL, 7)), Run("random-w11", (GL, 7, 11))],
             lambda: [Run("small-w7", (GL, 7), SMALL), Run("small-w11", (GL, 7, 11), SMALL)]),
    "accum": ([Run("random-w7", (GL, 7)), Run("random-w11", (GL, 11))],
              lambda: [Run("small-w7", (GL, 7), SMALL), Run("small-w11", (GL, 11), SMALL)]),
    "plonk": ([Run("random", (GL, 7, 7, 9, 2, 7, 1))],
              lambda: [Run("small-n%d-b%d-w%d" % (n, b, w), (GL, 7, w, n, b, 7, 1), blob=GD.plonk_blob(n, b, 10 * n + b), blob_args=True)
                       for n in (4, 6) for b in (1, 2) for w in (7, 11)]),
    # (emu_air has no periodic columns: its own generator in the directed mode; emu_air_per also reads gl_directed's program)
    "air": ([Run("random", (GL, 7, 7))], lambda: [Run("small-w%d" % w, (GL, 7, w), SMALL) for w in (7, 11)]),
    "air_per": ([Run("random", (GL, 7, 7))],
                lambda: [Run("small-w%d" % w, (GL, 7, w), SMALL) for w in (7, 11)] +
                        [Run("program-n%d-b%d-w%d-tin%d" % (n, b, w, tin), (GL, 7, w, n, b), blob=GD.air_blob(w, n, b, bool(tin)), blob_args=True)
                         for n in (4, 6) for b in (1, 2) for w in (7, 11) for tin in (0, 1)]),
}
_CENSUS = {}


def census_of(kind, exes_census, exes_plain, emulator, tmp_path):
    """({stage: {fn: {outcome: count}}} of the default runs, the same summed over the directed runs); every directed run also on
    the plain build when there is one.  Kept per (compiler, emulator): the assertions below share the runs"""
    if (kind, emulator) not in _CENSUS:
        random_runs, directed = RUNS[emulator]
        directed = directed()
        rnd, tot = {}, {}
        with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:
            jobs = [("r", pool.submit(run_emu, exes_census[emulator], r, tmp_path, "r%d" % i)) for i, r in enumerate(random_runs)]
            jobs += [("d", pool.submit(run_emu, exes_census[emulator], r, tmp_path, "d%d" % i)) for i, r in enumerate(directed)]
            if exes_plain:
                jobs += [("p", pool.submit(run_emu, exes_plain[emulator], r, tmp_path, "p%d" % i)) for i, r in enumerate(directed)]
            for what, job in jobs:
                out = job.result()
                if what != "p":
                    merge(rnd if what == "r" else tot, parse_census(out))
        stage = lambda cen: {key[1]: fns for key, fns in cen.items()}
        _CENSUS[(kind, emulator)] = (stage(rnd), stage(tot))
    return _CENSUS[(kind, emulator)]


def _count(cen, stage, fn, outcome=None):
    oc = cen.get(stage, {}).get(fn, {})
    return sum(oc.values()) if outcome is None else oc.get(outcome, 0)


def _exes(request, cxx):
    if cxx == "g++":
        return "g++", request.getfixturevalue("census_gxx"), request.getfixturevalue("plain_gxx")
    return "clang++", request.getfixturevalue("census_clang"), None      # (the census build checks every output too)


@pytest.mark.parametrize("cxx", ["g++", "clang++"])
@pytest.mark.parametrize("emulator", EMULATORS)
def test_directed_inputs_reach_the_ge_p_outcome_in_every_stage(request, tmp_path, emulator, cxx):
    kind, exes_census, exes_plain = _exes(request, cxx)
    rnd, tot = census_of(kind, exes_census, exes_plain, emulator, tmp_path)
    stages = sorted(set(rnd) | set(tot))
    assert stages and all(not s.startswith("mont.") for s in stages), stages     # (the Montgomery policy calls nothing of gl64.h)
    missing = []
    print("\n%-26s %-14s %12s %10s %12s %10s" % ("stage", "function", "random calls", "ge_p", "directed", "ge_p"))
    for s in stages:
        for fn in DIRECTED_FNS:
            called = _count(rnd, s, fn) + _count(tot, s, fn)
            if called:
                print("%-26s %-14s %12d %10d %12d %10d" % (s, fn, _count(rnd, s, fn), _count(rnd, s, fn, "ge_p"), _count(tot, s, fn),
                                                           _count(tot, s, fn, "ge_p")))
                if not _count(tot, s, fn, "ge_p"):
                    missing.append((s, fn))
        print("%-26s %-14s %12s %10d %12s %10d" % (s, "sub/sub32 wrap", "", _count(rnd, s, "sub", "wrap") + _count(rnd, s, "sub32", "wrap"), "",
                                                   _count(tot, s, "sub", "wrap") + _count(tot, s, "sub32", "wrap")))
    assert not missing, "stages in which the function runs but no directed input makes it take its '>= p' outcome: %r" % missing


@pytest.mark.parametrize("cxx", ["g++", "clang++"])
def test_poseidon_shares_and_borrows(request, tmp_path, cxx):
    """the `lin` family at width 12 alone: the shares of the permutation stage; acc_reduce's sub32 and sub borrow on it (the
    product (p - 1)(p - 1) has a zero lower half and 0xFFFFFFFE on top); the default run all but never takes add's '>= p' there"""
    kind, exes_census, _ = _exes(request, cxx)
    rnd, _ = census_of(kind, exes_census, None if cxx != "g++" else request.getfixturevalue("plain_gxx"), "poseidon", tmp_path)
    assert _count(rnd, "permute", "add") > 10000 and 10000 * _count(rnd, "permute", "add", "ge_p") < _count(rnd, "permute", "add")   # < 0.01 %
    run = [r for r in poseidon_runs() if r.label == "lin-w12"]
    cen = {key[1]: fns for key, fns in parse_census(run_emu(exes_census["poseidon"], run[0], tmp_path, "lin12")).items()}
    adds, reds = _count(cen, "permute", "add"), _count(cen, "permute", "mad_eps_canon")
    assert adds == reds == 200 * 30 * 12
    print("\nlin, width 12, permute: add ge_p %d of %d, mad_eps_canon ge_p %d of %d, sub32 borrows %d, sub borrows %d" % (
        _count(cen, "permute", "add", "ge_p"), adds, _count(cen, "permute", "mad_eps_canon", "ge_p"), reds,
        _count(cen, "permute", "sub32", "wrap"), _count(cen, "permute", "sub", "wrap")))
    assert 20 * _count(cen, "permute", "add", "ge_p") >= adds
    assert 10 * _count(cen, "permute", "mad_eps_canon", "ge_p") >= reds
    for stage in ("permute", "sponge", "merkle_leaf", "merkle_verify"):
        assert _count(cen, stage, "sub32", "wrap") > 0 and _count(cen, stage, "sub", "wrap") > 0, stage


def test_the_quotient_part_of_the_combinations_stays_undirected(request, tmp_path):
    """the stages NOT_SEPARABLE speaks of: the product count of deep_combine_lane / mpcs_combine_lane is dominated by the quotient
    part (per point K products by 1 / (x - z_k) against one S-accumulation), and small inputs do not direct it: the share of
    mad_eps_canon calls that take '>= p' is no higher on the directed runs than on the default ones, where the edge words p - 1, 0
    and p + k meet.  (The additions of the S-accumulation are directed: the first test holds these stages to that.)"""
    kind, exes_census, exes_plain = _exes(request, "g++")
    for emulator in ("deep", "mpcs"):
        rnd, tot = census_of(kind, exes_census, exes_plain, emulator, tmp_path)
        for policy in ("gl.", "w7."):
            for body in ("combine", "check"):
                stage = "%s%s_%s" % (policy, emulator, body)
                calls_r, calls_d = _count(rnd, stage, "mad_eps_canon"), _count(tot, stage, "mad_eps_canon")
                hit_r, hit_d = _count(rnd, stage, "mad_eps_canon", "ge_p"), _count(tot, stage, "mad_eps_canon", "ge_p")
                print("%-18s mad_eps_canon ge_p: default %d of %d, directed %d of %d" % (stage, hit_r, calls_r, hit_d, calls_d))
                assert calls_r and calls_d and hit_d * calls_r <= hit_r * calls_d, stage
                assert _count(tot, stage, "add", "ge_p") * _count(rnd, stage, "add") > 10 * _count(rnd, stage, "add", "ge_p") * _count(tot, stage, "add"), stage


def test_fold_model_is_the_reference_fold_and_the_cuts_hold_small_values():
    """gl_directed.fold_model -- the kernels' pipeline without the halves, 2^-eta at the end -- reproduces fri_ref.fold and
    fri_ext_ref.fold on every family; in a `cut e` layer both operands of every outer addition of step e are small signed (of
    the mixed first step: of its one addition), and all but a few of the step before are not; in an `out` layer the value entering the final
    product is small"""
    is_small = lambda c: all(min(x, GL - x) <= 2 for x in c)
    for form in GD.FOLD_FORMS:
        for eta in (1, 2, 3):
            for n, shift in ((eta + 1, 1), (eta + 5, GD.G), (9, GD.G)):
                for family in GD.fold_families(eta):
                    F, words, beta, want = GD.fold_case(form, eta, n, shift, family)
                    N, vals = F.size(0), [int(v) for v in words]
                    pairs = [(vals[i] % GL, vals[N + i] % GL if form == "ext" else 0) for i in range(N)]
                    b = (int(beta[0]) % GL, 0 if form == "base" else int(beta[1]) % GL)
                    out, steps = GD.fold_model(F, pairs, b)
                    got = [c[0] for c in out] + ([] if form == "base" else [c[1] for c in out])
                    assert got == want.tolist(), (form, eta, n, family)
                    operands = lambda e: [(s1, s2[:1] if form == "mix" and e == 0 else s2) for leaf in steps[e] for s1, s2, _, _ in leaf]
                    if family.startswith("cut"):
                        e = int(family[3:])
                        assert all(is_small(s1) and is_small(s2) for s1, s2 in operands(e)), (form, eta, n, family)
                        if e:
                            few = sum(is_small(s1) and is_small(s2) for s1, s2 in operands(e - 1))      # (U = 0 and an even V: by chance)
                            assert 20 * few <= len(operands(e - 1)), (form, eta, n, family)
                    if family == "out":
                        two = pow(2, eta, GL)
                        assert all(is_small((c[0] * two % GL, c[1] * two % GL)) for c in out), (form, eta, n)


def test_families_hold_what_they_promise():
    """window_words fill [p, 2^64) and hold 2^64 - 1; the constructors' expected values are those of the references on reduced
    operands; the product scans' prefixes stay small (asserted inside the constructors, on accum_ref's output)"""
    w = GD.window_words(1000, 1)
    assert w.dtype == np.uint64 and (w >= np.uint64(GL)).all() and int(w[-1]) == 2**64 - 1 and len(set(w.tolist())) > 990
    assert int(GD.window_words(1, 2)[0]) == 2**64 - 1
    Pm, st, want = GD.poseidon_states("lin", 12, 3)
    assert Pm.alpha == 1 and all(sum(1 for v in row if v) == 2 and all(v in (0, 1, GL - 1) for v in row) for row in Pm.mds)
    assert ((st <= 2) | (st >= np.uint64(GL - 2))).all() and (want < np.uint64(GL)).all()
    for op in ("sum", "prod"):
        for n in GD.SCAN_SIZES:
            x, want, _ = GD.scan_base(op, n, 0)
            assert x.shape == want.shape == (n,) and (want < np.uint64(GL)).all()
            for w in (GD.W_SHIFT, GD.W_PLAIN):
                x, want, _ = GD.scan_ext(op, w, n, 1)
                assert x.shape == want.shape == (2, n)
    a, b, s, want = GD.ext_case("mul", 7, 65, window=True)
    assert (a >= np.uint64(GL)).all() and (want < np.uint64(GL)).all()
