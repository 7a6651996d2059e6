"""Times what the fixed round and the periodic columns add (ronk_air_create_per, ronk_stark_create_fixed) and checks what they must
not slow, after warm-up, median of `rounds`.  Three measurements:
  (1) the programs tools/air_time.py times through ronk_air_quotient_dev (the PLONK quotient as a program, the S-box row) on this
      library against the parent commit's library, which is loaded through RONK_LIB_PATH in a child process of its own: runs in
      the order A (parent) / B (this) / A (parent).  The new operand case must not slow programs that do not use it: B is "not
      slower" when it is within the larger of the spread of the two A runs and 2 % (the spread DESIGN section 22 reports).
  (2) the S-box row with its three round constants as periodic columns of period 8 (tests/stark_fixed_programs.py sbox_periodic)
      against the same constants as a three-column base group of M words: the ratio and the bytes per row each form reads.
  (3) ronk_stark_prove_dev of the gate instance with its five selectors in the fixed round against the same eight columns as ONE
      trace round on the parent's entry points and library (that form binds the selectors to nothing: it is run for time only),
      A (parent) / B (this) / A (parent), wall clock with a synchronisation per proof; and ronk_stark_fixed_commit_dev alone, the
      extension and the tree of the five columns that leave the proof.  The fixed form must not be slower beyond the A spread.
Every run is a child process under a time limit, and the driver stops at the first one that fails or times out.  One JSON line
per measurement, appended to --out.  Without --parent-lib only (2) and the B runs are made.

usage: python tools/stark_fixed_time.py --parent-lib PATH [--iters 10] [--warmup 2] [--rounds 3] [--log2-sizes 20,22] [--fields gl,mont]
                                        [--limit 300] [--out profiles/stark_fixed_time_mi355x.jsonl]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log2-sizes", default="20,22")
ap.add_argument("--fields", default="gl,mont")
ap.add_argument("--measurements", default="air,per,gate")
ap.add_argument("--parent-lib", default=None, help="libronk_ntt.so built from the parent commit")
ap.add_argument("--limit", type=int, default=300, help="seconds per child process")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stark_fixed_time_mi355x.jsonl"))
ap.add_argument("--case", default=None, help="internal: measurement,field,log2_m,run of the one case this process runs")
args = ap.parse_args()

PRIMES = {"gl": (0xFFFFFFFF00000001, 7), "mont": (0xFFFFFFFC00000001, 10)}
ETA, LOG2_FINAL, Q, D = 2, 4, 32, 4
GATE_LOG2_B = 2
SPREAD_FLOOR = 0.02


# ---------------------------------------------------------------------------------------------------- the driver
def child(what, field, m, run, parent):
    """-> the JSON lines the child appended, or None when it failed"""
    cmd = [sys.executable, os.path.abspath(__file__), "--case", "%s,%s,%s,%s" % (what, field, m, run), "--out", args.out]
    for k in ("iters", "warmup", "rounds"):
        cmd += ["--" + k, str(getattr(args, k))]
    env = dict(os.environ)
    env.pop("RONK_LIB_PATH", None)
    if parent:
        env["RONK_LIB_PATH"] = os.path.abspath(args.parent_lib)
    before = os.path.getsize(args.out) if os.path.exists(args.out) else 0
    try:
        rc = subprocess.run(cmd, timeout=args.limit, env=env).returncode
    except subprocess.TimeoutExpired:
        rc = 124
    if rc != 0:
        print("%s %s 2^%s run %s ended with status %d: stopping" % (what, field, m, run, rc), flush=True)
        return None
    with open(args.out) as f:
        f.seek(before)
        return [json.loads(line) for line in f if line.strip()]


def emit_line(d):
    line = json.dumps(d)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def compare(what, field, m, runs):
    """A / B / A: for every op the three medians, the spread of the A runs, B over the faster A, and the verdict"""
    a0, b, a1 = ({d["op"]: d["ms_median"] for d in lines if "ms_median" in d} for lines in runs)
    for op in b:
        if op not in a0 or op not in a1:
            continue
        spread = abs(a0[op] - a1[op]) / min(a0[op], a1[op])
        over = b[op] / max(a0[op], a1[op]) - 1
        emit_line({"measurement": what, "field": field, "log2_m": int(m), "op": op + ": this over the parent", "a_before_ms": a0[op], "b_ms": b[op],
                   "a_after_ms": a1[op], "a_spread": round(spread, 4), "b_over_slower_a": round(over, 4),
                   "b_over_faster_a": round(b[op] / min(a0[op], a1[op]) - 1, 4), "allowed": round(max(spread, SPREAD_FLOOR), 4),
                   "not_slower": bool(b[op] / min(a0[op], a1[op]) - 1 <= max(spread, SPREAD_FLOOR))})


def driver():
    for field in args.fields.split(","):
        for m in args.log2_sizes.split(","):
            for what in args.measurements.split(","):
                if what == "per" or not args.parent_lib:
                    if child(what, field, m, "B", False) is None:
                        return 1
                    continue
                runs = []
                for run, parent in (("A0", True), ("B", False), ("A1", True)):
                    runs.append(child(what, field, m, run, parent))
                    if runs[-1] is None:
                        return 1
                compare(what, field, m, runs)
    return 0


# ---------------------------------------------------------------------------------------------------- one case
def case(what, field, log2_m, run):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    import air_programs as AP
    import air_ref as AR
    from ronkathon_amd import _lib as L
    lib = L.lib
    p, w = PRIMES[field]
    g = shift = w
    M = 1 << log2_m
    base = {"measurement": what, "field": field, "w": w, "log2_m": log2_m, "run": run, "parent_library": bool(os.environ.get("RONK_LIB_PATH"))}
    out = open(args.out, "a")

    def emit(d):
        line = json.dumps(dict(base, **d))
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def event_ms(fn):
        ts = []
        for _ in range(args.rounds):
            for k in range(args.warmup):
                fn(k)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(args.iters):
                fn(k)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) / args.iters)
        return ts

    def wall_ms(fn):
        ts = []
        for _ in range(args.rounds):
            fn(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.iters):
                fn(k)
                torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / args.iters)
        return ts

    def report(d, ts):
        med = float(np.median(ts))
        emit(dict(d, ms_median=round(med, 4), ms_all=[round(t, 4) for t in ts]))
        return med

    def rand(words):
        return torch.randint(-2**63, 2**63 - 1, (words,), dtype=torch.int64, device="cuda")

    def empty(words):
        return torch.empty(words, dtype=torch.int64, device="cuda")

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()

    def pointers(tensors):
        return (C.c_void_p * max(1, len(tensors)))(*[t.data_ptr() for t in tensors])

    torch.manual_seed(1)

    def air_handle(dom, prog, groups, n_ext, n_chal, periodic=None):
        h = C.c_void_p()
        ops, imm = (C.c_uint64 * len(prog.ops))(*prog.ops), (C.c_uint64 * max(1, len(prog.imm)))(*[v % p for v in prog.imm])
        common = (dom, len(groups), (C.c_uint32 * len(groups))(*groups), n_ext, n_chal, len(prog.imm), prog.n_regs, prog.n_constraints, ops,
                  len(prog.ops), imm)
        if periodic is None:
            L.check(lib.ronk_air_create(C.byref(h), *common))
        else:
            from ronkathon_amd import callers
            n_per, log2_period, values = callers.periodic_arrays(periodic)
            L.check(lib.ronk_air_create_per(C.byref(h), *common, n_per, log2_period, L.ptr(values)))
        return h

    if what in ("air", "per"):
        log2_b = 2 if what == "air" else 3
        dom = C.c_void_p()
        L.check(lib.ronk_plonk_create(C.byref(dom), p, g, w, log2_m - log2_b, log2_b, g, (C.c_uint64 * 3)(1, 2, 3)))
        T = empty(2 * M)

    if what == "air":
        # ---- (1) the programs of tools/air_time.py, inputs rotating over enough copies to exceed the 256 MiB Infinity Cache
        prog = AP.plonk()
        h = air_handle(dom, prog, (3, 5, 3, 1), 1, 2)
        copies = max(2, min(8, (512 << 20) // (14 * 8 * M)))
        sets = [tuple(rand(k * M) for k in (3, 5, 3, 1, 2)) for _ in range(copies)]
        chal, lam = rand(4), rand(6)
        report({"op": "air_quotient_dev plonk program", "ops": len(prog.ops)},
               event_ms(lambda k: L.check(lib.ronk_air_quotient_dev(h, pointers(sets[k % copies][:4]), pointers(sets[k % copies][4:]), chal.data_ptr(),
                                                                    lam.data_ptr(), None, T.data_ptr(), None))))
        L.check(lib.ronk_air_destroy(h))
        del sets
        prog = AP.sbox_row()
        h = air_handle(dom, prog, (3,), 0, 2)
        copies = max(2, min(16, (512 << 20) // (3 * 8 * M)))
        cols = [rand(3 * M) for _ in range(copies)]
        lam, T_in = rand(2 * prog.n_constraints), rand(2 * M)
        report({"op": "air_quotient_dev sbox program", "ops": len(prog.ops)},
               event_ms(lambda k: L.check(lib.ronk_air_quotient_dev(h, pointers([cols[k % copies]]), None, chal.data_ptr(), lam.data_ptr(),
                                                                    T_in.data_ptr(), T.data_ptr(), None))))
        L.check(lib.ronk_air_destroy(h))

    if what == "per":
        # ---- (2) the round constants as periodic columns against the same constants as base columns of M words
        import stark_fixed_programs as FP
        from ronkathon_amd.air import EXCEPT_LAST, FIRST, LAST, AirBuilder
        periodic = FP.round_constants(p)
        prog_per = FP.sbox_periodic_program()
        b = AirBuilder()          # the same program with base columns 3-5 in the place of the periodic columns
        s7 = []
        for c in range(3):
            t = b.base(c) + b.base(3 + c)
            t2 = t * t
            s7.append(t2 * t2 * t2 * t)
        for r in range(3):
            b.constrain(b.base(r, rot=1) - (AP.MDS3[r][0] * s7[0] + AP.MDS3[r][1] * s7[1] + AP.MDS3[r][2] * s7[2]), EXCEPT_LAST)
        b.constrain(b.base(0) - b.chal(0), FIRST)
        b.constrain(b.base(0) - b.chal(1), LAST)
        b.constrain(b.base(3, rot=1) - b.base(4))
        prog_base = AR.Program(*b.assemble())
        h_per, h_base = air_handle(dom, prog_per, (3,), 0, 2, periodic), air_handle(dom, prog_base, (3, 3), 0, 2)
        copies = max(2, min(16, (512 << 20) // (6 * 8 * M)))
        cols, consts = [rand(3 * M) for _ in range(copies)], [rand(3 * M) for _ in range(copies)]
        chal, lam = rand(4), rand(2 * prog_per.n_constraints)
        t_per = report({"op": "sbox with periodic constants", "ops": len(prog_per.ops), "column_bytes_per_row": 24, "table_words": 3 * 8 * 8},
                       event_ms(lambda k: L.check(lib.ronk_air_quotient_dev(h_per, pointers([cols[k % copies]]), None, chal.data_ptr(), lam.data_ptr(),
                                                                            None, T.data_ptr(), None))))
        t_base = report({"op": "sbox with the constants as base columns", "ops": len(prog_base.ops), "column_bytes_per_row": 48},
                        event_ms(lambda k: L.check(lib.ronk_air_quotient_dev(h_base, pointers([cols[k % copies], consts[k % copies]]), None,
                                                                             chal.data_ptr(), lam.data_ptr(), None, T.data_ptr(), None))))
        t_again = report({"op": "sbox with periodic constants (after)"},
                         event_ms(lambda k: L.check(lib.ronk_air_quotient_dev(h_per, pointers([cols[k % copies]]), None, chal.data_ptr(),
                                                                              lam.data_ptr(), None, T.data_ptr(), None))))
        emit({"op": "periodic over base columns", "ratio": round(min(t_per, t_again) / t_base, 4),
              "periodic_spread": round(abs(t_per - t_again) / min(t_per, t_again), 4), "bytes_per_row_periodic": 24 + 16, "bytes_per_row_base": 48 + 16})
        L.check(lib.ronk_air_destroy(h_per))
        L.check(lib.ronk_air_destroy(h_base))

    if what in ("air", "per"):
        L.check(lib.ronk_plonk_destroy(dom))

    if what == "gate":
        # ---- (3) the five selectors in the fixed round (this library) against eight columns in one trace round (the parent's)
        import poseidon_ref as PR
        import stark_fixed_programs as FP
        from ronkathon_amd.stark import Stark
        log2_n = log2_m - GATE_LOG2_B
        N = 1 << log2_n

        class F:
            ORDER = p
        par = PR.derive_params(p, 8, 7, 2, 4, 4)
        inst = FP.gate(p, N)
        sh = inst.shape
        sponge = (F,) + par.create_args()[1:]
        common = (sponge, g, w, log2_n, GATE_LOG2_B, shift, ETA, LOG2_FINAL, Q, D)
        fixed_form = not os.environ.get("RONK_LIB_PATH")
        wires, sel = np.array(inst.rounds[0], dtype=np.uint64), np.array(inst.fixed, dtype=np.uint64)
        d_seed, d_pub = dev(np.arange(1, D + 1, dtype=np.uint64)), dev(np.array([c for pair in inst.pub for c in pair], dtype=np.uint64))
        d_status = torch.zeros(1, dtype=torch.int32, device="cuda")
        if fixed_form:
            h = Stark(*common, sh.columns, sh.n_ext, sh.n_pub, sh.n_draw, tuple(sh.prog), n_fixed=5)
            d_trace, d_sel, d_fixed = dev(wires.ravel()), dev(sel.ravel()), empty(h.fixed_words)
            t_commit = report({"op": "stark_fixed_commit_dev: extension and tree of the five selectors, once", "fixed_mib": round(h.fixed_words * 8 / 2**20, 1)},
                              event_ms(lambda _k: h.fixed_commit_dev(d_sel, d_fixed)))
            h.set_fixed(d_fixed)
        else:
            h = Stark(*common, (8,), (0,), sh.n_pub, sh.n_draw, tuple(sh.prog))
            d_trace = dev(np.concatenate([sel.ravel(), wires.ravel()]))
        d_work, d_proof = empty(h.workspace_words), empty(h.proof_words)
        emit({"op": "sizes", "form": "fixed round of 5 + trace round of 3" if fixed_form else "one trace round of 8",
              "workspace_mib": round(h.workspace_words * 8 / 2**20, 1), "proof_words": h.proof_words})

        def prove(_k):
            h.prove_dev(d_seed, d_pub, d_trace, d_work, d_proof, d_status)

        prove(0)
        assert int(d_status.item()) == 0 and h.verify_dev(d_seed, d_pub, d_proof) == 0, "the proof of the valid trace is not accepted"
        t = report({"op": "stark_prove_dev gate (wall clock)"}, wall_ms(prove))
        if fixed_form:
            emit({"op": "the five selectors' extension and tree over a proof", "ratio": round(t_commit / t, 4)})
        h.close()
    out.close()


if __name__ == "__main__":
    if args.case:
        what, f, m, run = args.case.split(",")
        case(what, f, int(m), run)
    else:
        sys.exit(driver())
