"""Times the constraint-program quotient (ronk_air_quotient_dev) with hipEvents around `iters` back-to-back calls after warm-up, median
of `rounds`, and in the same process, on the same device:
  (1) the PLONK quotient written as a program (tests/air_programs.py plonk) against the fused ronk_plonk_quotient_dev on the same
      columns: the price of the interpreter.  No bar; the ratio is recorded.
  (2) a custom program -- a width-3 x^7 S-box row with a linear layer (EXCEPT_LAST), one FIRST and one LAST constraint
      (tests/air_programs.py sbox_row) -- against the same ops issued one pass per op through ronk_vec_* / ronk_ext2_vec_* on [M]
      arrays, the per-row Fermat inversions of x - 1 and x - w_l included (ronk_vec_inv_dev).  What does not depend on the call is
      prepared OUTSIDE the timed region in the composition's favour: the rotated copies of the columns, the arrays of x_i, of
      1 / (x_i^N - 1), of the immediates, the challenges and the weights.  The composition is timed before and after the fused
      launch (A / B / A); the fused launch must be faster than both.
Inputs rotate over enough copies to exceed the 256 MiB Infinity Cache.  Every (field, size) case runs in a child process of its own
under a time limit, and the driver stops at the first case that fails.  One JSON line per measurement, appended to --out.

usage: python tools/air_time.py [--iters 10] [--warmup 2] [--rounds 3] [--log2-sizes 20,22] [--log2-blowup 2] [--fields gl,mont]
                                [--limit 240] [--out profiles/air_time_mi355x.jsonl]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log2-sizes", default="20,22")
ap.add_argument("--log2-blowup", type=int, default=2)
ap.add_argument("--fields", default="gl,mont")
ap.add_argument("--limit", type=int, default=240, help="seconds per (field, size) case")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "air_time_mi355x.jsonl"))
ap.add_argument("--case", default=None, help="internal: field,log2_m of the one case this process runs")
args = ap.parse_args()

PRIMES = {"gl": (0xFFFFFFFF00000001, 7), "mont": (0xFFFFFFFC00000001, 10)}


def driver():
    for field in args.fields.split(","):
        for m in args.log2_sizes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--case", "%s,%s" % (field, m), "--out", args.out]
            for k in ("iters", "warmup", "rounds", "log2_blowup"):
                cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print("case %s 2^%s ended with status %d: stopping" % (field, m, rc), flush=True)
                return rc
    return 0


def case(field, log2_m):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    import air_programs as AP
    import air_ref as AR
    from ronkathon_amd import _lib as L
    lib = L.lib
    p, w = PRIMES[field]
    g = w
    M, log2_b = 1 << log2_m, args.log2_blowup
    B, N = 1 << log2_b, M >> log2_b
    base = {"field": field, "w": w, "log2_m": log2_m, "log2_blowup": log2_b}
    out = open(args.out, "a")

    def emit(d):
        line = json.dumps(dict(base, **d))
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def time_ms(fn):
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

    def report(d, ts):
        med = float(np.median(ts))
        emit(dict(d, ms_median=round(med, 4), ms_all=[round(t, 4) for t in ts]))
        return med

    def rand(words):
        return torch.randint(-2**63, 2**63 - 1, (words,), dtype=torch.int64, device="cuda")

    def empty(words):
        return torch.empty(words, dtype=torch.int64, device="cuda")

    def const(v, words=M):
        return torch.full((words,), v - 2**64 if v >= 2**63 else v, dtype=torch.int64, device="cuda")

    def pointers(tensors):
        return (C.c_void_p * max(1, len(tensors)))(*[t.data_ptr() for t in tensors])

    def handle(prog, groups, n_ext, n_chal):
        h = C.c_void_p()
        ops, imm = (C.c_uint64 * len(prog.ops))(*prog.ops), (C.c_uint64 * max(1, len(prog.imm)))(*[v % p for v in prog.imm])
        L.check(lib.ronk_air_create(C.byref(h), dom, len(groups), (C.c_uint32 * len(groups))(*groups), n_ext, n_chal, len(prog.imm),
                                    prog.n_regs, prog.n_constraints, ops, len(prog.ops), imm))
        return h

    torch.manual_seed(1)
    dom = C.c_void_p()
    L.check(lib.ronk_plonk_create(C.byref(dom), p, g, w, log2_m - log2_b, log2_b, g, (C.c_uint64 * 3)(1, 2, 3)))
    T = empty(2 * M)

    # ---- (1) the PLONK quotient: fused kernel against the same constraints as a program, 14 M words of input per copy
    copies = max(2, min(8, (512 << 20) // (14 * 8 * M)))
    sets = [tuple(rand(k * M) for k in (3, 5, 3, 1, 2)) for _ in range(copies)]
    alpha, beta, gamma = (rand(2) for _ in range(3))
    prog = AP.plonk()
    h = handle(prog, (3, 5, 3, 1), 1, 2)
    chal, lam = torch.cat([beta, gamma]), rand(6)

    def fused_plonk(k):
        a, q, s, pi, Z = sets[k % copies]
        L.check(lib.ronk_plonk_quotient_dev(dom, a.data_ptr(), q.data_ptr(), s.data_ptr(), pi.data_ptr(), Z.data_ptr(), alpha.data_ptr(),
                                            beta.data_ptr(), gamma.data_ptr(), T.data_ptr(), None))

    def program_plonk(k):
        s = sets[k % copies]
        L.check(lib.ronk_air_quotient_dev(h, pointers(s[:4]), pointers(s[4:]), chal.data_ptr(), lam.data_ptr(), None, T.data_ptr(), None))

    t_f0 = report({"op": "plonk_quotient_dev"}, time_ms(fused_plonk))
    t_p = report({"op": "air_quotient_dev plonk program", "ops": len(prog.ops), "n_regs": prog.n_regs}, time_ms(program_plonk))
    t_f1 = report({"op": "plonk_quotient_dev (after)"}, time_ms(fused_plonk))
    emit({"op": "plonk program over the fused plonk quotient", "ratio": round(t_p / min(t_f0, t_f1), 2)})
    L.check(lib.ronk_air_destroy(h))
    del sets

    # ---- (2) the S-box row: one launch against one pass per op
    prog = AP.sbox_row()
    h = handle(prog, (3,), 0, 2)
    copies = max(2, min(16, (512 << 20) // (3 * 8 * M)))
    cols = [rand(3 * M) for _ in range(copies)]
    chal, lam, T_in = rand(4), rand(2 * prog.n_constraints), rand(2 * M)

    def fused(k):
        L.check(lib.ronk_air_quotient_dev(h, pointers([cols[k % copies]]), None, chal.data_ptr(), lam.data_ptr(), T_in.data_ptr(), T.data_ptr(), None))

    # what the composition may prepare once: rotated copies, x_i, 1 / (x_i^N - 1), broadcast constants
    wM = pow(g, (p - 1) // M, p)
    wl = pow(pow(wM, B, p), -1, p)
    ninv = pow(N, -1, p)
    xs = np.empty(M, dtype=np.uint64)
    x = g % p
    for i in range(M):
        xs[i] = x
        x = x * wM % p
    d_x = torch.from_numpy(xs.view(np.int64)).cuda()
    sN, wB = pow(g, N, p), pow(wM, N, p)
    vinv = np.array([pow((sN * pow(wB, j, p) - 1) % p, -1, p) for j in range(B)], dtype=np.uint64)
    d_vinv = torch.from_numpy(np.tile(vinv, N).view(np.int64)).cuda()
    rolled = [{r: torch.roll(c.view(3, M), -r * B, 1).contiguous() for r in (0, 1)} for c in cols]
    d_imm = [const(v % p) for v in prog.imm]
    hc, hl = chal.cpu().numpy().view(np.uint64), lam.cpu().numpy().view(np.uint64)
    d_chal = [torch.cat([const(int(hc[2 * k])), const(int(hc[2 * k + 1]))]) for k in range(2)]
    d_lam = [torch.cat([const(int(hl[2 * j])), const(int(hl[2 * j + 1]))]) for j in range(prog.n_constraints)]
    d_one, d_wl, d_ninv, d_wln, zero = const(1), const(wl), const(ninv), const(wl * ninv % p), torch.zeros(M, dtype=torch.int64, device="cuda")
    regs = [empty(2 * M) for _ in range(prog.n_regs)]
    acc = [empty(2 * M) for _ in range(4)]
    tmp, tmp2, emb, d1, d2 = empty(2 * M), empty(2 * M), empty(2 * M), empty(M), empty(M)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    passes = [0]

    def P(t):
        return t.data_ptr()

    def vec(name, *a):
        passes[0] += 1
        L.check(getattr(lib, name)(*a, None))

    def composed(k):
        passes[0] = 0
        kind_of = [None] * prog.n_regs            # 0 base, 1 ext
        for a in acc:
            a.zero_()

        def read(o):
            kind, index, rot = AR.decode(o)
            if kind == AR.REG:
                return regs[index], kind_of[index]
            if kind == AR.BASE:
                return rolled[k % copies][rot][index], 0
            if kind == AR.CHAL:
                return d_chal[index], 1
            if kind == AR.IMM:
                return d_imm[index], 0
            return d_x, 0

        def embed(t):
            emb[:M].copy_(t)
            emb[M:].zero_()
            passes[0] += 1
            return emb

        for word in prog.ops:
            code, dst = word & 0xFF, (word >> 8) & 0xFF
            a, ta = read((word >> 16) & 0xFFFFFF)
            if code == AR.EMIT:
                j = (word >> 40) & 0xFFFFFF
                if ta:
                    vec("ronk_ext2_vec_mul_dev", p, w, P(d_lam[j]), P(a), P(tmp), M)
                else:
                    vec("ronk_ext2_vec_mul_base_dev", p, w, P(d_lam[j]), P(a), P(tmp), M)
                vec("ronk_ext2_vec_add_dev", p, w, P(acc[dst]), P(tmp), P(acc[dst]), M)
                continue
            assert code in (AR.ADD, AR.SUB, AR.MUL), "the builder writes no MOV, and this program has no NEG"
            b, tb = read((word >> 40) & 0xFFFFFF)
            name = {AR.ADD: "add", AR.SUB: "sub", AR.MUL: "mul"}[code]
            if not ta and not tb:
                vec("ronk_vec_%s_dev" % name, p, P(a), P(b), P(regs[dst]), M)
            elif code == AR.MUL and ta != tb:
                e, s = (a, b) if ta else (b, a)
                vec("ronk_ext2_vec_mul_base_dev", p, w, P(e), P(s), P(regs[dst]), M)
            else:
                a, b = a if ta else embed(a), b if tb else embed(b)
                vec("ronk_ext2_vec_%s_dev" % name, p, w, P(a), P(b), P(regs[dst]), M)
            kind_of[dst] = ta | tb
        # the divisors: (acc0 + acc3 (x - w_l)) / (x^N - 1) + acc1 / (N (x - 1)) + acc2 w_l / (N (x - w_l)) + T_in
        vec("ronk_vec_sub_dev", p, P(d_x), P(d_wl), P(d2), M)
        vec("ronk_ext2_vec_mul_base_dev", p, w, P(acc[3]), P(d2), P(tmp), M)
        vec("ronk_ext2_vec_add_dev", p, w, P(acc[0]), P(tmp), P(tmp), M)
        vec("ronk_ext2_vec_mul_base_dev", p, w, P(tmp), P(d_vinv), P(tmp), M)
        vec("ronk_vec_sub_dev", p, P(d_x), P(d_one), P(d1), M)
        passes[0] += 2
        L.check(lib.ronk_vec_inv_dev(p, P(d1), P(d1), M, st.data_ptr(), None))
        L.check(lib.ronk_vec_inv_dev(p, P(d2), P(d2), M, st.data_ptr(), None))
        vec("ronk_vec_mul_dev", p, P(d1), P(d_ninv), P(d1), M)
        vec("ronk_vec_mul_dev", p, P(d2), P(d_wln), P(d2), M)
        vec("ronk_ext2_vec_mul_base_dev", p, w, P(acc[1]), P(d1), P(tmp2), M)
        vec("ronk_ext2_vec_add_dev", p, w, P(tmp), P(tmp2), P(tmp), M)
        vec("ronk_ext2_vec_mul_base_dev", p, w, P(acc[2]), P(d2), P(tmp2), M)
        vec("ronk_ext2_vec_add_dev", p, w, P(tmp), P(tmp2), P(tmp), M)
        vec("ronk_ext2_vec_add_dev", p, w, P(tmp), P(T_in), P(T), M)

    # the two agree before either is timed
    composed(0)
    want = T.clone()
    fused(0)
    torch.cuda.synchronize()
    assert torch.equal(T, want), "the composition and the fused launch differ"
    t_c0 = report({"op": "sbox composition (before)", "passes": passes[0]}, time_ms(composed))
    t_f = report({"op": "air_quotient_dev sbox program", "ops": len(prog.ops), "n_regs": prog.n_regs}, time_ms(fused))
    t_c1 = report({"op": "sbox composition (after)", "passes": passes[0]}, time_ms(composed))
    emit({"op": "sbox fused over composition", "ratio_before": round(t_f / t_c0, 4), "ratio_after": round(t_f / t_c1, 4),
          "composition_spread": round(abs(t_c0 - t_c1) / min(t_c0, t_c1), 4), "fused_is_faster": bool(t_f < min(t_c0, t_c1))})
    L.check(lib.ronk_air_destroy(h))
    L.check(lib.ronk_plonk_destroy(dom))
    out.close()


if __name__ == "__main__":
    if args.case:
        f, m = args.case.split(",")
        case(f, int(m))
    else:
        sys.exit(driver())
