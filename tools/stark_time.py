"""Times the STARK layer (ronk_stark_*) after warm-up, median of `rounds`, and in the same process, on the same device:
  (1) ronk_stark_prove_dev (hipEvents around `iters` back-to-back calls) and ronk_stark_verify_dev (wall clock: it synchronises);
  (2) the prover's stages, each issued alone through the entry point the handle itself calls, on the handle's shapes: extension
      (ronk_lde_batch_dev), trees (ronk_mpcs_commit_dev of the trace round and of the quotient round), quotient
      (ronk_air_quotient_dev), split + re-extension (the inverse transform of T's planes, ronk_stark_split_dev,
      ronk_rs_encode_batch_dev), opening (ronk_mpcs_open_dev);
  (3) the split kernel alone against ronk_vec_mul_dev on as many bytes (6 M words: the split reads 2 M and writes 4 M, the product
      of 2 M words reads 4 M and writes 2 M), inputs rotating over enough copies to exceed the 256 MiB Infinity Cache;
  (4) ronk_stark_prove_dev against the same stages issued through the entry points that existed before this family, with the
      un-shift and the split on the host as tests/test_gpu_air.py does them: T's coefficients copied to the host, multiplied by
      s^-j through the host form ronk_vec_mul (the table prepared outside the timed region), cut into pieces with numpy, scaled
      into the coset basis the same way, copied back and encoded.  That path has no transcript, which is in its favour.  Wall
      clock with a synchronisation at the end of each run, ordered A / B / A; the spread of the two A runs is recorded.
Traces are valid (the proof is verified once before anything is timed).  Every (field, size, program) case runs in a child
process of its own under a time limit, and the driver stops at the first case that fails.  One JSON line per measurement,
appended to --out.

usage: python tools/stark_time.py [--iters 5] [--warmup 1] [--rounds 3] [--log2-sizes 20,22] [--fields gl,mont]
                                  [--programs fibonacci,sbox_row] [--limit 400] [--out profiles/stark_time_mi355x.jsonl]"""
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
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log2-sizes", default="20,22")
ap.add_argument("--fields", default="gl,mont")
ap.add_argument("--programs", default="fibonacci,sbox_row")
ap.add_argument("--limit", type=int, default=400, help="seconds per case")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stark_time_mi355x.jsonl"))
ap.add_argument("--case", default=None, help="internal: field,log2_m,program of the one case this process runs")
args = ap.parse_args()

PRIMES = {"gl": (0xFFFFFFFF00000001, 7), "mont": (0xFFFFFFFC00000001, 10)}
LOG2_B = {"fibonacci": 2, "sbox_row": 3}
ETA, LOG2_FINAL, Q, D = 2, 4, 32, 4


def driver():
    for field in args.fields.split(","):
        for m in args.log2_sizes.split(","):
            for prog in args.programs.split(","):
                cmd = [sys.executable, os.path.abspath(__file__), "--case", "%s,%s,%s" % (field, m, prog), "--out", args.out]
                for k in ("iters", "warmup", "rounds"):
                    cmd += ["--" + k, str(getattr(args, k))]
                try:
                    rc = subprocess.run(cmd, timeout=args.limit).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:
                    print("case %s 2^%s %s ended with status %d: stopping" % (field, m, prog, rc), flush=True)
                    return rc
    return 0


def case(field, log2_m, name):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    import poseidon_ref as PR
    import stark_programs as SP
    from ronkathon_amd import _lib as L
    from ronkathon_amd.stark import Stark
    lib = L.lib
    p, w = PRIMES[field]
    g = shift = w
    log2_b = LOG2_B[name]
    log2_n = log2_m - log2_b
    N, B, M = 1 << log2_n, 1 << log2_b, 1 << log2_m
    base = {"field": field, "w": w, "log2_m": log2_m, "log2_blowup": log2_b, "program": name}
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

    def wall_ms(fn, iters=None):
        iters, ts = args.iters if iters is None else iters, []
        for _ in range(args.rounds):
            fn(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(iters):
                fn(k)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / iters)
        return ts

    def report(d, ts):
        med = float(np.median(ts))
        emit(dict(d, ms_median=round(med, 4), ms_all=[round(t, 4) for t in ts]))
        return med

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()

    def empty(words):
        return torch.empty(words, dtype=torch.int64, device="cuda")

    def P(t):
        return t.data_ptr()

    class F:
        ORDER = p
    par = PR.derive_params(p, 8, 7, 2, 4, 4)
    inst = getattr(SP, name)(p, N)
    sh = inst.shape
    Cn = sh.columns[0]
    h = Stark((F,) + par.create_args()[1:], g, w, log2_n, log2_b, shift, ETA, LOG2_FINAL, Q, D, sh.columns, sh.n_ext, sh.n_pub, sh.n_draw,
              tuple(sh.prog))
    trace = np.array(inst.rounds[0], dtype=np.uint64)
    d_trace, d_seed = dev(trace.ravel()), dev(np.arange(1, D + 1, dtype=np.uint64))
    d_pub = dev(np.array([c for pair in inst.pub for c in pair], dtype=np.uint64))
    d_work, d_proof = empty(h.workspace_words), empty(h.proof_words)
    d_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    emit({"op": "sizes", "workspace_mib": round(h.workspace_words * 8 / 2**20, 1), "proof_words": h.proof_words, "queries": Q, "digest_len": D,
          "log2_arity": ETA, "log2_final": LOG2_FINAL})

    # ---- (1) the whole prover and the verifier
    def prove(_k):
        h.prove_dev(d_seed, d_pub, d_trace, d_work, d_proof, d_status)

    prove(0)
    assert int(d_status.item()) == 0 and h.verify_dev(d_seed, d_pub, d_proof) == 0, "the proof of the valid trace is not accepted"
    t_prove = report({"op": "stark_prove_dev"}, event_ms(prove))
    report({"op": "stark_verify_dev (wall clock)"}, wall_ms(lambda _k: h.verify_dev(d_seed, d_pub, d_proof)))

    # ---- (2) the stages, each alone, through the entry points the handle calls
    pos = L.PoseidonHandle(*par.create_args())
    mp = L.MpcsHandle(pos, g, w, log2_m, shift, ETA, LOG2_FINAL, log2_b, Q, D, 2, (Cn, 2 * B), (3, 1))
    pk, pn, inv2, enc = L.Plan(p, g, log2_n, Cn), L.Plan(p, g, log2_m, Cn), L.Plan(p, g, log2_m, 2), L.Plan(p, g, log2_m, 2 * B)
    dom, air = C.c_void_p(), C.c_void_p()
    L.check(lib.ronk_plonk_create(C.byref(dom), p, g, w, log2_n, log2_b, shift, (C.c_uint64 * 3)(1, 2, 3)))
    prog = sh.prog
    ops, imm = (C.c_uint64 * len(prog.ops))(*prog.ops), (C.c_uint64 * max(1, len(prog.imm)))(*[v % p for v in prog.imm])
    L.check(lib.ronk_air_create(C.byref(air), dom, 1, (C.c_uint32 * 1)(Cn), 0, 2, len(prog.imm), prog.n_regs, prog.n_constraints, ops,
                                len(prog.ops), imm))
    d_co, d_ext, d_coef0 = empty(Cn * N), empty(Cn * M), empty(Cn * N)
    d_T, d_c, d_coefQ, d_msg, d_MQ = empty(2 * M), empty(2 * M), empty(2 * M), empty(2 * M), empty(2 * B * M)
    d_tree0, d_treeQ = empty(mp.tree_words), empty(mp.tree_words)
    d_lam = torch.randint(0, 2**62, (2 * prog.n_constraints,), dtype=torch.int64, device="cuda")
    d_z = torch.randint(1, 2**62, (4,), dtype=torch.int64, device="cuda")
    d_mwork, d_mproof = empty(mp.workspace_words), empty(mp.proof_words)
    d_mst = torch.zeros(1, dtype=torch.int32, device="cuda")
    base_ptrs = (C.c_void_p * 1)(P(d_ext))

    def extension(_k):
        L.check(lib.ronk_lde_batch_dev(pk.h, pn.h, P(d_trace), P(d_co), P(d_ext), shift, None))

    def trees(_k):
        mp.commit_dev(0, P(d_ext), P(d_tree0))
        mp.commit_dev(1, P(d_MQ), P(d_treeQ))

    def quotient(_k):
        L.check(lib.ronk_air_quotient_dev(air, base_ptrs, None, P(d_pub), P(d_lam), None, P(d_T), None))

    def split_extend(_k):
        L.check(lib.ronk_ntt_inverse_dev(inv2.h, P(d_T), P(d_c), None))
        h.split(d_c, d_coefQ, d_msg, stream=0)
        L.check(lib.ronk_rs_encode_batch_dev(enc.h, P(d_msg), N, P(d_MQ), None))

    def opening(_k):
        mp.open_dev([P(d_ext), P(d_MQ)], [P(d_tree0), P(d_treeQ)], [P(d_coef0), P(d_coefQ)], P(d_z), P(d_seed), P(d_mwork), P(d_mproof), P(d_mst))

    L.check(lib.ronk_ntt_inverse_dev(pk.h, P(d_trace), P(d_coef0), None))
    extension(0); quotient(0); split_extend(0); trees(0)
    stage_sum = 0.0
    for label, fn in (("extension", extension), ("trees", trees), ("quotient", quotient), ("split + re-extension", split_extend), ("opening", opening)):
        stage_sum += report({"op": "stage: " + label}, event_ms(fn))
    emit({"op": "stages over prove_dev", "stage_sum_ms": round(stage_sum, 4), "ratio": round(stage_sum / t_prove, 3)})

    # ---- (3) the split kernel alone against the element-wise product on as many bytes
    copies = max(2, min(8, (512 << 20) // (6 * 8 * M)))
    cs = [torch.randint(-2**63, 2**63 - 1, (2 * M,), dtype=torch.int64, device="cuda") for _ in range(copies)]
    o1, o2 = [empty(2 * M) for _ in range(copies)], [empty(2 * M) for _ in range(copies)]
    t_split = report({"op": "stark_split_dev", "bytes": 48 * M}, event_ms(lambda k: h.split(cs[k % copies], o1[k % copies], o2[k % copies], stream=0)))
    t_mul = report({"op": "vec_mul_dev on as many bytes", "bytes": 48 * M},
                   event_ms(lambda k: L.check(lib.ronk_vec_mul_dev(p, P(cs[k % copies]), P(o1[k % copies]), P(o2[k % copies]), 2 * M, None))))
    emit({"op": "split over vec_mul", "ratio": round(t_split / t_mul, 3), "split_gb_per_s": round(48 * M / t_split / 1e6, 1),
          "vec_mul_gb_per_s": round(48 * M / t_mul / 1e6, 1)})
    del cs, o1, o2

    # ---- (4) the whole prover against the stages with the un-shift and the split on the host, A / B / A
    sinv = pow(shift, -1, p)
    table = np.empty(M, dtype=np.uint64)
    x = 1
    for j in range(M):
        table[j] = x
        x = x * sinv % p
    unshift = np.concatenate([table, table])
    up = np.empty(N, dtype=np.uint64)
    x = 1
    for k in range(N):
        up[k] = x
        x = x * shift % p
    to_coset = np.tile(up, 2 * B)
    h_c, h_coef, h_msg = np.empty(2 * M, dtype=np.uint64), np.empty(2 * M, dtype=np.uint64), np.empty(2 * M, dtype=np.uint64)

    one = L.Plan(p, g, log2_m, 1)

    def parent(_k):
        extension(0)
        mp.commit_dev(0, P(d_ext), P(d_tree0))
        quotient(0)
        for plane in (0, 1):
            L.check(lib.ronk_ntt_inverse_dev(one.h, P(d_T) + 8 * plane * M, P(d_c) + 8 * plane * M, None))
        L.check(lib.ronk_memcpy_d2h(L.ptr(h_c), P(d_c), 16 * M))
        L.check(lib.ronk_vec_mul(p, L.ptr(h_c), L.ptr(unshift), L.ptr(h_coef), 2 * M))
        pieces = np.ascontiguousarray(h_coef.reshape(2, B, N).transpose(1, 0, 2)).ravel()
        L.check(lib.ronk_vec_mul(p, L.ptr(pieces), L.ptr(to_coset), L.ptr(h_msg), 2 * M))
        L.check(lib.ronk_memcpy_h2d(P(d_coefQ), L.ptr(pieces), 16 * M))
        L.check(lib.ronk_memcpy_h2d(P(d_msg), L.ptr(h_msg), 16 * M))
        L.check(lib.ronk_rs_encode_batch_dev(enc.h, P(d_msg), N, P(d_MQ), None))
        mp.commit_dev(1, P(d_MQ), P(d_treeQ))
        opening(0)

    # the host path gives the device split's words
    split_extend(0)
    torch.cuda.synchronize()
    want = d_coefQ.clone(), d_MQ.clone()
    parent(0)
    torch.cuda.synchronize()
    assert torch.equal(d_coefQ, want[0]) and torch.equal(d_MQ, want[1]), "the host split and the device split differ"
    a0 = report({"op": "A: stark_prove_dev (wall clock, before)"}, wall_ms(prove))
    b = report({"op": "B: parent entry points with the host un-shift and split (wall clock)"}, wall_ms(parent, iters=max(1, args.iters // 2)))
    a1 = report({"op": "A: stark_prove_dev (wall clock, after)"}, wall_ms(prove))
    emit({"op": "prove_dev over the parent path", "ratio_before": round(a0 / b, 4), "ratio_after": round(a1 / b, 4),
          "a_spread": round(abs(a0 - a1) / min(a0, a1), 4), "prove_dev_is_faster": bool(max(a0, a1) < b)})
    L.check(lib.ronk_air_destroy(air))
    L.check(lib.ronk_plonk_destroy(dom))
    mp.close()
    pos.close()
    h.close()
    out.close()


if __name__ == "__main__":
    if args.case:
        f, m, prog = args.case.split(",")
        case(f, int(m), prog)
    else:
        sys.exit(driver())
