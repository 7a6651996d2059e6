"""Times proof-of-work grinding (ronk_pow_grind_dev) at the README's Poseidon parameters (width 12, alpha 7, 8 + 22 rounds, rate 8)
and what it adds to the FRI prover and the batched commitment, with hipEvents on the device:
  permute   ronk_poseidon_permute_dev on 2^22 states: the yardstick, in permutations per second.  With --parent-lib it is also
            measured on another build of the library (the parent commit's) in a process of its own in the same run.
  grind     b = 20 and 24 over 8 seeds: candidates per second taken as (nonce + 1) / time, summed over the seeds, for max_lanes = 0
            (the library's default) and for fixed lane counts around it; b = 12, where the default exceeds 2^b, against b = 0 (two
            launches and nothing to search): the time the overshoot costs.
  fri, pcs  ronk_fri_prove_dev and ronk_pcs_open_dev at 2^22 (arity 8, 64 queries, blowup 4) with b = 0 and b = 20; with
            --parent-lib also on the other build (b = 0 only: it has no grinding).
Every case runs in a child process of its own under a time limit, and the driver stops at the first case that fails.  One JSON line
per measurement, appended to --out.

usage: python tools/pow_time.py [--iters 5] [--warmup 1] [--rounds 3] [--fields gl,mont] [--cases permute,grind,fri,pcs] [--log2-n 22]
                                [--parent-lib PATH] [--limit 240] [--out profiles/pow_time_mi355x.jsonl]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--fields", default="gl,mont")
ap.add_argument("--cases", default="permute,grind,fri,pcs")
ap.add_argument("--log2-n", type=int, default=22)
ap.add_argument("--lanes", default="0,114688,229376,458752,917504", help="max_lanes values of the grind case (0: the library's default)")
ap.add_argument("--parent-lib", default="", help="another build of libronk_ntt.so: permute, fri and pcs are measured on it too")
ap.add_argument("--limit", type=int, default=240, help="seconds per case")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pow_time_mi355x.jsonl"))
ap.add_argument("--case", default=None, help="internal: name,field,label of the one case this process runs")
args = ap.parse_args()

PRIMES = {"gl": (0xFFFFFFFF00000001, 7), "mont": (0xFFFFFFFC00000001, 10)}
SEEDS, DIGEST, QUERIES, ETA, BLOWUP = 8, 4, 64, 3, 2


def driver():
    for field in args.fields.split(","):
        for name in args.cases.split(","):
            libs = [("this", "")]
            if args.parent_lib and name != "grind":
                libs.insert(0, ("parent", os.path.abspath(args.parent_lib)))
            for label, path in libs:
                cmd = [sys.executable, os.path.abspath(__file__), "--case", "%s,%s,%s" % (name, field, label), "--out", args.out,
                       "--lanes", args.lanes]
                for k in ("iters", "warmup", "rounds", "log2_n"):
                    cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
                env = dict(os.environ)
                if path:
                    env["RONK_LIB_PATH"] = path
                try:
                    rc = subprocess.run(cmd, timeout=args.limit, env=env).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:
                    print("case %s %s (%s) ended with status %d: stopping" % (name, field, label, rc), flush=True)
                    return rc
    return 0


def case(name, field, label):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    import poseidon_ref as PR      # the derivation of the Poseidon parameters
    from ronkathon_amd import _lib as L
    p, g = PRIMES[field]
    base = {"field": field, "lib": label, "case": name}
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

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()

    def rand(words):
        return torch.randint(-2**63, 2**63 - 1, (words,), dtype=torch.int64, device="cuda")

    torch.manual_seed(1)
    P = PR.derive_params(p, 12, 7, 22, 8, 8)
    pos = L.PoseidonHandle(*P.create_args())
    has_pow = hasattr(L.lib, "ronk_pow_grind_dev")

    if name == "permute":
        count = 1 << 22
        states = rand(count * 12)
        ts = time_ms(lambda k: pos.permute_dev(states.data_ptr(), count))
        med = float(np.median(ts))
        emit({"op": "poseidon_permute_dev", "states": count, "ms_median": round(med, 4), "ms_all": [round(t, 4) for t in ts],
              "Mperm_s": round(count / (med * 1e-3) / 1e6, 1)})

    elif name == "grind":
        rng = np.random.default_rng(7)
        seeds = [dev(rng.integers(0, 2**63, size=DIGEST, dtype=np.uint64) % np.uint64(p)) for _ in range(SEEDS)]
        work = torch.empty(L.lib.ronk_pow_workspace_words(), dtype=torch.int64, device="cuda")
        nonce = torch.zeros(1, dtype=torch.int64, device="cuda")

        def grind(seed, bits, lam, lanes):
            """-> (nonce, ms) of one call, prefix and search"""
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            pos.pow_grind_dev(seed.data_ptr(), DIGEST, bits, lam, lanes, work.data_ptr(), nonce.data_ptr())
            b.record()
            b.synchronize()
            return int(nonce.cpu().numpy().view(np.uint64)[0]), a.elapsed_time(b)

        grind(seeds[0], 12, 18, 0)   # the first launch of the kernels
        for bits in (20, 24):
            for lanes in (int(v) for v in args.lanes.split(",")):
                runs = [grind(s, bits, bits + 6, lanes) for s in seeds]
                cand, ms = sum(n + 1 for n, _ in runs), sum(t for _, t in runs)
                emit({"op": "pow_grind_dev", "bits": bits, "log2_limit": bits + 6, "max_lanes": lanes, "seeds": SEEDS,
                      "nonces": [n for n, _ in runs], "ms": [round(t, 4) for _, t in runs], "candidates": cand,
                      "Mcand_s": round(cand / (ms * 1e-3) / 1e6, 1)})
        for bits in (0, 12):
            runs = [grind(s, bits, 18, 0) for s in seeds for _ in range(3)]
            emit({"op": "pow_grind_dev_small", "bits": bits, "log2_limit": 18, "max_lanes": 0, "ms_median": round(float(np.median([t for _, t in runs])), 4),
                  "nonce_max": max(n for n, _ in runs)})

    elif name in ("fri", "pcs"):
        n = args.log2_n
        log2_final = n - ETA * max(1, -(-(n - 8) // ETA))
        blow = min(BLOWUP, log2_final)
        N = 1 << n
        shape = {"log2_n": n, "eta": ETA, "log2_final": log2_final, "queries": QUERIES, "digest": DIGEST}
        seed = dev(np.arange(1, DIGEST + 1, dtype=np.uint64))
        for bits in (0, 20) if has_pow else (0,):
            if name == "fri":
                h = L.FriHandle(pos, g, n, g, ETA, log2_final, blow, QUERIES, DIGEST)
                if bits:
                    h.set_pow(bits)
                evals = [rand(N) for _ in range(4)]
                work, proof = torch.empty(h.workspace_words, dtype=torch.int64, device="cuda"), torch.empty(h.proof_words, dtype=torch.int64, device="cuda")
                ts = time_ms(lambda k: h.prove_dev(evals[k % 4].data_ptr(), seed.data_ptr(), work.data_ptr(), proof.data_ptr()))
                emit(dict(shape, op="fri_prove_dev", pow_bits=bits, ms_median=round(float(np.median(ts)), 4), ms_all=[round(t, 4) for t in ts]))
            else:
                C_, K_ = 16, 2
                h = L.PcsHandle(pos, g, g, n, 1, ETA, log2_final, blow, QUERIES, DIGEST, C_, K_)
                if bits:
                    h.set_pow(bits)
                M, coef, z = rand(C_ * N), rand(C_ * (N >> blow)), rand(2 * K_)
                tree = torch.empty(h.tree_words, dtype=torch.int64, device="cuda")
                h.commit_dev(M.data_ptr(), tree.data_ptr())
                work, proof = torch.empty(h.workspace_words, dtype=torch.int64, device="cuda"), torch.empty(h.proof_words, dtype=torch.int64, device="cuda")
                st = torch.zeros(1, dtype=torch.int32, device="cuda")
                ts = time_ms(lambda k: h.open_dev(M.data_ptr(), tree.data_ptr(), coef.data_ptr(), z.data_ptr(), seed.data_ptr(), work.data_ptr(),
                                                  proof.data_ptr(), st.data_ptr()))
                emit(dict(shape, op="pcs_open_dev", columns=C_, points=K_, pow_bits=bits, ms_median=round(float(np.median(ts)), 4),
                          ms_all=[round(t, 4) for t in ts]))
            h.close()
            del work, proof
    pos.close()
    out.close()


if __name__ == "__main__":
    if args.case:
        nm, f, lb = args.case.split(",")
        case(nm, f, lb)
    else:
        sys.exit(driver())
