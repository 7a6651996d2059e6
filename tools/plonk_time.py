"""Times the fused PLONK quotient (ronk_plonk_quotient_dev) with hipEvents around `iters` back-to-back calls after warm-up, median of
`rounds`, and in the same run, on the same device:
  (a) ronk_vec_mul_dev on as many bytes as the quotient moves by the estimate 152 M (136 read, 16 written per row): the streaming
      yardstick of tools/accum_time.py;
  (b) ronk_deep_combine_dev at C = 16 columns and K = 2 points, which moves the same 144 bytes per point (16 words read, 2 written)
      through a lane of the same shape (four points at stride N / 4, one inversion).
Inputs rotate over enough copies to exceed the 256 MiB Infinity Cache.  Every (field, size) case runs in a child process of its own
under a time limit, and the driver stops at the first case that fails.  One JSON line per measurement, appended to --out.

usage: python tools/plonk_time.py [--iters 10] [--warmup 2] [--rounds 3] [--log2-sizes 20,22] [--log2-blowup 2] [--fields gl,mont]
                                  [--limit 240] [--out profiles/plonk_time_mi355x.jsonl]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_time_mi355x.jsonl"))
ap.add_argument("--case", default=None, help="internal: field,log2_m of the one case this process runs")
args = ap.parse_args()

PRIMES = {"gl": (0xFFFFFFFF00000001, 7), "mont": (0xFFFFFFFC00000001, 10)}
BYTES_PER_ROW = 152      # 17 words read (a, b, o, five selectors, three sigma, pi, Z and Z at the next row: two planes each), 2 written


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

    import poseidon_ref as PR      # the derivation of the Poseidon parameters the commitment handle wants
    from ronkathon_amd import _lib as L
    lib = L.lib
    p, w = PRIMES[field]
    g = w
    M, log2_b = 1 << log2_m, args.log2_blowup
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
        d = dict(d, ms_median=round(med, 4), ms_all=[round(t, 4) for t in ts])
        if "bytes" in d:
            d["TBs"] = round(d["bytes"] / (med * 1e-3) / 1e12, 3)
        emit(d)
        return med

    def rand(words):
        """random 64-bit words made on the device"""
        return torch.randint(-2**63, 2**63 - 1, (words,), dtype=torch.int64, device="cuda")

    def empty(words):
        return torch.empty(words, dtype=torch.int64, device="cuda")

    torch.manual_seed(1)
    # ---- the quotient: 14 M words of input per copy
    copies = max(2, min(8, (512 << 20) // (14 * 8 * M)))
    sets = [tuple(rand(k * M) for k in (3, 5, 3, 1, 2)) for _ in range(copies)]
    ch = [rand(2) for _ in range(3)]
    T = empty(2 * M)
    h = C.c_void_p()
    L.check(lib.ronk_plonk_create(C.byref(h), p, g, w, log2_m - log2_b, log2_b, g, (C.c_uint64 * 3)(1, 2, 3)))

    def quotient(k, with_pi=True):
        a, q, s, pi, Z = sets[k % copies]
        L.check(lib.ronk_plonk_quotient_dev(h, a.data_ptr(), q.data_ptr(), s.data_ptr(), pi.data_ptr() if with_pi else None, Z.data_ptr(),
                                            ch[0].data_ptr(), ch[1].data_ptr(), ch[2].data_ptr(), T.data_ptr(), None))

    est = BYTES_PER_ROW * M
    t_q = report({"op": "plonk_quotient_dev", "bytes": est, "bytes_per_row_estimate": BYTES_PER_ROW}, time_ms(quotient))
    report({"op": "plonk_quotient_dev_no_pi", "bytes": est - 8 * M, "bytes_per_row_estimate": BYTES_PER_ROW - 8},
           time_ms(lambda k: quotient(k, False)))
    L.check(lib.ronk_plonk_destroy(h))
    del sets
    # (a) the streaming yardstick: as many bytes through ronk_vec_mul_dev (two reads and a write of 8 bytes per element)
    m = est // 24
    ya, yb, yo = rand(m), rand(m), empty(m)
    t_mul = report({"op": "vec_mul_dev", "elements": m, "bytes": 24 * m},
                   time_ms(lambda k: L.check(lib.ronk_vec_mul_dev(p, ya.data_ptr(), yb.data_ptr(), yo.data_ptr(), m, None))))
    del ya, yb, yo
    # (b) the DEEP combination of a [16][M] matrix at two points: 16 words read and 2 written per point
    Cc, K = 16, 2
    P = PR.derive_params(p, 12, 7, 22, 8, 8)
    pos = L.PoseidonHandle(*P.create_args())
    eta = 3
    log2_final = log2_m - eta * max(1, -(-(log2_m - 8) // eta))
    pcs = L.PcsHandle(pos, g, w, log2_m, 1, eta, log2_final, min(2, log2_final), 64, 4, Cc, K)
    copies = max(2, min(8, (512 << 20) // (8 * M * Cc)))
    mats = [rand(Cc * M) for _ in range(copies)]
    d_y, d_z, d_alpha, G = rand(2 * K * Cc), rand(2 * K), rand(2), empty(2 * M)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_deep = report({"op": "deep_combine_dev", "columns": Cc, "points": K, "bytes": (Cc + 2) * 8 * M},
                    time_ms(lambda k: pcs.combine_dev(mats[k % copies].data_ptr(), d_y.data_ptr(), d_z.data_ptr(), d_alpha.data_ptr(),
                                                      G.data_ptr(), st.data_ptr())))
    emit({"op": "plonk_quotient_against_yardsticks", "quotient_over_vec_mul_same_bytes": round(t_q / t_mul, 2),
          "quotient_over_deep_combine": round(t_q / t_deep, 2)})
    pcs.close()
    out.close()


if __name__ == "__main__":
    if args.case:
        f, m = args.case.split(",")
        case(f, int(m))
    else:
        sys.exit(driver())
