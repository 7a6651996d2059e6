"""Times the scans and accumulators (ronk_vec_prefix_*_dev, ronk_ext2_vec_prefix_*_dev, ronk_perm_product_dev at W = 3,
ronk_logup_sum_dev at C = 2) with hipEvents around `iters` back-to-back calls after warm-up, median of `rounds`, and in the same
run, on the same buffers:
  (a) ronk_vec_mul_dev on as many bytes as the permutation product moves by the estimate (24 W + 48) N: the streaming yardstick;
  (b) the permutation terms composed from the element-wise entry points the library had before (per column ronk_ext2_vec_mul_base_dev,
      _add_dev, _mul_dev; one ronk_ext2_vec_inv_dev; the broadcast constants are prepared outside the timed region), followed by the
      new exclusive scan; its column is compared with the fused one.
Inputs rotate over enough copies to exceed the 256 MiB Infinity Cache.  Every (field, size) case runs in a child process of its own
under a time limit, and the driver stops at the first case that fails.  One JSON line per measurement, appended to --out.

usage: python tools/accum_time.py [--iters 10] [--warmup 2] [--rounds 3] [--log2-sizes 20,22] [--fields gl,mont] [--limit 240]
                                  [--out profiles/accum_time_mi355x.jsonl]"""
import argparse
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
ap.add_argument("--fields", default="gl,mont")
ap.add_argument("--columns", type=int, default=3)
ap.add_argument("--lookup-columns", type=int, default=2)
ap.add_argument("--limit", type=int, default=240, help="seconds per (field, size) case")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_time_mi355x.jsonl"))
ap.add_argument("--case", default=None, help="internal: field,log2_n of the one case this process runs")
args = ap.parse_args()

PRIMES = {"gl": (0xFFFFFFFF00000001, 7), "mont": (0xFFFFFFFC00000001, 10)}


def driver():
    for field in args.fields.split(","):
        for n in args.log2_sizes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--case", "%s,%s" % (field, n), "--out", args.out]
            for k in ("iters", "warmup", "rounds", "columns", "lookup_columns"):
                cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print("case %s 2^%s ended with status %d: stopping" % (field, n, rc), flush=True)
                return rc
    return 0


def case(field, n):
    sys.path.insert(0, ROOT)
    import torch

    from ronkathon_amd import _lib as L
    lib = L.lib
    p, w = PRIMES[field]
    N, W, C = 1 << n, args.columns, args.lookup_columns
    base = {"field": field, "w": w, "log2_n": n}
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
            d["GBs"] = round(d["bytes"] / (med * 1e-3) / 1e9, 1)
        emit(d)
        return med

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()

    def empty(words):
        return torch.empty(words, dtype=torch.int64, device="cuda")

    def const_planar(e):
        t = empty(2 * N)
        t[:N] = int(np.array([e[0]], dtype=np.uint64).view(np.int64)[0])
        t[N:] = int(np.array([e[1]], dtype=np.uint64).view(np.int64)[0])
        return t

    rng = np.random.default_rng(1)
    work = empty(lib.ronk_scan_workspace_words(N))
    total = empty(2)
    # ---- the scan families: an element is read twice and written once
    copies = max(2, min(8, (512 << 20) // (16 * N)))
    src = [dev(rng.integers(1, 2**63, size=2 * N, dtype=np.uint64)) for _ in range(copies)]
    dst = empty(2 * N)
    for name, fn, ew in (("vec_prefix_prod_dev", lib.ronk_vec_prefix_prod_dev, 1), ("vec_prefix_sum_dev", lib.ronk_vec_prefix_sum_dev, 1),
                         ("ext2_vec_prefix_prod_dev", lib.ronk_ext2_vec_prefix_prod_dev, 2),
                         ("ext2_vec_prefix_sum_dev", lib.ronk_ext2_vec_prefix_sum_dev, 2)):
        pre = (p,) if ew == 1 else (p, w)
        report({"op": name, "bytes": 3 * ew * 8 * N},
               time_ms(lambda k: L.check(fn(*pre, src[k % copies].data_ptr(), dst.data_ptr(), N, 1, total.data_ptr(), work.data_ptr(), None))))
    del src
    # ---- the permutation product
    copies = max(2, min(8, (512 << 20) // (24 * W * N)))
    sets = [tuple(dev(rng.integers(0, 2**63, size=W * N, dtype=np.uint64)) for _ in range(3)) for _ in range(copies)]
    beta, gamma = [int(v) % p for v in rng.integers(1, 2**62, size=2)], [int(v) % p for v in rng.integers(1, 2**62, size=2)]
    d_beta, d_gamma = dev(np.array(beta, dtype=np.uint64)), dev(np.array(gamma, dtype=np.uint64))
    Z, last, st = empty(2 * N), empty(2), torch.zeros(1, dtype=torch.int32, device="cuda")

    def perm(k):
        a, i, s = sets[k % copies]
        L.check(lib.ronk_perm_product_dev(p, w, a.data_ptr(), i.data_ptr(), s.data_ptr(), W, N, d_beta.data_ptr(), d_gamma.data_ptr(),
                                          Z.data_ptr(), last.data_ptr(), work.data_ptr(), st.data_ptr(), None))

    est = (24 * W + 48) * N
    t_perm = report({"op": "perm_product_dev", "columns": W, "bytes": est, "bytes_per_row_estimate": 24 * W + 48}, time_ms(perm))
    # (a) the streaming yardstick: as many bytes through ronk_vec_mul_dev (two reads and a write of 8 bytes per element)
    m = est // 24
    ya, yb, yo = dev(rng.integers(0, 2**63, size=m, dtype=np.uint64)), dev(rng.integers(0, 2**63, size=m, dtype=np.uint64)), empty(m)
    t_mul = report({"op": "vec_mul_dev", "elements": m, "bytes": 24 * m},
                   time_ms(lambda k: L.check(lib.ronk_vec_mul_dev(p, ya.data_ptr(), yb.data_ptr(), yo.data_ptr(), m, None))))
    del ya, yb, yo
    # (b) the terms from the element-wise entry points, then the new scan
    ONE, B, G = const_planar((1, 0)), const_planar(beta), const_planar(gamma)
    T1, T2, num, den = empty(2 * N), empty(2 * N), empty(2 * N), empty(2 * N)

    def composed(k):
        a, i, s = sets[k % copies]
        for c in range(W):
            off = 8 * c * N
            L.check(lib.ronk_ext2_vec_mul_base_dev(p, w, ONE.data_ptr(), a.data_ptr() + off, T1.data_ptr(), N, None))     # (a_c, 0)
            L.check(lib.ronk_ext2_vec_add_dev(p, w, T1.data_ptr(), G.data_ptr(), T1.data_ptr(), N, None))                  # + gamma
            for lab, acc in ((i, num), (s, den)):
                t = acc if c == 0 else T2
                L.check(lib.ronk_ext2_vec_mul_base_dev(p, w, B.data_ptr(), lab.data_ptr() + off, t.data_ptr(), N, None))    # beta label_c
                L.check(lib.ronk_ext2_vec_add_dev(p, w, t.data_ptr(), T1.data_ptr(), t.data_ptr(), N, None))
                if c:
                    L.check(lib.ronk_ext2_vec_mul_dev(p, w, acc.data_ptr(), T2.data_ptr(), acc.data_ptr(), N, None))
        L.check(lib.ronk_ext2_vec_inv_dev(p, w, den.data_ptr(), den.data_ptr(), N, None, None))
        L.check(lib.ronk_ext2_vec_mul_dev(p, w, num.data_ptr(), den.data_ptr(), num.data_ptr(), N, None))
        L.check(lib.ronk_ext2_vec_prefix_prod_dev(p, w, num.data_ptr(), num.data_ptr(), N, 1, total.data_ptr(), work.data_ptr(), None))

    passes = W * 8 - 2 + 2
    t_cmp = report({"op": "perm_composed", "columns": W, "elementwise_passes": passes}, time_ms(composed))
    perm(0)
    composed(0)
    torch.cuda.synchronize()
    emit({"op": "perm_fused_against_composed", "same_words": bool(torch.equal(Z, num)) and bool(torch.equal(last, total)),
          "composed_over_fused": round(t_cmp / t_perm, 2), "fused_over_vec_mul_same_bytes": round(t_perm / t_mul, 2),
          "status": int(st.item())})
    del ONE, B, G, T1, T2, num, den, sets
    # ---- the logUp sum: (16 C + 48) N bytes by the same estimate
    copies = max(2, min(8, (512 << 20) // (16 * C * N)))
    lsets = [tuple(dev(rng.integers(0, 2**63, size=C * N, dtype=np.uint64)) for _ in range(2)) for _ in range(copies)]

    def logup(k):
        v, mu = lsets[k % copies]
        L.check(lib.ronk_logup_sum_dev(p, w, v.data_ptr(), mu.data_ptr(), C, N, d_beta.data_ptr(), Z.data_ptr(), last.data_ptr(),
                                       work.data_ptr(), st.data_ptr(), None))

    report({"op": "logup_sum_dev", "columns": C, "bytes": (16 * C + 48) * N}, time_ms(logup))
    out.close()


if __name__ == "__main__":
    if args.case:
        f, n = args.case.split(",")
        case(f, int(n))
    else:
        sys.exit(driver())
