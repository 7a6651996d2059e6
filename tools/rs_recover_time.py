"""Times the product tree (ronk_poly_from_roots_dev) and Reed-Solomon erasure recovery (ronk_rs_recover_batch_dev) with hipEvents
around `iters` back-to-back calls after warm-up (the calls pipeline the way a caller's would; the first call of a shape builds its
level plans and is part of the warm-up).  One JSON line per case.

Cases: the tree for m = 2^16, 2^20, 2^21 roots; recovery at N = 2^17, k = 2^16, e = 2^16 (batch 1 and 16), N = 2^21, k = e = 2^20 and
N = 2^22, k = e = 2^21 (Goldilocks), with d_full = NULL.  --leaf-log2 L sets RONK_ROOTS_LEAF_LOG2 (the leaf-size A/B).

usage: python tools/rs_recover_time.py [--iters 20] [--warmup 3] [--rounds 3] [--leaf-log2 6]"""
import argparse
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--leaf-log2", type=int, default=0, help="6..8: RONK_ROOTS_LEAF_LOG2 for this process (0: the library default)")
ap.add_argument("--only", default="", help="comma list of case names to run (tree, recover)")
args = ap.parse_args()
if args.leaf_log2:
    os.environ["RONK_ROOTS_LEAF_LOG2"] = str(args.leaf_log2)   # read by the library at its first tree call

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ronkathon_amd import _lib as L  # noqa: E402

GP, GG = L.GOLDILOCKS_P, 7


def field_dev(seed, n):
    v = np.random.default_rng(seed).integers(0, 2**63, size=n, dtype=np.uint64)
    return torch.from_numpy(v.view(np.int64)).cuda()


def time_ms(fn):
    out = []
    for _ in range(args.rounds):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / args.iters)
    return out


def report(d, ts):
    d.update({"leaf_log2": args.leaf_log2 or 6, "ms_median": round(float(np.median(ts)), 4), "ms_all": [round(t, 4) for t in ts]})
    print(json.dumps(d), flush=True)


def main():
    only = set(args.only.split(",")) if args.only else {"tree", "recover"}
    if "tree" in only:
        for lm in (16, 20, 21):
            m = 1 << lm
            r = field_dev(lm, m)
            out = torch.empty(m + 1, dtype=torch.int64, device="cuda")
            ts = time_ms(lambda: L.check(L.lib.ronk_poly_from_roots_dev(GP, r.data_ptr(), m, out.data_ptr(), None)))
            report({"op": "ronk_poly_from_roots_dev", "m": m}, ts)
            del r, out
    if "recover" in only:
        for log2n, lk, B in ((17, 16, 1), (17, 16, 16), (21, 20, 1), (22, 21, 1)):
            N, k = 1 << log2n, 1 << lk
            e = N - k
            plan = L.Plan(GP, GG, log2n, B)
            msgs = field_dev(log2n, B * k) % 2**62
            ys = torch.empty(B * N, dtype=torch.int64, device="cuda")
            plan.rs_encode_batch_dev(msgs.data_ptr(), k, ys.data_ptr())
            er = torch.from_numpy(np.random.default_rng(B).choice(N, size=e, replace=False).astype(np.int64)).cuda()
            out = torch.empty(B * k, dtype=torch.int64, device="cuda")
            st = torch.empty(B, dtype=torch.int32, device="cuda")
            fn = lambda: plan.rs_recover_batch_dev(k, er.data_ptr(), e, ys.data_ptr(), out.data_ptr(), None, st.data_ptr())
            ts = time_ms(fn)
            torch.cuda.synchronize()
            ok = bool((st == 0).all().item()) and bool(torch.equal(out, msgs))
            report({"op": "ronk_rs_recover_batch_dev", "log2n": log2n, "k": k, "erased": e, "batch": B, "exact": ok}, ts)
            plan.close()
            del msgs, ys, er, out, st


if __name__ == "__main__":
    main()
