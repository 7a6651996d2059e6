"""Times ronk_poly_mul_sharded_dev (the sharded polynomial multiply) with the fused and the composed middle, alternating the two
plans in one process (RONK_SHARDED_MUL_FUSED / _UNFUSED; `fused_middle` = 0 on the fused arm: no instantiation matches there), and
ronk_poly_mul_dev (one GPU) at NTT sizes 2^22 / 2^23 for scale.  One JSON line per configuration.

Every rank is a LOGICAL rank on device 0: the exchanges are same-device copies and the kernels of all ranks share one GPU, so
this measures local kernels and same-device copies only -- NOT a scaling result.  Time per product = wall time of `iters`
back-to-back enqueued calls (after warm-up and a drain), divided by `iters`; the calls pipeline the way a caller's would.

usage: python tools/sharded_mul_time.py [--world 8] [--iters 20] [--warmup 3] [--sizes 22,24,26] [--rounds 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ronkathon_amd import _lib as L  # noqa: E402

NOTE = "logical ranks on one GPU: local kernels and same-device copies only, not a scaling result"


def dev_alloc(elems, fill_seed=None):
    h = C.c_void_p()
    L.check(L.lib.ronk_dev_alloc(C.byref(h), elems * 8))
    if fill_seed is not None:
        x = np.random.default_rng(fill_seed).integers(0, 2**63, size=elems, dtype=np.uint64)
        L.check(L.lib.ronk_memcpy_h2d(h.value, L.ptr(x), elems * 8))
    return h.value


def time_calls(fn, sync, iters, warmup):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="fused / composed alternations per size")
    ap.add_argument("--sizes", default="22,24,26")
    ap.add_argument("--chunks", type=int, default=0)
    args = ap.parse_args()
    W = args.world
    for log2n in [int(s) for s in args.sizes.split(",")]:
        plans = {"fused": L.ShardedMulPlan(log2n, [0] * W, chunks=args.chunks, fused=True),
                 "composed": L.ShardedMulPlan(log2n, [0] * W, chunks=args.chunks, unfused=True)}
        per = plans["fused"].per_rank
        bufs = {k: [dev_alloc(per, 1000 * i + j if k != "out" else None) for j in range(W)] for i, k in enumerate(("a", "b", "out"))}
        times = {k: [] for k in plans}
        for _ in range(args.rounds):
            for name, mp in plans.items():
                times[name].append(time_calls(lambda: mp.mul_dev(bufs["a"], bufs["b"], bufs["out"]), mp.sync, args.iters, args.warmup))
        for name, mp in plans.items():
            print(json.dumps({"op": "ronk_poly_mul_sharded_dev", "log2n": log2n, "world": W, "chunks": mp.chunks, "middle": name,
                              "fused_middle": mp.fused_middle, "ms_per_product_median": float(np.median(times[name])),
                              "ms_per_product_all": [round(t, 4) for t in times[name]], "note": NOTE}), flush=True)
        for mp in plans.values():
            mp.close()
        for v in bufs.values():
            for p in v:
                L.lib.ronk_dev_free(p)
    for log2N in (22, 23):
        d = 1 << (log2N - 1)
        a, b, out = dev_alloc(d, 1), dev_alloc(d, 2), dev_alloc(2 * d)
        call = lambda: L.check(L.lib.ronk_poly_mul_dev(L.GOLDILOCKS_P, 7, a, d, b, d, out, None))
        ts = [time_calls(call, lambda: L.check(L.lib.ronk_dev_sync()), args.iters, args.warmup) for _ in range(args.rounds)]
        print(json.dumps({"op": "ronk_poly_mul_dev", "ntt_log2n": log2N, "degree_bound": d, "ms_per_product_median": float(np.median(ts)),
                          "ms_per_product_all": [round(t, 4) for t in ts], "note": "one GPU, single-GPU library multiply, for scale"}),
              flush=True)
        for p in (a, b, out):
            L.lib.ronk_dev_free(p)


if __name__ == "__main__":
    main()
