#!/usr/bin/env python3
"""Times the transform and the product over BN254's scalar field (csrc/fr_ntt_kernels.h) and, beside each transform, the
library's Goldilocks transform of the same byte size (2^k elements of 32 B = 2^(k+2) elements of 8 B), in the same process.

Protocol: every buffer resident in HBM; the calls of a region rotate over enough input / output pairs that their bytes
exceed 512 MiB (twice the 256 MiB Infinity Cache), so every call reads HBM-cold data; one hipEvent pair around a region of
`--steps` calls after `--warmup` untimed ones; the median of 5 regions.  Reports time per call, calls per second and the
fraction of 8 TB/s that the algorithmic 64 n bytes (one read and one write of n 32-byte elements) amount to.

usage: python tools/bench_fr_ntt.py [--sizes 16 20 22 24] [--mul-sizes 20 22] [--steps N] [--out profiles/fr_ntt_bench.json]
       python tools/bench_fr_ntt.py --one 22      (one size, few steps: the workload of a kernel trace)"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ronkathon_amd import _lib as L  # noqa: E402

HBM_PEAK = 8.0e12
COLD_BYTES = 512 << 20


def rand_words(n_words, top_mask=None):
    x = torch.randint(-2**63, 2**63 - 1, (n_words,), dtype=torch.int64, device="cuda")
    if top_mask is not None:
        x.view(-1, 4)[:, 3] &= top_mask      # below 2^253 < r: canonical
    return x


def regions(fn, steps, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(steps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return statistics.median(ms), ms


def pairs_for(bytes_per_call):
    return max(2, -(-COLD_BYTES // bytes_per_call))


def bench_fr(k, steps, warmup):
    n = 1 << k
    cnt = pairs_for(64 * n)
    ins = [rand_words(4 * n, (1 << 61) - 1) for _ in range(cnt)]
    outs = [torch.empty_like(ins[0]) for _ in range(cnt)]
    plan = L.FrPlan(k)
    t, all_ms = regions(lambda i: plan.forward_dev(ins[i % cnt].data_ptr(), outs[i % cnt].data_ptr()), steps, warmup)
    rows = plan.info()
    plan.close()
    return {"what": "fr_ntt_forward", "log2n": k, "passes_log2_rows": rows, "ms": t, "regions_ms": all_ms, "per_second": 1e3 / t,
            "algorithmic_bytes": 64 * n, "fraction_of_8TBps": 64 * n / (t * 1e-3) / HBM_PEAK, "buffers": cnt, "steps": steps}


def bench_gl(k, steps, warmup):
    """the Goldilocks transform of 2^k elements (8 B each)"""
    n = 1 << k
    cnt = pairs_for(16 * n)
    ins = [(rand_words(n) & ((1 << 62) - 1)) for _ in range(cnt)]
    outs = [torch.empty_like(ins[0]) for _ in range(cnt)]
    plan = L.Plan(0xFFFFFFFF00000001, 7, k)
    t, all_ms = regions(lambda i: plan.forward_dev(ins[i % cnt].data_ptr(), outs[i % cnt].data_ptr()), steps, warmup)
    plan.close()
    return {"what": "goldilocks_ntt_forward", "log2n": k, "ms": t, "regions_ms": all_ms, "per_second": 1e3 / t,
            "algorithmic_bytes": 16 * n, "fraction_of_8TBps": 16 * n / (t * 1e-3) / HBM_PEAK, "buffers": cnt, "steps": steps}


def bench_mul(k, steps, warmup):
    """a product whose NTT size is 2^k: two operands of 2^(k-1) coefficients"""
    d = 1 << (k - 1)
    cnt = pairs_for(32 * (4 * d))
    a = [rand_words(4 * d, (1 << 61) - 1) for _ in range(cnt)]
    b = [rand_words(4 * d, (1 << 61) - 1) for _ in range(cnt)]
    out = [torch.empty(4 * (2 * d - 1), dtype=torch.int64, device="cuda") for _ in range(cnt)]

    def fn(i):
        j = i % cnt
        L.check(L.lib.ronk_poly_mul_bn254_dev(a[j].data_ptr(), d, b[j].data_ptr(), d, out[j].data_ptr(), None))
    t, all_ms = regions(fn, steps, warmup)
    return {"what": "fr_poly_mul", "ntt_log2n": k, "d": d, "ms": t, "regions_ms": all_ms, "per_second": 1e3 / t, "buffers": cnt,
            "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[16, 20, 22, 24])
    ap.add_argument("--mul-sizes", type=int, nargs="*", default=[20, 22])
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--one", type=int, default=0)
    a = ap.parse_args()
    if a.one:
        r = bench_fr(a.one, a.steps or 4, 1)
        print(json.dumps(r), flush=True)
        return
    res = []
    for k in a.sizes:
        steps = a.steps or max(8, min(400, (1 << 26) >> k))
        for r in (bench_fr(k, steps, a.warmup), bench_gl(k + 2, steps, a.warmup)):
            res.append(r)
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    for k in a.mul_sizes:
        r = bench_mul(k, a.steps or max(8, min(100, (1 << 25) >> k)), a.warmup)
        res.append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        doc = {"device": torch.cuda.get_device_name(0), "protocol": __doc__.split("Protocol:")[1].split("usage:")[0].strip(), "results": res}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
