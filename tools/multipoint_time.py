"""Times multipoint evaluation (ronk_poly_eval_many_dev) and interpolation (ronk_poly_interpolate_dev) with hipEvents around `iters`
back-to-back calls after warm-up (the first call of a shape builds its level plans and is part of the warm-up).  One JSON line per
case, median of `rounds`.

Cases: m = d in {2^12, 2^16, 2^20} and d = 2^22 with m = 2^12, Goldilocks, plus m = d = 2^16 over one Montgomery prime; each in
the library's own choice of form and -- where the other form serves the size -- forced (RONK_MULTIPOINT_FORM), which is how the
crossover constants of csrc/ronk_multipoint.hip are found (--crossover: a finer grid of small sizes, both forms).
Two yardsticks from the same run: 256 calls of ronk_poly_eval_dev scaled to m (the only route without this entry point), and
ronk_poly_from_roots_dev of the same m (the walk down runs about as many batched transforms as the tree).

usage: python tools/multipoint_time.py [--iters 10] [--warmup 2] [--rounds 3] [--crossover] [--only eval,interp,yardsticks]"""
import argparse
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--crossover", action="store_true", help="the grid of small sizes in both forms instead of the table's cases")
ap.add_argument("--only", default="", help="comma list of: eval, interp, yardsticks")
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ronkathon_amd import _lib as L  # noqa: E402

GP = L.GOLDILOCKS_P
MONT = 0xFFFFFFFC00000001
DIRECT_MAX_WORK = 2**34


def field_dev(seed, n, p):
    v = np.random.default_rng(seed).integers(0, 2**63, size=n, dtype=np.uint64) % np.uint64(p)
    return torch.from_numpy(v.view(np.int64)).cuda()


def distinct_dev(seed, n, p):
    v = np.unique(np.random.default_rng(seed).integers(1, 2**63, size=n + n // 8 + 16, dtype=np.uint64) % np.uint64(p))[:n]
    assert v.size == n
    np.random.default_rng(seed + 1).shuffle(v)
    return torch.from_numpy(v.view(np.int64)).cuda()


def time_ms(fn, iters=None):
    iters = iters or args.iters
    out = []
    for _ in range(args.rounds):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return out


def report(d, ts):
    d.update({"ms_median": round(float(np.median(ts)), 4), "ms_all": [round(t, 4) for t in ts]})
    print(json.dumps(d), flush=True)


def with_form(name, fn):
    os.environ.pop("RONK_MULTIPOINT_FORM", None)
    if name != "auto":
        os.environ["RONK_MULTIPOINT_FORM"] = name
    try:
        return fn()
    finally:
        os.environ.pop("RONK_MULTIPOINT_FORM", None)


def case(p, m, d, only, forms):
    c, x = field_dev(m + d, d, p), distinct_dev(m, m, p)
    y = torch.empty(m, dtype=torch.int64, device="cuda")
    out = torch.empty(m, dtype=torch.int64, device="cuda")
    st = torch.empty(1, dtype=torch.int32, device="cuda")
    ev = lambda: L.check(L.lib.ronk_poly_eval_many_dev(p, c.data_ptr(), d, x.data_ptr(), m, y.data_ptr(), None))
    it = lambda: L.check(L.lib.ronk_poly_interpolate_dev(p, x.data_ptr(), y.data_ptr(), m, out.data_ptr(), st.data_ptr(), None))
    for name in forms:
        if "eval" in only and not (name == "direct" and m * d > 2**32):   # the direct form beyond 2^32 products: seconds per call
            report({"op": "ronk_poly_eval_many_dev", "p": p, "m": m, "d": d, "form": name}, with_form(name, lambda: time_ms(ev)))
        if "interp" in only and d == m and not (name == "direct" and m > 2**14):
            with_form("auto", ev)
            ts = with_form(name, lambda: time_ms(it))
            torch.cuda.synchronize()
            report({"op": "ronk_poly_interpolate_dev", "p": p, "m": m, "form": name, "exact": bool(torch.equal(out, c)) and int(st.item()) == 0}, ts)
    if "yardsticks" in only:
        one = torch.empty(1, dtype=torch.int64, device="cuda")
        xs = [int(v) for v in x[:256].cpu().numpy().view(np.uint64)]
        k = len(xs)

        def loop():
            for v in xs:
                L.check(L.lib.ronk_poly_eval_dev(p, c.data_ptr(), d, v, one.data_ptr(), None))
        ts = [t * m / k for t in time_ms(loop, iters=1)]
        report({"op": "ronk_poly_eval_dev x m (256 calls, scaled)", "p": p, "m": m, "d": d}, ts)
        z = torch.empty(m + 1, dtype=torch.int64, device="cuda")
        report({"op": "ronk_poly_from_roots_dev", "p": p, "m": m},
               time_ms(lambda: L.check(L.lib.ronk_poly_from_roots_dev(p, x.data_ptr(), m, z.data_ptr(), None))))


def main():
    only = set(args.only.split(",")) if args.only else {"eval", "interp", "yardsticks"}
    if args.crossover:
        for lm in range(6, 15):
            for ld in sorted({lm, 12, 16}):
                case(GP, 1 << lm, 1 << ld, only - {"yardsticks"}, ("direct", "tree"))
        return
    for lm, ld in ((12, 12), (16, 16), (20, 20), (12, 22)):
        case(GP, 1 << lm, 1 << ld, only, ("auto", "direct", "tree") if lm <= 16 else ("auto",))
    case(MONT, 1 << 16, 1 << 16, only, ("auto",))


if __name__ == "__main__":
    main()
