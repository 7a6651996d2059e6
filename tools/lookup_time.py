"""Times the lookup multiplicities (ronk_lookup_mult_dev) and the logUp quotient (ronk_logup_quotient_dev) with hipEvents around
`iters` back-to-back calls after warm-up, median of `rounds`, and in the same run, on the same device:
  multiplicities  n = 2^size rows, C = 2 columns, T = 2^16 and 2^20 table entries, lookups drawn uniformly from the table and all
      equal to one entry (the contention path), beside
      (a) ronk_vec_mul_dev on as many bytes as the call's arrays hold, 8 (C n + 2 T): the streaming yardstick of tools/accum_time.py;
      (b) the host path it replaces: a device-to-host copy of the columns and the table, counting with numpy (unique, searchsorted,
          bincount) and a host-to-device copy of m -- wall clock, median of `rounds` single runs;
  quotient  M = 2^size rows, C = 2 with the multiplicities and T_in, 96 bytes per row by the count of its arrays (vals 2, mult 2, S
      and S at the row B on 4, T_in 2 words read, 2 written: 12 words), beside
      (c) ronk_plonk_quotient_dev at the same M (its kernel and the files it is built from are those of the parent commit);
      (d) 6 C + 10 passes of ronk_ext2_vec_mul_dev over [2][M] arrays: as many elementwise passes as composing the same words from
          the ronk_ext2_vec_* family takes (the sums among them would cost fewer instructions and the same bytes).
Inputs -- the uniform and the all-equal columns, the yardstick's buffers, the quotients' columns -- rotate over enough copies to
exceed the 256 MiB Infinity Cache (up to 32 copies; the table and the workspace of a call are one set and stay).  Every (field,
size) case runs in a child process of its own under a time limit, and the driver stops at the first case that fails.  One JSON
line per measurement, appended to --out.

usage: python tools/lookup_time.py [--iters 10] [--warmup 2] [--rounds 3] [--log2-sizes 20,22] [--log2-blowup 2] [--fields gl,mont]
                                   [--limit 240] [--out profiles/lookup_time_mi355x.jsonl]"""
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
ap.add_argument("--log2-blowup", type=int, default=2)
ap.add_argument("--fields", default="gl,mont")
ap.add_argument("--limit", type=int, default=240, help="seconds per (field, size) case")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_time_mi355x.jsonl"))
ap.add_argument("--case", default=None, help="internal: field,log2_size of the one case this process runs")
args = ap.parse_args()

PRIMES = {"gl": (0xFFFFFFFF00000001, 7), "mont": (0xFFFFFFFC00000001, 10)}
COLUMNS = 2
QUOTIENT_BYTES_PER_ROW = 96
PLONK_BYTES_PER_ROW = 152      # the estimate of tools/plonk_time.py


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


def case(field, log2_size):
    sys.path.insert(0, ROOT)
    import torch

    from ronkathon_amd import _lib as L
    lib = L.lib
    p, w = PRIMES[field]
    g = w
    n = M = 1 << log2_size
    base = {"field": field, "log2_size": log2_size}
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
    # ---- multiplicities
    for log2_t in (16, 20):
        T = 1 << log2_t
        table = rand(T)
        copies = max(2, min(32, (512 << 20) // (8 * COLUMNS * n)))
        uniform = [table[torch.randint(0, T, (COLUMNS * n,), device="cuda")] for _ in range(copies)]
        equal = [table[k:k + 1].expand(COLUMNS * n).contiguous() for k in range(copies)]      # copy k: every cell holds entry k
        mult, missing, work = empty(T), empty(2), empty(lib.ronk_lookup_workspace_words(T))
        est = 8 * (COLUMNS * n + 2 * T)
        shape = {"log2_table": log2_t, "columns": COLUMNS, "bytes": est}
        times = {}
        for name, sets in (("uniform", uniform), ("all_equal", equal)):
            def call(k, sets=sets):
                L.check(lib.ronk_lookup_mult_dev(p, table.data_ptr(), T, sets[k % len(sets)].data_ptr(), COLUMNS, n, 1, mult.data_ptr(),
                                                 missing.data_ptr(), work.data_ptr(), None))
            times[name] = report(dict(shape, op="lookup_mult_dev", lookups=name), time_ms(call))
            torch.cuda.synchronize()
            assert missing.cpu().tolist() == [0, -1], "a lookup drawn from the table was reported missing"
        # (a) the streaming yardstick on as many bytes
        m = est // 24
        ycopies = max(2, min(32, (512 << 20) // (24 * m)))
        ys = [(rand(m), rand(m), empty(m)) for _ in range(ycopies)]

        def vec_mul(k):
            ya, yb, yo = ys[k % ycopies]
            L.check(lib.ronk_vec_mul_dev(p, ya.data_ptr(), yb.data_ptr(), yo.data_ptr(), m, None))

        t_mul = report({"op": "vec_mul_dev", "log2_table": log2_t, "elements": m, "bytes": 24 * m}, time_ms(vec_mul))
        del ys
        # (b) the host path: copy out, count, copy back
        host_ms = []
        for r in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hv, ht = uniform[r % copies].cpu().numpy().view(np.uint64), table.cpu().numpy().view(np.uint64)
            keys, first = np.unique(ht % np.uint64(p), return_index=True)
            pos = np.searchsorted(keys, hv % np.uint64(p))
            pos[pos == keys.size] = 0
            found = keys[pos] == hv % np.uint64(p)
            counts = np.bincount(first[pos[found]], minlength=T).astype(np.uint64)
            hm = np.where(counts == 0, counts, np.uint64(p) - counts)
            mult.copy_(torch.from_numpy(hm.view(np.int64)))
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        t_host = report({"op": "host_copy_numpy_count_copy", "log2_table": log2_t, "lookups": "uniform"}, host_ms)
        emit({"op": "lookup_mult_against_yardsticks", "log2_table": log2_t,
              "uniform_over_vec_mul_same_bytes": round(times["uniform"] / t_mul, 2),
              "all_equal_over_uniform": round(times["all_equal"] / times["uniform"], 2),
              "host_path_over_uniform": round(t_host / times["uniform"], 1)})
        del uniform, equal, table, mult, work
    # ---- the quotient: 10 M words of input per copy
    log2_b = args.log2_blowup
    copies = max(2, min(8, (512 << 20) // (10 * 8 * M)))
    sets = [tuple(rand(k * M) for k in (COLUMNS, COLUMNS, 2, 2)) for _ in range(copies)]
    alpha, lam, T_out = rand(2), rand(4), empty(2 * M)
    h = C.c_void_p()
    L.check(lib.ronk_plonk_create(C.byref(h), p, g, w, log2_size - log2_b, log2_b, g, (C.c_uint64 * 3)(1, 2, 3)))

    def quotient(k):
        v, m, S, Tin = sets[k % copies]
        L.check(lib.ronk_logup_quotient_dev(h, v.data_ptr(), m.data_ptr(), COLUMNS, S.data_ptr(), alpha.data_ptr(), lam.data_ptr(),
                                            Tin.data_ptr(), T_out.data_ptr(), None))

    t_q = report({"op": "logup_quotient_dev", "columns": COLUMNS, "bytes": QUOTIENT_BYTES_PER_ROW * M,
                  "bytes_per_row": QUOTIENT_BYTES_PER_ROW}, time_ms(quotient))
    del sets
    # (c) the PLONK quotient at the same M
    copies = max(2, min(8, (512 << 20) // (14 * 8 * M)))
    sets = [tuple(rand(k * M) for k in (3, 5, 3, 1, 2)) for _ in range(copies)]
    ch = [rand(2) for _ in range(3)]

    def plonk(k):
        a, q, s, pi, Z = sets[k % copies]
        L.check(lib.ronk_plonk_quotient_dev(h, a.data_ptr(), q.data_ptr(), s.data_ptr(), pi.data_ptr(), Z.data_ptr(), ch[0].data_ptr(),
                                            ch[1].data_ptr(), ch[2].data_ptr(), T_out.data_ptr(), None))

    t_p = report({"op": "plonk_quotient_dev", "bytes": PLONK_BYTES_PER_ROW * M, "bytes_per_row_estimate": PLONK_BYTES_PER_ROW}, time_ms(plonk))
    L.check(lib.ronk_plonk_destroy(h))
    del sets
    # (d) as many elementwise extension passes as the composed form takes
    passes = 6 * COLUMNS + 10
    copies = max(3, min(8, (512 << 20) // (16 * M)))
    arrs = [rand(2 * M) for _ in range(copies)]

    def composed(k):
        for j in range(passes):
            a, b, o = arrs[(k + j) % copies], arrs[(k + j + 1) % copies], arrs[(k + j + 2) % copies]
            L.check(lib.ronk_ext2_vec_mul_dev(p, w, a.data_ptr(), b.data_ptr(), o.data_ptr(), M, None))

    t_c = report({"op": "ext2_vec_mul_dev_passes", "passes": passes, "bytes": passes * 48 * M}, time_ms(composed))
    emit({"op": "logup_quotient_against_yardsticks", "quotient_over_plonk_quotient": round(t_q / t_p, 2),
          "composed_passes_over_quotient": round(t_c / t_q, 1)})
    out.close()


if __name__ == "__main__":
    if args.case:
        f, m = args.case.split(",")
        case(f, int(m))
    else:
        sys.exit(driver())
