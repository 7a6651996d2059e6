"""Times the Poseidon / Merkle family (ronk_poseidon_permute_dev, ronk_poseidon_sponge_dev, ronk_merkle_commit_dev) with hipEvents
around `iters` back-to-back calls after warm-up, median of `rounds`.  One JSON line per case.  The parameters are TEST parameters
(SplitMix64 round constants, a Cauchy matrix): alpha 7, 8 full + 22 partial rounds, rate = width - 4, digest 4.

Cases per (field, width in 8, 12, 16):
  permute   2^20 states                                          -> permutations / s
  sponge    the columns of a [16][2^20] matrix, 4 outputs         (the leaf level of the tree below)
  commit    ronk_merkle_commit_dev, 2^20 leaves x 16 elements
  levels    the same tree as one ronk_poseidon_sponge_dev launch per level (the unfused composition), summed
--cpu LIB times the C restatement (a shared object built from tests/emu/emu_poseidon.cpp with -DEMU_POSEIDON_LIB -fopenmp) on the
same tree, once.

usage: python tools/poseidon_time.py [--iters 10] [--warmup 2] [--rounds 3] [--fields gl,mont] [--widths 8,12,16] [--log2-leaves 20]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--fields", default="gl,mont")
ap.add_argument("--widths", default="8,12,16")
ap.add_argument("--log2-leaves", type=int, default=20)
ap.add_argument("--cpu", default="", help="path of the C restatement's shared object: time it on the width-12 tree")
ap.add_argument("--label", default="", help="copied into every line (e.g. lazy / eager for the A/B of two builds)")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import poseidon_ref as PR  # noqa: E402  (the derivation of the test parameters)
from ronkathon_amd import _lib as L  # noqa: E402

PRIMES = {"gl": PR.GOLDILOCKS, "mont": PR.MONT_P}
ALPHA, NUM_P, NUM_F, LEAF, DIGEST = 7, 22, 8, 16, 4


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
    d.update({"label": args.label, "ms_median": round(float(np.median(ts)), 4),
              "ms_all": [round(t, 4) for t in ts]})
    print(json.dumps(d), flush=True)
    return float(np.median(ts))


def main():
    n = 1 << args.log2_leaves
    rng = np.random.default_rng(1)
    mat = torch.from_numpy(rng.integers(0, 2**63, size=n * LEAF, dtype=np.uint64).view(np.int64)).cuda()
    for fname in args.fields.split(","):
        p = PRIMES[fname]
        for width in (int(w) for w in args.widths.split(",")):
            P = PR.derive_params(p, width, ALPHA, NUM_P, NUM_F, width - 4)
            h = L.PoseidonHandle(*P.create_args())
            base = {"field": fname, "width": width, "alpha": ALPHA, "rounds": NUM_P + NUM_F, "rate": width - 4}
            states = torch.from_numpy(rng.integers(0, 2**63, size=n * width, dtype=np.uint64).view(np.int64)).cuda()
            ms = report(dict(base, op="permute", count=n), time_ms(lambda: h.permute_dev(states.data_ptr(), n)))
            print(json.dumps(dict(base, op="permute", gperm_per_s=round(n / ms / 1e6, 4))), flush=True)
            out = torch.empty(n * DIGEST, dtype=torch.int64, device="cuda")
            report(dict(base, op="sponge_columns", items=n, len=LEAF, n_out=DIGEST),
                   time_ms(lambda: h.sponge_dev(mat.data_ptr(), n, LEAF, 1, n, out.data_ptr(), DIGEST)))
            report(dict(base, op="sponge_rows", items=n, len=LEAF, n_out=DIGEST),
                   time_ms(lambda: h.sponge_dev(mat.data_ptr(), n, LEAF, LEAF, 1, out.data_ptr(), DIGEST)))
            tree = torch.empty(L.merkle_tree_words(n, DIGEST), dtype=torch.int64, device="cuda")
            report(dict(base, op="merkle_commit_columns", leaves=n, leaf_len=LEAF, digest=DIGEST),
                   time_ms(lambda: h.merkle_commit_dev(mat.data_ptr(), n, LEAF, 1, n, DIGEST, tree.data_ptr())))

            def per_level():
                h.sponge_dev(mat.data_ptr(), n, LEAF, 1, n, tree.data_ptr(), DIGEST)
                cnt, off = n, 0
                while cnt > 1:   # even levels only here (n is a power of two): a node = the sponge of two adjacent digests
                    h.sponge_dev(tree.data_ptr() + 8 * off, cnt // 2, 2 * DIGEST, 2 * DIGEST, 1, tree.data_ptr() + 8 * (off + cnt * DIGEST), DIGEST)
                    off += cnt * DIGEST
                    cnt //= 2
            report(dict(base, op="merkle_one_sponge_launch_per_level", leaves=n, launches=args.log2_leaves + 1), time_ms(per_level))
            h.close()
    if args.cpu:
        lib = C.CDLL(args.cpu)
        vp, u64, u32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t
        lib.posref_merkle.argtypes = [u64, u32, u64, u32, u32, u32, vp, vp, vp, sz, sz, sz, sz, sz, vp]
        lib.posref_merkle.restype = None
        P = PR.derive_params(PR.GOLDILOCKS, 12, ALPHA, NUM_P, NUM_F, 8)
        rc = L.arr(P.rc); mds = L.arr([v for row in P.mds for v in row])
        leaves = mat.cpu().numpy().view(np.uint64)
        tree = np.empty(L.merkle_tree_words(n, DIGEST), dtype=np.uint64)
        t0 = time.time()
        lib.posref_merkle(P.p, 12, ALPHA, NUM_P, NUM_F, 8, L.ptr(rc), L.ptr(mds), L.ptr(leaves), n, LEAF, 1, n, DIGEST, L.ptr(tree))
        print(json.dumps({"op": "cpu_restatement_merkle", "field": "gl", "width": 12, "leaves": n, "leaf_len": LEAF,
                          "threads": os.environ.get("OMP_NUM_THREADS", ""), "seconds": round(time.time() - t0, 2)}), flush=True)


if __name__ == "__main__":
    main()
