"""Times the multi-matrix polynomial commitment (ronk_mpcs_combine_dev, ronk_mpcs_open_dev, ronk_mpcs_verify_dev) with hipEvents
around `iters` back-to-back calls after warm-up, median of `rounds`, and in the same run, on the same matrices, what the library
offered before it for R committed matrices:
  (a) the codeword: R calls of ronk_deep_combine_dev on per-round handles (round r with ITS points) plus R - 1 passes of
      ronk_ext2_vec_add_dev.  (That composition spends the powers of alpha per round, so its words are not the fused call's; the
      fused call's words are checked by tests/test_gpu_mpcs.py.)
  (b) the opening: the sum of R ronk_pcs_open_dev calls on the per-round handles;
  (c) the verifier: the sum of R ronk_pcs_verify_dev calls.
The default shape is the PLONK one: R = 4 with C = (8, 3, 2, 8), K = 2, masks (01, 01, 11, 01).  The matrices are real low-degree
extensions (coefficients through the library's NTT, coset shift 1), so every verifier's status is reported and must be 0; they
rotate over enough copies to exceed the 256 MiB Infinity Cache.  One JSON line per case.  The Poseidon parameters are TEST
parameters (width 12, alpha 7, 8 full + 22 partial rounds, rate 8).

usage: python tools/mpcs_time.py [--iters 10] [--warmup 2] [--rounds 3] [--log2-sizes 20,22] [--field gl] [--columns 8,3,2,8]
                                 [--points 2] [--masks 1,1,3,1]"""
import argparse
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log2-sizes", default="20,22")
ap.add_argument("--field", default="gl")
ap.add_argument("--eta", type=int, default=3)
ap.add_argument("--queries", type=int, default=64)
ap.add_argument("--columns", default="8,3,2,8")
ap.add_argument("--points", type=int, default=2)
ap.add_argument("--masks", default="1,1,3,1")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import ext2_ref as ER  # noqa: E402
import poseidon_ref as PR  # noqa: E402  (the derivation of the test parameters)
from ronkathon_amd import _lib as L  # noqa: E402

PRIMES = {"gl": (PR.GOLDILOCKS, 7), "mont": (PR.MONT_P, 10)}
DIGEST, BLOWUP = 4, 2


def time_ms(fn):
    """fn(k): call number k (selects the rotating input)"""
    out = []
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
        out.append(a.elapsed_time(b) / args.iters)
    return out


def report(d, ts):
    d.update({"ms_median": round(float(np.median(ts)), 4), "ms_all": [round(t, 4) for t in ts]})
    print(json.dumps(d), flush=True)
    return float(np.median(ts))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def main():
    p, g = PRIMES[args.field]
    w = g
    eta, Q, K = args.eta, args.queries, args.points
    Cs, masks = [int(v) for v in args.columns.split(",")], [int(v) for v in args.masks.split(",")]
    R, Ctot = len(Cs), sum(Cs)
    points_of = [[k for k in range(K) if (m >> k) & 1] for m in masks]
    P = PR.derive_params(p, 12, 7, 22, 8, 8)
    pos = L.PoseidonHandle(*P.create_args())
    rng = np.random.default_rng(1)
    for n in (int(v) for v in args.log2_sizes.split(",")):
        log2_final = n - eta * max(1, -(-(n - 8) // eta))
        blow = min(BLOWUP, log2_final)
        N, d = 1 << n, (1 << n) >> blow
        mp = L.MpcsHandle(pos, g, w, n, 1, eta, log2_final, blow, Q, DIGEST, K, Cs, masks)
        per = [L.PcsHandle(pos, g, w, n, 1, eta, log2_final, blow, Q, DIGEST, Cs[r], len(points_of[r])) for r in range(R)]
        base = {"field": args.field, "w": w, "log2_n": n, "eta": eta, "log2_final": log2_final, "queries": Q, "digest": DIGEST,
                "columns": Cs, "points": K, "masks": masks}
        # matrices: the values of C_r polynomials of degree < d on <w_N>, through the library's transform
        copies = max(2, min(8, (512 << 20) // (8 * N * Ctot)))
        coefs, mats = [[] for _ in range(copies)], [[] for _ in range(copies)]
        for r, C in enumerate(Cs):
            plan = L.Plan(p, g, n, batch=C)
            for k in range(copies):
                c = rng.integers(0, 2**63, size=(C, d), dtype=np.uint64) % np.uint64(p)
                padded = torch.zeros((C, N), dtype=torch.int64, device="cuda")
                padded[:, :d] = dev(c)
                m = torch.empty(C * N, dtype=torch.int64, device="cuda")
                plan.forward_dev(padded.data_ptr(), m.data_ptr())
                coefs[k].append(dev(c.ravel()))
                mats[k].append(m)
                del padded
            torch.cuda.synchronize()
            plan.close()
        ptrs = lambda sets: [[t.data_ptr() for t in s] for s in sets]      # noqa: E731
        mat_p, coef_p = ptrs(mats), ptrs(coefs)
        zs = [(int(rng.integers(1, 2**62)) % p, int(rng.integers(1, 2**62)) % p) for _ in range(K)]
        d_z = dev(np.array(ER.planar(zs), dtype=np.uint64))
        d_zr = [dev(np.array(ER.planar([zs[k] for k in points_of[r]]), dtype=np.uint64)) for r in range(R)]
        alpha = (int(rng.integers(1, 2**62)) % p, int(rng.integers(1, 2**62)) % p)
        d_alpha = dev(np.array(alpha, dtype=np.uint64))
        # the claims of copy 0: per round for the per-round handles, and in the proof's order for the fused call
        d_yr = [torch.empty(2 * len(points_of[r]) * Cs[r], dtype=torch.int64, device="cuda") for r in range(R)]
        for r in range(R):
            L.check(L.lib.ronk_ext2_poly_eval_batch_dev(p, w, coefs[0][r].data_ptr(), Cs[r], d, d_zr[r].data_ptr(), len(points_of[r]),
                                                        d_yr[r].data_ptr(), None))
        d_y = torch.cat([y[:y.numel() // 2] for y in d_yr] + [y[y.numel() // 2:] for y in d_yr])
        G = torch.empty(2 * N, dtype=torch.int64, device="cuda")
        Gr = [torch.empty(2 * N, dtype=torch.int64, device="cuda") for _ in range(R)]
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        # (a) the codeword
        nbytes = (Ctot + 2) * 8 * N
        t_fused = report(dict(base, op="mpcs_combine_dev", bytes=nbytes),
                         time_ms(lambda k: mp.combine_dev(mat_p[k % copies], d_y.data_ptr(), d_z.data_ptr(), d_alpha.data_ptr(), G.data_ptr(),
                                                          st.data_ptr())))

        def composed(k):
            for r in range(R):
                per[r].combine_dev(mat_p[k % copies][r], d_yr[r].data_ptr(), d_zr[r].data_ptr(), d_alpha.data_ptr(), Gr[r].data_ptr(),
                                   st.data_ptr())
            L.check(L.lib.ronk_ext2_vec_add_dev(p, w, Gr[0].data_ptr(), Gr[1].data_ptr(), G.data_ptr(), N, None))
            for r in range(2, R):
                L.check(L.lib.ronk_ext2_vec_add_dev(p, w, G.data_ptr(), Gr[r].data_ptr(), G.data_ptr(), N, None))

        t_comp = report(dict(base, op="composed_deep_combine_and_add", calls=R, add_passes=R - 1), time_ms(composed))
        print(json.dumps(dict(base, op="combine_fused_over_composed", ratio=round(t_fused / t_comp, 3),
                              fused_GBs=round(nbytes / (t_fused * 1e-3) / 1e9, 1))), flush=True)
        del Gr
        # (b) the opening, (c) the verifier
        seed = dev(np.arange(1, DIGEST + 1, dtype=np.uint64))
        trees = [[torch.empty(mp.tree_words, dtype=torch.int64, device="cuda") for _ in range(R)] for _ in range(copies)]
        for k in range(copies):
            for r in range(R):
                mp.commit_dev(r, mat_p[k][r], trees[k][r].data_ptr())
        tree_p = ptrs(trees)
        work = torch.empty(mp.workspace_words, dtype=torch.int64, device="cuda")
        proof = torch.empty(mp.proof_words, dtype=torch.int64, device="cuda")
        t_open = report(dict(base, op="mpcs_open_dev", proof_words=mp.proof_words, workspace_words=mp.workspace_words),
                        time_ms(lambda k: mp.open_dev(mat_p[k % copies], tree_p[k % copies], coef_p[k % copies], d_z.data_ptr(), seed.data_ptr(),
                                                      work.data_ptr(), proof.data_ptr(), st.data_ptr())))
        works = [torch.empty(h.workspace_words, dtype=torch.int64, device="cuda") for h in per]
        proofs = [torch.empty(h.proof_words, dtype=torch.int64, device="cuda") for h in per]

        def open_per_round(k):
            for r in range(R):
                per[r].open_dev(mat_p[k % copies][r], tree_p[k % copies][r], coef_p[k % copies][r], d_zr[r].data_ptr(), seed.data_ptr(),
                                works[r].data_ptr(), proofs[r].data_ptr(), st.data_ptr())

        t_open_r = report(dict(base, op="pcs_open_dev_per_round", proof_words=sum(h.proof_words for h in per)), time_ms(open_per_round))
        mp.open_dev(mat_p[0], tree_p[0], coef_p[0], d_z.data_ptr(), seed.data_ptr(), work.data_ptr(), proof.data_ptr(), st.data_ptr())
        open_per_round(0)
        roots = torch.cat([t[-DIGEST:] for t in trees[0]]).clone()
        t_ver = report(dict(base, op="mpcs_verify_dev"),
                       time_ms(lambda k: mp.verify_dev(roots.data_ptr(), d_z.data_ptr(), seed.data_ptr(), proof.data_ptr(), st.data_ptr())))
        torch.cuda.synchronize()
        status = int(st.item())
        sts = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(R)]

        def verify_per_round(k):
            for r in range(R):
                per[r].verify_dev(roots.data_ptr() + 8 * DIGEST * r, d_zr[r].data_ptr(), seed.data_ptr(), proofs[r].data_ptr(), sts[r].data_ptr())

        t_ver_r = report(dict(base, op="pcs_verify_dev_per_round"), time_ms(verify_per_round))
        torch.cuda.synchronize()
        print(json.dumps(dict(base, op="mpcs_over_per_round", mpcs_verify_status=status, pcs_verify_statuses=[int(s.item()) for s in sts],
                              open_ratio=round(t_open / t_open_r, 3), verify_ratio=round(t_ver / t_ver_r, 3),
                              proof_words=mp.proof_words, per_round_proof_words=sum(h.proof_words for h in per),
                              proof_ratio=round(mp.proof_words / sum(h.proof_words for h in per), 3))), flush=True)
        mp.close()
        for h in per:
            h.close()
        del mats, coefs, trees, work, proof, works, proofs, G, mat_p, coef_p, tree_p
        torch.cuda.empty_cache()
    pos.close()


if __name__ == "__main__":
    main()
