"""Times the batched FRI polynomial commitment (ronk_deep_combine_dev, ronk_pcs_open_dev, ronk_pcs_verify_dev) with hipEvents around
`iters` back-to-back calls after warm-up, median of `rounds`, and in the same run, on the same buffers:
  (a) the codeword G composed from the element-wise entry points the library had before the fused kernel, term by term (per column
      and point ronk_ext2_vec_mul_base_dev, _sub_dev, _mul_dev, _add_dev, one ronk_ext2_vec_inv_dev per point; the broadcast constants
      are prepared outside the timed region) and in the S_i / Y_k form (2 C + 6 K passes); both results are compared with the fused one;
  (b) the bytes the combine kernel moves, (C + 2) 8 N, over its time;
  (c) ronk_fri_prove_dev / ronk_fri_verify_dev on an extension handle with a planar input at the same N.
The matrix is a real low-degree extension (coefficients through the library's NTT, coset shift 1), so the verifier's status is
reported and must be 0.  Matrices rotate over enough copies to exceed the 256 MiB Infinity Cache.  One JSON line per case.  The
Poseidon parameters are TEST parameters (width 12, alpha 7, 8 full + 22 partial rounds, rate 8).

usage: python tools/pcs_time.py [--iters 10] [--warmup 2] [--rounds 3] [--log2-sizes 20,22] [--field gl] [--columns 16] [--points 2]"""
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
ap.add_argument("--columns", type=int, default=16)
ap.add_argument("--points", type=int, default=2)
ap.add_argument("--no-composed", action="store_true")
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


def const_planar(e, n):
    """the extension element e broadcast over n points, planar"""
    t = torch.empty(2 * n, dtype=torch.int64, device="cuda")
    t[:n] = int(np.array([e[0]], dtype=np.uint64).view(np.int64)[0])
    t[n:] = int(np.array([e[1]], dtype=np.uint64).view(np.int64)[0])
    return t


def main():
    p, g = PRIMES[args.field]
    w = g
    E = ER.Ext2(p, w)
    eta, Q, C, K = args.eta, args.queries, args.columns, args.points
    P = PR.derive_params(p, 12, 7, 22, 8, 8)
    pos = L.PoseidonHandle(*P.create_args())
    rng = np.random.default_rng(1)
    for n in (int(v) for v in args.log2_sizes.split(",")):
        log2_final = n - eta * max(1, -(-(n - 8) // eta))
        blow = min(BLOWUP, log2_final)
        N, d = 1 << n, (1 << n) >> blow
        pcs = L.PcsHandle(pos, g, w, n, 1, eta, log2_final, blow, Q, DIGEST, C, K)
        base = {"field": args.field, "w": w, "log2_n": n, "eta": eta, "log2_final": log2_final, "queries": Q, "digest": DIGEST,
                "columns": C, "points": K}
        # matrices: the values of C polynomials of degree < d on <w_N>, through the library's transform
        copies = max(2, min(8, (512 << 20) // (8 * N * C)))
        plan = L.Plan(p, g, n, batch=C)
        coefs, mats = [], []
        for _ in range(copies):
            c = rng.integers(0, 2**63, size=(C, d), dtype=np.uint64) % np.uint64(p)
            padded = torch.zeros((C, N), dtype=torch.int64, device="cuda")
            padded[:, :d] = dev(c)
            m = torch.empty(C * N, dtype=torch.int64, device="cuda")
            plan.forward_dev(padded.data_ptr(), m.data_ptr())
            coefs.append(dev(c.ravel()))
            mats.append(m)
            del padded
        torch.cuda.synchronize()
        plan.close()
        zs = [(int(rng.integers(1, 2**62)) % p, int(rng.integers(1, 2**62)) % p) for _ in range(K)]
        d_z = dev(np.array(ER.planar(zs), dtype=np.uint64))
        alpha = (int(rng.integers(1, 2**62)) % p, int(rng.integers(1, 2**62)) % p)
        d_alpha = dev(np.array(alpha, dtype=np.uint64))
        d_y = torch.empty(2 * K * C, dtype=torch.int64, device="cuda")
        t_eval = report(dict(base, op="ext2_poly_eval_batch_dev", coefficients=d),
                        time_ms(lambda k: L.check(L.lib.ronk_ext2_poly_eval_batch_dev(p, w, coefs[k % copies].data_ptr(), C, d, d_z.data_ptr(),
                                                                                       K, d_y.data_ptr(), None))))
        L.check(L.lib.ronk_ext2_poly_eval_batch_dev(p, w, coefs[0].data_ptr(), C, d, d_z.data_ptr(), K, d_y.data_ptr(), None))
        G = torch.empty(2 * N, dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        t_comb = report(dict(base, op="deep_combine_dev", bytes=(C + 2) * 8 * N),
                        time_ms(lambda k: pcs.combine_dev(mats[k % copies].data_ptr(), d_y.data_ptr(), d_z.data_ptr(), d_alpha.data_ptr(),
                                                          G.data_ptr(), st.data_ptr())))
        print(json.dumps(dict(base, op="deep_combine_rate", GBs=round((C + 2) * 8 * N / (t_comb * 1e-3) / 1e9, 1))), flush=True)
        if not args.no_composed:
            # (a) the same codeword from the element-wise entry points.  Outside the timed region: x_i, the broadcast constants.
            ys = d_y.cpu().numpy().view(np.uint64).tolist()
            y = [[(ys[k * C + c], ys[K * C + k * C + c]) for c in range(C)] for k in range(K)]
            xs = np.empty(N, dtype=np.uint64)
            wn, x = pow(g, (p - 1) >> n, p), 1
            for i in range(N):
                xs[i] = x
                x = x * wn % p
            X = torch.cat([dev(xs), torch.zeros(N, dtype=torch.int64, device="cuda")])
            Zc = [const_planar(z, N) for z in zs]
            ap_ = [E.one]
            for _ in range(K * C):
                ap_.append(E.mul(ap_[-1], alpha))
            A_kc = [[const_planar(ap_[k * C + c], N) for c in range(C)] for k in range(K)]
            AY_kc = [[const_planar(E.mul(ap_[k * C + c], y[k][c]), N) for c in range(C)] for k in range(K)]
            Qk, T, Gc = [torch.empty(2 * N, dtype=torch.int64, device="cuda") for _ in range(K)], torch.empty(2 * N, dtype=torch.int64, device="cuda"), torch.empty(2 * N, dtype=torch.int64, device="cuda")
            lib = L.lib

            def composed(kk):
                M = mats[kk % copies]
                Gc.zero_()
                for k in range(K):
                    L.check(lib.ronk_ext2_vec_sub_dev(p, w, X.data_ptr(), Zc[k].data_ptr(), Qk[k].data_ptr(), N, None))
                    L.check(lib.ronk_ext2_vec_inv_dev(p, w, Qk[k].data_ptr(), Qk[k].data_ptr(), N, None, None))
                    for c in range(C):
                        L.check(lib.ronk_ext2_vec_mul_base_dev(p, w, A_kc[k][c].data_ptr(), M.data_ptr() + 8 * c * N, T.data_ptr(), N, None))
                        L.check(lib.ronk_ext2_vec_sub_dev(p, w, T.data_ptr(), AY_kc[k][c].data_ptr(), T.data_ptr(), N, None))
                        L.check(lib.ronk_ext2_vec_mul_dev(p, w, T.data_ptr(), Qk[k].data_ptr(), T.data_ptr(), N, None))
                        L.check(lib.ronk_ext2_vec_add_dev(p, w, Gc.data_ptr(), T.data_ptr(), Gc.data_ptr(), N, None))

            t_cmp = report(dict(base, op="composed_per_term", passes=K * (2 + 4 * C)), time_ms(composed))
            pcs.combine_dev(mats[0].data_ptr(), d_y.data_ptr(), d_z.data_ptr(), d_alpha.data_ptr(), G.data_ptr(), st.data_ptr())
            composed(0)
            torch.cuda.synchronize()
            same = bool(torch.equal(G, Gc))
            # the S_i / Y_k form: S = sum_c alpha^c M_c once, then per point (S - Y_k) B_k / (x - z_k)
            Yk = [const_planar(tuple(sum(v) % p for v in zip(*[E.mul(ap_[c], y[k][c]) for c in range(C)])), N) for k in range(K)]
            Bk = [const_planar(ap_[k * C], N) for k in range(K)]
            S = torch.empty(2 * N, dtype=torch.int64, device="cuda")

            def composed_sy(kk):
                M = mats[kk % copies]
                Gc.zero_()
                S.zero_()
                for c in range(C):
                    L.check(lib.ronk_ext2_vec_mul_base_dev(p, w, A_kc[0][c].data_ptr(), M.data_ptr() + 8 * c * N, T.data_ptr(), N, None))
                    L.check(lib.ronk_ext2_vec_add_dev(p, w, S.data_ptr(), T.data_ptr(), S.data_ptr(), N, None))
                for k in range(K):
                    L.check(lib.ronk_ext2_vec_sub_dev(p, w, X.data_ptr(), Zc[k].data_ptr(), Qk[k].data_ptr(), N, None))
                    L.check(lib.ronk_ext2_vec_inv_dev(p, w, Qk[k].data_ptr(), Qk[k].data_ptr(), N, None, None))
                    L.check(lib.ronk_ext2_vec_sub_dev(p, w, S.data_ptr(), Yk[k].data_ptr(), T.data_ptr(), N, None))
                    L.check(lib.ronk_ext2_vec_mul_dev(p, w, T.data_ptr(), Bk[k].data_ptr(), T.data_ptr(), N, None))
                    L.check(lib.ronk_ext2_vec_mul_dev(p, w, T.data_ptr(), Qk[k].data_ptr(), T.data_ptr(), N, None))
                    L.check(lib.ronk_ext2_vec_add_dev(p, w, Gc.data_ptr(), T.data_ptr(), Gc.data_ptr(), N, None))

            t_sy = report(dict(base, op="composed_s_y_form", passes=2 * C + 6 * K), time_ms(composed_sy))
            composed_sy(0)
            torch.cuda.synchronize()
            same_sy = bool(torch.equal(G, Gc))
            print(json.dumps(dict(base, op="fused_against_composed", same_words_per_term=same, same_words_s_y=same_sy,
                                  per_term_over_fused=round(t_cmp / t_comb, 2), s_y_over_fused=round(t_sy / t_comb, 2))), flush=True)
            del X, Zc, A_kc, AY_kc, Qk, T, Gc, Yk, Bk, S
        # (c) the whole opening beside the FRI it wraps
        seed = dev(np.arange(1, DIGEST + 1, dtype=np.uint64))
        trees = [torch.empty(pcs.tree_words, dtype=torch.int64, device="cuda") for _ in range(copies)]
        t_commit = report(dict(base, op="pcs_commit_dev", leaves=N >> eta, leaf_len=C << eta),
                          time_ms(lambda k: pcs.commit_dev(mats[k % copies].data_ptr(), trees[k % copies].data_ptr())))
        for k in range(copies):
            pcs.commit_dev(mats[k].data_ptr(), trees[k].data_ptr())
        work = torch.empty(pcs.workspace_words, dtype=torch.int64, device="cuda")
        proof = torch.empty(pcs.proof_words, dtype=torch.int64, device="cuda")
        t_open = report(dict(base, op="pcs_open_dev", proof_words=pcs.proof_words, workspace_words=pcs.workspace_words),
                        time_ms(lambda k: pcs.open_dev(mats[k % copies].data_ptr(), trees[k % copies].data_ptr(), coefs[k % copies].data_ptr(),
                                                       d_z.data_ptr(), seed.data_ptr(), work.data_ptr(), proof.data_ptr(), st.data_ptr())))
        pcs.open_dev(mats[0].data_ptr(), trees[0].data_ptr(), coefs[0].data_ptr(), d_z.data_ptr(), seed.data_ptr(), work.data_ptr(),
                     proof.data_ptr(), st.data_ptr())
        root = trees[0][-DIGEST:].clone()
        t_verify = report(dict(base, op="pcs_verify_dev"),
                          time_ms(lambda k: pcs.verify_dev(root.data_ptr(), d_z.data_ptr(), seed.data_ptr(), proof.data_ptr(), st.data_ptr())))
        torch.cuda.synchronize()
        status = int(st.item())
        pcs.combine_dev(mats[0].data_ptr(), d_y.data_ptr(), d_z.data_ptr(), d_alpha.data_ptr(), G.data_ptr(), st.data_ptr())   # a codeword of low degree
        frx = L.FriHandle(pos, g, n, 1, eta, log2_final, blow, Q, DIGEST, w=w, input_ext=True)
        workx = torch.empty(frx.workspace_words, dtype=torch.int64, device="cuda")
        proofx = torch.empty(frx.proof_words, dtype=torch.int64, device="cuda")
        x_prove = report(dict(base, op="fri_prove_dev", ext=1, input_ext=1),
                         time_ms(lambda k: frx.prove_dev(G.data_ptr(), seed.data_ptr(), workx.data_ptr(), proofx.data_ptr())))
        x_verify = report(dict(base, op="fri_verify_dev", ext=1, input_ext=1),
                          time_ms(lambda k: frx.verify_dev(proofx.data_ptr(), seed.data_ptr(), st.data_ptr())))
        torch.cuda.synchronize()
        print(json.dumps(dict(base, op="pcs_over_fri", pcs_verify_status=status, fri_verify_status=int(st.item()),
                              open_minus_prove_ms=round(t_open - x_prove, 4), verify_minus_verify_ms=round(t_verify - x_verify, 4),
                              open_over_prove=round(t_open / x_prove, 3), verify_over_verify=round(t_verify / x_verify, 3),
                              eval_ms=round(t_eval, 4), combine_ms=round(t_comb, 4), commit_ms=round(t_commit, 4))), flush=True)
        frx.close()
        pcs.close()
        del mats, coefs, trees, work, proof, workx, proofx, G
        torch.cuda.empty_cache()
    pos.close()


if __name__ == "__main__":
    main()
