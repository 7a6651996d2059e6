"""Times the FRI family (ronk_fri_fold_dev per layer, ronk_fri_prove_dev, ronk_fri_verify_dev) with hipEvents around `iters`
back-to-back calls after warm-up, median of `rounds`, and in the same run two yardsticks from existing code: ronk_vec_mul_dev over
N_0 elements and the sum of ronk_merkle_commit_dev calls on the same layer shapes.  Inputs rotate over enough copies to exceed the
256 MiB Infinity Cache (at most 64), so the large layers are read from HBM.  One JSON line per case; the last line per size holds
the two derived figures: layer-0 fold / vec_mul, and prove minus the commits' sum.  The Poseidon parameters are TEST parameters
(width 12, alpha 7, 8 full + 22 partial rounds, rate 8), digest 4, arity 8, 64 queries.

With --ext the same cases are timed again on a handle with extension challenges (ronk_fri_create_ext, W = the generator; --input-ext:
layer 0 is planar pairs too) after the base-field ones, in the same run, and a last line per size holds the ratios.

usage: python tools/fri_time.py [--iters 10] [--warmup 2] [--rounds 3] [--log2-sizes 20,22,24] [--field gl] [--ext] [--input-ext]"""
import argparse
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log2-sizes", default="20,22,24")
ap.add_argument("--field", default="gl")
ap.add_argument("--eta", type=int, default=3)
ap.add_argument("--queries", type=int, default=64)
ap.add_argument("--ext", action="store_true")
ap.add_argument("--input-ext", action="store_true")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

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


def main():
    p, g = PRIMES[args.field]
    eta, A, Q = args.eta, 1 << args.eta, args.queries
    P = PR.derive_params(p, 12, 7, 22, 8, 8)
    pos = L.PoseidonHandle(*P.create_args())
    rng = np.random.default_rng(1)
    for n in (int(v) for v in args.log2_sizes.split(",")):
        log2_final = n - eta * max(1, -(-(n - 8) // eta))
        fri = L.FriHandle(pos, g, n, g, eta, log2_final, min(BLOWUP, log2_final), Q, DIGEST)
        layers = (n - log2_final) // eta
        base = {"field": args.field, "log2_n": n, "eta": eta, "log2_final": log2_final, "layers": layers, "queries": Q, "digest": DIGEST}
        N = 1 << n
        copies = max(1, min(64, (512 << 20) // (8 * N)))
        src = [torch.from_numpy((rng.integers(0, 2**63, size=N, dtype=np.uint64) % np.uint64(p)).view(np.int64)).cuda() for _ in range(min(copies, 4))]
        ins = [src[k % len(src)].clone() for k in range(copies)]
        out = torch.empty(N, dtype=torch.int64, device="cuda")
        beta = torch.from_numpy(np.array([123456789], dtype=np.uint64).view(np.int64)).cuda()
        t_mul = report(dict(base, op="vec_mul_dev", words=N),
                       time_ms(lambda k: L.check(L.lib.ronk_vec_mul_dev(p, ins[k % copies].data_ptr(), ins[(k + 1) % copies].data_ptr(),
                                                                         out.data_ptr(), N, 0))))
        t_fold, t_commit = [], []
        for l in range(layers):
            nl = N >> (eta * l)
            t_fold.append(report(dict(base, op="fold_dev", layer=l, words_in=nl),
                                 time_ms(lambda k: fri.fold_dev(l, ins[k % copies].data_ptr(), beta.data_ptr(), out.data_ptr()))))
            m = nl // A
            tree = torch.empty(L.merkle_tree_words(m, DIGEST), dtype=torch.int64, device="cuda")
            t_commit.append(report(dict(base, op="merkle_commit_dev", layer=l, leaves=m, leaf_len=A),
                                   time_ms(lambda k: pos.merkle_commit_dev(ins[k % copies].data_ptr(), m, A, 1, m, DIGEST, tree.data_ptr()))))
            del tree
        seed = torch.from_numpy(np.arange(1, DIGEST + 1, dtype=np.uint64).view(np.int64)).cuda()
        work = torch.empty(fri.workspace_words, dtype=torch.int64, device="cuda")
        proof = torch.empty(fri.proof_words, dtype=torch.int64, device="cuda")
        t_prove = report(dict(base, op="prove_dev", proof_words=fri.proof_words, workspace_words=fri.workspace_words),
                         time_ms(lambda k: fri.prove_dev(ins[k % copies].data_ptr(), seed.data_ptr(), work.data_ptr(), proof.data_ptr())))
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        t_verify = report(dict(base, op="verify_dev"), time_ms(lambda k: fri.verify_dev(proof.data_ptr(), seed.data_ptr(), st.data_ptr())))
        torch.cuda.synchronize()
        print(json.dumps(dict(base, op="derived", verify_status=int(st.item()), fold0_over_vec_mul=round(t_fold[0] / t_mul, 3),
                              folds_sum_ms=round(sum(t_fold), 4), commits_sum_ms=round(sum(t_commit), 4),
                              prove_minus_commits_ms=round(t_prove - sum(t_commit), 4), verify_ms=round(t_verify, 4))), flush=True)
        if args.ext:
            base_t = {"fold": t_fold, "prove": t_prove, "verify": t_verify}
            ie = bool(args.input_ext)
            frx = L.FriHandle(pos, g, n, g, eta, log2_final, min(BLOWUP, log2_final), Q, DIGEST, w=g, input_ext=ie)
            bx = dict(base, ext=1, input_ext=int(ie), w=g)
            pair = lambda k: (ins[k % copies], ins[(k + 1) % copies])      # two planes: two of the rotating arrays
            planar = [torch.cat(pair(k)) for k in range(min(copies, 8))]
            beta2 = torch.from_numpy(np.array([123456789, 987654321], dtype=np.uint64).view(np.int64)).cuda()
            out2 = torch.empty(2 * N, dtype=torch.int64, device="cuda")
            x_fold = []
            for l in range(layers):
                nl = N >> (eta * l)
                src_l = planar if (l > 0 or ie) else ins
                x_fold.append(report(dict(bx, op="fold_dev", layer=l, words_in=nl * (2 if (l > 0 or ie) else 1)),
                                     time_ms(lambda k: frx.fold_dev(l, src_l[k % len(src_l)].data_ptr(), beta2.data_ptr(), out2.data_ptr()))))
            workx = torch.empty(frx.workspace_words, dtype=torch.int64, device="cuda")
            proofx = torch.empty(frx.proof_words, dtype=torch.int64, device="cuda")
            ev = planar if ie else ins
            x_prove = report(dict(bx, op="prove_dev", proof_words=frx.proof_words, workspace_words=frx.workspace_words),
                             time_ms(lambda k: frx.prove_dev(ev[k % len(ev)].data_ptr(), seed.data_ptr(), workx.data_ptr(), proofx.data_ptr())))
            x_verify = report(dict(bx, op="verify_dev"), time_ms(lambda k: frx.verify_dev(proofx.data_ptr(), seed.data_ptr(), st.data_ptr())))
            torch.cuda.synchronize()
            print(json.dumps(dict(bx, op="ext_over_base", verify_status=int(st.item()),
                                  fold=[round(a / b, 3) for a, b in zip(x_fold, base_t["fold"])],
                                  prove=round(x_prove / base_t["prove"], 3), verify=round(x_verify / base_t["verify"], 3))), flush=True)
            frx.close()
            del planar, out2, workx, proofx
        fri.close()
        del ins, src, out, work, proof
        torch.cuda.empty_cache()
    pos.close()


if __name__ == "__main__":
    main()
