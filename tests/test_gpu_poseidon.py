"""Poseidon, its sponge and the Merkle commitment on the device (ronk_poseidon_*, ronk_merkle_*), bit-exact against the Python
restatement (tests/poseidon_ref.py) and, for trees too large for it, against the C restatement of tests/emu/emu_poseidon.cpp, which
the Python one pins here first.  The 64-bit primes run with TEST parameters derived in poseidon_ref.py (not a standard instance)."""
import ctypes as C
import json
import os
import subprocess
import time

import numpy as np
import pytest

import oracle as orc
import poseidon_ref as PR
import prime_classes as PC
import ronkathon_amd as R
from ronkathon_amd import _lib as L
from ronkathon_amd import callers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GP, GG = R.GOLDILOCKS_P, R.GOLDILOCKS_G
FIELDS = [PR.GOLDILOCKS, PR.MONT_P]
# MONT_P's sums all but never land in [p, 2^64) and never in a tile together with a carry: the primes of tests/prime_classes.py
# take every outcome of mont64::add and of PosMont::acc_mad's conditional subtraction
CLASS_FIELDS = PC.CLASS_FIELDS
CLASS_WIDTHS = (2, 8, 12, 16)     # the register widths' ends; at 16 the lazy accumulator holds its maximum of 16 products


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def cref():
    """the C restatement as a shared object (OpenMP over the nodes of a level)"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    so = os.path.join(ROOT, "build", "libposref.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_poseidon.cpp")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        tmp = "%s.tmp.%d" % (so, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-DEMU_POSEIDON_LIB", "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    vp, u64, u32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t
    lib.posref_merkle.argtypes = [u64, u32, u64, u32, u32, u32, vp, vp, vp, sz, sz, sz, sz, sz, vp]
    lib.posref_merkle.restype = None
    lib.posref_tree_words.argtypes = [sz, sz]
    lib.posref_tree_words.restype = sz
    return lib


def c_tree(cref, P, leaves, n, leaf_len, item_stride, elem_stride, d):
    rc = L.arr(P.rc); mds = L.arr([v for row in P.mds for v in row])
    tree = np.empty(cref.posref_tree_words(n, d), dtype=np.uint64)
    cref.posref_merkle(P.p, P.width, P.alpha, P.num_p, P.num_f, P.rate, L.ptr(rc), L.ptr(mds), L.ptr(leaves), n, leaf_len, item_stride,
                       elem_stride, d, L.ptr(tree))
    return tree


def words(seed, size, p):
    """field words with the edges mixed in: 0, p - 1 and values >= p (reduced by the library)"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2**63, size=size, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=size, dtype=np.uint64)
    k = rng.integers(0, 8, size=size)
    v[k == 0] = np.uint64(p - 1)
    v[k == 1] = 0
    v[k == 2] = np.uint64(p) + rng.integers(0, min(5, 2**64 - p), size=int((k == 2).sum()), dtype=np.uint64)
    return v


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def handle(P):
    return L.PoseidonHandle(*P.create_args())


def test_reference_vector_f101():
    """src/hashes/poseidon/tests/mod.rs:85-91 through ronk_poseidon_hash"""
    with open(os.path.join(ROOT, "tests", "golden", "poseidon_f101_w16.json")) as f:
        v = json.load(f)
    pos = callers.Poseidon(R.PlutoBaseField, v["width"], v["alpha"], v["num_p"], v["num_f"], v["rc"], v["mds"])
    assert pos.hash([0] * 16) == v["hash_zero_state"] == 20
    assert pos.hash([]) == 20
    P = PR.Params(101, 16, 3, v["num_p"], v["num_f"], 15, v["rc"], v["mds"])
    for x in ([1], [100, 0, 55], list(range(16)), [101, 202, 5]):
        assert pos.permute(x) == PR.permute(P, x + [0] * (16 - len(x)))
    with pytest.raises(L.RonkPanic) as e:
        pos.hash([0] * 17)
    assert e.value.code == L.ERR_INDEX
    sp = callers.PoseidonSponge(R.PlutoBaseField, 16, 3, v["num_p"], v["num_f"], 6, v["rc"], v["mds"])
    P6 = PR.Params(101, 16, 3, v["num_p"], v["num_f"], 6, v["rc"], v["mds"])
    assert sp.absorb([1, 2, 3]).absorb(list(range(20))).squeeze(9) == PR.sponge(P6, [1, 2, 3] + list(range(20)), 9)


def check_permutation(torch, p, widths):
    for width in widths:
        alpha = (3, 5, 7, 11)[width % 4]
        P = PR.derive_params(p, width, alpha, 3, 4 + (width & 1), max(1, width - 1))
        h = handle(P)
        count = 70
        st = words(width, count * width, p)
        st[:width] = np.uint64(p - 1)
        d = dev(torch, st)
        h.permute_dev(d.data_ptr(), count)
        got = host(torch, d).reshape(count, width)
        for i in range(count):
            assert got[i].tolist() == PR.permute(P, [int(x) for x in st[i * width:(i + 1) * width]]), (p, width, i)
        h.close()


@pytest.mark.parametrize("p", FIELDS)
def test_permutation_all_widths(torch, p):
    check_permutation(torch, p, range(2, 17))


@pytest.mark.parametrize("p", CLASS_FIELDS)
def test_permutation_prime_classes(torch, p):
    check_permutation(torch, p, CLASS_WIDTHS)


def check_sponge(torch, p, widths):
    for width in widths:
        for rate in sorted({1, max(1, width // 2), width - 1}):
            alpha = (3, 5, 7, 11)[(width + rate) % 4]
            P = PR.derive_params(p, width, alpha, 3, 4, rate)
            h = handle(P)
            items, maxlen = 4, 3 * rate + 2
            mat = words(width * 100 + rate, items * maxlen, p)
            d_rows = dev(torch, mat)                                           # item i = row i (contiguous)
            d_cols = dev(torch, mat.reshape(items, maxlen).T.copy())           # item i = column i of a [maxlen][items] matrix
            for length in sorted({0, 1, rate - 1, rate, rate + 1, 3 * rate + 2}):
                want_all = [PR.sponge(P, [int(x) for x in mat[i * maxlen:i * maxlen + length]], rate + 3) for i in range(items)]
                for n_out in sorted({1, rate, rate + 3}):
                    for d_in, (i_s, e_s) in ((d_rows, (maxlen, 1)), (d_cols, (1, items))):
                        out = torch.full((items * n_out,), -1, dtype=torch.int64, device="cuda")
                        h.sponge_dev(d_in.data_ptr(), items, length, i_s, e_s, out.data_ptr(), n_out)
                        got = host(torch, out).reshape(items, n_out)
                        for i in range(items):
                            assert got[i].tolist() == want_all[i][:n_out], (p, width, rate, length, n_out, i_s)
                if length == 0:
                    assert all(v == 0 for w in want_all for v in w[:rate])     # no permutation before the first rate outputs
            h.close()


@pytest.mark.parametrize("p", FIELDS)
def test_sponge_all_widths_both_layouts(torch, p):
    check_sponge(torch, p, range(2, 17))


@pytest.mark.parametrize("p", CLASS_FIELDS)
def test_sponge_both_layouts_prime_classes(torch, p):
    check_sponge(torch, p, CLASS_WIDTHS)


def _check_tree(torch, P, h, n, leaf_len, d, seed):
    leaves = words(seed, n * leaf_len, P.p)
    ref = PR.MerkleTree(P, [[int(x) for x in leaves[i * leaf_len:(i + 1) * leaf_len]] for i in range(n)], d)
    flat = np.array(ref.flat(), dtype=np.uint64)
    assert L.merkle_tree_words(n, d) == flat.size
    off = 0
    for lvl, nodes in enumerate(ref.levels):
        assert L.merkle_level_offset(n, d, lvl) == off
        off += len(nodes) * d
    d_leaves = dev(torch, leaves)
    d_tree = torch.full((flat.size,), -1, dtype=torch.int64, device="cuda")
    h.merkle_commit_dev(d_leaves.data_ptr(), n, leaf_len, leaf_len, 1, d, d_tree.data_ptr())
    assert np.array_equal(host(torch, d_tree), flat), ("tree", P.p, n)
    # the same leaves as the columns of a [leaf_len][n] matrix
    d_cols = dev(torch, leaves.reshape(n, leaf_len).T.copy())
    d_tree2 = torch.full((flat.size,), -1, dtype=torch.int64, device="cuda")
    h.merkle_commit_dev(d_cols.data_ptr(), n, leaf_len, 1, n, d, d_tree2.data_ptr())
    assert np.array_equal(host(torch, d_tree2), flat), ("tree from columns", P.p, n)
    # proofs for every index and two beyond
    depth = len(ref.levels) - 1
    idx = np.arange(n + 2, dtype=np.uint64)
    d_idx = dev(torch, idx)
    d_paths = torch.full((max(idx.size * depth * d, 1),), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((idx.size,), 77, dtype=torch.int32, device="cuda")
    L.merkle_open_dev(d_tree.data_ptr(), n, d, d_idx.data_ptr(), idx.size, d_paths.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    st = d_st.cpu().numpy()
    paths = host(torch, d_paths)[:idx.size * depth * d].reshape(idx.size, depth * d)
    good = []
    for i in range(n + 2):
        try:
            proof = ref.get_proof(i)
        except IndexError:
            assert st[i] == L.ERR_INDEX and not paths[i].any(), (n, i)
            continue
        assert st[i] == 0 and paths[i].tolist() == [w for sib, _ in proof for w in sib], (n, i)
        good.append(i)
    assert good
    # verify: every true path is accepted ...
    g = np.array(good, dtype=np.uint64)
    gl = np.concatenate([leaves[i * leaf_len:(i + 1) * leaf_len] for i in good])
    gp = paths[good].copy() if depth else np.zeros((len(good), 0), dtype=np.uint64)
    d_root = d_tree[flat.size - d:]

    def verify(lv, ix, pa):
        ok = torch.full((len(ix),), 5, dtype=torch.int32, device="cuda")
        dl, di, dp = dev(torch, lv), dev(torch, ix), dev(torch, pa.reshape(-1) if pa.size else np.zeros(1, dtype=np.uint64))
        h.merkle_verify_dev(dl.data_ptr(), len(ix), leaf_len, leaf_len, 1, di.data_ptr(), dp.data_ptr(), n, d, d_root.data_ptr(),
                            ok.data_ptr())
        torch.cuda.synchronize()
        return ok.cpu().numpy()

    assert (verify(gl, g, gp) == 1).all(), ("verify", n)
    # ... and one flipped word, a wrong index or a wrong leaf is rejected
    if depth:
        rng = np.random.default_rng(seed)
        bad = gp.copy()
        col = rng.integers(0, depth * d, size=len(good))
        bad[np.arange(len(good)), col] ^= np.uint64(1) << np.uint64(int(rng.integers(0, 20)))
        assert (verify(gl, g, bad) == 0).all(), ("flipped word", n)
        # the neighbour's index swaps the two halves of the first node: MerkleTree::prove accepts that exactly when the two
        # leaves have the same digest (the edge values make equal neighbouring leaves likely in a large tree)
        twin = np.array([1 if ref.levels[0][i] == ref.levels[0][i ^ 1] else 0 for i in good], dtype=np.int32)
        assert np.array_equal(verify(gl, g ^ np.uint64(1), gp), twin), ("wrong index", n)
        assert not twin.all()
        assert (verify(gl, g + np.uint64(2 * n), gp) == 0).all(), ("index out of range", n)
    if n > 1:
        wl = gl.copy().reshape(len(good), leaf_len)
        wl[:, 0] = (wl[:, 0] % np.uint64(P.p - 1)) + np.uint64(1) if leaf_len else wl[:, 0]
        same = wl[:, 0] % np.uint64(P.p) == gl.reshape(len(good), leaf_len)[:, 0] % np.uint64(P.p)
        assert (verify(wl.reshape(-1), g, gp)[~same] == 0).all(), ("wrong leaf", n)
    return flat


@pytest.mark.parametrize("p", FIELDS)
def test_merkle_against_python_tree(torch, p):
    P = PR.derive_params(p, 5, 5, 3, 4, 3)
    h = handle(P)
    for n in (1, 2, 3, 5, 64, 257, 4096, 5000):
        _check_tree(torch, P, h, n, 4 if n < 4096 else 2, 2, 1000 + n)
    h.close()
    # digest_len == rate (two permutations per node) and a wide state
    P = PR.derive_params(p, 12, 7, 2, 2, 8)
    h = handle(P)
    for n, d in ((257, 8), (5, 1), (300, 4)):
        _check_tree(torch, P, h, n, 9, d, 2000 + n)
    h.close()


@pytest.mark.parametrize("p", CLASS_FIELDS)
def test_merkle_odd_level_prime_classes(torch, p):
    """300 leaves: more than one workgroup of 256 nodes, and the levels 75 and 19 are odd (the last node pairs with itself)"""
    P = PR.derive_params(p, 12, 7, 2, 2, 8)
    h = handle(P)
    _check_tree(torch, P, h, 300, 9, 4, 2300)
    h.close()


def test_host_forms_and_python_tree():
    P = PR.derive_params(PR.GOLDILOCKS, 8, 7, 3, 4, 4)
    leaves = [[(i * 131 + j * 7) % 1000 for j in range(5)] for i in range(13)]
    t = callers.MerkleTree((R.GoldilocksField,) + P.create_args()[1:], leaves, 4)
    ref = PR.MerkleTree(P, leaves, 4)
    assert t.root_hash() == ref.root_hash() and t.tree.tolist() == ref.flat()
    for i in range(14):
        try:
            want = ref.get_proof(i)
        except IndexError:
            with pytest.raises(L.RonkPanic) as e:
                t.get_proof(i)
            assert e.value.code == L.ERR_INDEX
            continue
        proof = t.get_proof(i)
        assert proof == want
        assert t.prove(leaves[i], proof)
        assert not t.prove(leaves[(i + 1) % 13], proof)
        assert not t.prove(leaves[i], proof[:-1])
    one = callers.MerkleTree((R.GoldilocksField,) + P.create_args()[1:], [[1, 2, 3]], 4)
    assert one.get_proof(0) == [] and one.root_hash() == PR.sponge(P, [1, 2, 3], 4) and one.prove([1, 2, 3], [])
    h = handle(P)
    assert L.lib.ronk_merkle_commit_dev(h.h, C.c_void_p(16), 0, 3, 3, 1, 4, C.c_void_p(16), None) == L.ERR_INVALID    # n_leaves == 0
    assert L.lib.ronk_merkle_commit_dev(h.h, C.c_void_p(16), 4, 3, 3, 1, 5, C.c_void_p(16), None) == L.ERR_INVALID    # digest > rate
    h.close()


@pytest.mark.parametrize("p", FIELDS)
def test_large_trees_against_c_restatement(torch, cref, p):
    """2^16 leaves x 8 elements: the whole tree.  2^20 leaves x 16 elements (width 12, rate 8, alpha 7, 8 + 22 rounds, digest 4):
    the root and the paths of 1024 indices (0, n - 1 and 1022 seeded ones).  The 2^20 size is kept: its CPU side measured well
    under two minutes on 16 threads."""
    # the C restatement is pinned by the Python one first
    Ps = PR.derive_params(p, 6, 5, 2, 3, 4)
    n, ll, d = 37, 5, 3
    lv = words(5, n * ll, p)
    want = PR.MerkleTree(Ps, [[int(x) for x in lv[i * ll:(i + 1) * ll]] for i in range(n)], d).flat()
    assert c_tree(cref, Ps, lv, n, ll, ll, 1, d).tolist() == want
    P = PR.derive_params(p, 12, 7, 22, 8, 8)
    h = handle(P)
    d = 4
    # 2^16 x 8, as the columns of an [8][2^16] matrix
    n, ll = 1 << 16, 8
    mat = words(6, n * ll, p)
    t0 = time.time()
    want = c_tree(cref, P, mat, n, ll, 1, n, d)
    print("C restatement 2^16 x 8: %.1f s" % (time.time() - t0))
    d_mat = dev(torch, mat)
    d_tree = torch.full((want.size,), -1, dtype=torch.int64, device="cuda")
    h.merkle_commit_dev(d_mat.data_ptr(), n, ll, 1, n, d, d_tree.data_ptr())
    assert np.array_equal(host(torch, d_tree), want)
    del d_mat, d_tree
    # 2^20 x 16, contiguous leaves
    n, ll = 1 << 20, 16
    mat = words(7, n * ll, p)
    t0 = time.time()
    want = c_tree(cref, P, mat, n, ll, ll, 1, d)
    print("C restatement 2^20 x 16: %.1f s" % (time.time() - t0))
    d_mat = dev(torch, mat)
    d_tree = torch.full((want.size,), -1, dtype=torch.int64, device="cuda")
    h.merkle_commit_dev(d_mat.data_ptr(), n, ll, ll, 1, d, d_tree.data_ptr())
    torch.cuda.synchronize()
    root = host(torch, d_tree[want.size - d:])
    assert root.tolist() == want[-d:].tolist()
    rng = np.random.default_rng(11)
    idx = np.concatenate([np.array([0, n - 1], dtype=np.uint64), rng.integers(0, n, size=1022, dtype=np.uint64)])
    depth = 20
    d_idx = dev(torch, idx)
    d_paths = torch.full((idx.size * depth * d,), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((idx.size,), 77, dtype=torch.int32, device="cuda")
    L.merkle_open_dev(d_tree.data_ptr(), n, d, d_idx.data_ptr(), idx.size, d_paths.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    paths = host(torch, d_paths).reshape(idx.size, depth, d)
    for q, i in enumerate(idx):
        i = int(i); off = 0; cnt = n
        for l in range(depth):
            s = (i >> l) ^ 1
            assert paths[q, l].tolist() == want[off + s * d: off + s * d + d].tolist(), (q, l)
            off += cnt * d; cnt = (cnt + 1) // 2
    ok = torch.full((idx.size,), 5, dtype=torch.int32, device="cuda")
    d_l = dev(torch, np.concatenate([mat[int(i) * ll:(int(i) + 1) * ll] for i in idx]))
    h.merkle_verify_dev(d_l.data_ptr(), idx.size, ll, ll, 1, d_idx.data_ptr(), d_paths.data_ptr(), n, d, d_tree[want.size - d:].data_ptr(),
                        ok.data_ptr())
    torch.cuda.synchronize()
    assert (ok.cpu().numpy() == 1).all()
    h.close()


def test_pipeline_lde_then_commit(torch, cref):
    """ronk_lde_batch_dev (16 x 2^12 -> 2^14), then ronk_merkle_commit_dev on its output with strides (1, N): the tree over the
    oracle's extension values, and an opened column verifies"""
    lk, ln, batch = 12, 14, 16
    K, N = 1 << lk, 1 << ln
    pk = L.Plan(GP, GG, lk, batch); pn = L.Plan(GP, GG, ln, batch)
    ev = words(21, K * batch, GP) % np.uint64(GP)
    d_ev = dev(torch, ev)
    d_co = torch.empty(K * batch, dtype=torch.int64, device="cuda"); d_out = torch.empty(N * batch, dtype=torch.int64, device="cuda")
    L.check(L.lib.ronk_lde_batch_dev(pk.h, pn.h, d_ev.data_ptr(), d_co.data_ptr(), d_out.data_ptr(), 1, 0))
    want_mat = np.concatenate([orc.fft(GP, GG, np.concatenate([orc.ifft(GP, GG, ev[b * K:(b + 1) * K]), np.zeros(N - K, dtype=np.uint64)]))
                               for b in range(batch)])
    P = PR.derive_params(GP, 12, 7, 22, 8, 8)
    h = handle(P)
    d = 4
    want = c_tree(cref, P, want_mat, N, batch, 1, N, d)
    d_tree = torch.full((want.size,), -1, dtype=torch.int64, device="cuda")
    h.merkle_commit_dev(d_out.data_ptr(), N, batch, 1, N, d, d_tree.data_ptr())
    assert np.array_equal(host(torch, d_tree), want)
    # one column of the Python restatement pins the leaf digest
    col = 4097
    assert want[col * d:(col + 1) * d].tolist() == PR.sponge(P, [int(want_mat[b * N + col]) for b in range(batch)], d)
    idx = dev(torch, np.array([col], dtype=np.uint64))
    depth = ln
    d_path = torch.zeros(depth * d, dtype=torch.int64, device="cuda"); d_st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    L.merkle_open_dev(d_tree.data_ptr(), N, d, idx.data_ptr(), 1, d_path.data_ptr(), d_st.data_ptr())
    ok = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    # the opened column, read in place from the extension (item stride 1, element stride N, starting at the column)
    h.merkle_verify_dev(d_out.data_ptr() + 8 * col, 1, batch, 1, N, idx.data_ptr(), d_path.data_ptr(), N, d,
                        d_tree[want.size - d:].data_ptr(), ok.data_ptr())
    torch.cuda.synchronize()
    assert int(d_st.item()) == 0 and int(ok.item()) == 1
    pk.close(); pn.close(); h.close()


def test_commit_under_stream_capture(torch):
    """ronk_merkle_commit_dev uses no library workspace: recorded into a graph and replayed twice, the same tree"""
    P = PR.derive_params(GP, 8, 5, 4, 4, 4)
    h = handle(P)
    n, ll, d = 70000, 6, 4        # the leaf launch, nine level launches (an odd level among them) and the one-workgroup top
    size = L.merkle_tree_words(n, d)
    s = torch.cuda.Stream()
    d_leaves = torch.zeros(n * ll, dtype=torch.int64, device="cuda")
    d_tree = torch.zeros(size, dtype=torch.int64, device="cuda")
    d_plain = torch.zeros(size, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        h.merkle_commit_dev(d_leaves.data_ptr(), n, ll, ll, 1, d, d_tree.data_ptr(), st)
    for rep in range(2):
        lv = words(30 + rep, n * ll, GP)
        d_leaves.copy_(torch.from_numpy(lv.view(np.int64)))
        d_tree.fill_(-1)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        h.merkle_commit_dev(d_leaves.data_ptr(), n, ll, ll, 1, d, d_plain.data_ptr())
        got, plain = host(torch, d_tree), host(torch, d_plain)
        assert np.array_equal(got, plain)
        ref = PR.sponge(P, [int(x) for x in lv[5 * ll:6 * ll]], d)
        assert got[5 * d:6 * d].tolist() == ref
    h.close()
