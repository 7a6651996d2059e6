"""The Goldilocks kernels outside the NTT on the DIRECTED inputs of tests/gl_directed.py, through the C ABI.

Uniform residues take the ">= p without a carry" outcome of gl64::add / mad_eps_canon / PosGl::acc_reduce with probability 2^-32
per call, so the parity tests of these kernels never see it; small signed values take it all the time (the census of
tests/test_emu_gl_directed.py counts how often, body by body, on the host emulators).  The device forms of those functions -- the
asm blocks of mad_eps_canon and sub32, the __builtin_addc chains under the device compiler -- exist on the GPU only, and here the
same families run on them: every output bit-exact against the Python references, and every output word below p, asserted on a
line of its own: a kernel that stores p for 0 fails there.

Handles and calls are those of the other GPU tests (test_gpu_fri, _fri_ext, _ext2, _poseidon, _accum, _pcs, _mpcs, _plonk,
_air_per)."""
import numpy as np
import pytest

import gl_directed as GD
import test_gpu_air_per as TAP
import test_gpu_fri as TF
import test_gpu_fri_ext as TFX
import test_gpu_mpcs as TM
import test_gpu_pcs as TP
import test_gpu_plonk as TPL
from ronkathon_amd import _lib as L
from test_gpu_accum import garbage, scan_dev, work_for
from test_gpu_ext2 import run_dev
from test_gpu_fri import dev, host
from test_gpu_poseidon import handle

pytestmark = pytest.mark.gpu

GL = GD.P
WS = (GD.W_SHIFT, GD.W_PLAIN)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def check_words(got, want, what):
    got, want = np.asarray(got, dtype=np.uint64).reshape(-1), np.asarray(want, dtype=np.uint64).reshape(-1)
    assert got.shape == want.shape, what
    over = np.flatnonzero(got >= np.uint64(GL))
    assert over.size == 0, ("an output word is not below p", what, over[:4].tolist(), got[over[:4]].tolist())
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (what, diff.size, diff[:4].tolist(), got[diff[:4]].tolist(), want[diff[:4]].tolist())


# ------------------------------------------------------------------------------------------------ P: Poseidon, sponge, Merkle
# Deliberate deviation: the issue asks for counts 1, 63, 64, 65 and 4097 at every width and for 1001 leaves, and for tests of a few
# seconds; the Python permutation costs 0.2 ms a state at width 3 and 3 ms at width 16, so 4097 states (and 1001 leaves) run for
# every family at widths 3 and 8 and for the `lin` family at widths 12 and 16, where the reference takes up to
# 12 s.  A lane owns one state whatever the width and the family, so the grid-stride tail is the same code in all of them.
PERMUTE_COUNTS = (1, 63, 64, 65)
PERMUTE_COUNTS_LARGE = PERMUTE_COUNTS + (4097,)
FAMILY_WIDTH = [(f, w) for f in GD.POSEIDON_FAMILIES for w in GD.POSEIDON_WIDTHS]


@pytest.mark.parametrize("family,width", FAMILY_WIDTH)
def test_permutation(torch, family, width):
    counts = PERMUTE_COUNTS_LARGE if width <= 8 or family == "lin" else PERMUTE_COUNTS
    Pm, st, want = GD.poseidon_states(family, width, max(counts))
    h = handle(Pm)
    for count in counts:
        d = dev(torch, st[:count].reshape(-1))
        h.permute_dev(d.data_ptr(), count)
        check_words(host(torch, d), want[:count], (family, width, count))
    h.close()


def test_permutation_of_window_words(torch):
    """states of words in [p, 2^64): the library reduces them, the reference too"""
    for width in GD.POSEIDON_WIDTHS:
        Pm = GD.poseidon_params("lin", width)
        st = GD.window_words(65 * width, width).reshape(65, width)
        want = [GD.PR.permute(Pm, [int(v) for v in row]) for row in st]
        h = handle(Pm)
        d = dev(torch, st.reshape(-1))
        h.permute_dev(d.data_ptr(), 65)
        check_words(host(torch, d), want, ("window", width))
        h.close()


def check_sponge(torch, family, width, window):
    items = 65
    Pm, mat, want = GD.poseidon_sponge(family, width, items, window)
    maxlen, n_out = mat.shape[1], Pm.rate + 1
    h = handle(Pm)
    d_rows, d_cols = dev(torch, mat.reshape(-1)), dev(torch, mat.T.copy().reshape(-1))      # (len, 1) and (1, N)
    for length in GD.sponge_lengths(Pm.rate):
        for d_in, (i_s, e_s) in ((d_rows, (maxlen, 1)), (d_cols, (1, items))):
            out = torch.full((items * n_out,), -1, dtype=torch.int64, device="cuda")
            h.sponge_dev(d_in.data_ptr(), items, length, i_s, e_s, out.data_ptr(), n_out)
            check_words(host(torch, out), want[length], (family, width, length, i_s, "window" if window else "small"))
    h.close()


@pytest.mark.parametrize("family,width", FAMILY_WIDTH)
def test_sponge_both_layouts(torch, family, width):
    check_sponge(torch, family, width, False)


def test_sponge_of_window_words(torch):
    check_sponge(torch, "lin", 12, True)


@pytest.mark.parametrize("family,width", FAMILY_WIDTH)
def test_merkle_commit(torch, family, width):
    """5 and 64 leaves: the one-workgroup climb with an odd level; 1001: the level launches above 256 nodes (every family at
    width 8, `lin` at 12 and 16; width 3 has rate 2 and so a digest of 2: its 1001 leaves run too)"""
    for n in (5, 64) + ((1001,) if width in (3, 8) or family == "lin" else ()):
        Pm, leaves, d, flat = GD.poseidon_tree(family, width, n)
        ll = leaves.shape[1]
        h = handle(Pm)
        assert L.merkle_tree_words(n, d) == flat.size
        d_tree = torch.full((flat.size,), -1, dtype=torch.int64, device="cuda")
        d_rows, d_cols = dev(torch, leaves.reshape(-1)), dev(torch, leaves.T.copy().reshape(-1))
        h.merkle_commit_dev(d_rows.data_ptr(), n, ll, ll, 1, d, d_tree.data_ptr())
        check_words(host(torch, d_tree), flat, (family, width, n))
        d_tree.fill_(-1)
        h.merkle_commit_dev(d_cols.data_ptr(), n, ll, 1, n, d, d_tree.data_ptr())
        check_words(host(torch, d_tree), flat, (family, width, n, "columns"))
        h.close()


# ------------------------------------------------------------------------------------------------ E: extension elements
def ext_call(torch, op, w, n, a, b, s, e):
    d_a = dev(torch, a.reshape(-1))
    if op in ("add", "sub", "mul"):
        return run_dev(torch, getattr(L.lib, "ronk_ext2_vec_%s_dev" % op), GL, w, n, d_a, dev(torch, b.reshape(-1)))
    if op == "neg":
        return run_dev(torch, L.lib.ronk_ext2_vec_neg_dev, GL, w, n, d_a)
    if op == "mul_base":
        return run_dev(torch, L.lib.ronk_ext2_vec_mul_base_dev, GL, w, n, d_a, dev(torch, s))
    if op == "pow":
        return run_dev(torch, L.lib.ronk_ext2_vec_pow_dev, GL, w, n, d_a, e)
    d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_inv = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
    L.check(L.lib.ronk_ext2_vec_inv_dev(GL, w, d_a.data_ptr(), d_inv.data_ptr(), n, d_st.data_ptr(), 0))
    return host(torch, d_inv)       # (0, 0) is written for a zero element, which small signed pairs hold now and then


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("op", GD.EXT_OPS)
def test_extension_ops(torch, op, w):
    """small signed planar operands (B = 8) at every size, one run with window_words operands; pow with e = 1 .. 4"""
    for n in GD.EXT_SIZES:
        for e in ((1, 2, 3, 4) if op == "pow" and n <= 65 else (3,)):
            a, b, s, want = GD.ext_case(op, w, n, False, e)
            check_words(ext_call(torch, op, w, n, a, b, s, e), want, (op, w, n, e))
    a, b, s, want = GD.ext_case(op, w, 65, True, 4)
    check_words(ext_call(torch, op, w, 65, a, b, s, 4), want, (op, w, "window"))


def test_extension_square_of_a_small_difference(torch):
    """a0 = 2^48 t, (2^48)^2 = -1: a0^2 + W a1^2 is a small difference, the one way the addition inside a SQUARE sees a sum in
    [p, 2^64) (the squares of small values are both positive)"""
    n = 65
    for w in WS:
        E = GD.X2.Ext2(GL, w)
        a = GD.small_signed((2, n), 21, 8)
        a[0] = np.array([int(v) * (1 << 48) % GL for v in a[0]], dtype=np.uint64)
        els = [(int(x), int(y)) for x, y in zip(a[0], a[1])]
        d_a = dev(torch, a.reshape(-1))
        for e in (2, 3, 4):
            want = GD.X2.planar([E.pow(x, e) for x in els])
            check_words(run_dev(torch, L.lib.ronk_ext2_vec_pow_dev, GL, w, n, d_a, e), want, ("pow", w, e))
        want = GD.X2.planar([E.mul(x, x) for x in els])
        check_words(run_dev(torch, L.lib.ronk_ext2_vec_mul_dev, GL, w, n, d_a, d_a), want, ("mul by itself", w))


# ------------------------------------------------------------------------------------------------ F: the FRI fold
def fold_call(torch, form, eta, n, shift, w, words, beta):
    if form == "base":
        I = TF.Instance(GL, n, eta, TF.fold_final(n, eta), 0, shift=shift)
        d_in, d_beta = dev(torch, words), dev(torch, beta)      # (held: a temporary's block would be handed to the next tensor)
        d_out = torch.full(((1 << n) >> eta,), -1, dtype=torch.int64, device="cuda")
        I.h.fold_dev(0, d_in.data_ptr(), d_beta.data_ptr(), d_out.data_ptr())
        got = host(torch, d_out)
    else:
        I = TFX.Instance(GL, n, eta, TF.fold_final(n, eta), 0, int(form == "ext"), shift=shift, w=w)
        got = I.fold_dev(torch, 0, words, [int(v) for v in beta])
    I.close()
    return got


@pytest.mark.parametrize("eta", [1, 2, 3])
@pytest.mark.parametrize("form,w", [("base", 7), ("mix", 7), ("mix", 11), ("ext", 7), ("ext", 11)])
def test_fold(torch, form, w, eta):
    """layer sizes 2^(eta+1), 2^(eta+5) and 2^9, coset shifts 1 and g; the families small, cut 0 .. eta - 1, out and the four
    betas (0, 1, p - 1 and words of the window)"""
    for n in (eta + 1, eta + 5, 9):
        for shift in (1, GD.G):
            for family in GD.fold_families(eta):
                F, words, beta, want = GD.fold_case(form, eta, n, shift, family, w)
                check_words(fold_call(torch, form, eta, n, shift, w, words, beta), want, (form, w, eta, n, shift, family))


# ------------------------------------------------------------------------------------------------ S: scans
@pytest.mark.parametrize("op", ["sum", "prod"])
@pytest.mark.parametrize("w", (None,) + WS)
def test_scans(torch, op, w):
    for n in GD.SCAN_SIZES:
        d_work = work_for(torch, n)
        for exclusive in (0, 1):
            x, want, total = GD.scan_base(op, n, exclusive) if w is None else GD.scan_ext(op, w, n, exclusive)
            d_a, d_out = dev(torch, x.reshape(-1)), garbage(torch, x.size)
            got_total = scan_dev(torch, GL, w, op, d_a, d_out, n, exclusive, True, d_work)
            check_words(host(torch, d_out), want, (op, w, n, exclusive))
            check_words(got_total, [total] if w is None else list(total), (op, w, n, "total"))
            scan_dev(torch, GL, w, op, d_a, d_a, n, exclusive, False, d_work)            # in place
            check_words(host(torch, d_a), want, (op, w, n, exclusive, "in place"))


# ------------------------------------------------------------------------------------------------ D: the DEEP combinations
@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("n", [6, 8, 10])
def test_deep_combine(torch, n, w):
    eta = 2
    for C in (1, 8, 16):
        for K in (1, 2):
            I = TP.Instance(GL, n, eta, TF.fold_final(n, eta), 0, C, K, shift=GD.G if (C + K) % 2 else 1, w=w)
            for alpha in GD.DEEP_ALPHAS:
                for window in ((False, True) if alpha == (1, 1) and C == 8 else (False,)):
                    M, ys, zs, want = GD.deep_case(I.S, alpha, window)
                    d_M = dev(torch, M.reshape(-1))
                    got, st = I.combine_dev(torch, d_M, ys, zs, alpha)
                    assert st == 0
                    check_words(got, want, ("deep", n, w, C, K, alpha, window))
            I.close()


@pytest.mark.parametrize("w", WS)
def test_mpcs_combine_plonk_shape(torch, w):
    I = TM.Instance(GL, 8, 2, 4, 0, 2, TM.PLONK_COLUMNS, TM.PLONK_MASKS, w=w)
    for alpha in GD.DEEP_ALPHAS:
        Ms, ys, zs, want = GD.mpcs_case(I.S, alpha)
        d_Ms = [dev(torch, m.reshape(-1)) for m in Ms]
        got, st = I.combine_dev(torch, d_Ms, ys, zs, alpha)
        assert st == 0
        check_words(got, want, ("mpcs", w, alpha))
    I.close()


# ------------------------------------------------------------------------------------------------ Q: the PLONK quotient
@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("log2_n,log2_b", [(4, 1), (4, 2), (6, 1), (6, 2)])
def test_plonk_quotient(torch, log2_n, log2_b, w):
    """small signed wires, selectors, sigma, pi, Z and challenges: the gate sum is a chain of small additions and products"""
    c = TPL.Case(torch, GL, w, log2_n + log2_b, log2_b, host=GD.plonk_arrays(log2_n, log2_b, 31 + log2_n))
    M = c.M
    for with_pi in (True, False):
        d_T = TPL.garbage(torch, 2 * M)
        c.call(torch, d_T, with_pi=with_pi)
        check_words(host(torch, d_T), c.want_all(with_pi=with_pi), ("plonk", w, log2_n, log2_b, with_pi))
    assert c.inputs_unchanged(torch)
    c.handle.close()


# ------------------------------------------------------------------------------------------------ Q: constraint programs
@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("log2_n,log2_b", [(4, 1), (4, 2), (6, 1), (6, 2)])
def test_air_quotient(torch, log2_n, log2_b, w):
    """gl_directed's program -- every opcode and operand kind on base and on extension registers, the four constraint kinds, a
    periodic column of period 4, rotated cells -- on small signed columns, challenge, weights and periodic values; T_in absent,
    present and in place"""
    M = 1 << (log2_n + log2_b)
    for tin in (False, True):
        prog, base, ext, chal, lam, periodic, T_in, want = GD.air_case(w, log2_n, log2_b, tin)
        a = TAP.AirPer(GL, w, log2_n, log2_b, prog, GD.AIR_GROUPS, GD.AIR_N_EXT, GD.AIR_N_CHAL, periodic)
        d_base, d_ext, d_chal, d_lam = [dev(torch, base)], [dev(torch, ext)], dev(torch, chal), dev(torch, lam)
        d_T_in = dev(torch, T_in) if tin else None
        d_T = torch.full((2 * M,), -1, dtype=torch.int64, device="cuda")
        a.call(d_base, d_ext, d_chal, d_lam, d_T_in, d_T)
        check_words(host(torch, d_T), want, ("air", w, log2_n, log2_b, tin))
        if tin:
            a.call(d_base, d_ext, d_chal, d_lam, d_T_in, d_T_in)
            check_words(host(torch, d_T_in), want, ("air", w, log2_n, log2_b, "in place"))
        a.close()
