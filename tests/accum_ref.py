"""Pure-Python restatement of the running products and sums, the permutation grand product and the logUp running sum
(include/ronk_ntt.h "running products and sums") on Python integers.  The reference has no prover, so this file is the normative
restatement of those semantics; the extension is that of tests/ext2_ref.py.  A test helper, not product code; it shares nothing
with the library."""
from ext2_ref import Ext2, pairs, planar  # noqa: F401  (re-exported for the tests)


def scan(values, comb, identity, exclusive):
    """-> (out, total): out[i] = a[0] o .. o a[i], or with exclusive out[0] = e and out[i] = a[0] o .. o a[i-1]"""
    out, run = [], identity
    for v in values:
        nxt = comb(run, v)
        out.append(run if exclusive else nxt)
        run = nxt
    return out, run


def base_scan(p, words, op, exclusive):
    """op: 'prod' or 'sum' over F_p; any integers in, canonical out"""
    vals = [int(v) % p for v in words]
    if op == "prod":
        return scan(vals, lambda a, b: a * b % p, 1 % p, exclusive)
    return scan(vals, lambda a, b: (a + b) % p, 0, exclusive)


def ext_scan(E, elements, op, exclusive):
    """the same over pairs of E (an ext2_ref.Ext2)"""
    vals = [E.el(v) for v in elements]
    if op == "prod":
        return scan(vals, E.mul, E.one, exclusive)
    return scan(vals, E.add, E.zero, exclusive)


def perm_factors(E, wires, labels, beta, gamma, i):
    """prod_c (a_c[i] + beta label_c[i] + gamma)"""
    f = E.one
    for a, l in zip(wires, labels):
        f = E.mul(f, E.add(E.add(E.embed(a[i]), E.mul_base(beta, int(l[i]) % E.p)), gamma))
    return f


def perm_product(E, wires, ids, sigma, beta, gamma):
    """wires, ids, sigma: W columns of N words; beta, gamma: pairs.  -> (Z[0..N-1], Z[N], status): Z[0] = 1,
    Z[i+1] = Z[i] num_i / den_i; a row with den_i = 0 contributes the factor ZERO and sets status 1"""
    beta, gamma = E.el(beta), E.el(gamma)
    n = len(wires[0])
    Z, run, status = [], E.one, 0
    for i in range(n):
        Z.append(run)
        num, den = perm_factors(E, wires, ids, beta, gamma, i), perm_factors(E, wires, sigma, beta, gamma, i)
        inv = E.inv(den)
        if inv is None:
            status, inv = 1, E.zero
        run = E.mul(run, E.mul(num, inv))
    return Z, run, status


def logup_sum(E, vals, mult, alpha):
    """vals (and mult, or None for all ones): C columns of N words.  -> (S[0..N-1], S[N], status): S[0] = 0,
    S[i+1] = S[i] + sum_c m_c[i] / (alpha + v_c[i]); a zero denominator makes that term ZERO and sets status 1"""
    alpha = E.el(alpha)
    n = len(vals[0])
    S, run, status = [], E.zero, 0
    for i in range(n):
        S.append(run)
        for c, col in enumerate(vals):
            inv = E.inv(E.add(alpha, E.embed(col[i])))
            if inv is None:
                status = 1
                continue
            run = E.add(run, E.mul_base(inv, 1 if mult is None else int(mult[c][i]) % E.p))
    return S, run, status


def cycle_instance(rng, n, columns, variables):
    """a random copy-constraint instance: every cell of the [columns][n] table draws one of `variables` variable ids; sigma is the
    cyclic shift inside each variable's cells, ids are the cell numbers plus one, a cell's wire value depends on its variable
    only.  -> (wires, ids, sigma) as numpy uint64 arrays [columns][n]"""
    import numpy as np
    cells = columns * n
    var = rng.integers(0, variables, size=cells)
    order = np.argsort(var, kind="stable")                 # the cells grouped by variable
    sorted_var = var[order]
    nxt = np.roll(order, -1)                               # the next cell of the group ...
    last = np.ones(cells, dtype=bool)
    last[:-1] = sorted_var[1:] != sorted_var[:-1]
    first = np.ones(cells, dtype=bool)
    first[1:] = last[:-1]
    starts = np.maximum.accumulate(np.where(first, np.arange(cells), 0))
    nxt[last] = order[starts[last]]                        # ... and from the last back to the first
    sigma = np.empty(cells, dtype=np.uint64)
    sigma[order] = (nxt + 1).astype(np.uint64)
    ids = np.arange(1, cells + 1, dtype=np.uint64)
    value = rng.integers(0, 2**63, size=variables, dtype=np.uint64)
    wires = value[var]
    return wires.reshape(columns, n), ids.reshape(columns, n), sigma.reshape(columns, n)


# ------------------------------------------------------------------------------------------------ the same values, faster
# The two functions above are the definition.  The GPU suite checks whole columns of up to 16 x 65537 cells against it; these
# forms compute the same values with the arithmetic written out on local integers and ONE modular inversion per call
# (Montgomery's trick over all denominators), and tests/test_accum_ref.py holds them to the definition.
def _batch_inverse_norms(p, norms):
    """1 / x for every non-zero x of the list (zero stays zero): prefix products, one pow, and back"""
    pre, run = [], 1
    for x in norms:
        pre.append(run)
        if x:
            run = run * x % p
    inv = pow(run, p - 2, p)
    out = [0] * len(norms)
    for k in range(len(norms) - 1, -1, -1):
        x = norms[k]
        if x:
            out[k] = inv * pre[k] % p
            inv = inv * x % p
    return out


def perm_product_fast(E, wires, ids, sigma, beta, gamma):
    """columns as lists of Python integers"""
    p, w = E.p, E.w
    (b0, b1), (g0, g1) = E.el(beta), E.el(gamma)
    n = len(wires[0])
    nums, dens = [], []
    for labels, acc in ((ids, nums), (sigma, dens)):
        f0, f1 = [1 % p] * n, [0] * n
        for col, lab in zip(wires, labels):
            n0, n1 = [], []
            for a, l, x0, x1 in zip(col, lab, f0, f1):
                t0, t1 = (a + b0 * l + g0) % p, (b1 * l + g1) % p
                n0.append((x0 * t0 + w * x1 * t1) % p)
                n1.append((x0 * t1 + x1 * t0) % p)
            f0, f1 = n0, n1
        acc.extend(zip(f0, f1))
    inv = _batch_inverse_norms(p, [(d0 * d0 - w * d1 * d1) % p for d0, d1 in dens])
    Z, r0, r1, status = [], 1 % p, 0, 0
    for (n0, n1), (d0, d1), v in zip(nums, dens, inv):
        Z.append((r0, r1))
        if v == 0:
            status = 1
        q0, q1 = d0 * v % p, -d1 * v % p                        # 1 / den, or ZERO
        t0, t1 = (n0 * q0 + w * n1 * q1) % p, (n0 * q1 + n1 * q0) % p
        r0, r1 = (r0 * t0 + w * r1 * t1) % p, (r0 * t1 + r1 * t0) % p
    return Z, (r0, r1), status


def logup_sum_fast(E, vals, mult, alpha):
    """columns as lists of Python integers"""
    p, w = E.p, E.w
    a0, a1 = E.el(alpha)
    rows = list(zip(*vals))
    d0s = [(a0 + v) % p for row in rows for v in row]                        # row-major over (i, c)
    wa = w * a1 * a1 % p
    inv = iter(_batch_inverse_norms(p, [(d * d - wa) % p for d in d0s]))
    ds = iter(d0s)
    ones = (1,) * len(vals)
    S, r0, r1, status = [], 0, 0, 0
    for ms in (zip(*mult) if mult is not None else (ones for _ in rows)):
        S.append((r0, r1))
        for m in ms:
            v = next(inv)
            if v == 0:
                status = 1
            t = m * v % p
            r0, r1 = (r0 + t * next(ds)) % p, (r1 - t * a1) % p
    return S, (r0, r1), status
