"""Directed Goldilocks NTT inputs for the branches a uniformly random residue all but never takes (test helper, numpy + oracle).

gl64.h's `add`, `add_lazy` and `mad_eps_canon` each have an outcome that needs a sum to land in [p, 2^64): a window of 2^32 - 1
values out of 2^64.  Sums of SMALL SIGNED integers -- t in [-B, B] stored as t mod p -- land there all the time: (p - 1) + 1 = p,
(p - 2) + 2 = p, ...  A transform only sees such sums where its intermediate values are small, so every family below places small
signed values at one cut of the decimation-in-frequency pipeline that plan.h / ntt_tile.h run and pulls them back to the input
through the (exactly invertible) steps before the cut:

  small    the input itself is small: the first butterflies of the first pass
  pre      the OUTPUT is small (x = ifft(s), or fft(s) for the inverse transform): the last stages of the last pass, the
           `keep0` pair of dif_stage among them; the expected output is s itself
  colpre   the first pass's butterfly outputs are small, before the inter-pass twiddle
  cut      the general form: the state entering round j of pass q, or that round's butterfly outputs before its twiddle

The pipeline restated here (plan.h, ntt_tile.h): the passes split the index most significant part first (n = R1 * R2 [* R3],
pass q transforms digit q and multiplies by omega_Nq^(k_q * rest), Nq = R_q * ... * R_last; the n^-1 of an inverse plan of several
passes rides on the first of these twiddles); a pass of 2^logr rows runs rounds of radix 16, 16, 2^(logr - 8), or 16, 2^(logr - 4)
for logr <= 8, each but the last followed by omega_R'^(k_i * m), R' the rows the round started from and m the row digits still to
come.  All field arithmetic is the oracle's; `model_transform` runs every step and must reproduce the oracle's fft / ifft
(tests/test_emu_gl_branches.py checks it), which pins the restatement.

Everything is deterministic from `seed`."""
import numpy as np

import oracle as orc

P, G = orc.GOLDILOCKS_P, orc.GOLDILOCKS_G
_P64 = np.uint64(P)


def small_signed(shape, seed, B=2):
    """t uniform in [-B, B], stored as t mod p"""
    t = np.random.default_rng(seed).integers(-B, B + 1, size=shape, dtype=np.int64)
    return np.where(t < 0, _P64 - (-t).astype(np.uint64), t.astype(np.uint64)).astype(np.uint64)


def _rows(x, fn):
    return np.stack([fn(P, G, r) for r in x])


def fft(x, inverse=False):
    """the oracle's transform of every row of a [batch][n] array"""
    return _rows(x, orc.ifft if inverse else orc.fft)


def small(n, batch, seed=1, B=2):
    return small_signed((batch, n), seed, B)


def pre(n, batch, inverse, seed=2, B=2):
    """(x, s): s small signed, the transform of x in the given direction is s"""
    s = small_signed((batch, n), seed, B)
    return fft(s, not inverse), s


def pass_radices(logr):
    """radices of the rounds of a 2^logr-row pass (ntt_tile.h)"""
    if logr <= 4:
        return [1 << logr]
    if logr <= 8:
        return [16, 1 << (logr - 4)]
    return [16, 16, 1 << (logr - 8)]


_TAB = {}


def _table(n):
    """omega_n^e, e in [0, n), omega_n = g^((p-1)/n)"""
    if n not in _TAB:
        w = orc.primitive_root_of_unity(P, G, n) if n > 1 else 1
        t = np.ones(1, dtype=np.uint64)
        step = w
        while t.size < n:
            t = np.concatenate([t, orc.vec_mul(P, t, np.full(t.size, step, dtype=np.uint64))])
            step = orc.mul(P, step, step)
        _TAB[n] = t
    return _TAB[n]


def _ax(ndim, axis, size):
    shape = [1] * ndim
    shape[axis] = size
    return np.arange(size, dtype=np.int64).reshape(shape)


def _index(ndim, axes, sizes, most_significant_first=True):
    """the mixed-radix index over `axes` as a broadcastable int64 array"""
    e = np.zeros([1] * ndim, dtype=np.int64)
    order = list(zip(axes, sizes))
    if not most_significant_first:
        order = order[::-1]
    for a, r in order:
        e = e * r + _ax(ndim, a, r)
    return e


class Pipeline:
    """the steps of a plan with passes of 2^logrs[q] rows; the state is a [batch, digit, digit, ...] array, digits of the input
    index most significant first; a transformed digit stays on its axis"""

    def __init__(self, n, logrs, inverse, radices=None):
        assert sum(logrs) == n.bit_length() - 1
        self.n, self.inverse = n, inverse
        self.radices = [list(r) for r in radices] if radices else [pass_radices(l) for l in logrs]
        assert all(int(np.prod(r)) == 1 << l for r, l in zip(self.radices, logrs))
        self.shape = [r for rs in self.radices for r in rs]
        nd = 1 + len(self.shape)
        self.steps = []      # (q, j, kind, payload): kind "dft" (axis) or "tw" (exponent of omega_n, extra scalar factor)
        ax0 = 1
        for q, rs in enumerate(self.radices):
            axes = list(range(ax0, ax0 + len(rs)))
            later = list(range(ax0 + len(rs), nd))
            for j, r in enumerate(rs):
                self.steps.append((q, j, "dft", axes[j]))
                if j + 1 < len(rs):
                    rrem = int(np.prod(rs[j:]))
                    m = _index(nd, axes[j + 1:], rs[j + 1:])
                    self.steps.append((q, j, "tw", (_ax(nd, axes[j], r) * m * (n // rrem), 1)))
            last = q + 1 == len(self.radices)
            scale = orc.inverse(P, n % P) if inverse and (q == 0) else 1
            if not last:
                nq = int(np.prod(self.shape[ax0 - 1:]))
                kpass = _index(nd, axes, rs, most_significant_first=False)
                c = _index(nd, later, [self.shape[a - 1] for a in later])
                self.steps.append((q, len(rs) - 1, "tw", (kpass * c * (n // nq), scale)))
            elif scale != 1:
                self.steps.append((q, len(rs) - 1, "tw", (np.zeros([1] * nd, dtype=np.int64), scale)))
            ax0 += len(rs)

    def _dft(self, st, axis, undo):
        r = st.shape[axis]
        tab = _table(self.n)
        x = np.ascontiguousarray(np.moveaxis(st, axis, 0)).reshape(r, -1)
        neg = self.inverse != undo                      # omega^-1: the inverse transform, or a forward step undone
        # radix-2 decimation in frequency down the r rows, then the bit reversal undone
        s = r
        while s > 1:
            h = s // 2
            v = x.reshape(r // s, 2, h, -1)
            a, b = np.ascontiguousarray(v[:, 0]), np.ascontiguousarray(v[:, 1])
            e = np.arange(h, dtype=np.int64) * (self.n // s)
            if neg:
                e = (self.n - e) % self.n
            w = np.ascontiguousarray(np.broadcast_to(tab[e][None, :, None], a.shape))
            x = np.stack([orc.vec_add(P, a, b), orc.vec_mul(P, orc.vec_sub(P, a, b), w)], axis=1).reshape(r, -1)
            s = h
        bits = r.bit_length() - 1
        out = x[[int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(r)]]
        if undo:
            out = orc.vec_mul(P, out, np.full(out.shape, orc.inverse(P, r), dtype=np.uint64))
        shp = list(st.shape)
        shp.insert(0, shp.pop(axis))
        return np.moveaxis(out.reshape(shp), 0, axis)

    def _tw(self, st, payload, undo):
        e, scale = payload
        e = e % self.n
        if self.inverse != undo:
            e = (self.n - e) % self.n
        w = _table(self.n)[np.broadcast_to(e, (1,) + tuple(st.shape[1:]))]
        if scale != 1:
            w = orc.vec_mul(P, w, np.full(w.shape, orc.inverse(P, scale) if undo else scale, dtype=np.uint64))
        return orc.vec_mul(P, np.ascontiguousarray(st), np.ascontiguousarray(np.broadcast_to(w, st.shape)))

    def apply(self, st, steps, undo=False):
        for (_, _, kind, payload) in (reversed(steps) if undo else steps):
            st = self._dft(st, payload, undo) if kind == "dft" else self._tw(st, payload, undo)
        return st

    def cut_steps(self, q, j, before_twiddle):
        """the steps before the cut: (a) everything before round j of pass q, or (b) up to and including its butterflies"""
        idx = next(i for i, s in enumerate(self.steps) if s[:3] == (q, j, "dft"))
        return self.steps[:idx + 1] if before_twiddle else self.steps[:idx]


def model_transform(x, logrs, inverse, radices=None):
    """every step of the pipeline on a [batch][n] array, outputs in natural order: must equal the oracle's fft / ifft"""
    batch, n = x.shape
    pl = Pipeline(n, logrs, inverse, radices)
    st = pl.apply(x.reshape([batch] + pl.shape), pl.steps)
    nd = st.ndim
    return np.ascontiguousarray(st.transpose([0] + list(range(nd - 1, 0, -1)))).reshape(batch, n)


def cut(n, batch, inverse, logrs, q, j, before_twiddle, radices=None, seed=4, B=2):
    """the input whose state (a) entering round j of pass q, or (b) after that round's butterflies and before its twiddle
    (before_twiddle), is small signed"""
    pl = Pipeline(n, logrs, inverse, radices)
    s = small_signed([batch] + pl.shape, seed, B)
    return np.ascontiguousarray(pl.apply(s, pl.cut_steps(q, j, before_twiddle), undo=True)).reshape(batch, n)


def colpre(n, batch, inverse, log_r1, seed=3, B=2):
    """every column of the [R1][n / R1] view is the inverse R1-point transform (in the plan's direction) of a small signed
    column: cut (b) at the first pass's last round, with the pass taken as one round"""
    r1 = 1 << log_r1
    s = small_signed((batch, r1, n // r1), seed, B)
    cols = np.ascontiguousarray(s.transpose(0, 2, 1)).reshape(-1, r1)
    x = fft(cols, not inverse)
    if inverse:      # fft undoes an UNSCALED inverse transform up to the factor R1 that ifft would have divided by
        x = orc.vec_mul(P, x, np.full(x.shape, orc.inverse(P, r1), dtype=np.uint64))
    return np.ascontiguousarray(x.reshape(batch, n // r1, r1).transpose(0, 2, 1)).reshape(batch, n)


def families(n, batch, inverse, logrs, cuts=None):
    """[(name, x, s)]: small, pre, colpre (plans of several passes) and the cuts of the pipeline -- all of them, or the
    (q, j, before_twiddle) listed; s is the small signed array a `pre` input was built from (its expected output), else None"""
    logrs = list(logrs)
    x, s = pre(n, batch, inverse)
    out = [("small", small(n, batch), None), ("pre", x, s)]
    if len(logrs) > 1:
        out.append(("colpre", colpre(n, batch, inverse, logrs[0]), None))
    for q, logr in enumerate(logrs):
        for j in range(len(pass_radices(logr))):
            for before in (False, True):
                if (q, j, before) == (0, 0, False) or (cuts is not None and (q, j, before) not in cuts):
                    continue      # (the first of them is `small`)
                out.append(("cut:q%d.j%d.%s" % (q, j, "b" if before else "a"),
                            cut(n, batch, inverse, logrs, q, j, before, seed=100 + 16 * q + 2 * j + before), None))
    return out
