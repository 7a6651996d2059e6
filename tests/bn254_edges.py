"""Edge vectors for csrc/bn254.h and the MSM pipeline (TEST INFRASTRUCTURE; pure Python over integers and oracle/bn254.py).

Shared by tests/test_bn254_edges_host.py (the host build of bn254.h: the __int128 fallback of acc_mad) and
tests/test_gpu_bn254_edges.py (the device: the inline assembly), so that both run the identical operands against the
identical expectations.

FIELD.  The kernels hold field elements as RAW 256-bit integers, Montgomery form, any representative in [0, 2p).  The
expectations here are raw and exact, from integer arithmetic that does not restate the limb code:

    fp_mul(a, b)   m = (a b mod 2^256)(-1/p) mod 2^256,  out = (a b + m p) / 2^256        (the Montgomery product itself)
    fp_add(a, b)   s = a + b;  s - 2p if s >= 2p else s
    fp_sub(a, b)   d = a - b;  d + 2p if d < 0 else d
    fp_neg(a)      0 -> 0, otherwise 2p - a
    fp_canon(a)    a mod p                                   (contract: a < 3p, two conditional subtractions)
    fp_to_mont(a)  fp_mul(a, 2^512 mod p)                    (any 256-bit a: a R2 + m p < 2^256 * 2p as R2 < p)
    fp_from_mont   fp_mul(a, 1) mod p
    fp_is_zero     a in {0, p};   fp_is_zero_exact  a == 0;   fp_geq_p  a >= p   (any 256-bit a)

POINTS.  A group element k*G is presented as XYZZ = (x l^2, y l^3, l^2, l^3) in Montgomery form for several l, every
coordinate independently as v or v + p; infinity as ZZ = 0 and as ZZ = p (the weak zero).  An expected output is a GROUP
ELEMENT: the test normalises x = X/ZZ, y = Y/ZZZ and compares with oracle.bn254.add / neg / mul, and checks the
invariants (infinite exactly when ZZ in {0, p}; ZZ^3 == ZZZ^2; every coordinate below 2p).  The XYZZ formulas are not
restated here.

ZERO-DIFFERENCE CLASSES.  xyzz_add and xyzz_madd decide "same x" / "same y" by fp_is_zero(U2 - U1) resp. (S2 - S1),
where both sides are raw values below 2p congruent mod p; the difference is then
    "zero"    exactly 0                       (U2 == U1)
    "plus_p"  p without a borrow              (U2 == U1 + p)
    "borrow"  p through fp_sub's borrow branch (U2 == U1 - p; d = -p, + 2p)
equal_cases() searches scalings l1, l2 in 2 .. SEARCH_L-1 and the sixteen (for the affine operand of madd: four) "+p"
choices per operand, in a fixed order, for the first operands of every (X class, Y class) combination, for add, madd and
madd with neg = 1.  Which classes the operands meet is computed by `classes()` from the operand products alone
(U = X * ZZ', S = Y * ZZZ' as Montgomery products -- the one place this module looks inside the formulas, because the
class is a property of exactly those two differences).  All nine combinations are reachable for all three ops within
that search (asserted by the host test's census), so nothing is left out.

MSM.  Cases are (signed multipliers a_i, scalars k_i, env): the points are a_i * G from oracle.bn254.multiples (negative
a: the negated point; 0: the point at infinity), so that the expected result is ONE oracle scalar multiplication,
(sum k_i a_i mod r) * G.  `env` sets RONK_MSM_C (window bits) and RONK_MSM_CH (entries per task); see msm_cases().
"""
import functools
import itertools
import random

from oracle import bn254 as o

P, R = o.P, o.R
P2 = 2 * P
RR = 1 << 256
NINV = (-pow(P, -1, RR)) % RR
R1 = RR % P              # Montgomery form of 1
R2 = RR * RR % P

# op codes and words per element (a, b, out) of csrc/bn254_probe.h
OPS = {
    "fp_mul": (0, 4, 4, 4), "fp_add": (1, 4, 4, 4), "fp_sub": (2, 4, 4, 4), "fp_neg": (3, 4, 0, 4), "fp_canon": (4, 4, 0, 4),
    "fp_to_mont": (5, 4, 0, 4), "fp_from_mont": (6, 4, 0, 4), "fp_is_zero": (7, 4, 0, 1), "fp_is_zero_exact": (8, 4, 0, 1),
    "fp_geq_p": (9, 4, 0, 1),
    "xyzz_add": (16, 16, 16, 16), "xyzz_dbl": (17, 16, 0, 16), "xyzz_madd": (18, 16, 8, 16), "xyzz_madd_neg": (19, 16, 8, 16),
    "on_curve": (20, 8, 0, 1),
}


def mont(a, b):
    """the raw Montgomery product: no reduction of the result"""
    m = (a * b % RR) * NINV % RR
    return (a * b + m * P) >> 256


def to_m(v):
    """canonical Montgomery form of the residue v"""
    return v * RR % P


def pack(rows):
    """[[256-bit integers]] (or a flat list of them) -> little-endian bytes, 4 x 64-bit words per integer"""
    return b"".join(v.to_bytes(32, "little") for r in rows for v in (r if isinstance(r, (list, tuple)) else (r,)))


def unpack(buf, per, size=32):
    """bytes -> rows of `per` integers of `size` bytes each"""
    vals = [int.from_bytes(buf[i:i + size], "little") for i in range(0, len(buf), size)]
    return [vals[i:i + per] for i in range(0, len(vals), per)]


def pack_msm(mult, scalars):
    """(points as n x 8 words: x, y in standard form, infinity all zero; scalars as n x 4 words), as bytes"""
    pts = [point_of(a) or (0, 0) for a in mult]
    return pack(pts), pack(scalars)


# ------------------------------------------------------------------------------------------------------------ field
def _edge_values():
    top2p = P2 >> 224
    e = [0, 1, P - 1, P, P + 1, P2 - 1, R1, R2]
    for k in range(32, 256, 32):
        e += [1 << k, (1 << k) - 1]
    low7 = (1 << 224) - 1
    for t in (0, 1, P >> 224, top2p - 1, top2p):
        v = (t << 224) | low7
        if v < P2:
            e.append(v)
    for i in range(8):                                   # a single non-zero limb
        for limb in (0xFFFFFFFF, 0x80000000, 1):
            v = limb << (32 * i)
            if v >= P2:
                v = top2p << 224                         # the largest top limb that stays below 2p
            e.append(v)
    out = []
    for v in e:
        assert 0 <= v < P2
        if v not in out:
            out.append(v)
    return out


EDGES = _edge_values()
_rng = random.Random(0xB254)
VALUES = EDGES + [_rng.randrange(P2) for _ in range(200)]            # every one below 2p
PAIRS = list(itertools.product(VALUES, VALUES))                      # every pair, edges and random values alike
MORE = [_rng.randrange(P2) for _ in range(150)]                      # so that the unary arrays span more than one block
WIDE = [P2, P2 + 1, 3 * P - 1, 3 * P, RR - 1, RR - 2, 1 << 255, (1 << 255) - 1, RR - P, RR - P2] + \
       [_rng.randrange(RR) for _ in range(150)]                      # up to 2^256 - 1
BELOW_3P = [v for v in WIDE if v < 3 * P] + [P2 + _rng.randrange(P) for _ in range(150)]

FIELD_MODEL = {
    "fp_mul": mont,
    "fp_add": lambda a, b: a + b - P2 if a + b >= P2 else a + b,
    "fp_sub": lambda a, b: a - b + P2 if a < b else a - b,
    "fp_neg": lambda a: 0 if a == 0 else P2 - a,
    "fp_canon": lambda a: a % P,
    "fp_to_mont": lambda a: mont(a, R2),
    "fp_from_mont": lambda a: mont(a, 1) % P,
    "fp_is_zero": lambda a: int(a in (0, P)),
    "fp_is_zero_exact": lambda a: int(a == 0),
    "fp_geq_p": lambda a: int(a >= P),
}
WEAK_OUT = ("fp_mul", "fp_add", "fp_sub", "fp_neg")                  # outputs that must stay below 2p
_UNARY_DOMAIN = {"fp_neg": MORE, "fp_canon": MORE + BELOW_3P, "fp_to_mont": MORE + WIDE, "fp_from_mont": MORE,
                 "fp_is_zero": MORE, "fp_is_zero_exact": MORE, "fp_geq_p": MORE + WIDE}


@functools.lru_cache(maxsize=None)
def field_vectors():
    """[(name, a values, b values or None, expected values)]; every array longer than one block of 256 and no multiple of
    256, plus every op once more at n = 1"""
    out = []
    for name, model in FIELD_MODEL.items():
        if OPS[name][2]:
            a = [x for x, _ in PAIRS]; b = [y for _, y in PAIRS]
            want = [model(x, y) for x, y in PAIRS]
        else:
            a = VALUES + _UNARY_DOMAIN[name]; b = None
            want = [model(x) for x in a]
        assert len(a) > 256 and len(a) % 256 != 0, (name, len(a))
        if name in WEAK_OUT:
            assert all(0 <= w < P2 for w in want), name
        out.append((name, a, b, want))
        one = [P2 - 1]
        out.append((name, one, one if b else None, [model(P2 - 1, P2 - 1) if b else model(P2 - 1)]))
    return out


# ------------------------------------------------------------------------------------------------------------ points
def present(pt, l=1, mask=0):
    """pt (an oracle point or None) as raw XYZZ words [X, Y, ZZ, ZZZ]: scaling l, bit i of mask adds p to coordinate i"""
    if pt is None:
        return [0, 0, 0, 0]
    x, y = pt
    l2, l3 = l * l % P, l * l * l % P
    v = [to_m(x * l2 % P), to_m(y * l3 % P), to_m(l2), to_m(l3)]
    return [c + P if (mask >> i) & 1 else c for i, c in enumerate(v)]


def present_affine(pt, mask=0):
    """pt as the raw affine operand [x, y] of madd (Montgomery form; exact (0, 0) = infinity)"""
    if pt is None:
        return [0, 0]
    v = [to_m(pt[0]), to_m(pt[1])]
    return [c + P if (mask >> i) & 1 else c for i, c in enumerate(v)]


INFINITIES = [[0, 0, 0, 0], [0, 0, P, P], [to_m(5), to_m(7), P, 0], [P, P2 - 1, 0, 0]]   # ZZ = 0 and the weak zero ZZ = p


def normalise(w):
    """raw XYZZ words -> the group element (oracle encoding), checking the representation's invariants"""
    X, Y, ZZ, ZZZ = w
    assert all(0 <= c < P2 for c in w), "a coordinate is not below 2p: %r" % (w,)
    assert (pow(ZZ, 3, P) * pow(RR, -3, P) - pow(ZZZ, 2, P) * pow(RR, -2, P)) % P == 0, "ZZ^3 != ZZZ^2: %r" % (w,)
    if ZZ % P == 0:
        assert ZZ in (0, P)
        return None
    return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)


def check_points(name, cases, got):
    """`got` (rows of raw XYZZ words, one per case) against the cases' expected group elements and the invariants"""
    assert len(got) == len(cases)
    for (label, a, b, want), g in zip(cases, got):
        try:
            have = normalise(g)
        except AssertionError as e:
            raise AssertionError("%s %s: %s" % (name, label, e))
        assert have == want, (name, label, a, b, g)


def check_field(name, a, b, want, got):
    """`got` (rows of one integer) against the raw expected values, bit for bit; weak outputs below 2p"""
    assert len(got) == len(want)
    bad = [(i, a[i], b[i] if b else None, g[0], w) for i, (g, w) in enumerate(zip(got, want)) if g[0] != w]
    assert not bad, (name, len(bad), bad[:3])
    if name in WEAK_OUT:
        assert all(g[0] < P2 for g in got)


def _diff_class(u1, u2):
    assert (u1 - u2) % P == 0 and 0 <= u1 < P2 and 0 <= u2 < P2
    return {0: "zero", P: "plus_p", -P: "borrow"}[u2 - u1]


def classes(name, a, b):
    """the (X, Y) zero-difference classes the operands of an equal-point add / madd meet (module docstring)"""
    if name == "xyzz_add":
        return (_diff_class(mont(a[0], b[2]), mont(b[0], a[2])), _diff_class(mont(a[1], b[3]), mont(b[1], a[3])))
    qy = b[1] if name == "xyzz_madd" else FIELD_MODEL["fp_neg"](b[1])
    return (_diff_class(a[0], mont(b[0], a[2])), _diff_class(a[1], mont(qy, a[3])))


CLASSES = ("zero", "plus_p", "borrow")
SEARCH_L = 30


@functools.lru_cache(maxsize=None)
def equal_cases():
    """{(op, X class, Y class): (a words, b words, expected point)} for P + P: the first operands, in the order l1, l2 in
    2 .. SEARCH_L-1 (l2 = 1 for the affine operand), masks ascending, that meet each combination"""
    k = 5
    pt = o.mul(k, o.G)
    want = o.mul(2 * k, o.G)
    found = {}
    for name in ("xyzz_add", "xyzz_madd", "xyzz_madd_neg"):
        todo = set(itertools.product(CLASSES, CLASSES))
        bpt = o.neg(pt) if name == "xyzz_madd_neg" else pt
        l2s = range(2, SEARCH_L) if name == "xyzz_add" else (1,)
        for l1, l2 in itertools.product(range(2, SEARCH_L), l2s):
            for ma in range(16):
                a = present(pt, l1, ma)
                for mb in range(16 if name == "xyzz_add" else 4):
                    b = present(bpt, l2, mb) if name == "xyzz_add" else present_affine(bpt, mb)
                    cl = classes(name, a, b)
                    if cl in todo:
                        todo.discard(cl)
                        found[(name,) + cl] = (a, b, want)
            if not todo:
                break
    return found


@functools.lru_cache(maxsize=None)
def point_vectors():
    """{op: [(label, a words, b words or None, expected point)]} for xyzz_add, xyzz_dbl, xyzz_madd, xyzz_madd_neg"""
    rng = random.Random(0x6254)
    g = {k: o.mul(k, o.G) for k in (1, 2, 3, 5, 7, 10, 11)}
    g[o.R - 1] = o.mul(o.R - 1, o.G)
    ks = list(g)
    ls = (1, 2, 3, 29, P - 1, rng.randrange(2, P))
    out = {"xyzz_add": [], "xyzz_dbl": [], "xyzz_madd": [], "xyzz_madd_neg": []}
    add, dbl = out["xyzz_add"], out["xyzz_dbl"]

    def masks(n):
        return [0, (1 << n) - 1] + [rng.randrange(1 << n) for _ in range(2)]

    for ka, kb in itertools.product(ks, ks):
        pa, pb = g[ka], g[kb]
        kind = "P+P" if ka == kb else "P+(-P)" if (ka + kb) % o.R == 0 else "P+Q"
        for la, lb in ((1, 1), (2, 3), (ls[4], ls[5]), (29, 29)):
            for ma, mb in zip(masks(4), masks(4)):
                add.append(("%s %d,%d l=%d,%d m=%d,%d" % (kind, ka, kb, la % 100, lb % 100, ma, mb),
                            present(pa, la, ma), present(pb, lb, mb), o.add(pa, pb)))
        for neg, name in ((False, "xyzz_madd"), (True, "xyzz_madd_neg")):
            for la in ls[:4]:
                for ma, mb in zip(masks(4), masks(2)):
                    out[name].append(("%s %d,%d l=%d m=%d,%d" % (kind, ka, kb, la, ma, mb), present(pa, la, ma),
                                      present_affine(pb, mb), o.add(pa, o.neg(pb) if neg else pb)))
    for ka in ks:                                                    # the same representation on both sides, every mask
        for la in ls:
            for ma in range(16):
                w = present(g[ka], la, ma)
                add.append(("P+P same repr %d l=%d m=%d" % (ka, la % 100, ma), w, w, o.add(g[ka], g[ka])))
                dbl.append(("dbl %d l=%d m=%d" % (ka, la % 100, ma), w, None, o.add(g[ka], g[ka])))
    for i, inf in enumerate(INFINITIES):                             # infinity on either side and on both
        dbl.append(("dbl inf%d" % i, inf, None, None))
        for j, inf2 in enumerate(INFINITIES):
            add.append(("inf%d+inf%d" % (i, j), inf, inf2, None))
        for ka in ks[:4]:
            for la, ma in ((1, 0), (3, 5), (29, 15)):
                w = present(g[ka], la, ma)
                add.append(("inf%d+P %d" % (i, ka), inf, w, g[ka]))
                add.append(("P+inf%d %d" % (i, ka), w, inf, g[ka]))
        for neg, name in ((False, "xyzz_madd"), (True, "xyzz_madd_neg")):
            out[name].append(("inf%d+(0,0)" % i, inf, [0, 0], None))  # an affine operand (0, 0)
            for ka in ks:                                            # madd into an infinite accumulator
                for mb in range(4):
                    out[name].append(("inf%d+q %d m=%d" % (i, ka, mb), inf, present_affine(g[ka], mb), o.neg(g[ka]) if neg else g[ka]))
    for name in ("xyzz_madd", "xyzz_madd_neg"):
        for ka in ks:
            for la, ma in ((1, 0), (3, 5), (29, 15)):
                out[name].append(("P+(0,0) %d" % ka, present(g[ka], la, ma), [0, 0], g[ka]))
    for (name, cx, cy), (a, b, want) in sorted(equal_cases().items()):   # every zero-difference class, by name
        out[name].append(("P+P class X:%s Y:%s" % (cx, cy), a, b, want))
    # P + (-P) in the X classes as well: negate the second operand of the class cases of add (Y: 2p - Y, still weak)
    for (name, cx, cy), (a, b, want) in sorted(equal_cases().items()):
        if name == "xyzz_add":
            nb = [b[0], P2 - b[1], b[2], b[3]]
            add.append(("P+(-P) class X:%s" % cx, a, nb, None))
    for v in out.values():
        assert len(v) % 256 != 0
    return out


@functools.lru_cache(maxsize=None)
def on_curve_vectors():
    """[(raw affine words, expected 0 / 1)]: curve points with either coordinate as v or v + p, and near misses"""
    out = []
    for k in (1, 2, 3, 5, 1000, o.R - 1):
        pt = o.mul(k, o.G)
        for m in range(4):
            out.append((present_affine(pt, m), 1))
            q = present_affine(pt, m)
            out.append(([q[0], (q[1] + 1) % P2], 0))
            out.append(([(q[0] + 1) % P2, q[1]], 0))
    out += [([0, 0], 0), ([P, P], 0), ([0, P], 0)]                      # (0, 0) is the encoding of infinity, not a curve point
    return out


# --------------------------------------------------------------------------------------------------------------- MSM
MULT_N = 1 << 12


@functools.lru_cache(maxsize=None)
def multiples():
    return o.multiples(MULT_N)


def point_of(a):
    """a * G for a signed multiplier |a| <= MULT_N; 0 -> None"""
    if a == 0:
        return None
    pt = multiples()[abs(a) - 1]
    return o.neg(pt) if a < 0 else pt


def expected(mult, scalars):
    return o.mul(sum(k * a for k, a in zip(scalars, mult)) % R, o.G)


def windows(c):
    return (257 + c - 1) // c


def digit_scalars(c):
    """the scalars every window size must recode right (signed digits in [-2^(c-1), 2^(c-1)], carry into the next window)"""
    half = 1 << (c - 1)
    full = [w for w in range(windows(c)) if c * w + c <= 256]          # windows that lie wholly below bit 256
    return [
        sum(half << (c * w) for w in full),                            # every digit 2^(c-1): the top bucket, no carry
        sum((half + 1) << (c * w) for w in full),                      # every digit 2^(c-1) + 1: a carry through all windows
        RR - 1,                                                        # carries into the window above bit 255
        R - 1, R,
        # the only non-zero digit, in the top window that holds scalar bits.  Where c divides 256 (c = 8, 16) the window
        # above it starts at bit 256 and only ever receives a carry, so this is digit 2^(c-1) of the window below the top one
        1 << 255,
        0,
    ]


def _case(name, mult, scalars, c, ch=None, meets=()):
    assert len(mult) == len(scalars)
    env = {"RONK_MSM_C": str(c)}
    if ch is not None:
        env["RONK_MSM_CH"] = str(ch)
    return {"name": name, "mult": list(mult), "scalars": list(scalars), "env": env, "c": c, "meets": list(meets)}


def digit_cases():
    """one case per window size c = 5 .. 16: every scalar of digit_scalars(c), each on two points"""
    out = []
    for c in range(5, 17):
        ks = [k for k in digit_scalars(c) for _ in (0, 1)]
        out.append(_case("digits c=%d" % c, range(1, len(ks) + 1), ks, c))
    return out


FOLD_T = (1, 2, 24, 25, 64, 1024, 1025, 1088, 1089)
FOLD_C = 10


def fold_cases():
    """equal scalars: one bucket per window holds all n entries, cut in T tasks of CH entries -- T on both sides of
    collect / heavy (24 | 25) and of direct / sliced heavy (1024 | 1025, where len = ceil(T / 64) leaves empty tail
    slices; 1088 = 64 * 17 fills every slice, 1089 starts len = 18)"""
    rng = random.Random(0xF01D)
    out = []
    for t in FOLD_T:
        k = rng.randrange(R)
        out.append(_case("fold T=%d CH=1" % t, range(1, t + 1), [k] * t, FOLD_C, 1))
    n = 24 * 16 + 5                                                    # T = 25 with a ragged last task of 5 entries
    out.append(_case("fold T=25 CH=16 ragged", range(1, n + 1), [rng.randrange(R)] * n, FOLD_C, 16))
    return out


def stage_cases():
    """equal and opposite operands directed at each stage that calls the complete group law.  `meets` names what the case
    is FOR, as (stage, kind) pairs of stage_events(); the CPU test asserts it on the generated operands.

    Which additions meet which operands depends on the order of a bucket's run, which comes from the LDS cursors of the
    sort's placing pass; nothing but observed behaviour says that it is the input order (it is for the runs of at most 64
    entries of one wavefront; above that not even that).  The expected RESULT of every case holds for any order.  The
    TARGETING of the "opposite partials" and positional cases is for the input order, which is what stage_events() models;
    the "cancelling bucket" cases do not need it: a bucket of finite points whose sum is infinite forces an addition of
    opposite operands somewhere in its fold, whatever the order (the first infinite result has finite operands)."""
    c = FOLD_C
    out = []
    k = 0x1234567 << (3 * c)                                           # some digits in the windows 3 .. 5
    a, q = 7, 11
    # collect (T <= 24): two equal partials; opposite partials with a finite sum; a bucket that cancels
    out.append(_case("collect equal partials", [a] * 32, [k] * 32, c, 16, [("collect", "equal")]))
    out.append(_case("collect opposite partials", [a] * 16 + [-a] * 16 + [q] * 16, [k] * 48, c, 16, [("collect", "opposite")]))
    out.append(_case("collect cancelling bucket", [a] * 16 + [-a] * 16 + [q], [k] * 32 + [1], c, 16, [("collect", "opposite")]))
    # heavy, one workgroup folds the bucket (24 < T <= 1024): the tree adds lane t and lane t + 16 first, so P and -P sit
    # 16 entries apart
    out.append(_case("heavy equal partials", [a] * 26, [k] * 26, c, 1, [("heavy", "equal")]))
    out.append(_case("heavy opposite partials", [a] * 8 + [q] * 8 + [-a] * 8 + [q] * 2, [k] * 26, c, 1, [("heavy", "opposite")]))
    out.append(_case("heavy cancelling bucket", [a] * 13 + [-a] * 13 + [q], [k] * 26 + [1], c, 1, [("heavy", "opposite")]))
    # the sliced path (T > 1024): slices of len = 17 tasks, one per lane; a slice's tree adds lane 0 and 16, then j and j + 8:
    # every full slice holds P on lanes 1 .. 7 against -P on lanes 9 .. 15 (its sum is Q); the slice sums are equal (Q)
    t = 1026
    out.append(_case("sliced heavy equal partials", [a] * t, [k] * t, c, 1, [("sliced0", "equal"), ("sliced1", "equal")]))
    slice_pattern = [a] * 8 + [-a] * 8 + [q]
    out.append(_case("sliced heavy opposite partials", [slice_pattern[i % 17] for i in range(t)], [k] * t, c, 1,
                     [("sliced0", "opposite"), ("sliced1", "equal")]))
    out.append(_case("sliced heavy cancelling bucket", [a] * 513 + [-a] * 513 + [q], [k] * t + [1], c, 1,
                     [("sliced0", "opposite"), ("sliced1", "opposite")]))
    for cc in (5, c):
        for w in (0, 1, windows(cc) - 2):
            s = cc * w
            elsewhere = 1 << (cc * (w + 1))                            # the balancing point goes to the window above
            # bit-plane: digits 1 and 3 are buckets 0 and 2 of one group of 4, both in plane 0
            out.append(_case("bitplane equal c=%d w=%d" % (cc, w), [a, a], [1 << s, 3 << s], cc, None, [("bitplane", "equal")]))
            out.append(_case("bitplane opposite c=%d w=%d" % (cc, w), [a, -a], [1 << s, 3 << s], cc, None, [("bitplane", "opposite")]))
            # 4-to-1 sums: digits d and d + 4 are the same lane of neighbouring groups
            for d in (1, 2, 3):
                out.append(_case("sum equal c=%d w=%d d=%d" % (cc, w, d), [a, a], [d << s, (d + 4) << s], cc, None, [("sum", "equal")]))
                out.append(_case("sum opposite c=%d w=%d d=%d" % (cc, w, d), [a, -a, q], [d << s, (d + 4) << s, elsewhere], cc, None,
                                 [("sum", "opposite")]))
    for cc in (5, 7):                                                  # a window in which every bucket holds the same point
        nb = 1 << (cc - 1)
        out.append(_case("every bucket the same point c=%d" % cc, [a] * nb, [d << cc for d in range(1, nb + 1)], cc, None,
                         [("bitplane", "equal"), ("sum", "equal")]))
    # host tail: the same point under the same digit in two windows; then operands the tail's own additions meet as equal
    # and as opposite group elements in different representations: 2^c * (P from window w+1) against 2^(c-1) * (2P) in window w
    out.append(_case("tail same digit two windows", [a, a], [5 << c, 5 << (4 * c)], c))
    half = 1 << (c - 1)
    out.append(_case("tail equal operands", [a, 2 * a], [1 << (3 * c), half << (2 * c)], c, None, [("tail", "equal")]))
    out.append(_case("tail opposite operands", [a, -2 * a, q], [1 << (3 * c), half << (2 * c), 1], c, None, [("tail", "opposite")]))
    return out


def signed_digits(k, c):
    """the W signed digits of k in [-2^(c-1), 2^(c-1)]: a raw digit above 2^(c-1) borrows 2^c from the window above"""
    out, carry = [], 0
    for w in range(windows(c)):
        raw = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        carry = int(raw > (1 << (c - 1)))
        out.append(raw - (carry << c))
    assert carry == 0 and sum(d << (c * w) for w, d in enumerate(out)) == k
    return out


def stage_events(case):
    """An integer model of the pipeline's SHAPE (msm_kernels.h, msm_common.h): group elements are multiples of G mod r, a
    bucket's run is in input order, and every addition of two finite operands x, y is recorded as (stage, "equal") if
    x == y and (stage, "opposite") if x == -y.  Stages: "accumulate" (mixed additions of a task of CH entries), "collect"
    (T <= 24 tasks, in sequence), "heavy" (24 < T <= 1024: lane t takes tasks t, t + 256, ...; tree over 256 lanes),
    "sliced0" / "sliced1" (T > 1024: 64 slices of ceil(T / 64) tasks, each folded like "heavy"; then the slice sums),
    "bitplane" (groups of 4 buckets per bit of the weight), "sum" (4-to-1 stages), "tail" (the host's Horner steps).
    Returns (events, total multiplier); the total must be sum k_i a_i mod r."""
    c, n = case["c"], len(case["mult"])
    nb = 1 << (c - 1)
    ch = int(case["env"].get("RONK_MSM_CH", max(16, n // nb // 4)))
    events = set()

    def add(x, y, stage):
        if x is None or y is None:
            return y if x is None else x
        if (x - y) % R == 0:
            events.add((stage, "equal"))
        elif (x + y) % R == 0:
            events.add((stage, "opposite"))
        return (x + y) % R or None

    def fold(items, stage):                                            # one workgroup: strided per lane, then the tree
        red = [None] * 256
        for i, v in enumerate(items):
            red[i % 256] = add(red[i % 256], v, stage)
        s = 128
        while s:
            for t in range(s):
                red[t] = add(red[t], red[t + s], stage)
            s >>= 1
        return red[0]

    runs = {}
    for a, k in zip(case["mult"], case["scalars"]):
        for w, d in enumerate(signed_digits(k, c)):
            if d and a:
                runs.setdefault((w, abs(d) - 1), []).append(a % R if d > 0 else -a % R)
    rows = {}
    for w in range(windows(c)):
        buckets = [None] * nb
        for b in range(nb):
            run = runs.get((w, b), [])
            tasks = []
            for i in range(0, len(run), ch):
                acc = None
                for v in run[i:i + ch]:
                    acc = add(acc, v, "accumulate")
                tasks.append(acc)
            if len(tasks) <= 24:
                acc = None
                for v in tasks:
                    acc = add(acc, v, "collect")
            elif len(tasks) <= 1024:
                acc = fold(tasks, "heavy")
            else:
                ln = (len(tasks) + 63) // 64
                acc = fold([fold(tasks[lo:lo + ln], "sliced0") for lo in range(0, len(tasks), ln)], "sliced1")
            buckets[b] = acc
        for kk in range(c):
            cur = []
            for g in range(nb // 4):
                acc = None
                for b in range(4 * g, 4 * g + 4):
                    if ((b + 1) >> kk) & 1:
                        acc = add(acc, buckets[b], "bitplane")
                cur.append(acc)
            while len(cur) > 1:
                nxt = []
                for o in range(0, len(cur), 4):
                    acc = None
                    for v in cur[o:o + 4]:
                        acc = add(acc, v, "sum")
                    nxt.append(acc)
                cur = nxt
            rows[(w, kk)] = cur[0]
    total = None
    for w in reversed(range(windows(c))):
        total = None if total is None else (total << c) % R or None
        win = None
        for kk in reversed(range(c)):
            win = None if win is None else 2 * win % R or None
            win = add(win, rows[(w, kk)], "tail")
        total = add(total, win, "tail")
    return events, total or 0


def msm_cases():
    """every MSM case small enough for the host pipeline as well (n <= 2000)"""
    out = digit_cases() + fold_cases() + stage_cases()
    assert len({cs["name"] for cs in out}) == len(out) and all(len(cs["mult"]) <= 2000 for cs in out)
    return out


# the sort's chunk and the scan's fan-out, from the constants of ronk_msm.hip (MsmWork::alloc, msm_scan)
SORT_CHUNK = 32768
SCAN_LANES, SCAN_PER, SCAN_BLOCKS = 256, 4, 1024


def default_window(n):
    """pick_window of ronk_msm.hip without RONK_MSM_C"""
    lg = 0
    while (1 << lg) < n:
        lg += 1
    c = 10 if lg <= 17 else lg - 5
    if lg < 10:
        c = 6 if lg < 6 else lg
    return min(c, 15)


def sort_shape(n, c):
    """(chunks, keys * chunks, per) as the host code derives them"""
    chunk = SORT_CHUNK
    while (n + chunk - 1) // chunk > 64:
        chunk *= 2
    chunks = (n + chunk - 1) // chunk
    m = windows(c) * (1 << (c - 1)) * chunks
    per = SCAN_PER
    while (m + SCAN_LANES * per - 1) // (SCAN_LANES * per) > SCAN_BLOCKS:
        per *= 2
    return chunks, m, per


SORT_CASES = ((32767, None), (32768, None), (32769, None), (65537, 16))


def sort_case(n, c):
    """(multipliers, scalars, env): the 2^12 multiples of G tiled, random 256-bit scalars with some short ones and a zero"""
    rng = random.Random(n)
    ks = [rng.getrandbits(256) for _ in range(n)]
    for i in range(0, n, 7):
        ks[i] &= (1 << 192) - 1
    for i in range(0, n, 11):
        ks[i] &= (1 << 128) - 1
    ks[5] = 0
    mult = [i % MULT_N + 1 for i in range(n)]
    return mult, ks, ({} if c is None else {"RONK_MSM_C": str(c)})
