"""The edge vectors of tests/bn254_edges.py on the DEVICE.  The device build of csrc/bn254.h is not the code the CPU suite
runs: acc_mad / acc_mad2 are inline assembly there (v_mad_u64_u32 with an explicit carry-out, wait states, v_addc_co_u32)
and an __int128 fallback on the host.  ronk_bn254_probe_dev applies one function of the header to raw limbs, so:

  primitives  every field op on weakly reduced operands in [0, 2p), raw and bit-exact against integer models; the group law
              (add, dbl, madd in both signs) on every operand representation, normalised and compared with the oracle,
              including the three ways U2 - U1 comes out "zero" -- on the default and on a side stream;
  pipeline    directed scalars for every window size, the fold thresholds (collect | heavy | sliced heavy) through
              RONK_MSM_CH, equal and opposite operands at each stage that calls the complete group law, and the sort's chunk
              boundary and the scan's wider fan-out, each against one oracle scalar multiplication.

tests/test_bn254_edges_host.py runs the same vectors through the host build first."""
import os

import numpy as np
import pytest

import bn254_edges as E
from ronkathon_amd import _lib as L
from ronkathon_amd import callers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def side(torch):
    return torch.cuda.Stream()


def dev(torch, raw):
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint64).view(np.int64).copy()).cuda()


def probe(torch, stream, name, a, b):
    """ronk_bn254_probe_dev over the rows `a` (and `b`) on `stream` (None: the default stream) -> rows of integers"""
    op, wa, wb, wo = E.OPS[name]
    n = len(a)
    da = dev(torch, E.pack(a))
    db = dev(torch, E.pack(b)) if wb else None
    assert da.numel() == wa * n and (db is None or db.numel() == wb * n)
    out = torch.full((wo * n,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                                   # uploads and the fill are on the default stream
    L.check(L.lib.ronk_bn254_probe_dev(op, da.data_ptr(), db.data_ptr() if wb else None, out.data_ptr(), n,
                                       stream.cuda_stream if stream is not None else None))
    (stream if stream is not None else torch.cuda.current_stream()).synchronize()
    raw = out.cpu().numpy().view(np.uint64).tobytes()
    return E.unpack(raw, wo // 4, 32) if wo >= 4 else E.unpack(raw, 1, 8)


STREAMS = ("default", "side")


@pytest.mark.parametrize("which", STREAMS)
@pytest.mark.parametrize("idx", range(2 * len(E.FIELD_MODEL)), ids=[n + s for n in E.FIELD_MODEL for s in ("", "-n1")])
def test_field_raw(torch, side, idx, which):
    name, a, b, want = E.field_vectors()[idx]
    got = probe(torch, side if which == "side" else None, name, a, b)
    E.check_field(name, a, b, want, got)


@pytest.mark.parametrize("which", STREAMS)
@pytest.mark.parametrize("name", ["xyzz_add", "xyzz_dbl", "xyzz_madd", "xyzz_madd_neg"])
def test_point_raw(torch, side, name, which):
    stream = side if which == "side" else None
    cases = E.point_vectors()[name]
    binary = E.OPS[name][2] != 0
    E.check_points(name, cases, probe(torch, stream, name, [c[1] for c in cases], [c[2] for c in cases] if binary else None))
    one = cases[-1:]
    E.check_points(name, one, probe(torch, stream, name, [one[0][1]], [one[0][2]] if binary else None))


@pytest.mark.parametrize("which", STREAMS)
def test_on_curve_raw(torch, side, which):
    v = E.on_curve_vectors()
    got = probe(torch, side if which == "side" else None, "on_curve", [q for q, _ in v], None)
    assert [g[0] for g in got] == [w for _, w in v]


def test_probe_leaves_the_rest_alone(torch):
    """n elements are written and not one word more; n = 0 writes nothing"""
    name, a, b, want = E.field_vectors()[0]
    n = 300
    da, db = dev(torch, E.pack(a[:n + 5])), dev(torch, E.pack(b[:n + 5]))
    out = torch.full((4 * (n + 5),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L.check(L.lib.ronk_bn254_probe_dev(E.OPS[name][0], da.data_ptr(), db.data_ptr(), out.data_ptr(), 0, None))
    torch.cuda.synchronize()
    assert bool((out == -1).all())
    L.check(L.lib.ronk_bn254_probe_dev(E.OPS[name][0], da.data_ptr(), db.data_ptr(), out.data_ptr(), n, None))
    torch.cuda.synchronize()
    h = out.cpu().numpy().view(np.uint64)
    assert [r[0] for r in E.unpack(h[:4 * n].tobytes(), 1)] == want[:n]
    assert (h[4 * n:] == np.uint64(2**64 - 1)).all()


# ------------------------------------------------------------------------------------------------------------ pipeline
def with_msm_env(env, call):
    """call() with RONK_MSM_C / RONK_MSM_CH set from `env` alone (the library reads them per call); put back whatever happens"""
    saved = {k: os.environ.get(k) for k in ("RONK_MSM_C", "RONK_MSM_CH")}
    try:
        for k in saved:
            os.environ.pop(k, None)
        os.environ.update(env)
        return call()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


MSM = E.msm_cases()


@pytest.mark.parametrize("case", MSM, ids=[cs["name"] for cs in MSM])
def test_msm_case(case):
    pts = [E.point_of(a) for a in case["mult"]]
    want = E.expected(case["mult"], case["scalars"])
    assert with_msm_env(case["env"], lambda: callers.msm_bn254(pts, case["scalars"])) == want


@pytest.mark.parametrize("n,c", E.SORT_CASES)
def test_msm_sort_and_scan_shapes(torch, n, c):
    """n on both sides of the counting sort's chunk of 32768 scalars, and three chunks at c = 16: more than 256 * 4 * 1024 keys x
    chunks, where the scan doubles its entries per lane"""
    chunks, m, per = E.sort_shape(n, c if c else E.default_window(n))
    assert chunks == (n + E.SORT_CHUNK - 1) // E.SORT_CHUNK
    if c == 16:
        assert chunks == 3 and m > E.SCAN_LANES * E.SCAN_PER * E.SCAN_BLOCKS and per == 8
    else:
        assert per == 4
    mult, ks, env = E.sort_case(n, c)
    want = E.expected(mult, ks)
    pw, sw = E.pack_msm(mult, ks)
    dp, ds = dev(torch, pw), dev(torch, sw)
    out = np.zeros(8, dtype=np.uint64)
    L.check(with_msm_env(env, lambda: L.lib.ronk_msm_bn254_dev(dp.data_ptr(), ds.data_ptr(), n, L.ptr(out), None)))
    x, y = E.unpack(out.tobytes(), 2)[0]
    assert (None if x == 0 and y == 0 else (x, y)) == want
