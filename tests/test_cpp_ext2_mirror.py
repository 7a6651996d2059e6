"""Builds tests/cpp/test_ext2_mirror.cpp, which instantiates every member of the C++ mirror of the quadratic extension
(GaloisField2<P, W> in ronkathon_amd/host/ronkathon.hpp): the scalar operators, host values, on the reference's vectors
(tests/golden/gf101_2_vectors.json) and identities without a device; the array forms on the GPU."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = os.path.join(ROOT, "build", "test_ext2_mirror")
    src = os.path.join(ROOT, "tests", "cpp", "test_ext2_mirror.cpp")
    lib = os.path.join(ROOT, "ronkathon_amd")
    deps = [src, os.path.join(lib, "host", "ronkathon.hpp"), os.path.join(ROOT, "include", "ronk_ntt.h"), os.path.join(lib, "libronk_ntt.so")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", tmp, src, "-L" + lib, "-lronk_ntt", "-Wl,-rpath," + lib,
                               "-Wl,-rpath-link,/opt/rocm/lib"])
        os.replace(tmp, out)
    return out


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.strip()


def test_scalar_operators_on_the_golden_vectors(exe):
    with open(os.path.join(ROOT, "tests", "golden", "gf101_2_vectors.json")) as f:
        golden = json.load(f)
    assert (golden["p"], golden["w"]) == (101, 99)       # PlutoBaseFieldExtension = GaloisField2<101, 99>
    for op in ("add", "sub", "mul"):
        for c in golden[op]:
            assert run(exe, "scalar", op, *c["a"], *c["b"]).split() == [str(v) for v in c["out"]], (op, c)
    for c in golden["neg"]:
        assert run(exe, "scalar", "neg", *c["a"]).split() == [str(v) for v in c["out"]]
    assert run(exe, "scalar", "order", *golden["primitive_element"], golden["primitive_element_order"]) == "1"
    assert run(exe, "scalar", "order", 10, 0, golden["primitive_element_order"]) == "0"      # a base element has a smaller order


def test_identities(exe):
    assert "ALL OK" in run(exe, "identities")


@pytest.mark.gpu
def test_array_forms_on_gpu(exe):
    assert "ALL OK" in run(exe, "device")
