"""rust/ronk-goldilocks/in_tree/ronkathon.patch: the edit that makes ronkathon's own `poly.fft()` / `a * b` / `a / b` call
sites reach the GPU for `Goldilocks` (row N3 of SURVEY.md 8f).  The suite compiles no Rust, so what can be checked is
checked, from the repository alone: the patch applies cleanly (`git apply --check`) to the pre-image its own hunks record, it is the one the
generator produces from the crate's current sources, and the vendored FFI block is the crate's FFI block."""
import importlib.util
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "rust", "ronk-goldilocks", "in_tree", "ronkathon.patch")


def new_file_body(patch, path):
    """content of a file the patch creates (lines after its hunk header, '+' stripped)"""
    marker = "+++ b/" + path + "\n"
    i = patch.index(marker)
    j = patch.find("\ndiff --git ", i)
    body = patch[i + len(marker): j + 1 if j >= 0 else len(patch)]
    lines = body.splitlines(keepends=True)
    assert lines[0].startswith("@@ -0,0 +1,")
    assert all(ln.startswith("+") for ln in lines[1:])
    return "".join(ln[1:] for ln in lines[1:])


def test_patch_vendors_the_crate_ffi_verbatim():
    patch = open(PATCH).read()
    ffi = open(os.path.join(ROOT, "rust", "ronk-goldilocks", "src", "ffi.rs")).read()
    assert new_file_body(patch, "src/algebra/field/goldilocks/ffi.rs") == ffi
    gpu = new_file_body(patch, "src/algebra/field/goldilocks/gpu.rs")
    assert "ronkathon::" not in gpu and "use super::{" in gpu and "fn fft_gpu" in gpu
    disp = new_file_body(patch, "src/polynomial/dispatch.rs")
    for item in ("default fn fft_impl", "default fn ifft_impl", "default fn dft_impl", "default fn evaluate_impl",
                 "default fn quotient_and_remainder_impl", "Accelerated::fft_gpu(self)", "Accelerated::mul_gpu(&self, &rhs)"):
        assert item in disp, item
    assert "unimplemented!" not in patch


def patch_preimages(patch):
    """the edited files as far as the patch shows them: context and removed lines of every hunk, in order"""
    out = {}
    for part in re.split(r"(?m)^(?=diff --git )", patch):
        if not part or "\nnew file mode" in part:
            continue
        path = re.match(r"diff --git a/(\S+)", part).group(1)
        out[path] = "".join(ln[1:] for ln in part.splitlines(keepends=True)
                            if ln.startswith((" ", "-")) and not ln.startswith("--- "))
    return out


def load_generator():
    """tools/make_in_tree_patch.py as a module (its command line is parsed at import: give it an empty one)"""
    argv, sys.argv = sys.argv, [os.path.join(ROOT, "tools", "make_in_tree_patch.py")]
    try:
        spec = importlib.util.spec_from_file_location("make_in_tree_patch", sys.argv[0])
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
    finally:
        sys.argv = argv
    return gen


def test_patch_applies_to_its_preimage_and_is_current(tmp_path):
    patch = open(PATCH).read()
    pre = patch_preimages(patch)
    assert sorted(pre) == ["Cargo.toml", "src/algebra/field/mod.rs", "src/polynomial/arithmetic.rs", "src/polynomial/mod.rs"]
    scratch = tmp_path / "ronkathon"
    for rel, text in pre.items():
        (scratch / rel).parent.mkdir(parents=True, exist_ok=True)
        (scratch / rel).write_text(text)
    subprocess.check_call(["git", "init", "-q", "."], cwd=scratch)
    subprocess.check_call(["git", "apply", "--check", PATCH], cwd=scratch)
    subprocess.check_call(["git", "apply", PATCH], cwd=scratch)
    mod = (scratch / "src" / "polynomial" / "mod.rs").read_text()
    for name in ("evaluate_reference", "quotient_and_remainder_reference", "dft_reference", "fft_reference", "ifft_reference"):
        assert "fn " + name in mod
    assert "default fn mul" in (scratch / "src" / "polynomial" / "arithmetic.rs").read_text()
    assert "pub mod goldilocks;" in (scratch / "src" / "algebra" / "field" / "mod.rs").read_text()
    for f in ("build.rs", "src/polynomial/dispatch.rs", "src/algebra/field/goldilocks/mod.rs", "src/algebra/field/goldilocks/ffi.rs",
              "src/algebra/field/goldilocks/gpu.rs"):
        assert (scratch / f).is_file()
    # the committed patch is what the generator makes today: its edits turn each pre-image into the patched file (the
    # anchors of polynomial/mod.rs reach past the hunks' context, so that file is checked by the names above), and the new
    # files are the generator's output from the crate's sources, byte for byte
    gen = load_generator()
    for rel, edit in (("Cargo.toml", gen.edit_cargo), ("src/algebra/field/mod.rs", gen.edit_field_mod),
                      ("src/polynomial/arithmetic.rs", gen.edit_polynomial_arithmetic)):
        assert edit(pre[rel]) == (scratch / rel).read_text(), rel
    crate = os.path.join(ROOT, "rust", "ronk-goldilocks", "src")
    new = "".join([gen.udiff(None, gen.BUILD_RS, "build.rs"),
                   gen.udiff(None, gen.vendor_ffi(gen.read(os.path.join(crate, "ffi.rs"))), "src/algebra/field/goldilocks/ffi.rs"),
                   gen.udiff(None, gen.vendor_gpu(gen.read(os.path.join(crate, "polynomial.rs"))), "src/algebra/field/goldilocks/gpu.rs"),
                   gen.udiff(None, gen.vendor_field(gen.read(os.path.join(crate, "field.rs"))), "src/algebra/field/goldilocks/mod.rs"),
                   gen.udiff(None, gen.DISPATCH_RS, "src/polynomial/dispatch.rs")])
    assert patch[patch.index("diff --git a/build.rs"):] == new, "rust sources changed: re-run tools/make_in_tree_patch.py and commit the patch"
