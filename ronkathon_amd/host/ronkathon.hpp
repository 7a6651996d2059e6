// ronkathon.hpp -- C++ host mirror of ronkathon's field / polynomial surface over the C ABI.
//
// The reference is Rust (nightly) and no Rust toolchain exists in this image, so the host side
// above include/ronk_ntt.h is written in C++ with the SAME names, argument meaning and error
// behaviour as the reference, so that tests read like the reference's own:
//   PrimeField<P>            src/algebra/field/prime/mod.rs:39-140, prime/arithmetic.rs:3-71
//   Field / FiniteField      src/algebra/field/mod.rs:17-76   (ZERO, ONE, inverse, pow, PRIMITIVE_ELEMENT,
//                                                              primitive_root_of_unity)
//   Polynomial<B, F, D>      src/polynomial/mod.rs:34-515, src/polynomial/arithmetic.rs:16-146
// A reference panic becomes a thrown ronkathon::Panic carrying the same message.
// Scalars are host values (like the Rust value type); every array operation goes to the GPU
// through libronk_ntt.so -- there is no CPU implementation behind this header.
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ronk_ntt.h"

namespace ronkathon {

struct Panic : std::runtime_error {
  int code;
  explicit Panic(int c) : std::runtime_error(ronk_strerror(c)), code(c) {}
};
inline void check(int rc) { if (rc != RONK_OK) throw Panic(rc); }

// ---- PrimeField<P>: #[repr(transparent)]-like wrapper of the canonical residue
template <uint64_t P>
struct PrimeField {
  uint64_t value = 0;
  static constexpr uint64_t ORDER = P;                       // Finite::ORDER, src/algebra/mod.rs:8-13
  constexpr PrimeField() = default;
  static PrimeField new_(uint64_t v) {                       // prime/mod.rs:48-51 (asserts primality)
    check(ronk_check_prime(P));
    PrimeField f; f.value = v % P; return f;
  }
  PrimeField(uint64_t v) { *this = new_(v); }                // From<usize>
  static PrimeField ZERO() { PrimeField f; f.value = 0; return f; }
  static PrimeField ONE() { PrimeField f; f.value = 1 % P; return f; }
  static PrimeField PRIMITIVE_ELEMENT() {                    // prime/mod.rs:87-90
    uint64_t g; check(ronk_primitive_element(P, &g)); PrimeField f; f.value = g; return f;
  }
  static PrimeField primitive_root_of_unity(uint64_t n) {    // field/mod.rs:70-75
    uint64_t w; check(ronk_root_of_unity(P, PRIMITIVE_ELEMENT().value, n, &w)); PrimeField f; f.value = w; return f;
  }
  PrimeField pow(uint64_t e) const {                         // prime/mod.rs:74-84
    unsigned __int128 r = 1 % P, b = value;
    while (e) { if (e & 1) r = r * b % P; b = b * b % P; e >>= 1; }
    PrimeField f; f.value = (uint64_t)r; return f;
  }
  std::optional<PrimeField> inverse() const {                // prime/mod.rs:62-72
    if (value == 0) return std::nullopt;
    return pow(P - 2);
  }
  friend PrimeField operator+(PrimeField a, PrimeField b) { PrimeField f; f.value = (uint64_t)(((unsigned __int128)a.value + b.value) % P); return f; }
  friend PrimeField operator-(PrimeField a, PrimeField b) { PrimeField f; f.value = a.value >= b.value ? a.value - b.value : a.value - b.value + P; return f; }
  friend PrimeField operator*(PrimeField a, PrimeField b) { PrimeField f; f.value = (uint64_t)((unsigned __int128)a.value * b.value % P); return f; }
  friend PrimeField operator/(PrimeField a, PrimeField b) {  // self * rhs.inverse().unwrap()
    auto i = b.inverse(); if (!i) throw Panic(RONK_ERR_ZERO_INVERSE); return a * *i;
  }
  PrimeField operator-() const { return ZERO() - *this; }
  // FieldExt (field/mod.rs:79-84; prime/mod.rs:142-226)
  bool euler_criterion() const { return pow((P - 1) / 2).value == 1; }
  // Tonelli-Shanks as the reference writes it: (smaller root, larger root); ZERO -> (0, 0); a non-residue is its assert
  std::pair<PrimeField, PrimeField> sqrt() const {
    if (value == 0) return {ZERO(), ZERO()};
    if (P == 2) throw Panic(RONK_ERR_UNSUPPORTED);           // the reference's search for a non-residue never ends over F_2
    if (!euler_criterion()) throw Panic(RONK_ERR_NOT_RESIDUE);
    uint64_t q = P - 1, s = 0;
    while ((q & 1) == 0) { q >>= 1; s++; }
    PrimeField z = new_(2);
    while (z.euler_criterion()) z = z + ONE();
    uint64_t m = s;
    PrimeField c = z.pow(q), t = pow(q), r = pow((q + 1) / 2);
    for (;;) {
      if (t.value == 1) { PrimeField nr = -r; return nr.value < r.value ? std::make_pair(nr, r) : std::make_pair(r, nr); }
      uint64_t i = 1;
      PrimeField t_pow = t.pow(2);
      while (t_pow.value != 1) { t_pow = t_pow.pow(2); i++; }
      PrimeField b = c.pow((uint64_t)1 << (m - i - 1));
      m = i; c = b.pow(2); t = t * c; r = r * b;
    }
  }
  // the same over arrays, on the GPU (ronk_vec_euler / ronk_vec_sqrt)
  static std::vector<uint64_t> vec_euler(const std::vector<PrimeField>& a) {
    std::vector<uint64_t> out(a.size());
    check(ronk_vec_euler(P, reinterpret_cast<const uint64_t*>(a.data()), out.data(), a.size()));
    return out;
  }
  static std::pair<std::vector<PrimeField>, std::vector<PrimeField>> vec_sqrt(const std::vector<PrimeField>& a) {
    std::vector<PrimeField> r0(a.size()), r1(a.size());
    check(ronk_vec_sqrt(P, reinterpret_cast<const uint64_t*>(a.data()), reinterpret_cast<uint64_t*>(r0.data()),
                        reinterpret_cast<uint64_t*>(r1.data()), a.size()));
    return {r0, r1};
  }
  friend bool operator==(PrimeField a, PrimeField b) { return a.value == b.value; }
  friend bool operator!=(PrimeField a, PrimeField b) { return a.value != b.value; }
};
static_assert(sizeof(PrimeField<101>) == sizeof(uint64_t), "PrimeField must be layout-compatible with u64");

using PlutoBaseField = PrimeField<101>;                       // prime/mod.rs:26
using PlutoScalarField = PrimeField<17>;                      // prime/mod.rs:30
using GoldilocksField = PrimeField<RONK_GOLDILOCKS_P>;        // the new 64-bit FiniteField implementor

// ---- GaloisField<2, P> with the irreducible t^2 - W (field/extension/mod.rs, arithmetic.rs, gf_101_2.rs): coeffs in increasing
//      degree.  Scalar operators are host values; the array forms run on the GPU on PLANAR arrays ([2][n] words, c0 plane first).
template <uint64_t P, uint64_t W>
struct GaloisField2 {
  using Base = PrimeField<P>;
  std::array<Base, 2> coeffs{};
  static constexpr uint64_t BASE_ORDER = P;
  GaloisField2() = default;
  static GaloisField2 new_(std::array<Base, 2> c) { check(ronk_ext2_check(P, W)); GaloisField2 f; f.coeffs = c; return f; }
  GaloisField2(Base x) { coeffs = {x, Base::ZERO()}; }                          // From<PrimeField<P>>
  static GaloisField2 ZERO() { return GaloisField2(); }
  static GaloisField2 ONE() { return GaloisField2(Base::ONE()); }
  friend GaloisField2 operator+(GaloisField2 a, GaloisField2 b) { GaloisField2 f; f.coeffs = {a.coeffs[0] + b.coeffs[0], a.coeffs[1] + b.coeffs[1]}; return f; }
  friend GaloisField2 operator-(GaloisField2 a, GaloisField2 b) { GaloisField2 f; f.coeffs = {a.coeffs[0] - b.coeffs[0], a.coeffs[1] - b.coeffs[1]}; return f; }
  GaloisField2 operator-() const { return ZERO() - *this; }
  friend GaloisField2 operator*(GaloisField2 a, GaloisField2 b) {                // the product reduced modulo t^2 - W
    const Base w = Base::new_(W);
    GaloisField2 f;
    f.coeffs = {a.coeffs[0] * b.coeffs[0] + w * a.coeffs[1] * b.coeffs[1], a.coeffs[0] * b.coeffs[1] + a.coeffs[1] * b.coeffs[0]};
    return f;
  }
  friend GaloisField2 operator*(GaloisField2 a, Base s) { GaloisField2 f; f.coeffs = {a.coeffs[0] * s, a.coeffs[1] * s}; return f; }   // Mul<PrimeField<P>>
  friend GaloisField2 operator+(GaloisField2 a, Base s) { return a + GaloisField2(s); }
  friend GaloisField2 operator-(GaloisField2 a, Base s) { return a - GaloisField2(s); }
  Base norm() const { return coeffs[0] * coeffs[0] - Base::new_(W) * coeffs[1] * coeffs[1]; }
  std::optional<GaloisField2> inverse() const {                                  // (a0, -a1) / norm; None for zero
    auto n = norm().inverse();
    if (!n) return std::nullopt;
    GaloisField2 f; f.coeffs = {coeffs[0] * *n, (-coeffs[1]) * *n}; return f;
  }
  friend GaloisField2 operator/(GaloisField2 a, GaloisField2 b) {
    auto i = b.inverse(); if (!i) throw Panic(RONK_ERR_ZERO_INVERSE); return a * *i;
  }
  GaloisField2 pow(uint64_t e) const {
    GaloisField2 r = ONE(), b = *this;
    while (e) { if (e & 1) r = r * b; b = b * b; e >>= 1; }
    return r;
  }
  friend bool operator==(GaloisField2 a, GaloisField2 b) { return a.coeffs == b.coeffs; }
  friend bool operator!=(GaloisField2 a, GaloisField2 b) { return !(a == b); }
  // array forms on planar words (ronk_ext2_vec_*)
  static std::vector<uint64_t> vec_add(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) { return vec2(ronk_ext2_vec_add, a, b); }
  static std::vector<uint64_t> vec_sub(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) { return vec2(ronk_ext2_vec_sub, a, b); }
  static std::vector<uint64_t> vec_mul(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) { return vec2(ronk_ext2_vec_mul, a, b); }
  static std::vector<uint64_t> vec_neg(const std::vector<uint64_t>& a) {
    std::vector<uint64_t> out(a.size()); check(ronk_ext2_vec_neg(P, W, a.data(), out.data(), a.size() / 2)); return out;
  }
  static std::vector<uint64_t> vec_mul_base(const std::vector<uint64_t>& a, const std::vector<uint64_t>& s) {
    if (a.size() != 2 * s.size()) throw Panic(RONK_ERR_INVALID);
    std::vector<uint64_t> out(a.size()); check(ronk_ext2_vec_mul_base(P, W, a.data(), s.data(), out.data(), s.size())); return out;
  }
  static std::vector<uint64_t> vec_pow(const std::vector<uint64_t>& a, uint64_t e) {
    std::vector<uint64_t> out(a.size()); check(ronk_ext2_vec_pow(P, W, a.data(), e, out.data(), a.size() / 2)); return out;
  }
  static std::vector<uint64_t> vec_inv(const std::vector<uint64_t>& a) {
    std::vector<uint64_t> out(a.size()); check(ronk_ext2_vec_inv(P, W, a.data(), out.data(), a.size() / 2)); return out;
  }
 private:
  template <class Fn>
  static std::vector<uint64_t> vec2(Fn fn, const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) {
    if (a.size() != b.size() || a.size() % 2) throw Panic(RONK_ERR_INVALID);
    std::vector<uint64_t> out(a.size()); check(fn(P, W, a.data(), b.data(), out.data(), a.size() / 2)); return out;
  }
};
using PlutoBaseFieldExtension = GaloisField2<101, 99>;        // X^2 + 2 over F_101 (gf_101_2.rs)

// ---- bases (polynomial/mod.rs:48-72)
struct Monomial { friend bool operator==(Monomial, Monomial) { return true; } };
template <class F> struct Lagrange {
  std::vector<F> nodes;
  friend bool operator==(const Lagrange& a, const Lagrange& b) { return a.nodes == b.nodes; }
};

template <class B, class F, size_t D> struct Polynomial;

template <class F, size_t D>
struct Polynomial<Lagrange<F>, F, D> {
  std::array<F, D> coefficients;
  Lagrange<F> basis;
  // Polynomial::<Lagrange<F>,F,D>::new (mod.rs:358-365): assert_eq!((ORDER - 1) % n, 0); nodes = [w^i]
  static Polynomial new_(const std::array<F, D>& c) {
    Polynomial p; p.coefficients = c; p.basis.nodes.resize(D);
    check(ronk_lagrange_nodes(F::ORDER, F::PRIMITIVE_ELEMENT().value, reinterpret_cast<uint64_t*>(p.basis.nodes.data()), D));
    return p;
  }
  size_t num_terms() const { return D; }
  F evaluate(F x) const {                                    // mod.rs:382-415 (barycentric)
    F r; check(ronk_lagrange_eval(F::ORDER, reinterpret_cast<const uint64_t*>(coefficients.data()),
                                  reinterpret_cast<const uint64_t*>(basis.nodes.data()), D, x.value, &r.value));
    return r;
  }
  Polynomial<Monomial, F, D> ifft() const;                   // mod.rs:430-453
  friend bool operator==(const Polynomial& a, const Polynomial& b) { return a.coefficients == b.coefficients && a.basis == b.basis; }
};

template <class F, size_t D>
struct Polynomial<Monomial, F, D> {
  std::array<F, D> coefficients;
  Monomial basis;
  static Polynomial new_(const std::array<F, D>& c) { Polynomial p; p.coefficients = c; return p; }   // mod.rs:98
  template <size_t N> static Polynomial from(const std::array<F, N>& c) {                              // mod.rs:503-515
    Polynomial p; p.coefficients.fill(F::ZERO());
    for (size_t i = 0; i < (N < D ? N : D); i++) p.coefficients[i] = c[i];
    return p;
  }
  const uint64_t* raw() const { return reinterpret_cast<const uint64_t*>(coefficients.data()); }
  uint64_t* raw() { return reinterpret_cast<uint64_t*>(coefficients.data()); }
  size_t num_terms() const { return D; }
  size_t degree() const { for (size_t i = D; i-- > 0;) if (coefficients[i] != F::ZERO()) return i; return 0; }   // mod.rs:113-115
  F leading_coefficient() const { for (size_t i = D; i-- > 0;) if (coefficients[i] != F::ZERO()) return coefficients[i]; return F::ZERO(); }
  F evaluate(F x) const { F r; check(ronk_poly_eval(F::ORDER, raw(), D, x.value, &r.value)); return r; }        // mod.rs:133-139
  template <size_t D2> Polynomial<Monomial, F, D + D2> pow_mult(F coeff) const {                                  // mod.rs:153-157
    Polynomial<Monomial, F, D + D2> r; r.coefficients.fill(F::ZERO());
    std::array<F, D> c; c.fill(coeff);
    check(ronk_vec_mul(F::ORDER, raw(), reinterpret_cast<const uint64_t*>(c.data()), r.raw() + D2, D));
    return r;
  }
  Polynomial<Lagrange<F>, F, D> dft() const {                 // mod.rs:240-258: any D | ORDER-1
    std::array<F, D> out;
    check(ronk_dft(F::ORDER, F::PRIMITIVE_ELEMENT().value, raw(), reinterpret_cast<uint64_t*>(out.data()), D));
    return Polynomial<Lagrange<F>, F, D>::new_(out);
  }
  Polynomial<Lagrange<F>, F, D> fft() const {                 // mod.rs:273-292
    static_assert(D != 0 && (D & (D - 1)) == 0, "fft: D must be a power of two");  // [(); D.is_power_of_two() as usize - 1]:
    Polynomial<Lagrange<F>, F, D> r; r.basis.nodes.resize(D);
    check(ronk_fft(F::ORDER, F::PRIMITIVE_ELEMENT().value, raw(), reinterpret_cast<uint64_t*>(r.coefficients.data()),
                   reinterpret_cast<uint64_t*>(r.basis.nodes.data()), D));
    return r;
  }
  std::pair<Polynomial, Polynomial> quotient_and_remainder_dyn(const uint64_t* b, size_t d2) const {  // mod.rs:170-225
    std::pair<Polynomial, Polynomial> qr;
    check(ronk_poly_divrem(F::ORDER, raw(), D, b, d2, qr.first.raw(), qr.second.raw()));
    return qr;
  }
  friend bool operator==(const Polynomial& a, const Polynomial& b) { return a.coefficients == b.coefficients; }
  Polynomial operator-() const { Polynomial r; check(ronk_vec_neg(F::ORDER, raw(), r.raw(), D)); return r; }   // arithmetic.rs:77-95
};

template <class F, size_t D>
Polynomial<Monomial, F, D> Polynomial<Lagrange<F>, F, D>::ifft() const {
  static_assert(D != 0 && (D & (D - 1)) == 0, "ifft: D must be a power of two");
  Polynomial<Monomial, F, D> r;
  check(ronk_ifft(F::ORDER, F::PRIMITIVE_ELEMENT().value, reinterpret_cast<const uint64_t*>(coefficients.data()), r.raw(), D));
  return r;
}

// impl Add / Sub (arithmetic.rs:16-68): result has len(lhs) coefficients
template <class F, size_t D, size_t D2>
Polynomial<Monomial, F, D> operator+(const Polynomial<Monomial, F, D>& a, const Polynomial<Monomial, F, D2>& b) {
  Polynomial<Monomial, F, D> r; check(ronk_poly_add(F::ORDER, a.raw(), D, b.raw(), D2, r.raw())); return r;
}
template <class F, size_t D, size_t D2>
Polynomial<Monomial, F, D> operator-(const Polynomial<Monomial, F, D>& a, const Polynomial<Monomial, F, D2>& b) {
  Polynomial<Monomial, F, D> r; check(ronk_poly_sub(F::ORDER, a.raw(), D, b.raw(), D2, r.raw())); return r;
}
// impl Mul (arithmetic.rs:97-119): D + D2 - 1 coefficients
template <class F, size_t D, size_t D2>
Polynomial<Monomial, F, D + D2 - 1> operator*(const Polynomial<Monomial, F, D>& a, const Polynomial<Monomial, F, D2>& b) {
  Polynomial<Monomial, F, D + D2 - 1> r;
  check(ronk_poly_mul(F::ORDER, F::PRIMITIVE_ELEMENT().value, a.raw(), D, b.raw(), D2, r.raw()));
  return r;
}
// impl Div / Rem (arithmetic.rs:121-146)
template <class F, size_t D, size_t D2>
Polynomial<Monomial, F, D> operator/(const Polynomial<Monomial, F, D>& a, const Polynomial<Monomial, F, D2>& b) {
  return a.quotient_and_remainder_dyn(b.raw(), D2).first;
}
template <class F, size_t D, size_t D2>
Polynomial<Monomial, F, D> operator%(const Polynomial<Monomial, F, D>& a, const Polynomial<Monomial, F, D2>& b) {
  return a.quotient_and_remainder_dyn(b.raw(), D2).second;
}

// ---- Reed-Solomon (src/codes/reed_solomon.rs) ---------------------------------------------------------
template <class F> struct Coordinate { F x, y; };                                                   // :27-35
template <size_t N, size_t K, class F> struct Codeword { std::array<Coordinate<F>, N> data; };       // :20-25
template <size_t K, class F>
struct Message {                                                                                     // :14-18
  std::array<F, K> data;
  static Message new_(std::array<F, K> d) { return Message{d}; }                                     // :39
  // Message::encode::<N> (:42-52): x_i = root^i, y_i = polynomial.evaluate(root^i)
  template <size_t N> Codeword<N, K, F> encode() const {
    static_assert(N >= K, "Code size must be greater than or equal to K");                            // assert_ge, :108-110
    std::array<uint64_t, N> xs, ys;
    check(ronk_rs_encode(F::ORDER, F::PRIMITIVE_ELEMENT().value, reinterpret_cast<const uint64_t*>(data.data()), K, N,
                         xs.data(), ys.data()));
    Codeword<N, K, F> cw;
    for (size_t i = 0; i < N; i++) { cw.data[i].x.value = xs[i]; cw.data[i].y.value = ys[i]; }
    return cw;
  }
  // Message::decode::<M> (:54-106): interpolate the first K coordinates
  template <size_t M> static Message decode(const Codeword<M, K, F>& cw) {
    static_assert(M >= K, "Code size must be greater than or equal to K");
    std::array<uint64_t, K> xs, ys;
    for (size_t i = 0; i < K; i++) { xs[i] = cw.data[i].x.value; ys[i] = cw.data[i].y.value; }
    Message m;
    check(ronk_rs_decode(F::ORDER, xs.data(), ys.data(), K, reinterpret_cast<uint64_t*>(m.data.data())));
    return m;
  }
  // erasure decoding of encode::<N>'s y-coordinates from ALL survivors, O(N log N) (ronk_rs_recover): the values at `erased`
  // are ignored; returns the message, `full` receives the repaired y-coordinates.  Throws RONK_ERR_NOT_CODEWORD for survivors
  // on no polynomial of degree < K.
  template <size_t N> static Message recover(const std::array<F, N>& ys, const std::vector<uint64_t>& erased, std::array<F, N>* full = nullptr) {
    static_assert(N >= K, "Code size must be greater than or equal to K");
    Message m;
    check(ronk_rs_recover(F::ORDER, F::PRIMITIVE_ELEMENT().value, N, K, erased.empty() ? nullptr : erased.data(), erased.size(),
                          reinterpret_cast<const uint64_t*>(ys.data()), reinterpret_cast<uint64_t*>(m.data.data()),
                          full ? reinterpret_cast<uint64_t*>(full->data()) : nullptr));
    return m;
  }
};

// prod_i (x - roots[i]), monic, roots.size() + 1 coefficients (the product tree, ronk_poly_from_roots)
template <class F> std::vector<F> poly_from_roots(const std::vector<F>& roots) {
  std::vector<F> out(roots.size() + 1);
  check(ronk_poly_from_roots(F::ORDER, roots.empty() ? nullptr : reinterpret_cast<const uint64_t*>(roots.data()), roots.size(),
                             reinterpret_cast<uint64_t*>(out.data())));
  return out;
}

// f at every point of xs (Polynomial::evaluate in a loop, src/shamir/mod.rs:33-60) in one call (ronk_poly_eval_many)
template <class F> std::vector<F> poly_eval_many(const std::vector<F>& coeffs, const std::vector<F>& xs) {
  std::vector<F> out(xs.size());
  check(ronk_poly_eval_many(F::ORDER, reinterpret_cast<const uint64_t*>(coeffs.data()), coeffs.size(),
                            reinterpret_cast<const uint64_t*>(xs.data()), xs.size(), reinterpret_cast<uint64_t*>(out.data())));
  return out;
}
// the xs.size() coefficients of the polynomial through (xs[i], ys[i]), any distinct nodes (ronk_poly_interpolate); coincident
// nodes throw RONK_ERR_ZERO_INVERSE
template <class F> std::vector<F> poly_interpolate(const std::vector<F>& xs, const std::vector<F>& ys) {
  std::vector<F> out(xs.size());
  check(xs.size() == ys.size() ? RONK_OK : RONK_ERR_INVALID);
  check(ronk_poly_interpolate(F::ORDER, reinterpret_cast<const uint64_t*>(xs.data()), reinterpret_cast<const uint64_t*>(ys.data()),
                              xs.size(), reinterpret_cast<uint64_t*>(out.data())));
  return out;
}

// ---- KZG commit / open (src/kzg/setup.rs:45-78) over AffinePoint<PlutoExtendedCurve> (src/curve/mod.rs:66-73) --------
struct AffinePoint {                       // Point(x, y) with x = x0 + x1 t, y = y0 + y1 t in GF(101^2), or Infinity
  std::array<uint64_t, 5> w{0, 0, 0, 0, 1};
  static AffinePoint Infinity() { return AffinePoint{}; }
  static AffinePoint new_(uint64_t x0, uint64_t x1, uint64_t y0, uint64_t y1) { AffinePoint p; p.w = {x0, x1, y0, y1, 0}; return p; }
  friend bool operator==(const AffinePoint& a, const AffinePoint& b) { return a.w == b.w; }
};
inline const ronk_curve& PlutoExtendedCurve() { static const ronk_curve c{101, 99, 0, 3}; return c; }   // pluto_curve.rs:39-51
// ---- Poseidon over a 64-bit prime field and a Merkle tree on its sponge (hashes/poseidon/mod.rs:56-149, sponge.rs:69-275,
// tree/merkle.rs:31-99 with the sponge as the hash).  Constants come from the caller, as in the reference.
template <class F> class Poseidon {
 public:
  Poseidon(size_t width, size_t alpha, size_t num_p, size_t num_f, size_t rate, const std::vector<F>& rc, const std::vector<F>& mds)
      : width_(width), rate_(rate) {
    if (rc.size() != (num_p + num_f) * width || mds.size() != width * width) throw Panic(RONK_ERR_INVALID);
    check(ronk_poseidon_create(&h_, F::ORDER, (uint32_t)width, alpha, (uint32_t)num_p, (uint32_t)num_f, (uint32_t)rate,
                               reinterpret_cast<const uint64_t*>(rc.data()), reinterpret_cast<const uint64_t*>(mds.data())));
  }
  Poseidon(const Poseidon&) = delete;
  Poseidon& operator=(const Poseidon&) = delete;
  ~Poseidon() { if (h_) ronk_poseidon_destroy(h_); }
  const ronk_poseidon* raw() const { return h_; }
  size_t width() const { return width_; }
  size_t rate() const { return rate_; }
  // Poseidon::hash: pad with ZERO, permute, state[1]
  F hash(const std::vector<F>& state) const {
    std::vector<F> out(width_);
    check(ronk_poseidon_hash(h_, state.empty() ? nullptr : reinterpret_cast<const uint64_t*>(state.data()), state.size(),
                             reinterpret_cast<uint64_t*>(out.data())));
    return out[1];
  }

 private:
  ronk_poseidon* h_ = nullptr;
  size_t width_, rate_;
};

enum class LeftOrRight { Left, Right };
// MerkleTree over a Poseidon sponge: leaves are n x leaf_len field elements, row-major; every level is kept (leaves first)
template <class F> class MerkleTree {
 public:
  using Proof = std::vector<std::pair<std::vector<F>, LeftOrRight>>;
  MerkleTree(const Poseidon<F>& hasher, const std::vector<F>& leaves, size_t leaf_len, size_t digest_len)
      : hasher_(hasher), n_(leaf_len ? leaves.size() / leaf_len : 0), d_(digest_len), tree_(ronk_merkle_tree_words(n_, d_)) {
    check(ronk_merkle_commit(hasher.raw(), reinterpret_cast<const uint64_t*>(leaves.data()), n_, leaf_len, d_,
                             reinterpret_cast<uint64_t*>(tree_.data())));
  }
  size_t depth() const { size_t l = 0; while (ronk_merkle_level_offset(n_, d_, l + 1) < tree_.size()) l++; return l; }
  std::vector<F> root_hash() const { return std::vector<F>(tree_.end() - d_, tree_.end()); }
  // throws RONK_ERR_INDEX where the reference's get_proof indexes out of bounds
  Proof get_proof(size_t leaf_index) const {
    const size_t dep = depth();
    std::vector<F> path(dep * d_ + 1);
    uint64_t idx = leaf_index; int status = 0;
    check(ronk_merkle_open(reinterpret_cast<const uint64_t*>(tree_.data()), n_, d_, &idx, 1, reinterpret_cast<uint64_t*>(path.data()), &status));
    check(status);
    Proof pr;
    for (size_t l = 0; l < dep; l++)
      pr.push_back({std::vector<F>(path.begin() + l * d_, path.begin() + (l + 1) * d_), ((leaf_index >> l) & 1) ? LeftOrRight::Left : LeftOrRight::Right});
    return pr;
  }
  bool prove(const std::vector<F>& leaf, const Proof& proof) const {
    if (proof.size() != depth()) return false;
    uint64_t idx = 0;
    std::vector<F> path;
    for (size_t l = 0; l < proof.size(); l++) {
      if (proof[l].first.size() != d_) return false;
      if (proof[l].second == LeftOrRight::Left) idx |= (uint64_t)1 << l;
      path.insert(path.end(), proof[l].first.begin(), proof[l].first.end());
    }
    if (path.empty()) path.resize(1);
    int ok = 0;
    check(ronk_merkle_verify(hasher_.raw(), reinterpret_cast<const uint64_t*>(leaf.data()), 1, leaf.size(), &idx,
                             reinterpret_cast<const uint64_t*>(path.data()), n_, d_, reinterpret_cast<const uint64_t*>(&*(tree_.end() - d_)), &ok));
    return ok == 1;
  }

 private:
  const Poseidon<F>& hasher_;
  size_t n_, d_;
  std::vector<F> tree_;
};

namespace kzg {
// commit(coeffs, g1_srs): SUM g1_srs[i] * coeffs[i]
template <class S>
AffinePoint commit(const std::vector<S>& coeffs, const std::vector<AffinePoint>& g1_srs, const ronk_curve& curve = PlutoExtendedCurve()) {
  std::vector<uint64_t> pts, sc;
  for (auto& p : g1_srs) pts.insert(pts.end(), p.w.begin(), p.w.end());
  for (auto& c : coeffs) sc.push_back(c.value);
  AffinePoint out;
  check(ronk_curve_msm(&curve, pts.data(), g1_srs.size(), sc.data(), sc.size(), out.w.data()));
  return out;
}
// open::<D>(coeffs, eval_point, g1_srs): commit(poly.div([-z, 1]).coefficients, g1_srs)
template <class S, size_t D>
AffinePoint open(const std::array<S, D>& coeffs, S eval_point, const std::vector<AffinePoint>& g1_srs) {
  auto poly = Polynomial<Monomial, S, D>::new_(coeffs);
  auto divisor = Polynomial<Monomial, S, 2>::new_(std::array<S, 2>{-eval_point, S::ONE()});
  auto q = poly / divisor;
  return commit(std::vector<S>(q.coefficients.begin(), q.coefficients.end()), g1_srs);
}
}  // namespace kzg

// ---- the same commit over a production-size group: BN254 (alt_bn128) G1, y^2 = x^3 + 3 -------------------------------
// ronkathon's field traits are usize-wide (src/algebra/mod.rs:8-13), so the 254-bit types are plain data here: four 64-bit
// little-endian limbs per coordinate / scalar, standard form, (0, 0) = the point at infinity (what ronk_msm_bn254 takes).
namespace bn254 {
using Limbs = std::array<uint64_t, 4>;
struct G1Affine {
  Limbs x{0, 0, 0, 0}, y{0, 0, 0, 0};
  static G1Affine Infinity() { return G1Affine{}; }
  static G1Affine Generator() { G1Affine g; g.x = {1, 0, 0, 0}; g.y = {2, 0, 0, 0}; return g; }
  friend bool operator==(const G1Affine& a, const G1Affine& b) { return a.x == b.x && a.y == b.y; }
};
static_assert(sizeof(G1Affine) == 64, "G1Affine is passed to the C ABI as 8 words");
// kzg::commit (src/kzg/setup.rs:48-60): SUM g1_srs[i] * coeffs[i]; asserts like the reference that the SRS is long enough
inline G1Affine commit(const std::vector<Limbs>& coeffs, const std::vector<G1Affine>& g1_srs) {
  if (g1_srs.size() < coeffs.size()) throw Panic(RONK_ERR_INDEX);
  G1Affine out;
  check(ronk_msm_bn254(reinterpret_cast<const uint64_t*>(g1_srs.data()), reinterpret_cast<const uint64_t*>(coeffs.data()),
                       coeffs.size(), reinterpret_cast<uint64_t*>(&out)));
  return out;
}
// kzg::open (src/kzg/setup.rs:63-78) on the same curve: poly.div([-eval_point, ONE]) over BN254's scalar field, then commit of the
// quotient; also hands back poly(eval_point).  Same assert on the SRS length as commit.
struct Opening { G1Affine proof; Limbs value; };
inline Opening open(const std::vector<Limbs>& coeffs, const Limbs& eval_point, const std::vector<G1Affine>& g1_srs) {
  Opening o;
  check(ronk_kzg_open_bn254(reinterpret_cast<const uint64_t*>(coeffs.data()), coeffs.size(), eval_point.data(),
                            reinterpret_cast<const uint64_t*>(g1_srs.data()), g1_srs.size(), reinterpret_cast<uint64_t*>(&o.proof),
                            o.value.data()));
  return o;
}
}  // namespace bn254

// ---- heap- / device-resident polynomials, plans, the sharded transform ------------------------------------------------
// The counterpart of rust/ronk-goldilocks/src/device.rs: the reference's Polynomial<B, F, D> stores [F; D] inline
// (src/polynomial/mod.rs:34-44), which the stack cannot hold at D = 2^22; these carry the same data without a template
// length and keep it in HBM between operations.  Goldilocks (p = 2^64 - 2^32 + 1, generator 7) only.  Same values and
// panics as fft (mod.rs:273-323), ifft (:430-484), Mul (arithmetic.rs:97-119), evaluate (mod.rs:133-139), Div by a linear
// divisor (kzg::open, src/kzg/setup.rs:63-78).
namespace device {
constexpr uint64_t P = RONK_GOLDILOCKS_P, G = RONK_GOLDILOCKS_G;

class DevicePoly {
 public:
  explicit DevicePoly(size_t len) : len_(len) {
    void* p = nullptr;
    check(ronk_dev_alloc(&p, len * 8));
    ptr_ = static_cast<uint64_t*>(p);
  }
  explicit DevicePoly(const std::vector<uint64_t>& coefficients) : DevicePoly(coefficients.size()) {
    check(ronk_memcpy_h2d(ptr_, coefficients.data(), len_ * 8));
  }
  DevicePoly(DevicePoly&& o) noexcept : ptr_(o.ptr_), len_(o.len_) { o.ptr_ = nullptr; }
  DevicePoly(const DevicePoly&) = delete;
  DevicePoly& operator=(const DevicePoly&) = delete;
  ~DevicePoly() { if (ptr_) { ronk_dev_sync(); ronk_dev_free(ptr_); } }
  size_t size() const { return len_; }
  uint64_t* data() { return ptr_; }
  const uint64_t* data() const { return ptr_; }
  std::vector<uint64_t> to_host() const {
    std::vector<uint64_t> v(len_);
    check(ronk_dev_sync());
    check(ronk_memcpy_d2h(v.data(), ptr_, len_ * 8));
    return v;
  }
  DevicePoly mul(const DevicePoly& rhs) const {            // impl Mul: len + rhs.len - 1 coefficients
    DevicePoly out(len_ + rhs.len_ - 1);
    check(ronk_poly_mul_dev(P, G, ptr_, len_, rhs.ptr_, rhs.len_, out.ptr_, nullptr));
    return out;
  }
  uint64_t evaluate(uint64_t x) const {                    // Polynomial::<Monomial>::evaluate
    DevicePoly y(1);
    check(ronk_poly_eval_dev(P, ptr_, len_, x, y.ptr_, nullptr));
    return y.to_host()[0];
  }
  // self / [b0, b1] and the remainder's constant term: kzg::open's poly.div([-z, 1])
  std::pair<DevicePoly, uint64_t> div_linear(uint64_t b0, uint64_t b1) const {
    DevicePoly q(len_), r(1);
    check(ronk_poly_div_linear_dev(P, ptr_, len_, b0, b1, q.ptr_, r.ptr_, nullptr));
    const uint64_t rem = r.to_host()[0];
    return {std::move(q), rem};
  }

 private:
  uint64_t* ptr_ = nullptr;
  size_t len_ = 0;
};

// ronk_plan: twiddles + scratch for one (n = 2^log2n, batch); two_lanes = ronk_plan_opts::in_flight = 2
class Plan {
 public:
  Plan(uint32_t log2n, uint64_t batch = 1, bool two_lanes = false) : log2n_(log2n), batch_(batch) {
    ronk_plan_opts o = RONK_PLAN_OPTS_DEFAULT;
    if (two_lanes) o.in_flight = 2;
    check(ronk_plan_create_opts(&h_, P, G, log2n, batch, -1, &o));
  }
  Plan(const Plan&) = delete;
  Plan& operator=(const Plan&) = delete;
  ~Plan() { if (h_) ronk_plan_destroy(h_); }
  size_t n() const { return (size_t)1 << log2n_; }
  int in_flight() const { return ronk_plan_in_flight(h_); }
  // every polynomial handed to the plan holds exactly batch * n elements (the library sees bare pointers: a shorter
  // buffer would be read / written out of bounds) -- the Rust mirror asserts the same (rust/.../device.rs)
  void need(const DevicePoly& p) const { if (p.size() != n() * batch_) throw Panic(RONK_ERR_INVALID); }
  void forward(const DevicePoly& src, DevicePoly& dst) const { need(src); need(dst); check(ronk_ntt_forward_dev(h_, src.data(), dst.data(), nullptr)); }
  void inverse(const DevicePoly& src, DevicePoly& dst) const { need(src); need(dst); check(ronk_ntt_inverse_dev(h_, src.data(), dst.data(), nullptr)); }
  // K unrelated polynomials per call: the library keeps two transforms in flight
  void forward_many(const std::vector<const DevicePoly*>& src, const std::vector<DevicePoly*>& dst) const {
    std::vector<const uint64_t*> in;
    std::vector<uint64_t*> out;
    if (src.size() != dst.size()) throw Panic(RONK_ERR_INVALID);
    for (auto* p : src) { need(*p); in.push_back(p->data()); }
    for (auto* p : dst) { need(*p); out.push_back(p->data()); }
    check(ronk_ntt_forward_many_dev(h_, in.data(), out.data(), in.size(), nullptr));
  }
  // host vectors through the plan (a batch is pipelined over its polynomials: upload | transform | download)
  // erasure decoding of `batch` codewords (encode layout, batch x n) that lost the same positions (ronk_rs_recover_batch_dev):
  // msgs receives batch x k coefficients; returns one status per row (0 or RONK_ERR_NOT_CODEWORD; a malformed list throws)
  std::vector<int> recover_batch(size_t k, const std::vector<uint64_t>& erased, const DevicePoly& ys, DevicePoly& msgs) const {
    need(ys);
    if (msgs.size() != k * batch_) throw Panic(RONK_ERR_INVALID);
    DevicePoly er(erased.empty() ? std::vector<uint64_t>{0} : erased), status((batch_ + 1) / 2);
    check(ronk_rs_recover_batch_dev(h_, k, er.data(), erased.size(), ys.data(), msgs.data(), nullptr, reinterpret_cast<int*>(status.data()),
                                    nullptr));
    const std::vector<uint64_t> w = status.to_host();
    std::vector<int> st(batch_);
    for (size_t b = 0; b < batch_; b++) st[b] = (int)(uint32_t)(w[b / 2] >> (32 * (b % 2)));
    for (int e : st) if (e == RONK_ERR_ZERO_INVERSE || e == RONK_ERR_INDEX) throw Panic(e);
    return st;
  }
  std::vector<uint64_t> forward_host(const std::vector<uint64_t>& x) const {
    if (x.size() != n() * batch_) throw Panic(RONK_ERR_INVALID);
    std::vector<uint64_t> y(x.size());
    check(ronk_ntt_forward(h_, x.data(), y.data(), nullptr));
    return y;
  }

 private:
  ronk_plan* h_ = nullptr;
  uint32_t log2n_;
  uint64_t batch_;
};

// ronk_sharded_plan: one transform over `devices` (four-step; exchange = peer-copy mesh or RCCL)
class ShardedPlan {
 public:
  ShardedPlan(uint32_t log2n, const std::vector<int>& devices, bool inverse = false, int chunks = 0, int exchange = RONK_EXCHANGE_MESH)
      : n_((size_t)1 << log2n) {
    check(ronk_sharded_plan_create_ex(&h_, log2n, inverse ? 1 : 0, devices.data(), (int)devices.size(), chunks, exchange));
  }
  // the same over any odd prime p with 2^log2n | p - 1 and primitive element g (ronk_sharded_plan_create_p)
  ShardedPlan(uint64_t p, uint64_t g, uint32_t log2n, const std::vector<int>& devices, bool inverse = false, int chunks = 0,
              int exchange = RONK_EXCHANGE_MESH)
      : n_((size_t)1 << log2n) {
    check(ronk_sharded_plan_create_p(&h_, p, g, log2n, inverse ? 1 : 0, devices.data(), (int)devices.size(), chunks, exchange));
  }
  ShardedPlan(const ShardedPlan&) = delete;
  ShardedPlan& operator=(const ShardedPlan&) = delete;
  ~ShardedPlan() { if (h_) ronk_sharded_plan_destroy(h_); }
  std::vector<uint64_t> transform(const std::vector<uint64_t>& x) const {   // natural order in and out
    if (x.size() != n_) throw Panic(RONK_ERR_INVALID);
    std::vector<uint64_t> y(n_);
    check(ronk_ntt_sharded(h_, x.data(), y.data()));
    return y;
  }

 private:
  ronk_sharded_plan* h_ = nullptr;
  size_t n_;
};

// ronk_sharded_mul_plan: a * b over `devices` (flags: RONK_SHARDED_MUL_UNFUSED / RONK_SHARDED_MUL_FUSED, 0 = the measured default)
class ShardedMulPlan {
 public:
  ShardedMulPlan(uint64_t p, uint64_t g, uint32_t log2n, const std::vector<int>& devices, int chunks = 0,
                 int exchange = RONK_EXCHANGE_MESH, int flags = 0)
      : n_((size_t)1 << log2n) {
    check(ronk_sharded_mul_plan_create_p(&h_, p, g, log2n, devices.data(), (int)devices.size(), chunks, exchange, flags));
  }
  ShardedMulPlan(const ShardedMulPlan&) = delete;
  ShardedMulPlan& operator=(const ShardedMulPlan&) = delete;
  ~ShardedMulPlan() { if (h_) ronk_sharded_mul_plan_destroy(h_); }
  bool fused_middle() const {
    int f = 0;
    check(ronk_sharded_mul_plan_info(h_, nullptr, nullptr, nullptr, nullptr, &f));
    return f != 0;
  }
  // host coefficient vectors, a.size() + b.size() - 1 <= n: the product
  std::vector<uint64_t> mul(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) const {
    if (a.empty() || b.empty() || a.size() + b.size() - 1 > n_) throw Panic(RONK_ERR_INVALID);
    std::vector<uint64_t> out(a.size() + b.size() - 1);
    check(ronk_poly_mul_sharded(h_, a.data(), a.size(), b.data(), b.size(), out.data()));
    return out;
  }

 private:
  ronk_sharded_mul_plan* h_ = nullptr;
  size_t n_;
};
}  // namespace device

}  // namespace ronkathon
