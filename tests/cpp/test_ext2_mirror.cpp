// test_ext2_mirror.cpp -- the GaloisField<2, P>-shaped mirror of ronkathon_amd/host/ronkathon.hpp (GaloisField2<P, W>): every
// member is instantiated.  The scalar operators are host values and are checked on the cases the caller passes (the reference's
// vectors over F_101[t] / (t^2 + 2), read from tests/golden/gf101_2_vectors.json by tests/test_cpp_ext2_mirror.py):
//   test_ext2_mirror scalar <op> a0 a1 [b0 b1]      prints "c0 c1" of add / sub / mul / neg, or the order check of `order g0 g1 n`
//   test_ext2_mirror identities                     the reference's algebraic identities on fixed values; "ALL OK"
//   test_ext2_mirror device                         the array forms through the GPU against the scalar operators; "ALL OK"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../ronkathon_amd/host/ronkathon.hpp"

using namespace ronkathon;
using E = PlutoBaseFieldExtension;
using B = PlutoBaseField;
using G = GaloisField2<RONK_GOLDILOCKS_P, 7>;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static E el(const char* a, const char* b) { return E::new_({B(strtoull(a, nullptr, 0)), B(strtoull(b, nullptr, 0))}); }

template <class X>
static void identities(X x, X y, X z) {
  using Base = typename X::Base;
  CHECK(x + (-x) == X::ZERO() && -x == X::ZERO() - x);
  CHECK(x * (-x) == -(x * x) && x + y == y + x && x * y == y * x);
  CHECK(x * (y * z) == (x * y) * z && x - (y + z) == (x - y) - z && x * (y + z) == x * y + x * z);
  CHECK(x.pow(0) == X::ONE() && x.pow(1) == x && x.pow(4) == x * x * x * x);
  CHECK(x * *x.inverse() == X::ONE() && (x / y) * y == x && x / (y * z) == (x / y) / z);
  CHECK(!X::ZERO().inverse().has_value());
  CHECK((x + y) + (x - y) == x * Base(2));                    // Mul<PrimeField<P>>
  CHECK(x + Base(3) == x + X(Base(3)) && x - Base(3) == x - X(Base(3)) && x != x + Base(1));
  X conj = x; conj.coeffs[1] = -conj.coeffs[1];
  CHECK(x.pow(X::BASE_ORDER) == conj && (x * conj).coeffs[0] == x.norm() && (x * conj).coeffs[1] == Base::ZERO());
}

template <class X>
static std::vector<uint64_t> planar(const std::vector<X>& v) {
  std::vector<uint64_t> o(2 * v.size());
  for (size_t i = 0; i < v.size(); i++) { o[i] = v[i].coeffs[0].value; o[v.size() + i] = v[i].coeffs[1].value; }
  return o;
}

template <class X>
static void array_forms(std::vector<X> a, std::vector<X> b) {
  using Base = typename X::Base;
  const size_t n = a.size();
  std::vector<X> s(n), d(n), m(n), ng(n), mb(n), pw(n), iv(n);
  std::vector<uint64_t> sc(n);
  for (size_t i = 0; i < n; i++) {
    sc[i] = 5 + i;
    s[i] = a[i] + b[i]; d[i] = a[i] - b[i]; m[i] = a[i] * b[i]; ng[i] = -a[i]; mb[i] = a[i] * Base(sc[i]); pw[i] = a[i].pow(77);
    iv[i] = *a[i].inverse();
  }
  const auto pa = planar(a), pb = planar(b);
  CHECK(X::vec_add(pa, pb) == planar(s) && X::vec_sub(pa, pb) == planar(d) && X::vec_mul(pa, pb) == planar(m));
  CHECK(X::vec_neg(pa) == planar(ng) && X::vec_mul_base(pa, sc) == planar(mb) && X::vec_pow(pa, 77) == planar(pw));
  CHECK(X::vec_inv(pa) == planar(iv));
  bool threw = false;
  try { X::vec_inv(planar(std::vector<X>{a[0], X::ZERO()})); } catch (const Panic& e) { threw = e.code == RONK_ERR_ZERO_INVERSE; }
  CHECK(threw);
}

int main(int argc, char** argv) {
  if (argc >= 5 && !strcmp(argv[1], "scalar")) {
    const E a = el(argv[3], argv[4]);
    E r;
    if (!strcmp(argv[2], "neg")) r = -a;
    else if (!strcmp(argv[2], "order") && argc >= 6) {   // g^n == 1 and g^(n / q) != 1 for the primes q of 101^2 - 1 = 2^3 3 5^2 17
      const uint64_t n = strtoull(argv[5], nullptr, 0);
      bool ok = a.pow(n) == E::ONE();
      for (uint64_t q : {2, 3, 5, 17}) ok = ok && a.pow(n / q) != E::ONE();
      printf("%d\n", ok ? 1 : 0);
      return 0;
    } else if (argc >= 7) {
      const E b = el(argv[5], argv[6]);
      r = !strcmp(argv[2], "add") ? a + b : !strcmp(argv[2], "sub") ? a - b : a * b;
    } else return 2;
    printf("%llu %llu\n", (unsigned long long)r.coeffs[0].value, (unsigned long long)r.coeffs[1].value);
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "identities")) {
    identities(el("10", "20"), el("20", "10"), el("70", "80"));
    identities(E(B(33)), el("0", "1"), el("100", "100"));
    identities(G::new_({G::Base(123456789), G::Base(RONK_GOLDILOCKS_P - 1)}), G::new_({G::Base(1ull << 63), G::Base(7)}),
               G::new_({G::Base(0), G::Base(0xFFFFFFFFull)}));
  } else if (argc >= 2 && !strcmp(argv[1], "device")) {
    array_forms<E>({el("10", "20"), el("70", "80"), el("0", "1"), el("100", "0")}, {el("20", "10"), el("80", "70"), el("14", "9"), el("0", "0")});
    array_forms<G>({G::new_({G::Base(123456789), G::Base(RONK_GOLDILOCKS_P - 1)}), G::new_({G::Base(1ull << 63), G::Base(7)})},
              {G::new_({G::Base(5), G::Base(0)}), G::new_({G::Base(RONK_GOLDILOCKS_P - 2), G::Base(1ull << 40)})});
  } else return 2;
  if (fails) { printf("FAILED %d\n", fails); return 1; }
  printf("ALL OK\n");
  return 0;
}
