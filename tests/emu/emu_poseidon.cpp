// emu_poseidon.cpp -- the Poseidon / sponge / Merkle bodies of csrc/poseidon_kernels.h compiled for the host and compared with a
// plain `unsigned __int128 % p` restatement of the reference (src/hashes/poseidon/mod.rs:56-149, sponge.rs:69-275,
// src/tree/merkle.rs:31-99) in this file.  Test infrastructure only; never part of the product library.
//
//   emu_poseidon <p> <width> <alpha> <num_p> <num_f> <rate> <seed>     last line "OK ..." on success
//
// RONK_EMU_INPUT=<file> is the file mode (tests/gl_directed.py poseidon_blob: little-endian words n_states, n_words, rc, mds,
// the states, the words): the constants and the permutation states come from the file, the sponge and leaf inputs are drawn from
// its words in turn, and every output is still compared with the restatement.  RONK_EMU_SMALL=B (emu_ref.h) is the directed
// mode of the emulator's own generator: round constants, states and absorbed words in [-B, B], a matrix of two +-1 per row.
// -DRONK_GL64_CENSUS: emu_census.h.
//
// Built with -DEMU_POSEIDON_LIB -shared, the restatement alone is a small library (posref_*) that tests/test_gpu_poseidon.py
// uses for trees too large for the Python restatement (which pins it on small ones).  -fopenmp spreads the tree over threads.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "emu_ref.h"
typedef uint32_t u32;

// ---------------------------------------------------------------------------------------------------- the restatement
struct RefParams {
  u64 p;
  u32 width, num_p, num_f, rate;
  u64 alpha;
  const u64* rc;    // canonical
  const u64* mds;   // canonical, row-major
};
static void ref_permute(const RefParams& P, u64* st) {
  const u32 w = P.width;
  u64 t[16];
  for (u32 r = 0; r < P.num_f + P.num_p; r++) {
    for (u32 i = 0; i < w; i++) st[i] = r_add(st[i], P.rc[r * w + i], P.p);
    if (r < P.num_f / 2 || r >= P.num_p + P.num_f / 2)
      for (u32 i = 0; i < w; i++) st[i] = r_pow(st[i], P.alpha, P.p);
    else
      st[0] = r_pow(st[0], P.alpha, P.p);
    for (u32 i = 0; i < w; i++) {
      u64 a = 0;
      for (u32 j = 0; j < w; j++) a = r_add(a, r_mul(st[j], P.mds[i * w + j], P.p), P.p);
      t[i] = a;
    }
    for (u32 i = 0; i < w; i++) st[i] = t[i];
  }
}
static void ref_sponge(const RefParams& P, const u64* in, size_t len, size_t stride, u64* out, size_t n_out) {
  u64 st[16] = {0};
  const u32 cap = P.width - P.rate;
  u32 ai = 0;
  for (size_t j = 0; j < len; j++) {
    st[cap + ai] = r_add(st[cap + ai], in[j * stride] % P.p, P.p);
    if (++ai == P.rate) { ref_permute(P, st); ai = 0; }
  }
  if (ai) ref_permute(P, st);
  u32 si = 0;
  for (size_t k = 0; k < n_out; k++) {
    if (si == P.rate) { ref_permute(P, st); si = 0; }
    out[k] = st[cap + si++];
  }
}
static size_t ref_tree_words(size_t n, size_t d) {
  size_t w = 0;
  for (;;) { w += n * d; if (n == 1) break; n = (n + 1) / 2; }
  return w;
}
static void ref_merkle(const RefParams& P, const u64* leaves, size_t n, size_t leaf_len, size_t item_stride, size_t elem_stride, size_t d,
                       u64* tree) {
#pragma omp parallel for schedule(static)
  for (long long i = 0; i < (long long)n; i++) ref_sponge(P, leaves + (size_t)i * item_stride, leaf_len, elem_stride, tree + (size_t)i * d, d);
  u64* lvl = tree;
  size_t cnt = n;
  while (cnt > 1) {
    const size_t cn = (cnt + 1) / 2;
    u64* nxt = lvl + cnt * d;
#pragma omp parallel for schedule(static)
    for (long long t = 0; t < (long long)cn; t++) {
      u64 pair[32];
      const u64* l = lvl + (size_t)(2 * t) * d;
      const u64* r = ((size_t)(2 * t + 1) < cnt) ? l + d : l;
      for (size_t j = 0; j < d; j++) { pair[j] = l[j]; pair[d + j] = r[j]; }
      ref_sponge(P, pair, 2 * d, 1, nxt + (size_t)t * d, d);
    }
    lvl = nxt;
    cnt = cn;
  }
}

extern "C" {
void posref_permute(u64 p, u32 width, u64 alpha, u32 num_p, u32 num_f, const u64* rc, const u64* mds, u64* state) {
  RefParams P{p, width, num_p, num_f, 1, alpha, rc, mds};
  for (u32 i = 0; i < width; i++) state[i] %= p;
  ref_permute(P, state);
}
void posref_sponge(u64 p, u32 width, u64 alpha, u32 num_p, u32 num_f, u32 rate, const u64* rc, const u64* mds, const u64* in, size_t len,
                   u64* out, size_t n_out) {
  RefParams P{p, width, num_p, num_f, rate, alpha, rc, mds};
  ref_sponge(P, in, len, 1, out, n_out);
}
size_t posref_tree_words(size_t n, size_t d) { return ref_tree_words(n, d); }
void posref_merkle(u64 p, u32 width, u64 alpha, u32 num_p, u32 num_f, u32 rate, const u64* rc, const u64* mds, const u64* leaves, size_t n,
                   size_t leaf_len, size_t item_stride, size_t elem_stride, size_t d, u64* tree) {
  RefParams P{p, width, num_p, num_f, rate, alpha, rc, mds};
  ref_merkle(P, leaves, n, leaf_len, item_stride, elem_stride, d, tree);
}
}

#ifndef EMU_POSEIDON_LIB
// ---------------------------------------------------------------------------------------------------- the kernel bodies
#include "../../ronkathon_amd/csrc/poseidon_kernels.h"
#include "emu_census.h"
using namespace ronk;

// file mode: the states of the permutation check, and the words the other inputs are drawn from
static std::vector<u64> g_file_states, g_file_words;
static size_t g_file_next = 0;
static bool file_mode() { return !g_file_words.empty(); }
static u64 file_word() { const u64 v = g_file_words[g_file_next]; g_file_next = (g_file_next + 1) % g_file_words.size(); return v; }
static bool directed() { return file_mode() || emu_small(); }
static u64 directed_word(u64 p) { return file_mode() ? file_word() : small_word(p, emu_small()); }

static bool g_negatives = true;   // off for the all-equal matrix: its hash only sees the SUM of what it absorbs

struct Setup {
  RefParams P;
  std::vector<u64> rc, mds, tab;
  PoseidonConsts nat, sp;
  u32 W;
};
static void make_setup(Setup& S, u64 p, u32 width, u64 alpha, u32 num_p, u32 num_f, u32 rate, const std::vector<u64>& rc,
                       const std::vector<u64>& mds) {
  S.rc = rc; S.mds = mds;
  for (auto& c : S.rc) c %= p;
  for (auto& c : S.mds) c %= p;
  S.P = RefParams{p, width, num_p, num_f, rate, alpha, S.rc.data(), S.mds.data()};
  S.W = poseidon_padded_width(width);
  const u32 rounds = num_p + num_f;
  const size_t nrc = (size_t)rounds * S.W, nm = (size_t)S.W * S.W;
  S.tab.assign(2 * (nrc + nm), 0);
  poseidon_host_tables(p, width, rate, rounds, rc.data(), mds.data(), S.tab.data());   // the raw constants: reduced there
  PoseidonConsts k{};
  k.alpha = alpha; k.rounds = rounds; k.full_lo = num_f / 2; k.full_from = num_p + num_f / 2; k.rate = rate;
  if (p != gl64::P) {
    const mont64::Field mf = mont64::make_field(p);
    k.p = p; k.pinv = mf.pinv; k.r2 = mf.r2;
  }
  S.nat = k; S.nat.rc = S.tab.data(); S.nat.mds = S.tab.data() + nrc;
  S.sp = k; S.sp.rc = S.tab.data() + nrc + nm; S.sp.mds = S.tab.data() + 2 * nrc + nm;
}

template <class F, int W>
static void run_w(const Setup& S, u64 seed) {
  const u64 p = S.P.p;
  const u32 width = S.P.width, rate = S.P.rate;
  // ---- permutation: edge states and random ones, inputs >= p included
  {
    const F f(S.nat);
    census_stage("permute");
    std::vector<std::vector<u64>> states;
    states.push_back(std::vector<u64>(width, 0));
    states.push_back(std::vector<u64>(width, p - 1));
    states.push_back(std::vector<u64>(width, ~(u64)0));   // >= p
    states.push_back(std::vector<u64>(width, p));
    for (int t = 0; t < 24; t++) {
      std::vector<u64> s(width);
      for (auto& v : s) { const u64 c = rnd() % 8; v = c == 0 ? p - 1 : c == 1 ? 0 : c == 2 ? p + rnd() % 5 : rnd(); }
      states.push_back(s);
    }
    if (file_mode()) {
      states.clear();
      for (size_t i = 0; i + width <= g_file_states.size(); i += width) states.emplace_back(g_file_states.begin() + i, g_file_states.begin() + i + width);
    } else if (emu_small()) {
      states.assign(200, std::vector<u64>(width));
      for (auto& s : states)
        for (auto& v : s) v = small_word(p, emu_small());
    }
    for (auto& s : states) {
      std::vector<u64> want(s), got(s);
      for (auto& v : want) v %= p;
      ref_permute(S.P, want.data());
      poseidon_permute_words<F, W>(f, S.nat, width, got.data());
      CHECK(want == got, "permute p=%llu width=%u", (unsigned long long)p, width);
    }
  }
  // ---- sponge, both stride layouts
  {
    const F f(S.sp);
    const size_t lens[] = {0, 1, (size_t)rate - 1, rate, (size_t)rate + 1, 3 * (size_t)rate + 2};
    const size_t nouts[] = {1, rate, (size_t)rate + 3};
    const size_t items = 5, maxlen = 3 * (size_t)rate + 2;
    std::vector<u64> mat(items * maxlen);
    for (auto& v : mat) { const u64 c = rnd() % 8; v = c == 0 ? p - 1 : c == 1 ? 0 : c == 2 ? p + rnd() % 5 : rnd(); }
    if (directed()) for (auto& v : mat) v = directed_word(p);
    census_stage("sponge");
    for (size_t len : lens)
      for (size_t n_out : nouts)
        for (int layout = 0; layout < 2; layout++) {
          const size_t is = layout ? 1 : maxlen, es = layout ? items : 1;   // contiguous items / columns of a [maxlen][items] matrix
          for (size_t i = 0; i < items; i++) {
            std::vector<u64> want(n_out), got(n_out, ~(u64)0);
            ref_sponge(S.P, mat.data() + i * is, len, es, want.data(), n_out);
            const u64* src = mat.data() + i * is;
            poseidon_sponge<F, W>(f, S.sp, len, n_out, [&](u64 j) { return src[j * es]; }, [&](u64 q, u64 v) { got[q] = v; });
            CHECK(want == got, "sponge len=%zu n_out=%zu layout=%d", len, n_out, layout);
          }
        }
  }
  // ---- Merkle: the workgroup climb with the lanes run in turn, open and verify
  {
    const F f(S.sp);
    const u32 d = rate < 3 ? rate : 3;
    const size_t ns[] = {1, 2, 3, 5, 64, 257, 600};
    for (size_t n : ns) {
      const size_t leaf_len = 1 + seed % 5;
      std::vector<u64> leaves(n * leaf_len);
      for (auto& v : leaves) v = rnd();
      if (directed()) for (auto& v : leaves) v = directed_word(p);
      const size_t words = ref_tree_words(n, d);
      CHECK(words == merkle_level_offset(n, d, merkle_levels(n)), "tree words n=%zu", n);
      std::vector<u64> want(words), tree(words, ~(u64)0);
      ref_merkle(S.P, leaves.data(), n, leaf_len, leaf_len, 1, d, want.data());
      // the launches of ronk_merkle_commit_dev: the leaf sponges, one launch per level above 256 nodes, the top in one workgroup
      const u64 top = merkle_levels(n) - 1;
      std::vector<u64> bufa(MERKLE_BLOCK * d), bufb(MERKLE_BLOCK / 2 * d);
      auto lanes = [&](auto&& fn) { for (u32 t = 0; t < MERKLE_BLOCK; t++) fn(t); };
      census_stage("merkle_leaf");
      for (u64 i = 0; i < n; i++) {
        const u64* src = leaves.data() + i * leaf_len;
        u64* g = tree.data() + i * d;
        poseidon_sponge<F, W>(f, S.sp, leaf_len, d, [&](u64 j) { return src[j]; }, [&](u64 q, u64 v) { g[q] = v; });
      }
      u64 lvl = 0, n_lvl = n, off = 0;
      census_stage("merkle_node");
      while (n_lvl > MERKLE_BLOCK) {
        const u64 cn = (n_lvl + 1) / 2;
        for (u64 t = 0; t < cn; t++) merkle_level_node<F, W>(f, S.sp, tree.data() + off, n_lvl, d, tree.data() + off + n_lvl * d, t);
        off += n_lvl * d; n_lvl = cn; lvl++;
      }
      if (lvl < top) {
        const u32 cnt = (u32)n_lvl;
        for (u32 e = 0; e < cnt * d; e++) bufa[e] = tree[off + e];
        merkle_climb<F, W>(f, S.sp, bufa.data(), bufb.data(), 0, cnt, d, (u32)(top - lvl), n_lvl, off + n_lvl * d, tree.data(), lanes);
      }
      CHECK(want == tree, "merkle tree n=%zu", n);
      census_stage("merkle_verify");
      // open + verify every index
      const u64 depth = top;
      std::vector<u64> path(depth * d + 1), h(3 * d);
      const u64* root = want.data() + words - d;
      for (u64 i = 0; i < n + 2; i++) {
        const int bad = merkle_open_one(want.data(), n, d, i, path.data());
        // the reference's rule, restated: walking up, an even index whose right neighbour does not exist
        int want_bad = i >= n;
        { u64 idx = i, c = n; for (u64 l = 0; l < depth && !want_bad; l++) { if ((idx ^ 1) >= c) want_bad = 1; idx >>= 1; c = (c + 1) / 2; } }
        CHECK(bad == want_bad, "open status n=%zu i=%llu", n, (unsigned long long)i);
        if (bad) continue;
        const u64* src = leaves.data() + i * leaf_len;
        auto load = [&](u64 j) { return src[j]; };
        CHECK((merkle_verify_one<F, W>(f, S.sp, leaf_len, load, i, path.data(), n, d, root, h.data()) == 1), "verify n=%zu i=%llu", n,
              (unsigned long long)i);
        if (g_negatives && (i % 7 == 0 || n < 8)) {
          if (depth) {
            path[(i * 3) % (depth * d)] ^= 1;
            CHECK((merkle_verify_one<F, W>(f, S.sp, leaf_len, load, i, path.data(), n, d, root, h.data()) == 0), "flipped word accepted n=%zu i=%llu depth=%llu", n, (unsigned long long)i, (unsigned long long)depth);
            path[(i * 3) % (depth * d)] ^= 1;
            CHECK((merkle_verify_one<F, W>(f, S.sp, leaf_len, load, i ^ 1, path.data(), n, d, root, h.data()) == 0), "wrong index accepted n=%zu i=%llu", n, (unsigned long long)i);
          }
          const u64* other = leaves.data() + ((i + 1) % n) * leaf_len;
          if (n > 1)
            CHECK((merkle_verify_one<F, W>(f, S.sp, leaf_len, [&](u64 j) { return other[j]; }, i, path.data(), n, d, root, h.data()) == 0),
                  "wrong leaf accepted");
        }
      }
    }
  }
}

template <class F>
static void run_f(const Setup& S, u64 seed) {
  switch (S.W) {
    case 4: run_w<F, 4>(S, seed); break;
    case 8: run_w<F, 8>(S, seed); break;
    case 12: run_w<F, 12>(S, seed); break;
    default: run_w<F, 16>(S, seed); break;
  }
}
static void run(const Setup& S, u64 seed) {
  if (S.P.p == gl64::P) run_f<PosGl>(S, seed);
  else run_f<PosMont>(S, seed);
}

int main(int argc, char** argv) {
  if (argc < 8) { fprintf(stderr, "usage: emu_poseidon p width alpha num_p num_f rate seed\n"); return 2; }
  const u64 p = strtoull(argv[1], nullptr, 0);
  const u32 width = atoi(argv[2]);
  const u64 alpha = strtoull(argv[3], nullptr, 0);
  const u32 num_p = atoi(argv[4]), num_f = atoi(argv[5]), rate = atoi(argv[6]);
  const u64 seed = strtoull(argv[7], nullptr, 0);
  if (width < 2 || width > 16 || rate < 1 || rate >= width || !(p & 1)) { fprintf(stderr, "bad parameters\n"); return 2; }
  g_rng = seed;
  g_negatives = p > ((u64)1 << 32);   // digests of a small field collide by chance
  const u32 rounds = num_p + num_f;
  Setup S;
  // random constants, raw 64-bit words (reduced on "upload")
  std::vector<u64> rc((size_t)rounds * width), mds((size_t)width * width);
  for (auto& c : rc) c = rnd();
  for (auto& c : mds) c = rnd();
  if (const char* path = getenv("RONK_EMU_INPUT")) {
    FILE* fp = fopen(path, "rb");
    u64 head[2] = {0, 0};
    bool ok = fp && fread(head, 8, 2, fp) == 2 && head[0] < (1u << 20) && head[1] >= 1 && head[1] < (1u << 24);
    if (ok) {
      g_file_states.resize(head[0] * width);
      g_file_words.resize(head[1]);
      ok = fread(rc.data(), 8, rc.size(), fp) == rc.size() && fread(mds.data(), 8, mds.size(), fp) == mds.size() &&
           fread(g_file_states.data(), 8, g_file_states.size(), fp) == g_file_states.size() &&
           fread(g_file_words.data(), 8, g_file_words.size(), fp) == g_file_words.size() && fgetc(fp) == EOF;
    }
    if (fp) fclose(fp);
    if (!ok) { fprintf(stderr, "cannot read %s for width %u and %u rounds\n", path, width, rounds); return 2; }
  } else if (emu_small()) {
    for (auto& c : rc) c = small_word(p, emu_small());
    for (u32 i = 0; i < width; i++) {
      const u32 a = (u32)(rnd() % width), b = (a + 1 + (u32)(rnd() % (width - 1))) % width;
      for (u32 j = 0; j < width; j++) mds[(size_t)i * width + j] = j == a || j == b ? (rnd() & 1 ? 1 : p - 1) : 0;
    }
  }
  if (directed()) g_negatives = false;   // small constants are no hash: equal digests of different leaves are common
  make_setup(S, p, width, alpha, num_p, num_f, rate, rc, mds);
  run(S, seed);
  census_stage(nullptr);
  // the accumulator's worst case: every state word and every matrix entry p - 1, round constants zero; a row is then
  // width * (p - 1)^2 before its one reduction (not in the directed modes: those runs are about their own inputs)
  if (!directed()) {
    std::vector<u64> rc0((size_t)rounds * width, 0), m1((size_t)width * width, p - 1);
    Setup T;
    make_setup(T, p, width, alpha, num_p, num_f, rate, rc0, m1);
    g_negatives = false;
    run(T, seed + 1);
    if (p == gl64::P) {   // the three-word accumulator beyond the field: 16 products of 2^64 - 1 squared
      PosGl f(T.nat);
      PosGl::Acc a;
      f.acc_zero(a);
      for (int j = 0; j < 16; j++) f.acc_mad(a, ~(u64)0, ~(u64)0);
      const u64 m = (u64)(((u128)~(u64)0) % p);
      u64 want = 0;
      for (int j = 0; j < 16; j++) want = r_add(want, r_mul(m, m, p), p);
      CHECK(a.w[4] == 15, "top word %u", a.w[4]);
      CHECK(f.acc_reduce(a) == want, "160-bit reduction");
    }
  }
  if (g_fail) { printf("FAILED %d checks\n", g_fail); return 1; }
  printf("OK p=%llu width=%u W=%u alpha=%llu num_p=%u num_f=%u rate=%u lazy=%d\n", (unsigned long long)p, width, S.W,
         (unsigned long long)alpha, num_p, num_f, rate, RONK_POSEIDON_LAZY);
  return 0;
}
#endif
