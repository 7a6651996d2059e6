/*
 * ronk_ntt.h -- C ABI of libronk_ntt.so, the MI355X-native (gfx950, hand-written HIP)
 * finite-field / NTT / polynomial engine that sits behind ronkathon's
 * `Polynomial<B, F, D>` + `Field` / `FiniteField` trait surface.
 *
 * ronkathon (Rust) has no FFI of its own: the seam is its generic trait surface.  Each
 * entry point below states which reference item it replaces (paths relative to the
 * ronkathon repository).  INTEGRATION.md shows the Rust `extern "C"` block and the trait
 * impls a maintainer adds on the reference side.
 *
 * Conventions
 *  - every field element is a canonical residue in [0, p) stored as uint64_t -- exactly what
 *    `PrimeField<P>{ value: usize }` holds (src/algebra/field/prime/mod.rs:39-42); Montgomery
 *    form never crosses this boundary;
 *  - transforms are natural order in, natural order out, with omega = g^((p-1)/n)
 *    (src/algebra/field/mod.rs:70-75, src/polynomial/mod.rs:240-323);
 *  - buffers are caller-owned, no ownership transfer, no callbacks; functions without a
 *    `_dev` suffix take HOST pointers (and stage through HBM), `_dev` functions take DEVICE
 *    pointers and enqueue on `stream` (a hipStream_t, NULL = the null stream) without
 *    synchronising;
 *  - the reference reports errors by panicking; here every function returns 0 or a negative
 *    RONK_ERR_* code, and the Rust shim turns a non-zero code back into the same panic;
 *  - re-entrant: plans are immutable after creation.  A plan owns ONE scratch buffer: calls on one stream are
 *    ordered by the stream, and a `_dev` call that arrives on another stream than the plan's previous call is made
 *    to wait (event) for that call, so concurrent streams never corrupt each other -- they serialise on the plan.
 *    For transforms that should overlap, hand the library a batch or several arrays per call (ronk_plan_opts::in_flight,
 *    ronk_ntt_forward_many_dev) or use one plan per stream.  (While a stream is being captured into a
 *    hipGraph the guard is skipped: a captured graph must own its plan.)
 *  - the 64-bit hot path is the Goldilocks field p = 2^64 - 2^32 + 1 with generator g = 7;
 *    any other odd prime p < 2^64 (e.g. the reference's F_101, F_17, F_127) runs through a
 *    generic Montgomery path so that the reference's own test vectors pass on the GPU.
 *  - there is NO CPU fallback: without a HIP device every compute entry point returns
 *    RONK_ERR_NO_DEVICE.
 */
#ifndef RONK_NTT_H
#define RONK_NTT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RONK_GOLDILOCKS_P 0xFFFFFFFF00000001ull
#define RONK_GOLDILOCKS_G 7ull

/* error codes; messages via ronk_strerror() repeat the reference's panic texts */
#define RONK_OK 0
#define RONK_ERR_NO_ROOT (-1)       /* assert!(p_minus_one % n == 0, "n must divide p^q - 1"), field/mod.rs:72; polynomial/mod.rs:361 */
#define RONK_ERR_ZERO_INVERSE (-2)  /* inverse().unwrap() on ZERO, prime/arithmetic.rs:54, polynomial/mod.rs:196 */
#define RONK_ERR_NOT_POW2 (-3)      /* fft()/ifft() bound `D.is_power_of_two()`, polynomial/mod.rs:274, :431 */
#define RONK_ERR_NOT_PRIME (-4)     /* is_prime() panic "input is not a prime number", prime/mod.rs:92-100 */
#define RONK_ERR_NO_GENERATOR (-5)  /* find_primitive_element panic, prime/mod.rs:122 */
#define RONK_ERR_INDEX (-6)         /* slice index / unwrap-on-None panics (zero divisor, ragged division) */
#define RONK_ERR_INVALID (-7)       /* NULL pointer, zero length, bad plan */
#define RONK_ERR_HIP (-8)           /* a HIP runtime call failed; ronk_last_hip_error() has the text */
#define RONK_ERR_UNSUPPORTED (-9)   /* size outside what the kernels cover (stated per function) */
#define RONK_ERR_NO_DEVICE (-10)    /* no HIP device: the library never computes on the CPU */
#define RONK_ERR_NOT_ON_CURVE (-11) /* assert!(point.is_on_curve(), "Point is not on curve"), src/curve/mod.rs:79 */
#define RONK_ERR_NOT_RESIDUE (-13)  /* assert!(self.euler_criterion(), "Element is not a quadratic residue"), prime/mod.rs:179 */
#define RONK_ERR_RCCL (-12)         /* librccl.so could not be loaded or an RCCL call failed; ronk_last_hip_error() has the text */
#define RONK_ERR_NOT_CODEWORD (-14) /* the surviving values lie on no polynomial of degree < k (an error, not only erasures) */

const char* ronk_strerror(int code);
const char* ronk_last_hip_error(void);
int ronk_device_count(int* count);

/* ---- field: src/algebra/field/mod.rs:17-76, src/algebra/field/prime/{mod,arithmetic}.rs ---- */

/* FiniteField::PRIMITIVE_ELEMENT (prime/mod.rs:87-90, :110-123): the reference's heuristic for
 * small primes, the explicit generator 7 for Goldilocks (the heuristic returns a non-generator
 * there).  Host-side integer logic, no device work. */
int ronk_primitive_element(uint64_t p, uint64_t* g);
/* FiniteField::primitive_root_of_unity(n) (field/mod.rs:70-75) */
int ronk_root_of_unity(uint64_t p, uint64_t g, uint64_t n, uint64_t* out);
/* PrimeField::new's primality assertion (prime/mod.rs:48-51, :92-100): 0 or RONK_ERR_NOT_PRIME */
int ronk_check_prime(uint64_t p);

/* Element-wise Field operators over arrays (Add/Sub/Mul/Neg, prime/arithmetic.rs:3-65;
 * Field::inverse prime/mod.rs:62-72 -> RONK_ERR_ZERO_INVERSE if any a[i] == 0;
 * Field::pow prime/mod.rs:74-84).  These are also what Polynomial Add/Sub/Neg reduce to. */
int ronk_vec_add(uint64_t p, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int ronk_vec_sub(uint64_t p, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int ronk_vec_mul(uint64_t p, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int ronk_vec_neg(uint64_t p, const uint64_t* a, uint64_t* out, size_t n);
int ronk_vec_inv(uint64_t p, const uint64_t* a, uint64_t* out, size_t n);
int ronk_vec_pow(uint64_t p, const uint64_t* a, uint64_t e, uint64_t* out, size_t n);
/* FieldExt (src/algebra/field/mod.rs:79-84) over arrays.
 * euler_criterion (prime/mod.rs:142-172): out[i] = 1 when a[i]^((p-1)/2) == 1, else 0 (ZERO is no residue by this test).
 * sqrt (prime/mod.rs:174-226, Tonelli-Shanks): (r0[i], r1[i]) = the two roots of a[i], SMALLER FIRST as the reference returns
 * them; ZERO -> (0, 0); a non-residue is the reference's assert -> RONK_ERR_NOT_RESIDUE (the _dev form raises *d_status, which
 * may be NULL, and stores (0, 0) there).  p must be an odd prime (over F_2 the reference's search for a non-residue does not
 * terminate: RONK_ERR_UNSUPPORTED).  d_r0 may alias d_a. */
int ronk_vec_euler(uint64_t p, const uint64_t* a, uint64_t* out, size_t n);
int ronk_vec_sqrt(uint64_t p, const uint64_t* a, uint64_t* r0, uint64_t* r1, size_t n);
int ronk_vec_euler_dev(uint64_t p, const uint64_t* d_a, uint64_t* d_out, size_t n, void* stream);
int ronk_vec_sqrt_dev(uint64_t p, const uint64_t* d_a, uint64_t* d_r0, uint64_t* d_r1, size_t n, int* d_status, void* stream);
int ronk_vec_add_dev(uint64_t p, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
int ronk_vec_sub_dev(uint64_t p, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
int ronk_vec_mul_dev(uint64_t p, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);

/* ---- transforms: src/polynomial/mod.rs ---- */

typedef struct ronk_plan ronk_plan;

/* A plan fixes (p, g, n = 2^log2n, batch) on one device: twiddle tables in HBM, the pass
 * decomposition, and a scratch buffer of batch*n elements.  `batch` polynomials are stored
 * back to back ([batch][n], row-major).  device < 0 = current device.
 * Errors: RONK_ERR_NO_ROOT if 2^log2n does not divide p-1; RONK_ERR_NOT_PRIME. */
int ronk_plan_create(ronk_plan** out, uint64_t p, uint64_t g, uint32_t log2n, uint64_t batch, int device);
/* Same with planner tuning (-1 = default): tile_log2_columns = log2 of the widest tile (columns per workgroup;
 * default 4 -> one 128 KiB-LDS workgroup per CU at 2^11 rows, best for one transform at a time; 2 -> two
 * workgroups per CU, better when several transforms are in flight on different streams);
 * twiddle_matrix_log2_max = largest full inter-pass twiddle matrix (default: 18 = L2-resident only, and the whole matrix
 * at 2^21 / 2^22 points, where it pays for its extra read). */
int ronk_plan_create_tuned(ronk_plan** out, uint64_t p, uint64_t g, uint32_t log2n, uint64_t batch, int device,
                           int tile_log2_columns, int twiddle_matrix_log2_max);
/* Same through an options block (start from RONK_PLAN_OPTS_DEFAULT, then set what you need; -1 = default everywhere).
 * in_flight: 1 = every call runs on the caller's stream only; 2 = the library keeps TWO transforms in flight behind
 * this one handle: a batched call (batch >= 2, multi-pass sizes) runs the second half of the batch on an internal side
 * stream -- fork / join by events on the caller's stream, so stream order as the caller sees it is unchanged -- and
 * ronk_ntt_forward_many_dev / _inverse_many_dev spread K independent arrays over the two lanes.  -1 = automatic = 1
 * (measured: the lanes pay for independent arrays, not for the halves of one batched launch).
 * The reference has no counterpart (its fft() is a
 * single-threaded recursion, src/polynomial/mod.rs:295-323); this is how a caller with many independent polynomials
 * (kzg / Reed-Solomon batches) gets the concurrent rate without managing streams and plans itself. */
typedef struct ronk_plan_opts {
  int tile_log2_columns;        /* as in ronk_plan_create_tuned */
  int twiddle_matrix_log2_max;  /* as in ronk_plan_create_tuned */
  int in_flight;                /* -1 auto, 1, 2 */
  int split_log2_rows;          /* two-pass plans (2^13 .. 2^24): log2 of the first pass's rows, 0 = the planner's (balanced)
                                   choice; values that leave a pass outside 2^4 .. 2^12 rows are ignored */
  int three_pass_from_log2;     /* 0 = the planner's choice (23; 24 for ONE transform of 2^23); 13 .. 25: the smallest log2n that is
                                   split in THREE passes (the fused multiply asks for two-pass plans of a batch of two at 2^23).
                                   (Round 6: a named field in the place of reserved[0], which carried this knob unnamed -- same
                                   layout, same size.) */
  int reserved[3];              /* zero */
} ronk_plan_opts;
#define RONK_PLAN_OPTS_DEFAULT { -1, -1, -1, 0, 0, { 0, 0, 0 } }
int ronk_plan_create_opts(ronk_plan** out, uint64_t p, uint64_t g, uint32_t log2n, uint64_t batch, int device,
                          const ronk_plan_opts* opts);
/* 1 or 2: the lanes the plan actually uses (see ronk_plan_opts::in_flight) */
int ronk_plan_in_flight(const ronk_plan* plan);
int ronk_plan_destroy(ronk_plan* plan);
/* Which kernel family the plan runs on (2^4 <= n <= 2^30 for the tiled ones):
 *   1 = the tiled Goldilocks path (p = 2^64 - 2^32 + 1 with the explicit generator 7): shift twiddles inside a register round;
 *   2 = the SAME tile kernels over Montgomery arithmetic (R = 2^64): any other odd prime p < 2^64 -- PrimeField<P> is generic
 *       over P, src/algebra/field/prime/mod.rs:39-52 -- and Goldilocks with another generator, whenever g is a quadratic
 *       non-residue (then omega_n = g^((p-1)/n) has order exactly n for every power of two n | p - 1).  Coefficients stay
 *       canonical; twiddle tables hold w * 2^64 mod p.  About twice the arithmetic of path 1 per coefficient;
 *   0 = the radix-2 path (n < 16, n > 2^30, or a g that generates no full 2-power subgroup -- the reference's recursion
 *       src/polynomial/mod.rs:295-323 is then not the DFT and is restated stage by stage): one HBM pass per stage, n <= 2^32. */
int ronk_plan_path(const ronk_plan* plan);

/* Polynomial::<Monomial,F,D>::fft() (polynomial/mod.rs:273-323; same values as dft() :240-258).
 * `nodes`, if non-NULL, receives Lagrange::nodes = [omega^i] (mod.rs:358-365), n elements. */
int ronk_ntt_forward(ronk_plan* plan, const uint64_t* in, uint64_t* out, uint64_t* nodes);
/* Polynomial::<Lagrange<F>,F,D>::ifft() (polynomial/mod.rs:430-484), includes the D^-1 scale */
int ronk_ntt_inverse(ronk_plan* plan, const uint64_t* in, uint64_t* out);
/* device-resident forms; in == out is allowed; asynchronous on `stream` */
int ronk_ntt_forward_dev(ronk_plan* plan, const uint64_t* d_in, uint64_t* d_out, void* stream);
int ronk_ntt_inverse_dev(ronk_plan* plan, const uint64_t* d_in, uint64_t* d_out, void* stream);
/* `count` independent arrays of [batch][n] elements each in one call (Polynomial::fft / ifft of `count` unrelated
 * polynomials, src/polynomial/mod.rs:273-292, :430-453): d_in / d_out are HOST arrays of `count` DEVICE pointers.
 * With in_flight = 2 the arrays alternate between the caller's stream and the plan's side stream (second scratch);
 * asynchronous on `stream`, which sees the results of all of them in stream order. */
int ronk_ntt_forward_many_dev(ronk_plan* plan, const uint64_t* const* d_in, uint64_t* const* d_out, size_t count,
                              void* stream);
int ronk_ntt_inverse_many_dev(ronk_plan* plan, const uint64_t* const* d_in, uint64_t* const* d_out, size_t count,
                              void* stream);
/* Lagrange::<F>::new's node table [omega^i], i < n (polynomial/mod.rs:358-365) */
int ronk_lagrange_nodes(uint64_t p, uint64_t g, uint64_t* nodes, size_t n);

/* One-shot host-pointer forms of the two calls above for a single polynomial, the direct analogues of
 * `poly.fft()` / `lagrange.ifft()`: plans (twiddles, scratch) are kept in an internal LRU cache.
 * n not a power of two -> RONK_ERR_NOT_POW2; n does not divide p-1 -> RONK_ERR_NO_ROOT. */
int ronk_fft(uint64_t p, uint64_t g, const uint64_t* in, uint64_t* out, uint64_t* nodes, size_t n);
int ronk_ifft(uint64_t p, uint64_t g, const uint64_t* in, uint64_t* out, size_t n);

/* Polynomial::dft() for ANY n dividing p-1 (polynomial/mod.rs:240-258), e.g. n = 3, 5, 7, 25.
 * Direct O(n^2) kernel; power-of-two n >= 16 over Goldilocks is routed to the NTT. n <= 2^16. */
int ronk_dft(uint64_t p, uint64_t g, const uint64_t* in, uint64_t* out, size_t n);

/* plan introspection for benchmarks: number of kernel launches per transform, and the
 * average device time of each launch over `iters` forward (inverse != 0: inverse) transforms
 * measured with hipEvents on `stream`.  ms must hold ronk_plan_num_passes() floats. */
int ronk_plan_num_passes(const ronk_plan* plan);
int ronk_plan_time_passes(ronk_plan* plan, const uint64_t* d_in, uint64_t* d_out, int inverse, int iters,
                          float* ms, void* stream);

/* ---- polynomial arithmetic: src/polynomial/arithmetic.rs ---- */

/* impl Mul (arithmetic.rs:97-119): out has d + d2 - 1 coefficients.  Goldilocks: NTT -> pointwise
 * -> inverse NTT on the padded size; other primes: schoolbook kernel.  d, d2 >= 1. */
int ronk_poly_mul(uint64_t p, uint64_t g, const uint64_t* a, size_t d, const uint64_t* b, size_t d2, uint64_t* out);
int ronk_poly_mul_dev(uint64_t p, uint64_t g, const uint64_t* d_a, size_t d, const uint64_t* d_b, size_t d2,
                      uint64_t* d_out, void* stream);
/* impl Add / Sub (arithmetic.rs:16-68): rhs zero-extended or truncated to d = len(lhs) */
int ronk_poly_add(uint64_t p, const uint64_t* a, size_t d, const uint64_t* b, size_t d2, uint64_t* out);
int ronk_poly_sub(uint64_t p, const uint64_t* a, size_t d, const uint64_t* b, size_t d2, uint64_t* out);

/* ---- callers either side of the path ---- */

/* Polynomial::<Monomial>::evaluate (polynomial/mod.rs:133-139): sum c_i x^i */
int ronk_poly_eval(uint64_t p, const uint64_t* c, size_t d, uint64_t x, uint64_t* out);
/* same, coefficients resident in HBM, result (ONE element) written to device memory, asynchronous on `stream`
 * (a hipStream_t).  One 8 B/coefficient read of the array (chunked Horner, csrc/scan_kernels.h). */
int ronk_poly_eval_dev(uint64_t p, const uint64_t* d_c, size_t d, uint64_t x, uint64_t* d_out, void* stream);
/* Polynomial::<Lagrange<F>>::evaluate (polynomial/mod.rs:382-415): barycentric evaluation at x from the
 * values c[j] at nodes[j].  As in the reference, x equal to a node yields ZERO (its fold multiplies by
 * l(x) = 0); coincident nodes -> RONK_ERR_ZERO_INVERSE.  n <= 2^16 (O(n^2) weights, like the reference). 
 * More than 2^16 nodes: only node tables of the form Lagrange::new builds (nodes[i] = omega^i, omega of order n; any n | p-1)
 * -- then prod_{m != j}(x_j - x_m) = n / x_j and prod_i (x - x_i) = x^n - 1 give the same value in O(n); other tables of
 * that size are RONK_ERR_UNSUPPORTED (the _dev form sets bit 2 of *d_status, which it then requires). */
int ronk_lagrange_eval(uint64_t p, const uint64_t* c, const uint64_t* nodes, size_t n, uint64_t x, uint64_t* out);
/* quotient_and_remainder (polynomial/mod.rs:170-225) behind impl Div / Rem (arithmetic.rs:121-146);
 * quot and rem both have d coefficients.  Used by kzg::open (src/kzg/setup.rs:63-78). */
int ronk_poly_divrem(uint64_t p, const uint64_t* a, size_t d, const uint64_t* b, size_t d2, uint64_t* quot,
                     uint64_t* rem);
/* kzg::open's polynomial step on device (src/kzg/setup.rs:63-78: `poly.div([-z, 1])`): division by the linear
 * divisor b0 + b1*x, b1 != 0, as an affine suffix scan.  d_quot receives d coefficients (the top one ZERO, like the
 * reference's D-long quotient); d_rem (may be NULL) receives ONE element, the remainder's constant coefficient (its
 * other coefficients are ZERO).  d_quot may be d_c itself (the quotient written over the dividend); any other overlap
 * of the two is not allowed.  Up to 2^23 coefficients, out of place, with a 16-byte aligned dividend and b0 != 0, the call is ONE
 * launch that moves the algorithmic 16 bytes per coefficient; otherwise two launches (24 bytes).  Asynchronous on
 * `stream`.  NOT for hipGraph capture (nor is ronk_poly_eval_dev): the
 * workspace comes from an event-guarded pool whose slot would be baked into the graph while later calls reuse it; capture
 * the plan entry points (ronk_ntt_forward_dev / inverse_dev with a plan the graph owns) instead. */
int ronk_poly_div_linear_dev(uint64_t p, const uint64_t* d_c, size_t d, uint64_t b0, uint64_t b1, uint64_t* d_quot,
                             uint64_t* d_rem, void* stream);
/* Reed-Solomon Message::encode::<N> (src/codes/reed_solomon.rs:42-52): xs[i] = omega_N^i,
 * ys[i] = poly(omega_N^i) -- a size-N DFT of the zero-padded K-coefficient message. */
int ronk_rs_encode(uint64_t p, uint64_t g, const uint64_t* msg, size_t k, size_t n, uint64_t* xs, uint64_t* ys);
/* Reed-Solomon Message::decode (src/codes/reed_solomon.rs:54-106): Lagrange interpolation through the first k
 * coordinates (xs[j], ys[j]) of a (possibly erased) codeword -> the k message coefficients.  Coincident nodes are
 * the reference's `numerator / denominator` panic -> RONK_ERR_ZERO_INVERSE.  k <= 2^14 (O(k^2) work) for arbitrary nodes; for
 * the node sequences Message::encode produces (xs[j] = q^j, q of any order > k; Goldilocks) an O(k log k) form -- two
 * convolutions on the NTT path, the same interpolating polynomial -- is chosen on the device from k = 1024 on and covers
 * k <= 2^21; other node sets of that size are RONK_ERR_UNSUPPORTED (the _dev form: bit 2 of *d_status, then required). */
int ronk_rs_decode(uint64_t p, const uint64_t* xs, const uint64_t* ys, size_t k, uint64_t* out);
/* Batched Message::encode::<N> on device (src/codes/reed_solomon.rs:42-52), the production shape of a
 * Reed-Solomon / low-degree extension (1024 x 2^16): d_msgs holds plan.batch compact messages of k coefficients,
 * d_ys receives plan.batch x N y-coordinates (x_i = omega_N^i: ronk_lagrange_nodes).  The zero padding of
 * `Polynomial::from(message)` is implicit (no padded copy) for Goldilocks plans with N >= 2^13. */
int ronk_rs_encode_batch_dev(ronk_plan* plan, const uint64_t* d_msgs, size_t k, uint64_t* d_ys, void* stream);
/* prod_i (x - roots[i]): m + 1 coefficients, ascending, the top one ONE (monic); m = 0 gives [1].  Any values (reduced mod p):
 * repeats and zeros allowed.  A product tree on the device (csrc/roots_kernels.h): leaves of RONK_ROOTS_LEAF factors built
 * in one workgroup each, then one batched NTT product per level.  Any odd prime while m <= RONK_ROOTS_LEAF; beyond, every
 * prime with 2^ceil(log2 m) | p - 1 (the tree's top product; m is padded with the root ZERO to RONK_ROOTS_LEAF * 2^t);
 * otherwise RONK_ERR_UNSUPPORTED.  Workspace 6 x (m padded) words from the event-guarded pool; the level plans are cached by
 * the library.  Asynchronous on `stream`; not for hipGraph capture (RONK_ERR_UNSUPPORTED while capturing).  Calls of this and
 * ronk_rs_recover_batch_dev serialise on one library lock while they enqueue. */
#define RONK_ROOTS_LEAF 64
int ronk_poly_from_roots(uint64_t p, const uint64_t* roots, size_t m, uint64_t* out);
int ronk_poly_from_roots_dev(uint64_t p, const uint64_t* d_roots, size_t m, uint64_t* d_out, void* stream);
/* One polynomial at many arbitrary points (Polynomial::evaluate in a loop: Shamir's split, src/shamir/mod.rs:33-60):
 * out[i] = sum_j c[j] xs[i]^j as canonical residues, bit-identical to m calls of ronk_poly_eval.  Any points (reduced mod p;
 * repeats and ZERO allowed), any d >= 1 and m >= 1; NULL pointers or zero sizes: RONK_ERR_INVALID.
 * Tree form, O(m log^2 m + d log d): the product tree of ronk_poly_from_roots with every level retained, the inverse series of
 * its reversed root by the Newton ladder of the fast division (precision max(d, Mp): a longer f needs no division), then the
 * transposed walk down (csrc/multipoint_kernels.h) -- per level one batched forward transform of the windows and two inverses
 * with the sibling's retained transform multiplied on load.  Fields: what ronk_poly_from_roots needs for m points AND the
 * 2-adicity of the root's products, 2^(ceil(log2 max(d, Mp)) + 1) | p - 1 (Goldilocks always); m <= 2^24.
 * Direct form, any odd prime: one batched Horner kernel, O(m d), the coefficients staged in LDS and shared by a workgroup's
 * points; refused (RONK_ERR_UNSUPPORTED) beyond m d = 2^34.  The library picks the form at a measured crossover (DESIGN.md
 * section 11); the environment variable RONK_MULTIPOINT_FORM = direct | tree forces one (A/B runs; a form that does not serve
 * the call is then RONK_ERR_UNSUPPORTED).
 * Workspace of the tree form, in words, from the event-guarded pool: (2 levels + 9) Mp + 10 Lp + 8, Mp = m padded to
 * RONK_ROOTS_LEAF * 2^levels, Lp = the power of two >= max(d, Mp) -- (2 levels + 19) Mp + 8 for d <= Mp.
 * Asynchronous on `stream`; not for hipGraph capture (RONK_ERR_UNSUPPORTED while capturing).  Tree-form calls serialise on the
 * lock of ronk_poly_from_roots while they enqueue. */
int ronk_poly_eval_many_dev(uint64_t p, const uint64_t* d_c, size_t d, const uint64_t* d_xs, size_t m, uint64_t* d_out,
                            void* stream);
int ronk_poly_eval_many(uint64_t p, const uint64_t* c, size_t d, const uint64_t* xs, size_t m, uint64_t* out);
/* The m coefficients of the unique polynomial of degree < m through (xs[i], ys[i]) -- Lagrange interpolation through arbitrary
 * coordinates (Message::decode, src/codes/reed_solomon.rs:55-107; Shamir's combine): the polynomial ronk_rs_decode returns,
 * without its 2^14 limit.  Coincident nodes are the reference's `numerator / denominator` panic: the _dev form writes
 * RONK_ERR_ZERO_INVERSE to *d_status (required; 0 otherwise, written by the call), the host form returns it.
 * Tree form, O(m log^2 m): Z = prod (x - x_i) by the retained tree, Z'(x_i) by the walk of ronk_poly_eval_many on the same
 * tree, w_i = y_i / Z'(x_i) by chunked batch inversion, then one more walk up, N_S = N_L M_R + N_R M_L on the retained
 * transforms.  Fields as for the tree form above with d = m; m <= 2^24; workspace (2 levels + 21) Mp + 8 words.
 * Direct form: the O(m^2) kernels of ronk_rs_decode_dev, any odd prime, m <= 2^14; beyond that without the 2-adicity:
 * RONK_ERR_UNSUPPORTED.  Form choice, stream, capture and locking as above. */
int ronk_poly_interpolate_dev(uint64_t p, const uint64_t* d_xs, const uint64_t* d_ys, size_t m, uint64_t* d_out, int* d_status,
                              void* stream);
int ronk_poly_interpolate(uint64_t p, const uint64_t* xs, const uint64_t* ys, size_t m, uint64_t* out);
/* Reed-Solomon erasure decoding, the inverse of ronk_rs_encode_batch_dev (src/codes/reed_solomon.rs:42-106) on the same plan
 * (p, g, N = plan n >= 16, B = plan batch).  d_ys: B x N codeword values at x_i = omega_N^i.  d_erased: n_erased DISTINCT
 * positions (< N), shared by all B rows; their values in d_ys are ignored.  k == 0: RONK_ERR_INVALID; k > N or
 * n_erased > N - k: RONK_ERR_INDEX.  d_msgs: B x k recovered coefficients.  d_full (may be NULL, may be d_ys): the repaired
 * B x N codeword.  d_status (required, B ints, written by the call): 0, or RONK_ERR_NOT_CODEWORD for a row whose survivors do
 * not lie on one polynomial of degree < k (its d_msgs / d_full rows are then meaningless); RONK_ERR_ZERO_INVERSE (repeated
 * position -- the reference's coincident-node panic) or RONK_ERR_INDEX (position >= N) in EVERY entry for a malformed list.
 * O(N log N) per row: Z_E = prod_{i in E} (x - omega^i) by the product tree (fields as for ronk_poly_from_roots), then three
 * size-N transforms on the plan (four with d_full) and element-wise passes; the erased-set work is shared by the batch.
 * Needs a coset s * <omega_N> (s = g unless g^N = 1): N = p - 1 is RONK_ERR_UNSUPPORTED.  Peak workspace (words):
 * 2N + max(B N, 6 Mp) + N / 64 + 8, Mp = n_erased padded to RONK_ROOTS_LEAF * 2^t.  Asynchronous; not for capture. */
int ronk_rs_recover_batch_dev(ronk_plan* plan, size_t k, const uint64_t* d_erased, size_t n_erased, const uint64_t* d_ys,
                              uint64_t* d_msgs, uint64_t* d_full, int* d_status, void* stream);
/* one codeword, host pointers (a plan of batch 1 per call); returns RONK_ERR_NOT_CODEWORD for an inconsistent codeword, and
 * the list errors as above */
int ronk_rs_recover(uint64_t p, uint64_t g, size_t n, size_t k, const uint64_t* erased, size_t n_erased, const uint64_t* ys,
                    uint64_t* msg, uint64_t* full);
/* Low-degree extension: a batch of polynomials given by their values on {omega_K^i} (plan_k: n = K) -> their values on
 * coset_shift * {omega_N^i} (plan_n: n = N >= K, same batch and modulus).  = Message::encode::<N> of lagrange_poly.ifft()
 * (src/polynomial/mod.rs:430-453, src/codes/reed_solomon.rs:42-52), the coefficients multiplied by coset_shift^i first when
 * coset_shift != 1 (any field; 0 is RONK_ERR_UNSUPPORTED).  d_coeffs: batch x K scratch that receives the coefficients; d_out: batch x N. */
int ronk_lde_batch_dev(ronk_plan* plan_k, ronk_plan* plan_n, const uint64_t* d_evals, uint64_t* d_coeffs, uint64_t* d_out,
                       uint64_t coset_shift, void* stream);

/* kzg::commit (src/kzg/setup.rs:45-60): sum_i points[i] * scalars[i] with the reference's AffinePoint Add / Mul<ScalarField>
 * (src/curve/mod.rs:152-211) on y^2 = x^3 + a x + b over the quadratic extension F_p[u]/(u^2 - nr) of a small prime
 * field (p < 2^32; PlutoExtendedCurve: p = 101, nr = 99 (X^2 + 2), a = 0, b = 3 -- src/curve/pluto_curve.rs:39-51,
 * src/algebra/field/extension/gf_101_2.rs:12-18).  A point is 5 words: x0 x1 y0 y1 inf (inf != 0: Infinity).
 * n_points < n is the reference's assert (RONK_ERR_INDEX); an off-curve point is AffinePoint::new's panic
 * (RONK_ERR_NOT_ON_CURVE).  kzg::open = ronk_poly_divrem by [-z, 1] over the scalar field, then this. */
typedef struct ronk_curve { uint64_t p, nr, a, b; } ronk_curve;
int ronk_curve_msm(const ronk_curve* curve, const uint64_t* points, size_t n_points, const uint64_t* scalars, size_t n,
                   uint64_t out[5]);

/* kzg::commit on a production-size curve: sum_i scalars[i] * points[i] over BN254 (alt_bn128) G1,
 * y^2 = x^3 + 3 over F_p, p = 21888242871839275222246405745257275088696311157297823662689037894645226208583, by the bucket
 * method on the GPU (csrc/msm_kernels.h).  The reference's commit is the same sum as a fold of AffinePoint Mul / Add over
 * its 17-element toy group (src/kzg/setup.rs:48-60, src/curve/mod.rs:157-211); its field traits are usize-wide
 * (src/algebra/mod.rs:8-13), so a 254-bit curve is a new type on the Rust side.
 * points: n x 8 words -- x then y, each 4 x 64-bit little-endian limbs, standard (non-Montgomery) form, < p; (0, 0) is the
 * point at infinity.  scalars: n x 4 words, any 256-bit integers (e.g. residues mod the group order r).  out: 8 words, same
 * encoding as a point.  RONK_ERR_NOT_ON_CURVE: a coordinate >= p or y^2 != x^3 + 3 (AffinePoint::new's assert,
 * src/curve/mod.rs:79).  The _dev form takes device-resident points / scalars and a HOST result pointer: it enqueues
 * on `stream`, waits for it, and finishes the last ~270 dependent doublings on the host. */
int ronk_msm_bn254(const uint64_t* points, const uint64_t* scalars, size_t n, uint64_t out[8]);
int ronk_msm_bn254_dev(const uint64_t* d_points, const uint64_t* d_scalars, size_t n, uint64_t out[8], void* stream);

/* TEST HOOK, not a stable API: one function of the BN254 base-field / G1 arithmetic under the MSM kernels applied on the
 * device to n elements, raw limbs in, raw limbs out, no form conversion (Montgomery form, any representative in
 * [0, 2p), exactly as the kernels hold them).  op codes and element sizes: csrc/bn254_probe.h -- field operands and
 * results are 4 words, predicates write 1 word, an XYZZ point is 16 words (X, Y, ZZ, ZZZ), an affine operand 8.  d_b may
 * be NULL where the op is unary.  Asynchronous on `stream`; RONK_ERR_INVALID for an unknown op or a null pointer; n = 0
 * is a no-op. */
int ronk_bn254_probe_dev(int op, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, size_t n, void* stream);

/* kzg::open on the same curve (src/kzg/setup.rs:63-78): `poly.div([-eval_point, ONE])` over the SCALAR field of BN254,
 * r = 21888242871839275222246405745257275088548364400416034343698204186575808495617, then `commit(quotient, g1_srs)`.
 * coeffs: n x 4 words (4 x 64-bit little-endian limbs, standard form; taken mod r), ascending degree.  z: 4 words.
 * ronk_poly_div_linear_bn254_dev: the division alone -- quotient_and_remainder with a monic linear divisor
 * (src/polynomial/mod.rs:170-225): d_quot receives n entries, the top one ZERO (the reference's D-long quotient), d_rem
 * (device, 4 words, may be NULL) the remainder's constant term poly(z).  A suffix scan over 256-bit elements
 * (csrc/fr_scan_kernels.h, csrc/bn254_fr.h); synchronises `stream` (the multiplier tables are per call).
 * ronk_kzg_open_bn254(_dev): the division followed by ronk_msm_bn254_dev over (srs, quotient) -- the opening proof -- and
 * poly(z) in out_value (may be NULL).  srs: n x 8 words (points as for ronk_msm_bn254); n_srs < n is the reference's
 * assert (RONK_ERR_INDEX); the _dev form takes device-resident coefficients / SRS and an n x 4-word device buffer for
 * the quotient. */
int ronk_poly_div_linear_bn254_dev(const uint64_t* d_coeffs, size_t n, const uint64_t z[4], uint64_t* d_quot, uint64_t* d_rem,
                                   void* stream);
int ronk_kzg_open_bn254_dev(const uint64_t* d_coeffs, size_t n, const uint64_t z[4], const uint64_t* d_srs, uint64_t* d_quot,
                            uint64_t out_point[8], uint64_t out_value[4], void* stream);
int ronk_kzg_open_bn254(const uint64_t* coeffs, size_t n, const uint64_t z[4], const uint64_t* srs, size_t n_srs,
                        uint64_t out_point[8], uint64_t out_value[4]);

/* ---- NTT and polynomial product over the SCALAR field of BN254 (the field of ronk_kzg_open_bn254 above) ----
 * The reference's Polynomial::{fft, ifft} (src/polynomial/mod.rs:240-323, :430-453) and Mul
 * (src/polynomial/arithmetic.rs:97-119) are generic over F: FiniteField; these are their instances over Fr, what moves a
 * polynomial that kzg::commit / kzg::open work on between coefficients and values on a power-of-two domain.
 * Elements: 4 x 64-bit little-endian limbs, standard form, as everywhere above; inputs are any 256-bit integers, taken mod
 * r, outputs canonical.  Natural order in and out.  omega_n = 5^((r-1)/n) (src/algebra/field/mod.rs:70-75: 5 generates
 * Fr*, and r - 1 = 2^28 * odd, so n = 2^log2n with log2n <= 28; above that RONK_ERR_NO_ROOT, the reference's
 * "n must divide p^q - 1").  The inverse uses omega^-1 and includes 1/n.  Kernels: csrc/fr_ntt_kernels.h (DESIGN.md "NTT
 * over the BN254 scalar field").
 *
 * ronk_root_of_unity_bn254: omega_(2^log2n), host-side integer logic, no device work.
 * ronk_plan_create_bn254: tables for one size (both directions).  A transform is 1 to 4 passes of at most 2^10 rows each;
 * max_log2_tile (0 = default) caps the rows of every pass, so that a small transform can be made to take two or three
 * passes (testing); RONK_ERR_UNSUPPORTED when the cap would need more than four.  ronk_plan_info_bn254 reports the passes
 * and their log2 rows (entries past num_passes are 0).
 * ronk_ntt_forward_bn254_dev / _inverse_: `batch` transforms of rows that are contiguous in d_in and d_out; they enqueue on
 * `stream` and nothing else: no synchronisation, no allocation.  d_in == d_out is allowed.  Plans of two or more passes own
 * a scratch of `reserved` x n elements, one row at creation; a batch above `reserved` runs as slices of `reserved` rows one
 * behind the other.  ronk_plan_reserve_bn254 grows the scratch to `batch` rows so that such a batch runs as one set of
 * launches: it allocates and synchronises the device (call it beside plan creation, not on a capturing stream).  The
 * scratch is not guarded across streams: transforms that should overlap use one plan per stream.
 * ronk_ntt_forward_bn254 / _inverse_: host buffers, one transform (plan, staging and synchronisation inside).
 * ronk_poly_mul_bn254(_dev): exactly d + d2 - 1 coefficients (arithmetic.rs:97-119: the reference's product has D + D2 - 1)
 * through an NTT of the next power of two >= d + d2 - 1; RONK_ERR_UNSUPPORTED when that exceeds 2^28.  The _dev form
 * enqueues on `stream` and owns its scratch (the pooled workspace of ronk_poly_mul_dev, ronk_trim_workspace releases it);
 * the twiddle tables of each NTT size a product has used (0.3 % of that size's data at 2^20, 27 MiB at 2^28) stay cached per
 * device for the life of the process, outside that pool.  d_out may not overlap the operands.
 * RONK_ERR_INVALID: NULL pointer, zero length or batch; RONK_ERR_NO_DEVICE without a GPU (after the argument checks). */
int ronk_root_of_unity_bn254(uint32_t log2n, uint64_t out[4]);
typedef struct ronk_fr_plan ronk_fr_plan;
int ronk_plan_create_bn254(ronk_fr_plan** out, uint32_t log2n, uint32_t max_log2_tile);
int ronk_plan_info_bn254(const ronk_fr_plan* plan, uint32_t* num_passes, uint32_t log2_rows[4]);
int ronk_plan_reserve_bn254(ronk_fr_plan* plan, size_t batch);
int ronk_plan_destroy_bn254(ronk_fr_plan* plan);
int ronk_ntt_forward_bn254_dev(ronk_fr_plan* plan, const uint64_t* d_in, uint64_t* d_out, size_t batch, void* stream);
int ronk_ntt_inverse_bn254_dev(ronk_fr_plan* plan, const uint64_t* d_in, uint64_t* d_out, size_t batch, void* stream);
int ronk_ntt_forward_bn254(uint32_t log2n, const uint64_t* in, uint64_t* out);
int ronk_ntt_inverse_bn254(uint32_t log2n, const uint64_t* in, uint64_t* out);
int ronk_poly_mul_bn254_dev(const uint64_t* d_a, size_t d, const uint64_t* d_b, size_t d2, uint64_t* d_out, void* stream);
int ronk_poly_mul_bn254(const uint64_t* a, size_t d, const uint64_t* b, size_t d2, uint64_t* out);

/* ---- multi-GPU four-step building blocks (one process per GPU; the exchange between the two
 *      phases is an RCCL all-to-all issued by the host side, see ronkathon_amd/dist.py) ----
 * n = 2^log2n split as R x C with R = 2^(log2n - log2n/2) rows and C = 2^(log2n/2) columns;
 * rank `rank` of `world` owns columns [rank*C/world, (rank+1)*C/world) of the R x C input
 * (layout [R][C/world], row-major) and, after the exchange, rows [rank*R/world, ...) of the
 * twiddled intermediate (layout [R/world][C]); its output block is X[k1 + R*k2] for its k1
 * range, laid out [C][R/world] (k2-major). */
typedef struct ronk_dist_plan ronk_dist_plan;
int ronk_dist_plan_create(ronk_dist_plan** out, uint32_t log2n, int inverse, int rank, int world, int device);
int ronk_dist_plan_destroy(ronk_dist_plan* plan);
/* The same with the exchange split in `chunks` column chunks (a power of two, >= 16 columns per chunk): phase 1 of
 * chunk j writes the contiguous piece d_send[j*R*Cwc ..), Cwc = C/world/chunks, as `world` blocks [R/world][Cwc] (block h
 * for rank h), so the caller can ship chunk j while chunk j+1 is computed; the receiver stores the block of (source rank g,
 * chunk j) at d_recv[(g*chunks + j)*(R/world)*Cwc ..).  chunks = 1 is ronk_dist_plan_create. */
int ronk_dist_plan_create_chunked(ronk_dist_plan** out, uint32_t log2n, int inverse, int rank, int world, int device,
                                  int chunks);
/* The same over ANY field the single-GPU plans cover (round 6): p an odd prime with 2^log2n | p - 1 and g a primitive element
 * (a quadratic non-residue suffices; otherwise RONK_ERR_UNSUPPORTED -- the four-step has no radix-2 fallback); omega =
 * g^((p-1)/n) as in PrimeField<P> (src/algebra/field/mod.rs:70-75, prime/mod.rs:39-52).  The phases run the tile kernels over
 * Montgomery arithmetic.  ronk_dist_plan_create(_chunked) are the shorthands for (RONK_GOLDILOCKS_P, RONK_GOLDILOCKS_G). */
int ronk_dist_plan_create_p(ronk_dist_plan** out, uint64_t p, uint64_t g, uint32_t log2n, int inverse, int rank, int world,
                            int device, int chunks);
int ronk_dist_phase1_chunk_dev(ronk_dist_plan* plan, int chunk, const uint64_t* d_in, uint64_t* d_send, void* stream);
/* phase 1: R-point NTTs down the local columns, times omega_n^{c*k1}; output is written as `world`
 * consecutive send blocks, block h = rows k1 in h's range, layout [R/world][C/world] */
int ronk_dist_phase1_dev(ronk_dist_plan* plan, const uint64_t* d_in, uint64_t* d_send, void* stream);
/* phase 2: d_recv holds `world` blocks [R/world][C/world] (block g from rank g); C-point NTTs along
 * each local row k1; d_out[k2*(R/world) + (k1 - k1_0)] = X[k1 + R*k2] */
int ronk_dist_phase2_dev(ronk_dist_plan* plan, const uint64_t* d_recv, uint64_t* d_out, void* stream);

/* ---- device-resident forms of the callers above: no allocation, copy or synchronisation per call (workspace from an
 *      event-guarded pool), asynchronous on `stream`.  Conditions the reference reports by panicking are reported through a
 *      caller-owned device word `d_status` (the caller zeroes it and reads it when it synchronises; NULL where noted =
 *      "do not care"): non-zero = RONK_ERR_ZERO_INVERSE unless stated otherwise.  Inputs must be canonical residues. ---- */
int ronk_vec_neg_dev(uint64_t p, const uint64_t* d_a, uint64_t* d_out, size_t n, void* stream);
int ronk_vec_pow_dev(uint64_t p, const uint64_t* d_a, uint64_t e, uint64_t* d_out, size_t n, void* stream);
int ronk_vec_inv_dev(uint64_t p, const uint64_t* d_a, uint64_t* d_out, size_t n, int* d_status, void* stream);
/* Polynomial::dft (polynomial/mod.rs:240-258) for any n | p-1; see ronk_dft for the size limits */
int ronk_dft_dev(uint64_t p, uint64_t g, const uint64_t* d_in, uint64_t* d_out, size_t n, void* stream);
/* Polynomial::<Lagrange<F>>::evaluate (polynomial/mod.rs:382-415); d_out = ONE element; d_status may be NULL */
int ronk_lagrange_eval_dev(uint64_t p, const uint64_t* d_c, const uint64_t* d_nodes, size_t n, uint64_t x, uint64_t* d_out,
                           int* d_status, void* stream);
/* quotient_and_remainder (polynomial/mod.rs:170-225), any prime, any divisor; *d_status (required) receives 0 or the
 * RONK_ERR_* code of the reference's panic; d_rem may alias d_a.  The long-division kernel follows the reference's loop
 * (one workgroup, d * d2 steps).  Goldilocks, d2 >= 64 and d - d2 + 1 >= 2048: the operands' degrees are read back first
 * (the ONE exception to "no synchronisation per call": one stream synchronisation, 24 bytes) and, for a full-length divisor,
 * the O(n log n) Newton form on the NTT path runs, as behind ronk_poly_divrem.  A capturing stream keeps the long division. */
int ronk_poly_divrem_dev(uint64_t p, const uint64_t* d_a, size_t d, const uint64_t* d_b, size_t d2, uint64_t* d_quot,
                         uint64_t* d_rem, int* d_status, void* stream);
/* Round 6: the O(n log n) form serves EVERY odd prime whose p - 1 has the 2-adicity of the product sizes (2^(ceil(log2 d) + 1)
 * divides p - 1), not only Goldilocks -- behind ronk_poly_divrem and ronk_poly_divrem_dev alike; the products' transform
 * root is any quadratic non-residue found by the library (a product does not depend on it), so no generator is asked for.
 * Under stream capture ronk_poly_divrem_dev cannot probe the degrees: it captures the long division while that is a matter
 * of milliseconds (d2 * (d - d2 + 1) <= 1e9) and returns RONK_ERR_UNSUPPORTED beyond.
 *
 * quotient_and_remainder for FULL-LENGTH operands (a[d-1] != 0, b[d2-1] != 0, d >= d2): the same O(n log n) form with nothing
 * read back -- the divisor's leading coefficient is inverted on the device and the promise is checked there (*d_status =
 * RONK_ERR_INVALID when a top coefficient is ZERO: the outputs are then meaningless) -- so the call is asynchronous on `stream`
 * and capturable at any size (warm the workspace with one call outside the capture).  Fields as above, else
 * RONK_ERR_UNSUPPORTED.  For full-length operands the reference's loop is plain Euclidean division (mod.rs:170-225). */
int ronk_poly_divrem_full_dev(uint64_t p, const uint64_t* d_a, size_t d, const uint64_t* d_b, size_t d2, uint64_t* d_quot,
                              uint64_t* d_rem, int* d_status, void* stream);
/* Message::decode (src/codes/reed_solomon.rs:54-106); d_status may be NULL */
int ronk_rs_decode_dev(uint64_t p, const uint64_t* d_xs, const uint64_t* d_ys, size_t k, uint64_t* d_out, int* d_status,
                       void* stream);
/* kzg::commit (src/kzg/setup.rs:45-60); *d_status (required): bit 0 = RONK_ERR_NOT_ON_CURVE, bit 1 = RONK_ERR_ZERO_INVERSE.
 * With ronk_poly_div_linear_dev, kzg::open (setup.rs:63-78) never leaves the device. */
int ronk_curve_msm_dev(const ronk_curve* curve, const uint64_t* d_points, size_t n_points, const uint64_t* d_scalars, size_t n,
                       uint64_t* d_out, int* d_status, void* stream);

/* ---- the sharded transform as ONE call for a single-process host (the Rust host of BASELINE config 5): rank g of
 *      ndev = devices[g]; the exchange is a mesh of peer copies over xGMI issued by the library on per-peer copy
 *      streams, in `chunks` column chunks so that a chunk travels while the next one is computed (chunks <= 0: default,
 *      up to 4).  The reference has no counterpart: `Polynomial<B, F, D>` holds its coefficients inline
 *      (src/polynomial/mod.rs:34-44), so a degree this large never exists there.
 *      Errors: RONK_ERR_UNSUPPORTED (fewer than 16 rows / columns per rank and chunk, ndev not a power of two),
 *      RONK_ERR_INVALID (device ordinal out of range), RONK_ERR_HIP. */
typedef struct ronk_sharded_plan ronk_sharded_plan;
int ronk_sharded_plan_create(ronk_sharded_plan** out, uint32_t log2n, int inverse, const int* devices, int ndev, int chunks);
/* The same with the exchange chosen per plan: RONK_EXCHANGE_MESH = hipMemcpyPeerAsync copies, one copy stream per peer
 * (all xGMI links of a device busy at once); RONK_EXCHANGE_RCCL = every chunk's W x W blocks as one ncclGroup of
 * ncclSend / ncclRecv pairs (librccl.so is dlopen()ed on first use: RONK_ERR_RCCL if it is missing or a call fails;
 * ranks must be on distinct devices, else RONK_ERR_UNSUPPORTED).  Same results either way. */
#define RONK_EXCHANGE_MESH 0
#define RONK_EXCHANGE_RCCL 1
int ronk_sharded_plan_create_ex(ronk_sharded_plan** out, uint32_t log2n, int inverse, const int* devices, int ndev, int chunks,
                                int exchange);
/* The same over any field ronk_dist_plan_create_p takes (round 6): (p, g) as there; every rank's phases run the tile kernels
 * over Montgomery arithmetic.  ronk_sharded_plan_create(_ex) are the shorthands for the Goldilocks field. */
int ronk_sharded_plan_create_p(ronk_sharded_plan** out, uint64_t p, uint64_t g, uint32_t log2n, int inverse, const int* devices,
                               int ndev, int chunks, int exchange);
int ronk_sharded_plan_exchange(const ronk_sharded_plan* plan);
/* Diagnostics (bench.py --workload sharded): ONE transform in three SERIALISED stages -- every rank's phase 1, the whole
 * exchange, every rank's phase 2 -- all devices drained between them; ms[0..2] = wall milliseconds per stage.  The achieved
 * rate per directed link is n * 8 / ndev^2 bytes / ms[1].  Same d_out as ronk_ntt_sharded_dev (which overlaps the stages). */
int ronk_sharded_time_stages(ronk_sharded_plan* plan, const uint64_t* const* d_in, uint64_t* const* d_out, float* ms);
/* How a block travels between the ranks of a mesh-exchange plan, decided at plan creation and kept (never silent):
 * matrix[g * ndev + h] = RONK_PEER_SAME_DEVICE (ranks g and h share a GPU), RONK_PEER_DIRECT (hipDeviceCanAccessPeer said yes and
 * peer access is enabled: xGMI / PCIe peer-to-peer) or RONK_PEER_STAGED (refused: hipMemcpyPeerAsync stages through host
 * memory -- correct, roughly an order of magnitude slower).  `matrix` may be NULL; capacity >= ndev * ndev otherwise.
 * Returns the number of STAGED pairs (0 on a healthy xGMI node), or a negative error.  RONK_REQUIRE_PEER=1 in the environment
 * makes ronk_sharded_plan_create(_ex) fail with RONK_ERR_UNSUPPORTED instead of accepting a staged pair.
 * (The reference has no counterpart: it is single-threaded CPU code) */
#define RONK_PEER_SAME_DEVICE 0
#define RONK_PEER_DIRECT 1
#define RONK_PEER_STAGED 2
int ronk_sharded_plan_peer_access(const ronk_sharded_plan* plan, int* matrix, int capacity);
int ronk_sharded_plan_destroy(ronk_sharded_plan* plan);
/* R, C (n = R*C), elements per rank (n / ndev) and the number of column chunks in use; any pointer may be NULL */
int ronk_sharded_plan_info(const ronk_sharded_plan* plan, uint64_t* rows, uint64_t* cols, uint64_t* per_rank, int* chunks);
/* device-resident: d_in[g] = rank g's [R][C/ndev] column block on devices[g], d_out[g] = its [C][R/ndev] block of the
 * natural-order result (layouts as for ronk_dist_*).  Enqueues on the plan's own streams and returns; the buffers may
 * be reused after ronk_sharded_sync().  Successive calls pipeline (events guard the plan's send/receive buffers). */
int ronk_ntt_sharded_dev(ronk_sharded_plan* plan, const uint64_t* const* d_in, uint64_t* const* d_out);
int ronk_sharded_sync(ronk_sharded_plan* plan);
/* host pointers, natural order in and out (n elements each): scatter, transform, gather; synchronous */
int ronk_ntt_sharded(ronk_sharded_plan* plan, const uint64_t* in, uint64_t* out);

/* ---- the sharded polynomial multiply (reference `impl Mul`, src/polynomial/arithmetic.rs:97-119, at a size sharded over the
 *      node): same devices, chunks, exchange and field arguments as ronk_sharded_plan_create_p.  Per rank: forward phase 1 of a
 *      and b, exchange, a MIDDLE (forward phase 2 of both, pointwise product, phase 1 of an inverse whose split is the forward's
 *      swapped), exchange, inverse phase 2.  The forward's output block is the swapped inverse's input block, so the product
 *      comes back in the operands' own layout.  The middle is one fused kernel per inverse column chunk where an instantiation
 *      exists (log2n 18 .. 25, ndev * chunks >= 16) and it measured faster (by default log2n = 24; RONK_SHARDED_MUL_FUSED: wherever
 *      it exists); otherwise forward phase 2 writes both spectra and the inverse's phase 1 multiplies them on load.  Errors as for ronk_sharded_plan_create_p (both splits must be valid shapes). */
typedef struct ronk_sharded_mul_plan ronk_sharded_mul_plan;
#define RONK_SHARDED_MUL_UNFUSED 1   /* the composed middle */
#define RONK_SHARDED_MUL_FUSED 2     /* the fused middle wherever an instantiation matches (A/B; default: only where it measured faster) */
int ronk_sharded_mul_plan_create_p(ronk_sharded_mul_plan** out, uint64_t p, uint64_t g, uint32_t log2n, const int* devices,
                                   int ndev, int chunks, int exchange, int flags);
/* Goldilocks shorthand */
int ronk_sharded_mul_plan_create(ronk_sharded_mul_plan** out, uint32_t log2n, const int* devices, int ndev, int chunks,
                                 int exchange, int flags);
/* R, C, n / ndev, chunks in use, and whether the plan runs the fused middle (1) or the composed one (0); pointers may be NULL */
int ronk_sharded_mul_plan_info(const ronk_sharded_mul_plan* plan, uint64_t* rows, uint64_t* cols, uint64_t* per_rank,
                               int* chunks, int* fused_middle);
int ronk_sharded_mul_plan_destroy(ronk_sharded_mul_plan* plan);
/* d_a[g], d_b[g], d_out[g]: rank g's [R][C/ndev] column block of the zero-padded n-point vectors (the layout of
 * ronk_ntt_sharded_dev's input); d_out comes back in the same layout.  Computes the length-n CYCLIC convolution, which is a * b
 * when d + d2 - 1 <= n.  Enqueue-only on the plan's streams; successive calls pipeline; d_out[g] may be an input of the next
 * call (chaining), but not an input of the same call. */
int ronk_poly_mul_sharded_dev(ronk_sharded_mul_plan* plan, const uint64_t* const* d_a, const uint64_t* const* d_b,
                              uint64_t* const* d_out);
int ronk_sharded_mul_sync(ronk_sharded_mul_plan* plan);
/* host pointers: a (d coefficients), b (d2) -> out (d + d2 - 1) = ronk_poly_mul; d + d2 - 1 > n is RONK_ERR_INVALID; synchronous */
int ronk_poly_mul_sharded(ronk_sharded_mul_plan* plan, const uint64_t* a, size_t d, const uint64_t* b, size_t d2, uint64_t* out);

/* ---- Poseidon over the 64-bit fields and a Merkle commitment on its sponge.
 *      hashes::poseidon::{Poseidon, PoseidonSponge} (src/hashes/poseidon/mod.rs:56-149, sponge.rs:69-275), which the reference
 *      keeps generic over `F: Field` with caller-supplied constants, and tree::merkle::MerkleTree (src/tree/merkle.rs:31-99) with
 *      the sponge in the place of SHA-256.  Bit-exact restatement:
 *        permutation  for r in 0 .. num_f + num_p: state[i] += rc[r * width + i]; x -> x^alpha on every element when
 *                     r < num_f / 2 || r >= num_p + num_f / 2 (integer division: an odd num_f is legal), on state[0] otherwise;
 *                     state = mds * state with the DENSE matrix in every round (the optimised sparse partial rounds change the
 *                     caller's constants and are not offered).
 *        sponge       capacity = width - rate, state ZERO; element i of a chunk is added to state[capacity + i]; a one-shot absorb
 *                     of len elements runs ceil(len / rate) permutations, no padding, no length tag (len == 0: none, the squeeze
 *                     returns zeros); squeezing reads state[capacity + k], k < rate, and permutes each time rate elements have
 *                     been taken and more are wanted.
 *        tree         leaf digest = sponge(leaf elements) squeezing digest_len; node = sponge(left || right); levels pair up
 *                     from the left, an unpaired last node is hashed with itself; a proof is the sibling digests from the bottom
 *                     up, the sibling's side given by the parity of the index.
 *      The library ships NO parameter set: rc and mds come from the caller, as in the reference, and whether a given
 *      (width, alpha, rounds, matrix) is secure for a given prime is the caller's concern.
 *      Fields: Goldilocks (its own arithmetic) and any odd prime p < 2^64 (constants kept in Montgomery form on the device). */
typedef struct ronk_poseidon ronk_poseidon;
/* 2 <= width <= 16 (width < 2: RONK_ERR_INVALID, width > 16: RONK_ERR_UNSUPPORTED), 1 <= rate < width, alpha >= 1;
 * rc: (num_f + num_p) * width words, mds: width * width words row-major, both reduced mod p on upload.  A composite p:
 * RONK_ERR_NOT_PRIME (the test of ronk_check_prime); p == 2: RONK_ERR_UNSUPPORTED.  The handle lives on the current device. */
int ronk_poseidon_create(ronk_poseidon** out, uint64_t p, uint32_t width, uint64_t alpha, uint32_t num_p, uint32_t num_f,
                         uint32_t rate, const uint64_t* rc, const uint64_t* mds);
int ronk_poseidon_destroy(ronk_poseidon* h);
/* `count` states of `width` words each, row-major, permuted in place (a batch of Poseidon::hash, whose result is word 1). */
int ronk_poseidon_permute_dev(const ronk_poseidon* h, uint64_t* d_states, size_t count, void* stream);
/* Poseidon::hash on host pointers: `in` (len <= width words, else RONK_ERR_INDEX) padded with ZERO; out_state: the whole state. */
int ronk_poseidon_hash(const ronk_poseidon* h, const uint64_t* in, size_t len, uint64_t* out_state);
/* One sponge per item: element j of item i is d_in[i * item_stride + j * elem_stride]; d_out is n_items x n_out, row-major.
 * (item_stride, elem_stride) = (1, N) hashes the columns of a row-major [len][N] matrix -- what ronk_lde_batch_dev and
 * ronk_rs_encode_batch_dev leave behind -- with coalesced loads; (len, 1) is contiguous items.  Inputs >= p are reduced. */
int ronk_poseidon_sponge_dev(const ronk_poseidon* h, const uint64_t* d_in, size_t n_items, size_t len, size_t item_stride,
                             size_t elem_stride, uint64_t* d_out, size_t n_out, void* stream);
/* Layout of a tree: level 0 = the n_leaves leaf digests, level l + 1 = ceil(count_l / 2) nodes, the root last, digest_len words
 * per node.  ronk_merkle_level_offset: word offset of `level` (level = number of levels: the total, = ronk_merkle_tree_words). */
size_t ronk_merkle_tree_words(size_t n_leaves, size_t digest_len);
size_t ronk_merkle_level_offset(size_t n_leaves, size_t digest_len, size_t level);
/* MerkleTree::new: writes every level into the caller-owned d_tree (ronk_merkle_tree_words words).  Leaves are addressed as the
 * items of ronk_poseidon_sponge_dev; 1 <= digest_len <= rate and n_leaves >= 1, else RONK_ERR_INVALID.  Asynchronous, and it
 * uses NO library workspace, so it is legal under stream capture. */
int ronk_merkle_commit_dev(const ronk_poseidon* h, const uint64_t* d_leaves, size_t n_leaves, size_t leaf_len, size_t item_stride,
                           size_t elem_stride, size_t digest_len, uint64_t* d_tree, void* stream);
/* MerkleTree::get_proof for n_idx indices: d_paths is n_idx x depth x digest_len (depth = number of levels - 1; 0 for one leaf:
 * the leaf digest is the root).  d_status[q] = 0, or RONK_ERR_INDEX for index >= n_leaves and for the unpaired last node of an
 * odd level on the way up, where the reference indexes level[index + 1] out of bounds; that path is zero-filled. */
int ronk_merkle_open_dev(const uint64_t* d_tree, size_t n_leaves, size_t digest_len, const uint64_t* d_indices, size_t n_idx,
                         uint64_t* d_paths, int* d_status, void* stream);
/* MerkleTree::prove, one query per lane: d_ok[q] = 1 when the digest of leaf q (n_idx items, addressed as above), folded with
 * its path by the parity of d_indices[q], equals d_root (canonical words); else 0. */
int ronk_merkle_verify_dev(const ronk_poseidon* h, const uint64_t* d_leaves, size_t n_idx, size_t leaf_len, size_t item_stride,
                           size_t elem_stride, const uint64_t* d_indices, const uint64_t* d_paths, size_t n_leaves, size_t digest_len,
                           const uint64_t* d_root, int* d_ok, void* stream);
/* Host-pointer forms: contiguous leaves (n x leaf_len), synchronous.  ronk_merkle_open reads a HOST tree (no device work). */
int ronk_merkle_commit(const ronk_poseidon* h, const uint64_t* leaves, size_t n_leaves, size_t leaf_len, size_t digest_len,
                       uint64_t* tree);
int ronk_merkle_open(const uint64_t* tree, size_t n_leaves, size_t digest_len, const uint64_t* indices, size_t n_idx, uint64_t* paths,
                     int* status);
int ronk_merkle_verify(const ronk_poseidon* h, const uint64_t* leaves, size_t n_idx, size_t leaf_len, const uint64_t* indices,
                       const uint64_t* paths, size_t n_leaves, size_t digest_len, const uint64_t* root, int* ok);

/* ---- FRI over the 64-bit fields: the split-and-fold commit phase, Fiat-Shamir challenges from the caller's Poseidon handle,
 *      the query phase and the verifier, for ONE codeword that is already in device memory (what ronk_lde_batch_dev leaves
 *      behind).  The reference has no FRI; the semantics are fixed here and restated on Python integers in tests/fri_ref.py.
 *        field     that of the Poseidon handle: Goldilocks or any odd prime p < 2^64 with 2^log2_n | p - 1.
 *        domain    x_i = s w^i, i < N_0 = 2^log2_n, natural order, w = ronk_root_of_unity(p, g, N_0), s = coset_shift != 0;
 *                  layer 0 is the N_0 words f_0[i] = f(x_i).
 *        fold      f'[i] = (a + b) / 2 + beta (a - b) / (2 x_i) with a = f[i], b = f[i + N/2], i < N/2; the new domain is
 *                  s^2 <w^2>.  A layer of arity A = 2^log2_arity (2, 4 or 8) is log2_arity such folds with the challenges beta,
 *                  beta^2, beta^4: in coefficients g_k = sum_(j < A) beta^j c_(A k + j).  Output i < N/A reads only the coset
 *                  f[i + t N/A], t < A, which is Merkle leaf i of the layer (leaf_len = A, item_stride = 1, elem_stride = N/A in
 *                  the addressing of ronk_merkle_commit_dev).
 *        layers    L = (log2_n - log2_final) / log2_arity >= 1 (a remainder: RONK_ERR_INVALID), N_l = N_0 / A^l; layers
 *                  0 .. L - 1 are committed -- layer 0 by this call -- and layer L, 2^log2_final words, is sent in the clear.
 *        transcript  one-shot sponges of the handle, D = digest_len <= rate:  c_0 = seed (D words);  t_l = sponge(c_l || root_l)
 *                  squeezing D words, beta_l = t_l[0], c_(l+1) = t_l;  u = sponge(c_L || final layer) squeezing D words;  query q
 *                  has j_0 = sponge(u || [q])[0] & (N_0 / A - 1).  Repeated indices are allowed, and the bias of reducing a
 *                  sponge word below p before masking is ignored.
 *        queries   at layer l the leaf j_l = j_0 mod (N_l / A) is opened: its A values and log2(N_l / A) sibling digests.  Its
 *                  fold must equal slot j_l div (N_(l+1) / A) of the leaf opened at layer l + 1, and final[j_(L-1)] at the end.
 *        final     the interpolant of the final layer on s^(A^L) <w_(N_L)> has zero coefficients from N_L >> log2_blowup on
 *                  (log2_blowup <= log2_final <= 8).
 *        proof     canonical words: [L][D] roots, [N_L] final, then per layer l < L: [Q][A] leaf values, [Q][depth_l][D] paths.
 *                  Indices are not stored.
 *      Parameters and soundness are the caller's concern: on a handle of ronk_fri_create the challenge is a BASE-field element
 *      (ronk_fri_create_ext below draws it from the quadratic extension), and the query count, the blowup and the Poseidon
 *      constants decide what a proof is worth.  One column per call; several committed columns are opened through the batched
 *      FRI polynomial commitment below. */
typedef struct ronk_fri ronk_fri;
/* The argument checks of ronk_fri_create, host-side integer logic (p, rate: the Poseidon handle's): 2^log2_n does not divide
 * p - 1: RONK_ERR_NO_ROOT; log2_final > 8 or n_queries > 2^16: RONK_ERR_UNSUPPORTED; coset_shift = 0 (mod p), log2_arity outside
 * 1 .. 3, log2_blowup > log2_final, log2_n < log2_final + log2_arity or a remainder in the layer count, n_queries = 0, digest_len
 * = 0 or > rate, g without the full power-of-two order: RONK_ERR_INVALID. */
int ronk_fri_check(uint64_t p, uint32_t rate, uint64_t g, uint32_t log2_n, uint64_t coset_shift, uint32_t log2_arity,
                   uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len);
/* Sizes in words, 0 for sizes ronk_fri_check refuses.  Proof: as laid out above.  Workspace: the folded layers 1 .. L, the trees of
 * layers 0 .. L - 1 and L + (L + 2) D + L Q + Q words of transcript and query state. */
size_t ronk_fri_proof_words(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len);
size_t ronk_fri_workspace_words(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len);
/* The handle keeps the inverse-point tables of every layer and the verifier's state on the current device; it borrows `pos`,
 * which must outlive it.  Arguments are checked (ronk_fri_check) before a device is needed.  One verify call at a time per handle. */
int ronk_fri_create(ronk_fri** out, const ronk_poseidon* pos, uint64_t g, uint32_t log2_n, uint64_t coset_shift, uint32_t log2_arity,
                    uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len);
int ronk_fri_destroy(ronk_fri* fri);
/* One layer as a building block: d_in is layer `layer` (N_l words, any 64-bit values), *d_beta the challenge in device memory,
 * d_out receives N_l / A canonical words and must not overlap d_in.  Asynchronous. */
int ronk_fri_fold_dev(const ronk_fri* fri, uint32_t layer, const uint64_t* d_in, const uint64_t* d_beta, uint64_t* d_out, void* stream);
/* d_evals: layer 0; d_seed: D words; d_work: ronk_fri_workspace_words words and d_proof: ronk_fri_proof_words words, both
 * caller-owned.  Asynchronous on `stream` with no host round trip (the challenges stay in device memory); it uses no library
 * workspace.  Commits through ronk_merkle_commit_dev and opens through ronk_merkle_open_dev. */
int ronk_fri_prove_dev(const ronk_fri* fri, const uint64_t* d_evals, const uint64_t* d_seed, uint64_t* d_work, uint64_t* d_proof,
                       void* stream);
/* *d_status (written by the call) = 0, or a set of bits: 1 a Merkle path fails (checked by ronk_merkle_verify_dev), 2 a fold
 * mismatch, 4 the final layer is not of low degree.  Every check runs whatever the others find.  Asynchronous. */
int ronk_fri_verify_dev(const ronk_fri* fri, const uint64_t* d_proof, const uint64_t* d_seed, int* d_status, void* stream);
/* Host-pointer forms, synchronous. */
int ronk_fri_prove(const ronk_fri* fri, const uint64_t* evals, const uint64_t* seed, uint64_t* proof);
int ronk_fri_verify(const ronk_fri* fri, const uint64_t* proof, const uint64_t* seed, int* status);

/* ---- FRI with extension challenges: the same protocol with every challenge, and so every folded layer, in the quadratic
 *      extension F_p[t] / (t^2 - w) (see "quadratic extension" below; pairs (c0, c1), PLANAR arrays [2][n]).  A handle made by
 *      ronk_fri_create_ext is used through ronk_fri_fold_dev / prove_dev / verify_dev / prove / verify / destroy above; the handle
 *      knows its kind.  The semantics are those of the base form with these changes (restated in tests/fri_ext_ref.py):
 *        layers    layer 0 is [N_0] base words, embedded as (x, 0), when input_ext = 0, and [2][N_0] planar when input_ext = 1 (a
 *                  codeword that is already a random combination of columns: what ronk_deep_combine_dev writes); every layer
 *                  l >= 1 and the final layer are planar [2][N_l].
 *        fold      the same formula with beta in the extension and x_i in the base field; in coefficients still
 *                  g_k = sum_(j < A) beta^j c_(A k + j).  For ronk_fri_fold_dev, d_beta points at two words and d_out receives
 *                  [2][N_l / A] canonical words.
 *        leaves    leaf i of a planar layer is its A c0 values followed by its A c1 values: word j = c A + t of the leaf sits at
 *                  offset i + j m of the layer (m = N_l / A), so the leaf is leaf_len = 2 A, item_stride = 1, elem_stride = m in
 *                  the addressing of ronk_merkle_commit_dev.  A base layer 0 keeps leaf_len = A.
 *        transcript  c_0 = seed;  t_l = sponge(c_l || root_l) squeezing D words, beta_l = (t_l[0], t_l[1]), c_(l+1) = t_l;
 *                  u = sponge(c_L || final c0 plane || final c1 plane);  query indices as in the base form.
 *        queries   the fold of the opened leaf of layer l must equal the pair of words at slots s and A + s of the leaf opened at
 *                  layer l + 1, s = j_l div (N_(l+1) / A), and (final[j], final[N_L + j]) after the last committed layer.  Words
 *                  are compared as they stand: a word >= p is a mismatch.
 *        final     both planes are of low degree (the domain is in the base field, so the interpolant's coefficients are
 *                  low-degree componentwise).
 *        proof     [L][D] roots, [2][N_L] final, then per layer l < L: [Q][leaf_len_l] leaf values, [Q][depth_l][D] paths; in
 *                  words  L D + 2 N_L + sum_l Q (leaf_len_l + depth_l D),  leaf_len_0 = A (input_ext = 0) or 2 A, else 2 A.
 *        workspace planar layers 1 .. L, the trees of layers 0 .. L - 1 (leaf counts, and so tree sizes, are those of the base
 *                  form) and 2 L + (L + 2) D + L Q + Q words of transcript and query state; in words
 *                  sum_l (2 N_(l+1) + (2 N_l / A - 1) D) + 2 L + (L + 2) D + L Q + Q.
 *        status    bits 1 / 2 / 4 as in the base form.
 *      ronk_fri_check_ext: the codes of ronk_fri_check, then those of ronk_ext2_check(p, w), then RONK_ERR_INVALID for
 *      digest_len < 2 (a challenge takes two sponge words) and for input_ext other than 0 or 1.  The size functions return 0 for
 *      shapes that are refused.  One kernel per layer, no host round trip, caller-owned workspace and proof, as in the base form. */
int ronk_fri_check_ext(uint64_t p, uint32_t rate, uint64_t g, uint64_t w, uint32_t log2_n, uint64_t coset_shift, uint32_t log2_arity,
                       uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len, uint32_t input_ext);
size_t ronk_fri_proof_words_ext(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                                uint32_t input_ext);
size_t ronk_fri_workspace_words_ext(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                                    uint32_t input_ext);
int ronk_fri_create_ext(ronk_fri** out, const ronk_poseidon* pos, uint64_t g, uint64_t w, uint32_t log2_n, uint64_t coset_shift,
                        uint32_t log2_arity, uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len,
                        uint32_t input_ext);
/* The Q values j_0 that a proof's transcript implies (what the verifier derives before it checks anything), for both kinds of
 * handle: d_indices receives n_queries words.  It works in the handle's verifier state: one ronk_fri_verify_dev or
 * ronk_fri_query_indices_dev call at a time per handle.  Asynchronous. */
int ronk_fri_query_indices_dev(const ronk_fri* fri, const uint64_t* d_proof, const uint64_t* d_seed, uint64_t* d_indices, void* stream);

/* ---- batched FRI polynomial commitment with DEEP quotients: "these C committed polynomials take these values at the K points
 *      z_k" for the [C][N] matrix that ronk_lde_batch_dev leaves behind, on top of the Merkle commitment and the extension FRI
 *      above.  The reference has neither FRI nor DEEP; the semantics are fixed here and restated on Python integers in
 *      tests/deep_ref.py.  Field, extension (pairs, PLANAR arrays), domain x_i = s w^i (i < N = 2^log2_n), transcript sponge and
 *      tree are those of "FRI with extension challenges"; A = 2^log2_arity, m = N / A, D = digest_len.
 *        matrix    M: [C][N] row-major base words, M[c][i] = f_c(x_i) with deg f_c < d = N >> log2_blowup; words >= p are reduced.
 *        coef      [C][d] row-major, monomial basis, unscaled: sum_j coef[c][j] x_i^j = M[c][i].
 *        points    z: K extension elements, planar [2][K], chosen by the caller (drawn from their transcript after committing).
 *        claims    y: planar [2][K C], element k C + c = f_c(z_k) = sum_j coef[c][j] z_k^j.
 *        commit    leaf j < m holds the C A words M[c][j + t m] in the order c A + t: word q of the leaf sits at offset j + q m,
 *                  which is leaf_len = C A, item_stride = 1, elem_stride = m in the addressing of ronk_merkle_commit_dev.  One
 *                  leaf holds every column's values on the coset of FRI's layer-0 leaf j.  root_M: the tree's last D words.
 *        transcript  a = sponge(seed || root_M || z c0 plane || z c1 plane || y c0 plane || y c1 plane) squeezing D words;
 *                  alpha = (a[0], a[1]); the FRI seed is a.
 *        codeword  G[i] = sum_(k < K) sum_(c < C) alpha^(k C + c) (M[c][i] - y[k][c]) / (x_i - z_k), planar [2][N], canonical.
 *                  1 / (x_i - z_k) = (x_i - z0, z1) / ((x_i - z0)^2 - w z1^2).  The norm is zero only when z_k is the domain
 *                  point x_i; that term then contributes ZERO (as ronk_ext2_vec_inv_dev writes zero), and status bit 32 is set.
 *        opening   FRI with extension challenges on G (input_ext = 1) under the seed a -- exactly ronk_fri_prove_dev -- and
 *                  the matrix leaves at its query indices j_0.
 *        proof     canonical words: [2][K C] claims; the FRI proof, ronk_fri_proof_words_ext(.., 1) words; [Q][C A] matrix
 *                  leaf values; [Q][log2 m][D] paths.
 *        verifier  from root_M, z, the seed and the proof: recomputes a and alpha; runs ronk_fri_verify_dev under the seed a;
 *                  derives the indices; checks the matrix paths (ronk_merkle_verify_dev); recomputes G[j_0 + t m] for every
 *                  query and t < A from the opened matrix leaf, the claims, alpha and z, and compares it with words t and A + t
 *                  of the FRI proof's layer-0 leaf as they stand.
 *        status    the verifier: bits 1 / 2 / 4 as FRI reports them, 8 a matrix path fails, 16 a DEEP mismatch, 32 some z_k lies
 *                  on the domain; ronk_pcs_open_dev and ronk_deep_combine_dev: 0 or 32.  Every check runs whatever the others find.
 *        workspace D + Q words (a, open status), G [2][N], then ronk_fri_workspace_words_ext(.., 1) words.
 *      ronk_pcs_check: the codes of ronk_fri_check_ext with input_ext = 1, then RONK_ERR_INVALID for n_columns = 0 or n_points = 0,
 *      then RONK_ERR_UNSUPPORTED for n_columns > 1024, n_points > 8 or log2_n < 2.  The size functions return 0 for shapes that are
 *      refused.  Every _dev call is asynchronous on `stream` with no host round trip (alpha and the indices stay in device
 *      memory) and uses no library workspace; workspace and proof are caller-owned.  The handle keeps the domain's point table,
 *      the small table of the call in flight and the verifier's state: one call at a time per handle.  Goldilocks runs on its
 *      own arithmetic (with w = 7 the product with w is a shift), every other odd prime on the Montgomery policy. */
typedef struct ronk_pcs ronk_pcs;
int ronk_pcs_check(uint64_t p, uint32_t rate, uint64_t g, uint64_t w, uint32_t log2_n, uint64_t coset_shift, uint32_t log2_arity,
                   uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len, uint32_t n_columns,
                   uint32_t n_points);
size_t ronk_pcs_proof_words(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                            uint32_t n_columns, uint32_t n_points);
size_t ronk_pcs_workspace_words(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                                uint32_t n_columns, uint32_t n_points);
/* The handle owns an extension FRI handle with input_ext = 1 and borrows `pos`, which must outlive it. */
int ronk_pcs_create(ronk_pcs** out, const ronk_poseidon* pos, uint64_t g, uint64_t w, uint32_t log2_n, uint64_t coset_shift,
                    uint32_t log2_arity, uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len,
                    uint32_t n_columns, uint32_t n_points);
int ronk_pcs_destroy(ronk_pcs* pcs);
/* y = the values of n_columns base-field polynomials of d >= 1 coefficients each (d_coef: [n_columns][d] row-major) at n_points
 * <= 8 points of the extension (d_z: planar [2][n_points]); d_y: planar [2][n_points n_columns], element k n_columns + c.  Any
 * odd prime p with w a non-residue (ronk_ext2_check); n_columns = 0, n_points = 0 or d = 0: RONK_ERR_INVALID.  The coefficient
 * matrix is read once for all points. */
int ronk_ext2_poly_eval_batch_dev(uint64_t p, uint64_t w, const uint64_t* d_coef, uint32_t n_columns, size_t d, const uint64_t* d_z,
                                  uint32_t n_points, uint64_t* d_y, void* stream);
int ronk_ext2_poly_eval_batch(uint64_t p, uint64_t w, const uint64_t* coef, uint32_t n_columns, size_t d, const uint64_t* z,
                              uint32_t n_points, uint64_t* y);
/* The codeword G as a building block: d_alpha points at two words in device memory (as ronk_fri_fold_dev takes beta), d_G
 * receives [2][N] canonical words, *d_status 0 or 32.  The matrix is read once; G is the only N-sized write. */
int ronk_deep_combine_dev(const ronk_pcs* pcs, const uint64_t* d_M, const uint64_t* d_y, const uint64_t* d_z, const uint64_t* d_alpha,
                          uint64_t* d_G, int* d_status, void* stream);
/* The tree of the matrix into the caller-owned d_tree, ronk_merkle_tree_words(N / A, D) words. */
int ronk_pcs_commit_dev(const ronk_pcs* pcs, const uint64_t* d_M, uint64_t* d_tree, void* stream);
/* d_tree: what ronk_pcs_commit_dev wrote for d_M; d_coef: [C][d]; d_z: [2][K]; d_seed: D words; d_work: ronk_pcs_workspace_words
 * words; d_proof: ronk_pcs_proof_words words. */
int ronk_pcs_open_dev(const ronk_pcs* pcs, const uint64_t* d_M, const uint64_t* d_tree, const uint64_t* d_coef, const uint64_t* d_z,
                      const uint64_t* d_seed, uint64_t* d_work, uint64_t* d_proof, int* d_status, void* stream);
/* d_root: D words.  The verifier never sees the matrix. */
int ronk_pcs_verify_dev(const ronk_pcs* pcs, const uint64_t* d_root, const uint64_t* d_z, const uint64_t* d_seed, const uint64_t* d_proof,
                        int* d_status, void* stream);
/* Host-pointer forms, synchronous. */
int ronk_pcs_commit(const ronk_pcs* pcs, const uint64_t* M, uint64_t* tree);
int ronk_pcs_open(const ronk_pcs* pcs, const uint64_t* M, const uint64_t* tree, const uint64_t* coef, const uint64_t* z,
                  const uint64_t* seed, uint64_t* proof, int* status);
int ronk_pcs_verify(const ronk_pcs* pcs, const uint64_t* root, const uint64_t* z, const uint64_t* seed, const uint64_t* proof, int* status);

/* ---- proof of work (grinding) on a Poseidon handle, stand-alone and as the step between FRI's commit phase and its query phase.
 *      The reference has neither FRI nor grinding; the semantics are fixed here and restated on Python integers in tests/pow_ref.py.
 *        word      pow_word(seed, n) = the first word of the one-shot sponge(seed || [n]) (seed: seed_len words, any 64-bit values,
 *                  reduced on input), canonical -- exactly as FRI takes the word of a query index.
 *        nonce     the SMALLEST n < 2^log2_limit with pow_word(seed, n) & (2^bits - 1) == 0; the word 2^64 - 1 when there is none;
 *                  bits = 0 gives 0.  The bias of masking a word below p is ignored, as for the query indices.
 *        search    a prefix launch (one lane: the permutations of the seed-only chunks, once) and ONE search launch of T lanes:
 *                  lane g tries g, g + T, g + 2 T, ... and reloads the found word before every candidate; it stops at a candidate
 *                  >= the found word or >= 2^log2_limit, and a hit lowers the found word by a 64-bit atomic minimum.  The result is
 *                  the minimum whatever the execution order (csrc/pow_kernels.h has the argument).  T = max_lanes, or with
 *                  max_lanes = 0 a quarter of the lanes the device keeps resident for the kernel (measured the fastest); never
 *                  more than 2^log2_limit.  A candidate costs one permutation and no memory traffic; 2^bits candidates are expected.
 *      ronk_pow_check (host integer logic, no device): the codes of the Poseidon handle's field (p < 2: RONK_ERR_INVALID, p = 2:
 *      RONK_ERR_UNSUPPORTED, a composite p: RONK_ERR_NOT_PRIME), RONK_ERR_INVALID for rate = 0, then RONK_ERR_INVALID for
 *      2^bits >= p or 2^log2_limit >= p (a nonce must be a canonical, distinct field element), then RONK_ERR_UNSUPPORTED for
 *      bits > 40, log2_limit > 40 or seed_len > 4096.
 *      The _dev calls are asynchronous on `stream`, use no library workspace and are legal under stream capture.  d_work:
 *      ronk_pow_workspace_words words, caller-owned; d_nonce: one word.  ronk_pow_verify_dev writes *d_ok = 1 when *d_nonce is
 *      < 2^log2_limit and meets the condition, else 0; it does not check minimality.  The host forms are synchronous; ronk_pow_grind
 *      returns RONK_ERR_INDEX (and *nonce = 2^64 - 1) when nothing is found. */
int ronk_pow_check(uint64_t p, uint32_t rate, size_t seed_len, uint32_t bits, uint32_t log2_limit);
size_t ronk_pow_workspace_words(void);
int ronk_pow_grind_dev(const ronk_poseidon* h, const uint64_t* d_seed, size_t seed_len, uint32_t bits, uint32_t log2_limit,
                       size_t max_lanes, uint64_t* d_work, uint64_t* d_nonce, void* stream);
int ronk_pow_verify_dev(const ronk_poseidon* h, const uint64_t* d_seed, size_t seed_len, uint32_t bits, uint32_t log2_limit,
                        const uint64_t* d_nonce, int* d_ok, void* stream);
int ronk_pow_grind(const ronk_poseidon* h, const uint64_t* seed, size_t seed_len, uint32_t bits, uint32_t log2_limit, size_t max_lanes,
                   uint64_t* nonce);
int ronk_pow_verify(const ronk_poseidon* h, const uint64_t* seed, size_t seed_len, uint32_t bits, uint32_t log2_limit, uint64_t nonce,
                    int* ok);
/* Grinding in FRI, both kinds of handle.  ronk_fri_set_pow is called before the handle is used; its codes are those of
 * ronk_pow_check with seed_len = D, and bits = 0 restores the transcript above (byte-identical proofs, sizes and launches).  With
 * bits > 0 the transcript becomes: u as above;  nonce = the grind of the seed u;  u' = sponge(u || [nonce]) squeezing D words;
 * j_0 = sponge(u' || [q])[0] & (N_0 / A - 1).
 *        proof     one word more, the nonce, APPENDED at the end: every offset above is unchanged.
 *        workspace ronk_pow_workspace_words words more, at the end.
 *        sizes     the size functions above take no handle: ronk_fri_handle_proof_words / ronk_fri_handle_workspace_words give
 *                  the sizes of a handle, equal to theirs when bits = 0 (0 for a NULL handle).
 *        verifier  reads the last proof word and sets status bit 64 when it is >= 2^log2_limit or fails the condition; u' and the
 *                  indices are derived from the word as it stands (reduced on input), so every other check runs whatever this one
 *                  finds.  ronk_fri_query_indices_dev follows the same rule.
 *        prover    writes 2^64 - 1 when it finds nothing; ronk_fri_prove (host form) then returns RONK_ERR_INDEX.
 * The batched commitment forwards: ronk_pcs_set_pow sets its FRI handle; the embedded FRI proof is one word longer, so the
 * matrix-leaf section starts one word later; the openings follow FRI's indices; bit 64 passes through beside 8 / 16 / 32, and
 * ronk_pcs_open (host form) returns RONK_ERR_INDEX when nothing is found. */
int ronk_fri_set_pow(ronk_fri* fri, uint32_t bits, uint32_t log2_limit);
size_t ronk_fri_handle_proof_words(const ronk_fri* fri);
size_t ronk_fri_handle_workspace_words(const ronk_fri* fri);
int ronk_pcs_set_pow(ronk_pcs* pcs, uint32_t bits, uint32_t log2_limit);
size_t ronk_pcs_handle_proof_words(const ronk_pcs* pcs);
size_t ronk_pcs_handle_workspace_words(const ronk_pcs* pcs);

/* ---- multi-matrix polynomial commitment: R matrices, committed one after the other (each round's challenges are drawn after the
 *      previous commitment), each opened at its own subset of K extension points, combined into ONE DEEP codeword and opened under
 *      ONE FRI.  The semantics are fixed here and restated on Python integers in tests/mpcs_ref.py.  Field, extension, domain
 *      x_i = s w^i (i < N = 2^log2_n), transcript sponge, tree and FRI are those of the batched commitment above; A = 2^log2_arity,
 *      m = N / A, D = digest_len, Q = n_queries.
 *        shape     R = n_rounds matrices M_r, each [C_r][N] row-major base words, M_r[c][i] = f_(r,c)(x_i) with
 *                  deg f < d = N >> log2_blowup; K = n_points extension points z, planar [2][K]; point_masks[r]: bit k set means
 *                  round r is opened at z_k.  o_r = sum_(r' < r) C_r', C_tot = sum_r C_r.  All matrices share N and the blowup.
 *        commit    per round exactly the batched commitment's leaf layout with C = C_r (leaf_len = C_r A, item_stride = 1,
 *                  elem_stride = m): the tree that ronk_pcs_commit_dev writes on a handle of C_r columns.
 *        claims    y[r][k][c] = f_(r,c)(z_k) for k in mask_r only, ordered by round, then by the set bits of the mask ascending,
 *                  then by c; planar [2][Y], Y = sum_r popcount(mask_r) C_r.
 *        transcript  a = sponge(seed || root_0 || .. || root_(R-1) || z c0 plane || z c1 plane || y c0 plane || y c1 plane)
 *                  squeezing D words; alpha = (a[0], a[1]); the FRI seed is a.  Masks and shapes are handle parameters, as C and K
 *                  are above; binding the earlier rounds into `seed` is the caller's outer protocol.
 *        codeword  G[i] = sum_r sum_(k in mask_r) sum_(c < C_r) alpha^(k C_tot + o_r + c) (M_r[c][i] - y[r][k][c]) / (x_i - z_k),
 *                  planar [2][N], canonical: every (r, k, c) term has a power of alpha of its own.  A z_k on the domain
 *                  contributes zero and sets status bit 32.  For R = 1 with the full mask this is the codeword above, and
 *                  transcript, proof layout and proof words are those of ronk_pcs_*.
 *        proof     canonical words: [2][Y] claims; the extension FRI proof (input_ext = 1; with the nonce when grinding is set);
 *                  then for each round in turn [Q][C_r A] leaf values and [Q][log2 m][D] paths.
 *        verifier  from the [R][D] roots, z, the seed and the proof; it never sees a matrix.  Status bits 1 / 2 / 4 (64) as FRI
 *                  reports them, 8 a matrix path of any round fails, 16 a DEEP mismatch, 32 some z_k on the domain.  Every check
 *                  runs whatever the others find.
 *        workspace D + Q words (a, open status), G [2][N], then the FRI workspace: that of ronk_pcs_workspace_words, whatever R.
 *      ronk_mpcs_check (host integer logic): the codes of ronk_fri_check_ext with input_ext = 1; then RONK_ERR_INVALID for a NULL
 *      array, n_points = 0, n_rounds = 0, some C_r = 0, some mask 0 or >= 2^n_points, or a point that no mask selects; then
 *      RONK_ERR_UNSUPPORTED for n_points > 8, n_rounds > 8, C_tot > 1024 or log2_n < 2.  The size functions return 0 for refused
 *      shapes.  d_M, d_tree and d_coef are HOST arrays of R device pointers, passed on to the kernels by value: there is no
 *      device-side pointer table and no host round trip.  Every _dev call is asynchronous on `stream`, uses caller-owned
 *      workspace and proof and no library workspace; one call at a time per handle.  The combination is one launch that reads
 *      every matrix once and writes G only (csrc/mpcs_kernels.h).  ronk_mpcs_set_pow forwards to the embedded FRI handle as
 *      ronk_pcs_set_pow does, and ronk_mpcs_open (host form) returns RONK_ERR_INDEX when the search finds nothing. */
typedef struct ronk_mpcs ronk_mpcs;
int ronk_mpcs_check(uint64_t p, uint32_t rate, uint64_t g, uint64_t w, uint32_t log2_n, uint64_t coset_shift, uint32_t log2_arity,
                    uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len, uint32_t n_points,
                    uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* point_masks);
size_t ronk_mpcs_proof_words(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                             uint32_t n_points, uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* point_masks);
size_t ronk_mpcs_workspace_words(uint32_t log2_n, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                                 uint32_t n_points, uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* point_masks);
/* The handle owns an extension FRI handle with input_ext = 1, copies the two arrays and borrows `pos`, which must outlive it. */
int ronk_mpcs_create(ronk_mpcs** out, const ronk_poseidon* pos, uint64_t g, uint64_t w, uint32_t log2_n, uint64_t coset_shift,
                     uint32_t log2_arity, uint32_t log2_final, uint32_t log2_blowup, uint32_t n_queries, uint32_t digest_len,
                     uint32_t n_points, uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* point_masks);
int ronk_mpcs_destroy(ronk_mpcs* mpcs);
int ronk_mpcs_set_pow(ronk_mpcs* mpcs, uint32_t bits, uint32_t log2_limit);
size_t ronk_mpcs_handle_proof_words(const ronk_mpcs* mpcs);
size_t ronk_mpcs_handle_workspace_words(const ronk_mpcs* mpcs);
/* The tree of round `round`'s matrix ([C_round][N]) into the caller-owned d_tree, ronk_merkle_tree_words(N / A, D) words. */
int ronk_mpcs_commit_dev(const ronk_mpcs* mpcs, uint32_t round, const uint64_t* d_M, uint64_t* d_tree, void* stream);
/* The codeword G as a building block: d_y planar [2][Y], d_alpha two words in device memory, d_G [2][N], *d_status 0 or 32. */
int ronk_mpcs_combine_dev(const ronk_mpcs* mpcs, const uint64_t* const* d_M, const uint64_t* d_y, const uint64_t* d_z,
                          const uint64_t* d_alpha, uint64_t* d_G, int* d_status, void* stream);
/* d_tree[r]: what ronk_mpcs_commit_dev wrote for d_M[r]; d_coef[r]: [C_r][d]; d_z: [2][K]; d_seed: D words; d_work and d_proof:
 * ronk_mpcs_workspace_words and ronk_mpcs_proof_words words (with grinding, the handle's sizes).  *d_status: 0 or 32. */
int ronk_mpcs_open_dev(const ronk_mpcs* mpcs, const uint64_t* const* d_M, const uint64_t* const* d_tree, const uint64_t* const* d_coef,
                       const uint64_t* d_z, const uint64_t* d_seed, uint64_t* d_work, uint64_t* d_proof, int* d_status, void* stream);
/* d_roots: [R][D] words. */
int ronk_mpcs_verify_dev(const ronk_mpcs* mpcs, const uint64_t* d_roots, const uint64_t* d_z, const uint64_t* d_seed,
                         const uint64_t* d_proof, int* d_status, void* stream);
/* Host-pointer forms, synchronous: M, tree and coef are arrays of R host pointers. */
int ronk_mpcs_commit(const ronk_mpcs* mpcs, uint32_t round, const uint64_t* M, uint64_t* tree);
int ronk_mpcs_open(const ronk_mpcs* mpcs, const uint64_t* const* M, const uint64_t* const* tree, const uint64_t* const* coef,
                   const uint64_t* z, const uint64_t* seed, uint64_t* proof, int* status);
int ronk_mpcs_verify(const ronk_mpcs* mpcs, const uint64_t* roots, const uint64_t* z, const uint64_t* seed, const uint64_t* proof,
                     int* status);

/* ---- the quadratic extension F_p[t] / (t^2 - w) of a 64-bit prime field: the reference's GaloisField<2, P>
 *      (src/algebra/field/extension/, arithmetic.rs, gf_101_2.rs; PlutoBaseFieldExtension is p = 101, w = 99 = -2).  An element
 *      is the pair (c0, c1) = c0 + c1 t, the reference's coeffs in increasing degree.  Arrays are PLANAR: n elements are [2][n]
 *      words, the c0 plane first and the c1 plane at offset n (the layout of the extension FRI layers; the many-array transform
 *      over the two planes is the NTT of an extension-valued polynomial).  Inputs may be any 64-bit words and are reduced; outputs
 *      are canonical.  Goldilocks runs on its own arithmetic, every other odd prime on the Montgomery policy.  `out` may alias an
 *      input elementwise.  No library workspace is used: every _dev call is legal under stream capture.
 *      ronk_ext2_check (host-side integer logic): p == 2: RONK_ERR_UNSUPPORTED; a composite p: RONK_ERR_NOT_PRIME; w = 0 (mod p)
 *      or w a quadratic residue (Euler's criterion): RONK_ERR_INVALID.  Every entry point below checks the same first. */
int ronk_ext2_check(uint64_t p, uint64_t w);
int ronk_ext2_vec_add_dev(uint64_t p, uint64_t w, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, size_t n, void* stream);
int ronk_ext2_vec_sub_dev(uint64_t p, uint64_t w, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, size_t n, void* stream);
/* (a0 b0 + w a1 b1, (a0 + a1)(b0 + b1) - a0 b0 - a1 b1) */
int ronk_ext2_vec_mul_dev(uint64_t p, uint64_t w, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, size_t n, void* stream);
int ronk_ext2_vec_neg_dev(uint64_t p, uint64_t w, const uint64_t* d_a, uint64_t* d_out, size_t n, void* stream);
/* Mul<PrimeField<P>>: d_s holds n base words, both components of element i are multiplied by d_s[i] */
int ronk_ext2_vec_mul_base_dev(uint64_t p, uint64_t w, const uint64_t* d_a, const uint64_t* d_s, uint64_t* d_out, size_t n, void* stream);
/* pow by a u64 exponent (square-and-multiply; pow(_, 0) = (1, 0)) */
int ronk_ext2_vec_pow_dev(uint64_t p, uint64_t w, const uint64_t* d_a, uint64_t e, uint64_t* d_out, size_t n, void* stream);
/* inverse(): (a0, -a1) / (a0^2 - w a1^2).  *d_status (may be NULL) is set non-zero when an element is ZERO, and (0, 0) is
 * written for it -- as ronk_vec_inv_dev reports and writes a zero word. */
int ronk_ext2_vec_inv_dev(uint64_t p, uint64_t w, const uint64_t* d_a, uint64_t* d_out, size_t n, int* d_status, void* stream);
/* Host-pointer forms, synchronous.  ronk_ext2_vec_inv: a ZERO element is RONK_ERR_ZERO_INVERSE, as ronk_vec_inv. */
int ronk_ext2_vec_add(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int ronk_ext2_vec_sub(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int ronk_ext2_vec_mul(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int ronk_ext2_vec_neg(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n);
int ronk_ext2_vec_mul_base(uint64_t p, uint64_t w, const uint64_t* a, const uint64_t* s, uint64_t* out, size_t n);
int ronk_ext2_vec_pow(uint64_t p, uint64_t w, const uint64_t* a, uint64_t e, uint64_t* out, size_t n);
int ronk_ext2_vec_inv(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n);

/* ---- running products and sums, the permutation grand product and the logUp running sum: the accumulator columns a PLONK- or
 *      STARK-style prover builds from challenges drawn after its first commitment.  The reference stops at the permutation
 *      polynomials S_sigma1..3 (src/compiler/program.rs:146-226) and has no prover; the semantics are fixed here and restated on
 *      Python integers in tests/accum_ref.py.  Field: any odd prime p < 2^64 (Goldilocks on its own arithmetic, every other on the
 *      Montgomery policy); extension F_p[t] / (t^2 - w) as above, checked by ronk_ext2_check, arrays PLANAR [2][n] (with w = 7
 *      over Goldilocks the product with w is a shift).  Inputs may be any 64-bit words and are reduced; outputs are canonical.
 *        scans     o is * or +, its identity e is 1 or 0.  exclusive = 0: out[i] = a[0] o .. o a[i]; exclusive = 1: out[0] = e,
 *                  out[i] = a[0] o .. o a[i-1].  *d_total (may be NULL; one element: one word, or two for the extension) receives
 *                  a[0] o .. o a[n-1].  d_out == d_a is allowed.  Field arithmetic is exact: every blocking gives these words.
 *        permutation product   wires a, ids and sigma: [W][N] base words, row-major; beta, gamma: extension elements, two words
 *                  each in device memory (as ronk_fri_fold_dev takes beta).  num_i = prod_(c < W) (a_c[i] + beta id_c[i] + gamma),
 *                  den_i = prod_(c < W) (a_c[i] + beta sigma_c[i] + gamma); Z[0] = 1, Z[i+1] = Z[i] num_i / den_i.  d_Z: planar
 *                  [2][N], receives Z[0..N-1]; d_last (two words) receives Z[N]; whether Z[N] = 1 is the caller's check.  A row
 *                  with den_i = 0 contributes the factor ZERO (as ronk_ext2_vec_inv_dev writes zero) and sets *d_status = 1;
 *                  otherwise *d_status = 0 (required; written by the call).  The reference's labels are id_c[i] = (c + 1) omega^i
 *                  (Cell::label); the caller supplies the arrays, so any injective labelling works.
 *        logUp sum   values v: [C][N]; multiplicities m: [C][N] base words, d_mult == NULL means all ones, "-k" is the word p - k;
 *                  alpha: an extension element in device memory.  S[0] = 0, S[i+1] = S[i] + sum_(c < C) m_c[i] / (alpha + v_c[i]).
 *                  d_S: planar [2][N], receives S[0..N-1]; d_last receives S[N].  A zero denominator makes that term ZERO and sets
 *                  *d_status = 1 (else 0).
 *        workspace d_work: ronk_scan_workspace_words(n) words, caller-owned; 0 for n = 0 or n > 2^28.
 *      Errors, all found before a device is needed: NULL pointer (d_total and d_mult excepted), n = 0, n_columns = 0 or exclusive
 *      other than 0 or 1: RONK_ERR_INVALID; n > 2^28 or n_columns > 16: RONK_ERR_UNSUPPORTED; the codes of ronk_ext2_check (for the
 *      base-field scans: p < 2 RONK_ERR_INVALID, p = 2 RONK_ERR_UNSUPPORTED, else ronk_check_prime).  ronk_accum_check (host-side
 *      integer logic): the codes of ronk_ext2_check, then RONK_ERR_INVALID, then RONK_ERR_UNSUPPORTED as above.
 *      Every _dev call is asynchronous on `stream`: three kernel launches, no workgroup ever waits for another, no host round
 *      trip, no library workspace -- legal under stream capture.  Outputs must not overlap inputs, except the elementwise aliasing
 *      of the plain scans. */
size_t ronk_scan_workspace_words(size_t n);
int ronk_vec_prefix_prod_dev(uint64_t p, const uint64_t* d_a, uint64_t* d_out, size_t n, int exclusive, uint64_t* d_total,
                             uint64_t* d_work, void* stream);
int ronk_vec_prefix_sum_dev(uint64_t p, const uint64_t* d_a, uint64_t* d_out, size_t n, int exclusive, uint64_t* d_total,
                            uint64_t* d_work, void* stream);
int ronk_ext2_vec_prefix_prod_dev(uint64_t p, uint64_t w, const uint64_t* d_a, uint64_t* d_out, size_t n, int exclusive,
                                  uint64_t* d_total, uint64_t* d_work, void* stream);
int ronk_ext2_vec_prefix_sum_dev(uint64_t p, uint64_t w, const uint64_t* d_a, uint64_t* d_out, size_t n, int exclusive,
                                 uint64_t* d_total, uint64_t* d_work, void* stream);
int ronk_accum_check(uint64_t p, uint64_t w, uint32_t n_columns, size_t n);
int ronk_perm_product_dev(uint64_t p, uint64_t w, const uint64_t* d_wires, const uint64_t* d_ids, const uint64_t* d_sigma,
                          uint32_t n_columns, size_t n, const uint64_t* d_beta, const uint64_t* d_gamma, uint64_t* d_Z, uint64_t* d_last,
                          uint64_t* d_work, int* d_status, void* stream);
int ronk_logup_sum_dev(uint64_t p, uint64_t w, const uint64_t* d_vals, const uint64_t* d_mult, uint32_t n_columns, size_t n,
                       const uint64_t* d_alpha, uint64_t* d_S, uint64_t* d_last, uint64_t* d_work, int* d_status, void* stream);
/* Host-pointer forms, synchronous; they allocate their own workspace.  `total` may be NULL; `status` is required. */
int ronk_vec_prefix_prod(uint64_t p, const uint64_t* a, uint64_t* out, size_t n, int exclusive, uint64_t* total);
int ronk_vec_prefix_sum(uint64_t p, const uint64_t* a, uint64_t* out, size_t n, int exclusive, uint64_t* total);
int ronk_ext2_vec_prefix_prod(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n, int exclusive, uint64_t* total);
int ronk_ext2_vec_prefix_sum(uint64_t p, uint64_t w, const uint64_t* a, uint64_t* out, size_t n, int exclusive, uint64_t* total);
int ronk_perm_product(uint64_t p, uint64_t w, const uint64_t* wires, const uint64_t* ids, const uint64_t* sigma, uint32_t n_columns,
                      size_t n, const uint64_t* beta, const uint64_t* gamma, uint64_t* Z, uint64_t* last, int* status);
int ronk_logup_sum(uint64_t p, uint64_t w, const uint64_t* vals, const uint64_t* mult, uint32_t n_columns, size_t n,
                   const uint64_t* alpha, uint64_t* S, uint64_t* last, int* status);

/* ---- lookup multiplicities and the logUp quotient: the two steps either side of ronk_logup_sum_dev that make the running sum a
 *      complete, checkable lookup argument.  The reference has no prover; the semantics are fixed here and restated on Python
 *      integers in tests/lookup_ref.py.  Field: any odd prime p < 2^64, as for the base-field scans above.
 *        multiplicities   d_table [T] and d_vals [C][n] (row-major) are any 64-bit words; every comparison is between the words
 *                  REDUCED mod p, so 3 and p + 3 are equal.  Table entry j is the representative of its value when no smaller
 *                  index holds the same value.  d_mult [T], canonical: at a representative, the number of pairs (c, i) with
 *                  f_c[i] = t[j], taken mod p, or with negate = 1 p minus that (0 stays 0); at every other j, 0.  With negate = 1
 *                  it is exactly the m row ronk_logup_sum_dev wants for the table column.  d_missing (required, two words): [0]
 *                  the number of pairs (c, i) whose value is not in the table, [1] the smallest c n + i among them, or 2^64 - 1
 *                  when there is none.  Every word written is a function of the inputs alone, whatever the scheduling.
 *                  T, n <= 2^28, C <= 16.  d_work: ronk_lookup_workspace_words(T) words, caller-owned (an open-addressing table of
 *                  the power-of-two capacity >= 2 T, two words per slot); 0 for T = 0 or T > 2^28.  Outputs must not overlap
 *                  inputs or each other.
 *      Errors, in this order and before a device is needed: NULL pointer, T = 0, n = 0 or C = 0: RONK_ERR_INVALID; T or n > 2^28
 *      or C > 16: RONK_ERR_UNSUPPORTED; p < 2 RONK_ERR_INVALID, p = 2 RONK_ERR_UNSUPPORTED, else the code of ronk_check_prime;
 *      negate other than 0 or 1: RONK_ERR_INVALID.  ronk_lookup_check (host-side integer logic) reports those of the shape and
 *      the field.  The _dev call is asynchronous on `stream`: FOUR kernel launches (clear, build, count, finalise), integer atomics
 *      and launch boundaries only -- no lane or workgroup ever waits for another, every probe loop is bounded by the capacity --
 *      no host round trip, no library workspace: legal under stream capture.
 *        logUp quotient   on the domain of a ronk_plonk handle (below: N, B, M, x_i; its label multipliers are unused).  Inputs on
 *                  the coset, any 64-bit words: d_vals [C][M]; d_mult [C][M] or NULL for all ones; d_S planar [2][M], each plane
 *                  the extension of one plane of what ronk_logup_sum_dev wrote; d_alpha the logUp challenge (two words);
 *                  d_lambda two extension elements lambda0, lambda1 (four words), the powers of the quotient challenge this
 *                  constraint pair receives; d_T_in planar [2][M] or NULL for zero.
 *        row i     D_c = alpha + v_c[i];  P = prod_c D_c;  Q = sum_c m_c[i] prod_(c' != c) D_c'
 *                  R = (S_((i + B) mod M) - S_i) P - Q
 *                  T_out_i = T_in_i + lambda0 R / (x_i^N - 1) + lambda1 S_i / (N (x_i - 1))
 *                  The last term is lambda1 S L1 / (x^N - 1); nothing is divided by D_c and there is no status word.
 *        output    d_T_out planar [2][M], canonical.  d_T_out == d_T_in is allowed (row i reads T_in at row i only); it must not
 *                  overlap S, the values or the multiplicities.
 *      The caller's concern: the transition holds on every row of H only when S[N] = 0, that is when d_last of
 *      ronk_logup_sum_dev is zero; and T is a polynomial of degree below M only when C <= B (its coefficients from C N - C upward
 *      then vanish).  Errors: NULL pointer (d_mult and d_T_in excepted) or C = 0: RONK_ERR_INVALID; C > 16: RONK_ERR_UNSUPPORTED.
 *      One kernel launch, legal under stream capture.  The host-pointer forms are synchronous and allocate their own workspace.
 *      (ronk_plonk is declared with the PLONK quotient below.) */
struct ronk_plonk;
size_t ronk_lookup_workspace_words(size_t n_table);
int ronk_lookup_check(uint64_t p, size_t n_table, uint32_t n_columns, size_t n);
int ronk_lookup_mult_dev(uint64_t p, const uint64_t* d_table, size_t n_table, const uint64_t* d_vals, uint32_t n_columns, size_t n,
                         int negate, uint64_t* d_mult, uint64_t* d_missing, uint64_t* d_work, void* stream);
int ronk_lookup_mult(uint64_t p, const uint64_t* table, size_t n_table, const uint64_t* vals, uint32_t n_columns, size_t n, int negate,
                     uint64_t* mult, uint64_t* missing);
int ronk_logup_quotient_dev(const struct ronk_plonk* h, const uint64_t* d_vals, const uint64_t* d_mult, uint32_t n_columns,
                            const uint64_t* d_S, const uint64_t* d_alpha, const uint64_t* d_lambda, const uint64_t* d_T_in,
                            uint64_t* d_T_out, void* stream);
int ronk_logup_quotient(const struct ronk_plonk* h, const uint64_t* vals, const uint64_t* mult, uint32_t n_columns, const uint64_t* S,
                        const uint64_t* alpha, const uint64_t* lambda, const uint64_t* T_in, uint64_t* T_out);

/* ---- PLONK quotient: the quotient polynomial of a three-wire PLONK circuit on the evaluation coset, in ONE kernel launch.  The
 *      gate equation is the reference's a QL + b QR + a b QM + o QO + QC = 0 (src/compiler/program.rs:4-5,
 *      CommonPreprocessedInput); the reference has no prover, so the semantics are fixed here and restated on Python integers in
 *      tests/plonk_ref.py.  Field and extension as for the accumulators above (Goldilocks on its own arithmetic, every other odd
 *      prime on the Montgomery policy; planar [2][M] extension arrays).
 *        domain    N = 2^log2_n trace rows, B = 2^log2_blowup, M = N B; w_M = ronk_root_of_unity(p, g, M), w_N = w_M^B;
 *                  x_i = s w_M^i, i < M, natural order, s = coset_shift: what ronk_lde_batch_dev leaves behind.
 *        inputs    all on the coset, any 64-bit words (reduced): d_wires [3][M] = a, b, o; d_sel [5][M] = ql, qr, qm, qo, qc;
 *                  d_sigma [3][M]; d_pi [M] or NULL for zero; d_Z planar [2][M], each plane the extension of one plane of what
 *                  ronk_perm_product_dev wrote; alpha, beta, gamma: two words each in device memory.  The label multipliers
 *                  k[0..2] are base words fixed at creation (the reference uses 1, 2, 3, Cell::label): the identity label of
 *                  wire c at x is k_c x, generated in the kernel.  That the cosets k_c <w_N> are disjoint is the caller's concern.
 *        row i     G  = a ql + b qr + a b qm + o qo + qc + pi
 *                  P1 = Z_i prod_c (w_c + beta k_c x_i + gamma) - Z_((i + B) mod M) prod_c (w_c + beta sigma_c + gamma)
 *                  P2 = (Z_i - 1) L1(x_i),  L1(x) = (x^N - 1) / (N (x - 1))
 *                  T_i = (G + alpha P1 + alpha^2 P2) / (x_i^N - 1)
 *        output    d_T planar [2][M], canonical.  It must not overlap any input: row i reads Z at row i + B.
 *      ronk_plonk_check (host-side integer logic), in this order: the codes of ronk_ext2_check; RONK_ERR_INVALID for k == NULL,
 *      s = 0 or some k_c = 0 (mod p); RONK_ERR_NO_ROOT when M does not divide p - 1; RONK_ERR_UNSUPPORTED for log2_n < 1,
 *      log2(M) > 28 or s^M = 1 -- exactly the case where some x_i^N - 1 or x_i - 1 vanishes, so no division by zero is left and
 *      there is no status word.  Whether g has the full power-of-two order is the caller's concern, as with ronk_root_of_unity.
 *      The handle owns the two-level point table, the B values 1 / (x^N - 1), 1 / N and the k_c.  NULL pointers (d_pi excepted)
 *      are RONK_ERR_INVALID before any device work.  The _dev call is asynchronous on `stream`: one kernel launch, no library
 *      workspace, no host round trip -- legal under stream capture.  The host-pointer form is synchronous. */
typedef struct ronk_plonk ronk_plonk;
int ronk_plonk_check(uint64_t p, uint64_t g, uint64_t w, uint32_t log2_n, uint32_t log2_blowup, uint64_t coset_shift,
                     const uint64_t k[3]);
int ronk_plonk_create(ronk_plonk** out, uint64_t p, uint64_t g, uint64_t w, uint32_t log2_n, uint32_t log2_blowup,
                      uint64_t coset_shift, const uint64_t k[3]);
int ronk_plonk_destroy(ronk_plonk* h);
int ronk_plonk_quotient_dev(const ronk_plonk* h, const uint64_t* d_wires, const uint64_t* d_sel, const uint64_t* d_sigma,
                            const uint64_t* d_pi, const uint64_t* d_Z, const uint64_t* d_alpha, const uint64_t* d_beta,
                            const uint64_t* d_gamma, uint64_t* d_T, void* stream);
int ronk_plonk_quotient(const ronk_plonk* h, const uint64_t* wires, const uint64_t* sel, const uint64_t* sigma, const uint64_t* pi,
                        const uint64_t* Z, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma, uint64_t* T);

/* ---- constraint programs: a straight-line program over the columns of a trace, fixed at handle creation, evaluated at every row
 *      of the evaluation coset in ONE kernel launch, which adds sum_j lambda_j C_j (divisor of C_j's kind) onto T.  It is the
 *      general form of the two quotients above: a custom gate, a wider permutation, or a STARK AIR with "every row but the last"
 *      transitions and first / last-row boundary constraints.  The semantics are fixed here and restated on Python integers in
 *      tests/air_ref.py.
 *        domain    that of a ronk_plonk handle (above): N, B, M = N B, x_i = s w_M^i in natural order, w_N = w_M^B, the extension
 *                  F_p[t] / (t^2 - W) as planar pairs, Goldilocks on its own arithmetic and every other odd prime on the Montgomery
 *                  policy.  The handle refuses s^M = 1, so x_i - 1, x_i - w_N^-1 and x_i^N - 1 never vanish: no status word.  Its
 *                  label multipliers are unused.
 *        inputs    all on the coset, any 64-bit words (reduced).  G <= 8 base groups, group g a [C_g][M] matrix with its own
 *                  device pointer; base column indices are flat across the groups in order, sum C_g <= 64.  E <= 8 extension
 *                  columns, each a planar [2][M] array with its own pointer.  d_base and d_ext are HOST arrays of device pointers
 *                  (they travel to the kernel by value).  d_chal [n_chal][2], n_chal <= 32: the extension constants of the call.
 *                  d_lambda [J][2], J <= 64: one weight per constraint.  d_T_in planar [2][M] or NULL for zero; d_T_out == d_T_in
 *                  is allowed; d_T_out must not overlap anything else.
 *        program   n_regs <= 16 registers, imm[n_imm] base immediates (n_imm <= 256), ops[n_ops] (n_ops <= 4096), one uint64_t
 *                  per op: bits 0-7 the opcode, 8-15 dst, 16-39 operand a, 40-63 operand b.  An operand is 24 bits: bits 0-3 its
 *                  kind, 4-11 its index, 12-23 rot, a signed 12-bit number.
 *                    operand kinds   0 REG   register `index`
 *                                    1 BASE  base column `index` at row (i + rot B) mod M
 *                                    2 EXT   extension column `index` at row (i + rot B) mod M
 *                                    3 CHAL  challenge `index`
 *                                    4 IMM   immediate `index`
 *                                    5 X     the point x_i as a base element (index 0)
 *                                    6 PER   periodic column `index` (below), a base element
 *                                    rot is 0 for every kind but BASE, EXT and PER, and |rot| < N.
 *                    opcodes         0 MOV   dst <- a              (b is 0)
 *                                    1 ADD   dst <- a + b
 *                                    2 SUB   dst <- a - b
 *                                    3 MUL   dst <- a b
 *                                    4 NEG   dst <- -a             (b is 0)
 *                                    5 EMIT  constraint j (the raw 24 bits of b, j < J) has the value a and the kind dst
 *                  Every j is emitted exactly once, and a register is never read before it is written.  Every value is an
 *                  extension element, a base word v being (v, 0): that is the whole semantics.  ronk_air_create infers statically
 *                  which values are base elements (computed from BASE, IMM, X and such registers only) and runs base arithmetic on
 *                  them; that changes instruction counts, never a word of output.
 *        kinds     with w_l = w_N^(N-1) = w_N^-1, constraint j of value C_j adds to row i
 *                    0 ALL          (holds on every row of H)         lambda_j C_j / (x_i^N - 1)
 *                    1 FIRST        (holds on row 0)                  lambda_j C_j / (N (x_i - 1))
 *                    2 LAST         (holds on row N - 1)              lambda_j C_j w_l / (N (x_i - w_l))
 *                    3 EXCEPT_LAST  (holds on rows 0 .. N - 2)        lambda_j C_j (x_i - w_l) / (x_i^N - 1)
 *                  T_out_i = T_in_i + the sum of these, canonical.  FIRST is the P2 / S L1 convention of the two quotients above.
 *                  Degree is the caller's concern: T is a polynomial of degree below M only when every constraint's degree allows.
 *        periodic  n_per <= 16 columns that are part of the program, not inputs of a call: column k has the period
 *                  P = 2^log2_period[k] <= N and the values vals_k[0 .. P - 1]; per_values is the concatenation of the vals_k, any
 *                  64-bit words (reduced).  On H the column is vals_k[i mod P] at row i.  Its polynomial: with q_k of degree below P
 *                  and q_k(w_P^j) = vals_k[j], w_P = w_N^(N/P), the column is c_k(x) = q_k(x^(N/P)), of degree below N.  On the
 *                  coset, x_i w_N^rot = s w_M^(i + rot B) and (w_M^(N/P))^(P B) = 1, so the operand at row i with rotation rot is
 *                  tab_k[(i + rot B) mod (P B)] with tab_k[j] = q_k(s^(N/P) w_M^(j N/P)), j < P B.  P = 1 is a constant.  The handle
 *                  owns the tables, sum_k P_k B words of device memory built at creation (host integer arithmetic: the inverse
 *                  transform of vals_k over <w_P>, the scaling by s^(j N/P), the transform of length P B), and keeps the
 *                  coefficients of q_k on the host.  The verifier never needs a periodic column opened: ronk_air_cells does not
 *                  list PER operands, and ronk_air_eval_point evaluates q_k((z w_N^rot)^(N/P)) itself.  tests/air_per_ref.py
 *                  restates all of this and is normative for these words.
 *      ronk_air_check_per (host-side integer logic, no device), in this order; ronk_air_check is the case n_per = 0:
 *        1. RONK_ERR_INVALID      ops == NULL, n_columns == NULL with n_groups > 0, n_ops == 0, n_constraints == 0, some C_g == 0;
 *        2. RONK_ERR_UNSUPPORTED  a limit above is passed (n_groups, C_g, sum C_g, n_ext, n_chal, n_imm, n_regs, n_constraints,
 *                                 n_ops), log2_n < 1 or log2_n > 28;
 *        2a. RONK_ERR_UNSUPPORTED n_per > 16;
 *        2b. RONK_ERR_UNSUPPORTED some log2_period[k] > log2_n;
 *        2c. RONK_ERR_INVALID     log2_period == NULL with n_per > 0;
 *        3. RONK_ERR_INVALID      the first op, in program order, with an unknown opcode or operand kind, an index out of range
 *                                 (a register, a column, a challenge, an immediate, a periodic column: index >= n_per; X with an
 *                                 index; dst >= n_regs; an EMIT kind
 *                                 above 3), rot on an operand that is no column or |rot| >= N, b != 0 on MOV or NEG, a register
 *                                 read before it is written, an EMIT with j >= J or a j emitted before; at the end, a j never emitted.
 *      ronk_air_create_per gives these codes for the domain's log2_n, RONK_ERR_INVALID for a NULL out, domain or imm (with
 *      n_imm > 0) before them and for a NULL per_values (with n_per > 0) after them, and RONK_ERR_NO_DEVICE; ronk_air_create is
 *      the case n_per = 0.  The handle BORROWS the domain, which must outlive it; it owns the typed tape and the immediates in
 *      device memory.  ronk_air_quotient_dev: NULL pointers (d_T_in excepted; the arrays the program has none of excepted) are
 *      RONK_ERR_INVALID before any device work; asynchronous on `stream`: one kernel launch, no library workspace, no host round
 *      trip -- legal under stream capture.  ronk_air_quotient is the synchronous host-pointer form (base and ext: host arrays of
 *      host pointers).
 *      The verifier's side, host only: ronk_air_cells returns the number of distinct column cells the program reads and writes
 *      the first `cap` of them to `cells` (NULL with cap 0 to ask for the count) as 24-bit operands (kind, index, rot) in first-use
 *      order: cell k is what a verifier needs opened, column `index` at z w_N^rot.  ronk_air_eval_point runs the same program at
 *      the extension point z with X = z, cell k = cell_values[k] (a pair; chal and lambda are host arrays here), and returns the sum
 *      of the terms above with x_i replaced by z: what T(z) must equal.  RONK_ERR_INVALID for a NULL pointer or z^N = 1. */
typedef struct ronk_air ronk_air;
int ronk_air_check(uint32_t log2_n, uint32_t n_groups, const uint32_t* n_columns, uint32_t n_ext, uint32_t n_chal, uint32_t n_imm,
                   uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops, uint32_t n_ops);
int ronk_air_create(ronk_air** out, const ronk_plonk* domain, uint32_t n_groups, const uint32_t* n_columns, uint32_t n_ext,
                    uint32_t n_chal, uint32_t n_imm, uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops, uint32_t n_ops,
                    const uint64_t* imm);
int ronk_air_destroy(ronk_air* h);
int ronk_air_quotient_dev(const ronk_air* h, const uint64_t* const* d_base, const uint64_t* const* d_ext, const uint64_t* d_chal,
                          const uint64_t* d_lambda, const uint64_t* d_T_in, uint64_t* d_T_out, void* stream);
int ronk_air_quotient(const ronk_air* h, const uint64_t* const* base, const uint64_t* const* ext, const uint64_t* chal,
                      const uint64_t* lambda, const uint64_t* T_in, uint64_t* T_out);
uint32_t ronk_air_cells(const ronk_air* h, uint32_t* cells, uint32_t cap);
int ronk_air_eval_point(const ronk_air* h, const uint64_t z[2], const uint64_t* cell_values, const uint64_t* chal,
                        const uint64_t* lambda, uint64_t out[2]);

/* ---- STARK: trace columns into a proof and a proof into accept / reject, end to end on the device.  A ronk_stark handle joins the
 *      stages above -- the low-degree extension, the Merkle commitment, the constraint-program quotient, the multi-matrix
 *      commitment with its one FRI -- under one transcript, and adds the quotient split between them (csrc/stark_kernels.h).  The
 *      semantics are fixed here and restated on Python integers in tests/stark_ref.py, which is normative; the device reproduces
 *      it word for word.
 *        domain    that of a ronk_plonk handle: N = 2^log2_n trace rows, B = 2^log2_blowup, M = N B, x_i = s w_M^i, s^M != 1.  The
 *                  commitment domain is the SAME coset: the inner ronk_mpcs handle has log2_n = log2 M, coset_shift = s and
 *                  log2_blowup as given, so one extension of a trace round is both the committed matrix and the AIR's columns.
 *        rounds    R = n_rounds trace rounds, 1 <= R <= 4.  Round r is a [C_r][N] matrix of base words (below p) on H = <w_N>;
 *                  its last 2 E_r rows are the planes of E_r extension columns, c0 and c1 adjacent, so the pair is a planar
 *                  [2][M] array after extension.  The base part of round r (C_r - 2 E_r columns; none is allowed) is an AIR group,
 *                  the groups in round order; base column indices are flat across the rounds and extension columns are numbered
 *                  across the rounds in order.  The limits are those of ronk_air_check: sum of the base parts <= 64, sum E_r <= 8.
 *        challenges   the AIR's d_chal, n_chal <= 32 pairs: first the n_pub pairs the caller supplies (the public inputs), then the
 *                  n_draw[0] pairs drawn after round 0, then those after round 1, and so on; n_pub + sum n_draw[r] = n_chal.
 *        transcript   D = digest_len, sponge the handle's one-shot Poseidon sponge, squeezed words canonical.
 *                  t = sponge(seed[D] || pub as [n_pub][2] words) squeezing D words.  After the commitment of round r:
 *                  out = sponge(t || root_r) squeezing D + 2 n_draw[r] words, and two more for r = R - 1; t = out[:D], the draws
 *                  are the pairs that follow, and the extra last pair of round R - 1 is lambda.  The constraint weights are
 *                  lambda_j = lambda^j, j < J (lambda_0 = 1).
 *        quotient  T = ronk_air_quotient_dev on the extended rounds with T_in = NULL, planar [2][M].
 *        split     c_j (j < M): the monomial coefficients of T as extension elements, from the inverse transform of each plane
 *                  and the un-shift by s^-j.  Piece i < B is q_i(x) = sum_(k < N) c_(i N + k) x^k, so T(x) = sum_i x^(i N) q_i(x).
 *                  The quotient round is the [2 B][N] coefficient matrix, row 2 i + pl = plane pl of q_i, committed on the coset
 *                  like a trace round: it is round R of the inner commitment.
 *        points    after root_Q: out = sponge(t || root_Q) squeezing D + 2 words, t = out[:D], zeta = (out[D], out[D + 1]).
 *                  z_0 = zeta; for every distinct non-zero (rot mod N) in the order of ronk_air_cells, z_k = zeta w_N^(rot mod N).
 *                  K points, K <= 8.  The mask of trace round r: bit 0 and the bits of the rotations at which one of its columns
 *                  is read; the mask of the quotient round: bit 0.
 *        opening   ronk_mpcs_open_dev on the R + 1 rounds at z with seed t; its claims are the values of every round's
 *                  coefficient rows at the points of its mask (what ronk_ext2_poly_eval_batch_dev gives).
 *        proof     canonical words: the [R + 1][D] roots, then the inner handle's proof.
 *        verifier  rebuilds the transcript from seed, pub and the proof's roots, runs ronk_mpcs_verify_dev, then checks
 *                  sum_i zeta^(i N) (y_Q[2 i] + t y_Q[2 i + 1]) = ronk_air_eval_point(zeta, cells, chal, lambda_j), where cell
 *                  (BASE, flat index, rot) is that column's claim at the point of rot and cell (EXT, e, rot) is the c0-claim +
 *                  t times the c1-claim of its two rows.
 *        status    the inner bits 1 / 2 / 4 / 8 / 16 / 32 / 64 pass through; 128: zeta has a zero second word (such a zeta could
 *                  lie on a base-field domain: prover and verifier both set the bit and the proof is rejected; probability about
 *                  2^-64); 256: the out-of-domain identity fails, or cannot be evaluated because zeta^N = 1.  Every check runs
 *                  whatever the others find.  Degree is the caller's concern: a program whose degree exceeds what B allows, or a
 *                  trace that breaks a constraint, yields a proof that the verifier rejects with bit 256; the prover does not
 *                  detect it.
 *        fixed     n_fixed = C_F > 0 adds one preprocessed round: a [C_F][N] matrix of base words on H (no extension columns) that is
 *                  part of the statement -- selectors, a table, a ROM -- committed once, outside any proof, and bound to a handle by
 *                  its root.  It is AIR group 0: its columns take the flat base indices 0 .. C_F - 1 and the trace rounds follow;
 *                  the limits of ronk_air_check count it.  In the inner commitment it is round 0, the trace rounds are rounds
 *                  1 .. R and the quotient is round R + 1; its mask follows the rule of a trace round.  Transcript: after
 *                  t = sponge(seed || pub), t = sponge(t || root_F) squeezing D words (the step of a trace round with no draw),
 *                  then the rounds as above; the inner opening's root list starts with root_F.  The proof holds the [R + 1][D]
 *                  roots of the trace rounds and the quotient, then the inner proof on R + 2 rounds: it does NOT carry root_F, the
 *                  verifier uses its own, so a verifier that holds another root rejects with the bits the statuses above give
 *                  (no new bit).  The verifier maps a cell (BASE, index < C_F, rot) to the fixed round's claim.  The quotient
 *                  reads the fixed round's extension as d_base[0].  n_per periodic columns (log2_period, per_values) go to the
 *                  program through ronk_air_create_per ("constraint programs": periodic): they are never committed or opened.
 *                  tests/stark_fixed_ref.py restates this on top of tests/stark_ref.py and is normative for these words.
 *                    ronk_stark_fixed_words         the words of d_fixed: the extended matrix [C_F][M], the coefficients [C_F][N], the
 *                                                   tree (its last D words the root, as for every round), the coset-basis scratch
 *                                                   [C_F][N].  0 for a NULL handle or C_F = 0.  ronk_stark_workspace_words does not
 *                                                   count the fixed round.
 *                    ronk_stark_fixed_commit_dev    d_evals [C_F][N] into the caller-owned d_fixed: the steps of
 *                                                   ronk_stark_commit_round_dev without the draws; asynchronous, no host round trip.
 *                    ronk_stark_fixed_root_dev      the address of the root inside d_fixed (NULL for a NULL argument or C_F = 0).
 *                    ronk_stark_set_fixed_dev       the handle BORROWS the whole d_fixed: prover and verifier.
 *                    ronk_stark_set_fixed_root_dev  the handle borrows D words: a verifier; its prover stages are RONK_ERR_INVALID.
 *                  A setter replaces what an earlier one set and ends a sequence in flight.  With C_F > 0 and nothing set,
 *                  ronk_stark_begin_dev and ronk_stark_verify_dev return RONK_ERR_INVALID; with C_F = 0 the setters, the commit
 *                  and their host forms do.  ronk_stark_fixed_commit is the host-pointer form of the commit; ronk_stark_set_fixed
 *                  copies a host buffer of ronk_stark_fixed_words words (root_only != 0: the D words of a root) to device memory
 *                  that the handle then owns.
 *      ronk_stark_check_fixed (host integer logic, no device), in this order; ronk_stark_check and ronk_stark_create are the case
 *      n_fixed = n_per = 0, for which every word of every output is what it was without these arguments:
 *        1. the codes of ronk_air_check_per for the program on the groups above (the fixed round first) with n_ext = sum E_r, n_chal,
 *           n_per and log2_period as given;
 *        2. the codes of ronk_mpcs_check on the derived shape (log2 M, s, the blowup, K points, the R + 1 rounds and their masks,
 *           after the fixed round when there is one);
 *        3. the codes of ronk_plonk_check for the domain;
 *        4. RONK_ERR_INVALID for a NULL array, n_rounds = 0, some 2 E_r > C_r or n_pub + sum n_draw[r] != n_chal; then
 *           RONK_ERR_UNSUPPORTED for n_rounds > 4 or K > 8.
 *      Where step 4 would refuse the rounds, steps 1 to 3 run on what can be derived: the first four rounds, E_r clamped to
 *      C_r / 2, at most eight points, and no round at all for a NULL array.
 *      ronk_stark_create_fixed gives these codes, RONK_ERR_INVALID for a NULL out, pos or imm (with n_imm > 0) before them and for a
 *      NULL per_values (with n_per > 0) after them, and RONK_ERR_NO_DEVICE.
 *      The handle BORROWS pos, which must outlive it, and owns its ronk_plonk, ronk_air and ronk_mpcs handles and its transform
 *      plans.  ronk_stark_set_pow forwards to ronk_mpcs_set_pow; the size functions follow it and return 0 for a NULL handle.
 *        workspace caller-owned, ronk_stark_workspace_words words: t, the challenge table, lambda and the weights, zeta and the
 *                  points; per round (the quotient last) the extended matrix [C][M], the coefficients [C][N] and the tree; T;
 *                  the coset-basis scratch; the inner handle's workspace.
 *      The prover is staged, so that a caller can build accumulator columns from drawn challenges.  Every stage is asynchronous on
 *      `stream` with no host round trip; the trace words of a round are read, never written.
 *        ronk_stark_begin_dev          t from d_seed (D words) and d_pub ([n_pub][2] words; NULL with n_pub = 0); starts a sequence.
 *        ronk_stark_commit_round_dev   round r from d_evals ([C_r][N]): inverse transform, coset scaling, encode, tree, draws.
 *                                      Rounds go in order, 0 .. R - 1.
 *        ronk_stark_challenges_dev     the device address of the table in d_work ([n_chal][2] words; NULL for a NULL argument).  The
 *                                      challenges of round r are valid in stream order after its commit, and are usable directly
 *                                      as the d_alpha / d_beta / d_gamma of ronk_logup_sum_dev and ronk_perm_product_dev.
 *        ronk_stark_finish_dev         quotient, split, the quotient round, the points, the opening; d_proof receives
 *                                      ronk_stark_proof_words words, *d_status (device) 0 or the bits 32 and 128.
 *        ronk_stark_prove_dev          begin, commit round 0, finish, for R = 1 (else RONK_ERR_INVALID).
 *      One call sequence at a time per handle, on one workspace; a stage out of order, or on another workspace than begin's, is
 *      RONK_ERR_INVALID, and so is a NULL pointer.
 *      ronk_stark_verify_dev enqueues the transcript and the inner verifier on `stream`, synchronises the stream ONCE and runs the
 *      out-of-domain check on the host (ronk_air_eval_point is host-only): it is synchronous, *status is a HOST int, and it is not
 *      for stream capture.  ronk_stark_prove (R = 1) and ronk_stark_verify are the host-pointer forms; with grinding set,
 *      ronk_stark_prove returns RONK_ERR_INDEX when the search finds nothing, as ronk_mpcs_open does. */
typedef struct ronk_stark ronk_stark;
int ronk_stark_check(uint64_t p, uint32_t rate, uint64_t g, uint64_t w, uint32_t log2_n, uint32_t log2_blowup, uint64_t coset_shift,
                     uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len, uint32_t n_rounds,
                     const uint32_t* n_columns, const uint32_t* n_ext, uint32_t n_pub, const uint32_t* n_draw, uint32_t n_chal,
                     uint32_t n_imm, uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops, uint32_t n_ops);
int ronk_stark_create(ronk_stark** out, const ronk_poseidon* pos, uint64_t g, uint64_t w, uint32_t log2_n, uint32_t log2_blowup,
                      uint64_t coset_shift, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                      uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* n_ext, uint32_t n_pub, const uint32_t* n_draw,
                      uint32_t n_chal, uint32_t n_imm, uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops, uint32_t n_ops,
                      const uint64_t* imm);
int ronk_stark_destroy(ronk_stark* st);
int ronk_stark_set_pow(ronk_stark* st, uint32_t bits, uint32_t log2_limit);
size_t ronk_stark_proof_words(const ronk_stark* st);
size_t ronk_stark_workspace_words(const ronk_stark* st);
int ronk_stark_begin_dev(ronk_stark* st, const uint64_t* d_seed, const uint64_t* d_pub, uint64_t* d_work, void* stream);
int ronk_stark_commit_round_dev(ronk_stark* st, uint32_t round, const uint64_t* d_evals, uint64_t* d_work, void* stream);
const uint64_t* ronk_stark_challenges_dev(const ronk_stark* st, const uint64_t* d_work);
/* The split as a building block: d_c planar [2][M], the inverse transform of each plane of T (c'_j = c_j s^j); d_coef [2 B][N]
 * receives the pieces' coefficients c_(i N + k), d_msg [2 B][N] the same in the coset basis, c_(i N + k) s^k, which
 * ronk_rs_encode_batch_dev on an M-point plan of batch 2 B turns into the quotient matrix.  One launch; outputs must not overlap d_c. */
int ronk_stark_split_dev(const ronk_stark* st, const uint64_t* d_c, uint64_t* d_coef, uint64_t* d_msg, void* stream);
int ronk_stark_finish_dev(ronk_stark* st, uint64_t* d_work, uint64_t* d_proof, int* d_status, void* stream);
int ronk_stark_prove_dev(ronk_stark* st, const uint64_t* d_seed, const uint64_t* d_pub, const uint64_t* d_evals, uint64_t* d_work,
                         uint64_t* d_proof, int* d_status, void* stream);
int ronk_stark_verify_dev(ronk_stark* st, const uint64_t* d_seed, const uint64_t* d_pub, const uint64_t* d_proof, int* status,
                          void* stream);
int ronk_stark_prove(ronk_stark* st, const uint64_t* seed, const uint64_t* pub, const uint64_t* evals, uint64_t* proof, int* status);
int ronk_stark_verify(ronk_stark* st, const uint64_t* seed, const uint64_t* pub, const uint64_t* proof, int* status);

/* The entry points of the periodic columns ("constraint programs": periodic) and of the fixed round ("STARK": fixed), whose semantics
 * are stated above, are declared in a header of their own. */
#include "ronk_ntt_fixed.h"

/* ---- small device-memory helpers so a non-HIP host (ctypes, cgo, JNI) can stay device-resident ---- */
int ronk_dev_alloc(void** ptr, size_t bytes);
int ronk_dev_free(void* ptr);
int ronk_memcpy_h2d(void* dst, const void* src, size_t bytes);
int ronk_memcpy_d2h(void* dst, const void* src, size_t bytes);
int ronk_dev_sync(void);
/* The device the helpers above act on (the calling thread's current HIP device; plans carry their own ordinal).  A host that
 * places one block per GPU (device::DevicePoly of the Rust shim, the sharded transform's per-rank blocks) selects it around
 * every alloc / copy / free.  RONK_ERR_INVALID for an ordinal outside [0, ronk_device_count). */
int ronk_set_device(int device);
int ronk_get_device(int* device);
/* Releases the library's cached device workspace (the event-guarded buffer pool behind the Newton division, the fast
 * Reed-Solomon decode and the scans) once the work that used it has finished; buffers above 256 MiB are never cached.
 * Safe at any time; the next call that needs workspace allocates again. */
int ronk_trim_workspace(void);

#ifdef __cplusplus
}
#endif
#endif
