/* ronk_ntt_fixed.h -- part of include/ronk_ntt.h, which includes it: the entry points of the periodic columns of a constraint
 * program and of the fixed (preprocessed) round of the STARK.  Their semantics, codes and orders are stated in ronk_ntt.h, in the
 * sections "constraint programs" (periodic) and "STARK" (fixed), beside the entry points they extend; this file holds the
 * prototypes alone.  Every earlier entry point of the two families is the case of no periodic column and no fixed round, and
 * its outputs are word for word what they were. */
#ifndef RONK_NTT_FIXED_H
#define RONK_NTT_FIXED_H
#ifndef RONK_NTT_H
#error "include ronk_ntt.h, which includes this file"
#endif

/* ronk_air_check and ronk_air_create followed by n_per, log2_period[n_per] (and per_values: the concatenation of the 2^log2_period[k]
 * values of every column). */
int ronk_air_check_per(uint32_t log2_n, uint32_t n_groups, const uint32_t* n_columns, uint32_t n_ext, uint32_t n_chal, uint32_t n_imm,
                       uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops, uint32_t n_ops, uint32_t n_per,
                       const uint32_t* log2_period);
int ronk_air_create_per(ronk_air** out, const ronk_plonk* domain, uint32_t n_groups, const uint32_t* n_columns, uint32_t n_ext,
                        uint32_t n_chal, uint32_t n_imm, uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops, uint32_t n_ops,
                        const uint64_t* imm, uint32_t n_per, const uint32_t* log2_period, const uint64_t* per_values);

/* ronk_stark_check and ronk_stark_create followed by n_fixed, n_per, log2_period (and per_values). */
int ronk_stark_check_fixed(uint64_t p, uint32_t rate, uint64_t g, uint64_t w, uint32_t log2_n, uint32_t log2_blowup,
                           uint64_t coset_shift, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                           uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* n_ext, uint32_t n_pub, const uint32_t* n_draw,
                           uint32_t n_chal, uint32_t n_imm, uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops, uint32_t n_ops,
                           uint32_t n_fixed, uint32_t n_per, const uint32_t* log2_period);
int ronk_stark_create_fixed(ronk_stark** out, const ronk_poseidon* pos, uint64_t g, uint64_t w, uint32_t log2_n, uint32_t log2_blowup,
                            uint64_t coset_shift, uint32_t log2_arity, uint32_t log2_final, uint32_t n_queries, uint32_t digest_len,
                            uint32_t n_rounds, const uint32_t* n_columns, const uint32_t* n_ext, uint32_t n_pub, const uint32_t* n_draw,
                            uint32_t n_chal, uint32_t n_imm, uint32_t n_regs, uint32_t n_constraints, const uint64_t* ops, uint32_t n_ops,
                            const uint64_t* imm, uint32_t n_fixed, uint32_t n_per, const uint32_t* log2_period,
                            const uint64_t* per_values);
/* The fixed round: preprocessing into a caller-owned buffer, once and outside any proof, and its binding to a handle. */
size_t ronk_stark_fixed_words(const ronk_stark* st);
int ronk_stark_fixed_commit_dev(const ronk_stark* st, const uint64_t* d_evals, uint64_t* d_fixed, void* stream);
const uint64_t* ronk_stark_fixed_root_dev(const ronk_stark* st, const uint64_t* d_fixed);
int ronk_stark_set_fixed_dev(ronk_stark* st, const uint64_t* d_fixed);
int ronk_stark_set_fixed_root_dev(ronk_stark* st, const uint64_t* d_root);
int ronk_stark_fixed_commit(const ronk_stark* st, const uint64_t* evals, uint64_t* fixed);
int ronk_stark_set_fixed(ronk_stark* st, const uint64_t* fixed, int root_only);

#endif
