"""Stark: the ronk_stark handle (include/ronk_ntt.h "STARK") over an AirBuilder program -- trace columns into a proof and a proof
into accept / reject on the device.

    b = AirBuilder(); ...; program = b.assemble()
    st = Stark(sponge_params, g, w, log2_n, log2_blowup, coset_shift, log2_arity, log2_final, n_queries, digest_len,
               columns=(3,), n_ext=(0,), n_pub=2, n_draw=(0,), program=program)
    st.begin(d_seed, d_pub, d_work); st.commit_round(0, d_trace, d_work); st.finish(d_work, d_proof, d_status)
    status = st.verify(d_seed, d_pub, d_proof)

sponge_params = (field, width, alpha, num_p, num_f, rate, rc, mds) as for callers.MerkleTree.  The staged calls take torch tensors
of dtype int64 on the device (or raw device addresses) and enqueue on the current torch stream; between commit_round(r) and the
next stage, challenges(d_work) is the device address of the table, usable as the d_alpha of ronk_logup_sum_dev and its like.

With n_fixed > 0 the program's first n_fixed base columns are a preprocessed round that is part of the statement (selectors, a
table): fixed_commit / fixed_commit_dev build it once, outside any proof, and set_fixed binds it -- the whole buffer for a prover,
root_only=True and the root's words for a verifier.  periodic = one list of values per periodic column (AirBuilder.periodic), its
length the period: never committed, the verifier evaluates them itself.
There is no CPU path: without the library's device every call raises RonkPanic."""
import ctypes as C

from . import _lib as L


def _address(t):
    return None if t is None else t.data_ptr() if hasattr(t, "data_ptr") else int(t)


def _stream(stream):
    if stream is not None:
        return stream
    try:
        import torch
        return torch.cuda.current_stream().cuda_stream
    except Exception:  # noqa: BLE001  (no torch: the null stream)
        return 0


class Stark:
    def __init__(self, sponge_params, g, w, log2_n, log2_blowup, coset_shift, log2_arity, log2_final, n_queries, digest_len, columns, n_ext,
                 n_pub, n_draw, program, pow_bits=0, pow_log2_limit=None, n_fixed=0, periodic=()):
        """columns[r] rows in trace round r, the last 2 n_ext[r] of them the planes of extension columns; n_pub public pairs, then
        n_draw[r] pairs drawn after round r; program = (ops, imm, n_regs, n_constraints) as AirBuilder.assemble() gives it; n_fixed
        columns of the fixed round; periodic the values of the periodic columns"""
        field = sponge_params[0]
        ops, imm, n_regs, n_constraints = program
        if not (len(columns) == len(n_ext) == len(n_draw)):
            raise L.RonkPanic(L.ERR_INVALID, "columns, n_ext and n_draw have one entry per trace round")
        p = field.ORDER
        self.p, self.log2_n, self.log2_blowup, self.digest_len = p, log2_n, log2_blowup, digest_len
        self.columns, self.n_ext, self.n_pub, self.n_draw = tuple(columns), tuple(n_ext), n_pub, tuple(n_draw)
        self.n_chal = n_pub + sum(n_draw)
        self.n_fixed = n_fixed
        from .callers import periodic_arrays
        n_per, log2_period, per_values = periodic_arrays(periodic)
        self.poseidon = L.PoseidonHandle(p, *sponge_params[1:])
        a_ops, a_imm = L.arr([int(v) for v in ops]), L.arr([int(v) % p for v in imm])
        u32 = lambda v: (C.c_uint32 * max(1, len(v)))(*v)      # noqa: E731
        self.h = C.c_void_p()
        try:
            common = (C.byref(self.h), self.poseidon.h, g, w, log2_n, log2_blowup, coset_shift, log2_arity, log2_final, n_queries, digest_len,
                      len(columns), u32(columns), u32(n_ext), n_pub, u32(n_draw), self.n_chal, a_imm.size, n_regs, n_constraints, L.ptr(a_ops),
                      a_ops.size, L.ptr(a_imm) if a_imm.size else None)
            if n_fixed or n_per:
                L.check(L.lib.ronk_stark_create_fixed(*common, n_fixed, n_per, log2_period if n_per else None,
                                                      L.ptr(per_values) if n_per else None))
            else:
                L.check(L.lib.ronk_stark_create(*common))
            if pow_bits:
                L.check(L.lib.ronk_stark_set_pow(self.h, pow_bits, L.pow_default_limit(p, pow_bits) if pow_log2_limit is None else pow_log2_limit))
        except Exception:
            self.close()
            raise

    @property
    def proof_words(self):
        return L.lib.ronk_stark_proof_words(self.h)

    @property
    def workspace_words(self):
        return L.lib.ronk_stark_workspace_words(self.h)

    @property
    def fixed_words(self):
        """the words of the fixed round's buffer (0 without a fixed round)"""
        return L.lib.ronk_stark_fixed_words(self.h)

    @property
    def fixed_root_offset(self):
        """where the root's digest_len words lie in the fixed round's buffer"""
        at = 1 << 20
        return (L.lib.ronk_stark_fixed_root_dev(self.h, at) - at) // 8

    # ---- the fixed round: once, outside any proof
    def fixed_commit_dev(self, d_evals, d_fixed, stream=None):
        """d_evals [n_fixed][N] into the caller's d_fixed of fixed_words words; asynchronous"""
        L.check(L.lib.ronk_stark_fixed_commit_dev(self.h, _address(d_evals), _address(d_fixed), _stream(stream)))

    def fixed_root(self, d_fixed):
        """the device address of the root inside d_fixed"""
        return L.lib.ronk_stark_fixed_root_dev(self.h, _address(d_fixed))

    def fixed_commit(self, evals):
        """host columns [n_fixed][N] -> the buffer as a host array of fixed_words words"""
        import numpy as np
        e = L.arr(evals).ravel()
        if not self.n_fixed or e.size != self.n_fixed << self.log2_n:
            raise L.RonkPanic(L.ERR_INVALID, "the fixed round is [n_fixed][N]")
        out = np.empty(self.fixed_words, dtype=np.uint64)
        L.check(L.lib.ronk_stark_fixed_commit(self.h, L.ptr(e), L.ptr(out)))
        return out

    def set_fixed(self, fixed, root_only=False):
        """binds the fixed round: a host array (copied; the handle owns the copy) or a device tensor or address (borrowed, it must
        outlive the handle's use of it).  root_only: `fixed` is the digest_len words of the root, which serves a verifier only"""
        import numpy as np
        if isinstance(fixed, (np.ndarray, list, tuple)):
            a = L.arr(fixed).ravel()
            if a.size != (self.digest_len if root_only else self.fixed_words):
                raise L.RonkPanic(L.ERR_INVALID, "the buffer of fixed_commit, or the digest_len words of its root")
            L.check(L.lib.ronk_stark_set_fixed(self.h, L.ptr(a), 1 if root_only else 0))
        elif root_only:
            L.check(L.lib.ronk_stark_set_fixed_root_dev(self.h, _address(fixed)))
        else:
            L.check(L.lib.ronk_stark_set_fixed_dev(self.h, _address(fixed)))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            L.lib.ronk_stark_destroy(self.h)
        self.h = None
        if getattr(self, "poseidon", None) is not None:
            self.poseidon.close()
            self.poseidon = None

    def __del__(self):
        self.close()

    # ---- the staged prover, device tensors
    def begin(self, d_seed, d_pub, d_work, stream=None):
        L.check(L.lib.ronk_stark_begin_dev(self.h, _address(d_seed), _address(d_pub), _address(d_work), _stream(stream)))

    def commit_round(self, r, d_evals, d_work, stream=None):
        L.check(L.lib.ronk_stark_commit_round_dev(self.h, r, _address(d_evals), _address(d_work), _stream(stream)))

    def challenges(self, d_work):
        """the device address of the challenge table [n_chal][2] inside the workspace"""
        return L.lib.ronk_stark_challenges_dev(self.h, _address(d_work))

    def split(self, d_c, d_coef, d_msg, stream=None):
        """the quotient split alone (ronk_stark_split_dev): planar [2][M] -> the pieces' coefficients and their coset-basis form"""
        L.check(L.lib.ronk_stark_split_dev(self.h, _address(d_c), _address(d_coef), _address(d_msg), _stream(stream)))

    def finish(self, d_work, d_proof, d_status, stream=None):
        L.check(L.lib.ronk_stark_finish_dev(self.h, _address(d_work), _address(d_proof), _address(d_status), _stream(stream)))

    def prove_dev(self, d_seed, d_pub, d_evals, d_work, d_proof, d_status, stream=None):
        """one trace round: begin, commit round 0, finish"""
        L.check(L.lib.ronk_stark_prove_dev(self.h, _address(d_seed), _address(d_pub), _address(d_evals), _address(d_work), _address(d_proof),
                                           _address(d_status), _stream(stream)))

    def verify_dev(self, d_seed, d_pub, d_proof, stream=None):
        """-> the status: 0 accepts.  Synchronises the stream once"""
        st = C.c_int(-1)
        L.check(L.lib.ronk_stark_verify_dev(self.h, _address(d_seed), _address(d_pub), _address(d_proof), C.byref(st), _stream(stream)))
        return st.value

    # ---- host arrays
    def prove(self, seed, pub, trace):
        """one trace round [C_0][N] -> (the proof, the prover's status); RonkPanic(ERR_INDEX) when the grind finds no nonce"""
        import numpy as np
        s, t = L.arr([int(v) for v in seed]), L.arr(trace).ravel()
        pw = L.arr([int(c) for pair in pub for c in pair])
        if s.size != self.digest_len or pw.size != 2 * self.n_pub or len(self.columns) != 1 or t.size != self.columns[0] << self.log2_n:
            raise L.RonkPanic(L.ERR_INVALID, "a seed of digest_len words, n_pub pairs, one trace round [C_0][N]")
        proof, st = np.empty(self.proof_words, dtype=np.uint64), C.c_int(-1)
        L.check(L.lib.ronk_stark_prove(self.h, L.ptr(s), L.ptr(pw) if pw.size else None, L.ptr(t), L.ptr(proof), C.byref(st)))
        return proof, st.value

    def verify(self, seed, pub, proof):
        s, pr = L.arr([int(v) for v in seed]), L.arr(proof)
        pw = L.arr([int(c) for pair in pub for c in pair])
        if s.size != self.digest_len or pw.size != 2 * self.n_pub or pr.size != self.proof_words:
            raise L.RonkPanic(L.ERR_INVALID, "a seed of digest_len words, n_pub pairs, a proof of proof_words words")
        st = C.c_int(-1)
        L.check(L.lib.ronk_stark_verify(self.h, L.ptr(s), L.ptr(pw) if pw.size else None, L.ptr(pr), C.byref(st)))
        return st.value
