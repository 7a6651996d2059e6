"""ctypes binding of ronkathon_amd/libronk_ntt.so (the C ABI in include/ronk_ntt.h).

There is no CPU implementation behind this module: if the shared library is missing it
raises at import, and without a HIP device every compute call raises RonkPanic(-10).
"""
import ctypes as C
import os

import numpy as np

# PyTorch-ROCm wheels bundle their own HIP/HSA runtime.  In a process that uses both, torch's copy has to be
# mapped BEFORE the system runtime this library links against (the other order leaves torch with "No HIP GPUs
# are available" -- measured on ROCm 7.2 + torch 2.10/rocm7.0).  So: import torch first when it is installed.
# The library itself never calls into torch; callers hand it raw device pointers and hipStream_t values.
try:
    import torch  # noqa: F401
except Exception:  # noqa: BLE001  (no torch: nothing to order)
    pass

_HERE = os.path.dirname(os.path.abspath(__file__))
# RONK_LIB_PATH: developer A/B runs against another build of the SAME C ABI (e.g. last round's .so on the same box)
LIB_PATH = os.environ.get("RONK_LIB_PATH") or os.path.join(_HERE, "libronk_ntt.so")

GOLDILOCKS_P = 0xFFFFFFFF00000001
GOLDILOCKS_G = 7

OK, ERR_NO_ROOT, ERR_ZERO_INVERSE, ERR_NOT_POW2, ERR_NOT_PRIME = 0, -1, -2, -3, -4
ERR_NO_GENERATOR, ERR_INDEX, ERR_INVALID, ERR_HIP, ERR_UNSUPPORTED, ERR_NO_DEVICE = -5, -6, -7, -8, -9, -10
ERR_NOT_ON_CURVE = -11
ERR_RCCL = -12
ERR_NOT_RESIDUE = -13
ERR_NOT_CODEWORD = -14
ROOTS_LEAF = 64   # RONK_ROOTS_LEAF: factors per leaf of the product tree (ronk_poly_from_roots)
EXCHANGE_MESH, EXCHANGE_RCCL = 0, 1


class RonkPanic(Exception):
    """A non-zero return code: what the reference reports by panicking (same message text)."""

    def __init__(self, code, detail=""):
        msg = lib.ronk_strerror(code).decode()
        if code in (ERR_HIP, ERR_RCCL):
            msg += ": " + lib.ronk_last_hip_error().decode()
        super().__init__(msg + (" " + detail if detail else ""))
        self.code = code


if not os.path.exists(LIB_PATH):
    raise ImportError(
        "ronkathon_amd: %s not found -- build the HIP extension first (`make` at the repo root or "
        "`python -c 'import __graft_entry__ as g; g.build()'`).  There is no CPU fallback." % LIB_PATH)

lib = C.CDLL(LIB_PATH)

_u64, _sz, _pu, _vp, _int = C.c_uint64, C.c_size_t, C.POINTER(C.c_uint64), C.c_void_p, C.c_int
_SIG = {
    "ronk_strerror": (C.c_char_p, [_int]),
    "ronk_last_hip_error": (C.c_char_p, []),
    "ronk_device_count": (_int, [C.POINTER(_int)]),
    "ronk_primitive_element": (_int, [_u64, _pu]),
    "ronk_root_of_unity": (_int, [_u64, _u64, _u64, _pu]),
    "ronk_check_prime": (_int, [_u64]),
    "ronk_vec_add": (_int, [_u64, _vp, _vp, _vp, _sz]),
    "ronk_vec_sub": (_int, [_u64, _vp, _vp, _vp, _sz]),
    "ronk_vec_mul": (_int, [_u64, _vp, _vp, _vp, _sz]),
    "ronk_vec_neg": (_int, [_u64, _vp, _vp, _sz]),
    "ronk_vec_inv": (_int, [_u64, _vp, _vp, _sz]),
    "ronk_vec_pow": (_int, [_u64, _vp, _u64, _vp, _sz]),
    "ronk_vec_euler": (_int, [_u64, _vp, _vp, _sz]),
    "ronk_vec_sqrt": (_int, [_u64, _vp, _vp, _vp, _sz]),
    "ronk_vec_euler_dev": (_int, [_u64, _vp, _vp, _sz, _vp]),
    "ronk_vec_sqrt_dev": (_int, [_u64, _vp, _vp, _vp, _sz, _vp, _vp]),
    "ronk_vec_add_dev": (_int, [_u64, _vp, _vp, _vp, _sz, _vp]),
    "ronk_vec_sub_dev": (_int, [_u64, _vp, _vp, _vp, _sz, _vp]),
    "ronk_vec_mul_dev": (_int, [_u64, _vp, _vp, _vp, _sz, _vp]),
    "ronk_plan_create": (_int, [C.POINTER(_vp), _u64, _u64, C.c_uint32, _u64, _int]),
    "ronk_plan_create_tuned": (_int, [C.POINTER(_vp), _u64, _u64, C.c_uint32, _u64, _int, _int, _int]),
    "ronk_plan_create_opts": (_int, [C.POINTER(_vp), _u64, _u64, C.c_uint32, _u64, _int, _vp]),
    "ronk_plan_in_flight": (_int, [_vp]),
    "ronk_ntt_forward_many_dev": (_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), _sz, _vp]),
    "ronk_ntt_inverse_many_dev": (_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), _sz, _vp]),
    "ronk_plan_destroy": (_int, [_vp]),
    "ronk_plan_path": (_int, [_vp]),
    "ronk_ntt_forward": (_int, [_vp, _vp, _vp, _vp]),
    "ronk_ntt_inverse": (_int, [_vp, _vp, _vp]),
    "ronk_ntt_forward_dev": (_int, [_vp, _vp, _vp, _vp]),
    "ronk_ntt_inverse_dev": (_int, [_vp, _vp, _vp, _vp]),
    "ronk_lagrange_nodes": (_int, [_u64, _u64, _vp, _sz]),
    "ronk_fft": (_int, [_u64, _u64, _vp, _vp, _vp, _sz]),
    "ronk_ifft": (_int, [_u64, _u64, _vp, _vp, _sz]),
    "ronk_dft": (_int, [_u64, _u64, _vp, _vp, _sz]),
    "ronk_plan_num_passes": (_int, [_vp]),
    "ronk_plan_time_passes": (_int, [_vp, _vp, _vp, _int, _int, C.POINTER(C.c_float), _vp]),
    "ronk_poly_mul": (_int, [_u64, _u64, _vp, _sz, _vp, _sz, _vp]),
    "ronk_poly_mul_dev": (_int, [_u64, _u64, _vp, _sz, _vp, _sz, _vp, _vp]),
    "ronk_poly_add": (_int, [_u64, _vp, _sz, _vp, _sz, _vp]),
    "ronk_poly_sub": (_int, [_u64, _vp, _sz, _vp, _sz, _vp]),
    "ronk_poly_eval": (_int, [_u64, _vp, _sz, _u64, _pu]),
    "ronk_poly_eval_dev": (_int, [_u64, _vp, _sz, _u64, _vp, _vp]),
    "ronk_poly_div_linear_dev": (_int, [_u64, _vp, _sz, _u64, _u64, _vp, _vp, _vp]),
    "ronk_lagrange_eval": (_int, [_u64, _vp, _vp, _sz, _u64, _pu]),
    "ronk_poly_divrem": (_int, [_u64, _vp, _sz, _vp, _sz, _vp, _vp]),
    "ronk_rs_encode": (_int, [_u64, _u64, _vp, _sz, _sz, _vp, _vp]),
    "ronk_rs_decode": (_int, [_u64, _vp, _vp, _sz, _vp]),
    "ronk_rs_encode_batch_dev": (_int, [_vp, _vp, _sz, _vp, _vp]),
    "ronk_poly_from_roots": (_int, [_u64, _vp, _sz, _vp]),
    "ronk_poly_from_roots_dev": (_int, [_u64, _vp, _sz, _vp, _vp]),
    "ronk_poly_eval_many": (_int, [_u64, _vp, _sz, _vp, _sz, _vp]),
    "ronk_poly_eval_many_dev": (_int, [_u64, _vp, _sz, _vp, _sz, _vp, _vp]),
    "ronk_poly_interpolate": (_int, [_u64, _vp, _vp, _sz, _vp]),
    "ronk_poly_interpolate_dev": (_int, [_u64, _vp, _vp, _sz, _vp, _vp, _vp]),
    "ronk_rs_recover_batch_dev": (_int, [_vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "ronk_rs_recover": (_int, [_u64, _u64, _sz, _sz, _vp, _sz, _vp, _vp, _vp]),
    "ronk_lde_batch_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "ronk_curve_msm": (_int, [_vp, _vp, _sz, _vp, _sz, _vp]),
    "ronk_msm_bn254": (_int, [_vp, _vp, _sz, _vp]),
    "ronk_msm_bn254_dev": (_int, [_vp, _vp, _sz, _vp, _vp]),
    "ronk_bn254_probe_dev": (_int, [_int, _vp, _vp, _vp, _sz, _vp]),   # test hook (csrc/bn254_probe.h)
    "ronk_poly_div_linear_bn254_dev": (_int, [_vp, _sz, _vp, _vp, _vp, _vp]),
    "ronk_kzg_open_bn254_dev": (_int, [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ronk_kzg_open_bn254": (_int, [_vp, _sz, _vp, _vp, _sz, _vp, _vp]),
    "ronk_root_of_unity_bn254": (_int, [C.c_uint32, _vp]),
    "ronk_plan_create_bn254": (_int, [C.POINTER(_vp), C.c_uint32, C.c_uint32]),
    "ronk_plan_info_bn254": (_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ronk_plan_reserve_bn254": (_int, [_vp, _sz]),
    "ronk_plan_destroy_bn254": (_int, [_vp]),
    "ronk_ntt_forward_bn254_dev": (_int, [_vp, _vp, _vp, _sz, _vp]),
    "ronk_ntt_inverse_bn254_dev": (_int, [_vp, _vp, _vp, _sz, _vp]),
    "ronk_ntt_forward_bn254": (_int, [C.c_uint32, _vp, _vp]),
    "ronk_ntt_inverse_bn254": (_int, [C.c_uint32, _vp, _vp]),
    "ronk_poly_mul_bn254_dev": (_int, [_vp, _sz, _vp, _sz, _vp, _vp]),
    "ronk_poly_mul_bn254": (_int, [_vp, _sz, _vp, _sz, _vp]),
    "ronk_dist_plan_create": (_int, [C.POINTER(_vp), C.c_uint32, _int, _int, _int, _int]),
    "ronk_dist_plan_destroy": (_int, [_vp]),
    "ronk_dist_plan_create_chunked": (_int, [C.POINTER(_vp), C.c_uint32, _int, _int, _int, _int, _int]),
    "ronk_dist_plan_create_p": (_int, [C.POINTER(_vp), _u64, _u64, C.c_uint32, _int, _int, _int, _int, _int]),
    "ronk_dist_phase1_chunk_dev": (_int, [_vp, _int, _vp, _vp, _vp]),
    "ronk_dist_phase1_dev": (_int, [_vp, _vp, _vp, _vp]),
    "ronk_dist_phase2_dev": (_int, [_vp, _vp, _vp, _vp]),
    "ronk_vec_neg_dev": (_int, [_u64, _vp, _vp, _sz, _vp]),
    "ronk_vec_pow_dev": (_int, [_u64, _vp, _u64, _vp, _sz, _vp]),
    "ronk_vec_inv_dev": (_int, [_u64, _vp, _vp, _sz, _vp, _vp]),
    "ronk_dft_dev": (_int, [_u64, _u64, _vp, _vp, _sz, _vp]),
    "ronk_lagrange_eval_dev": (_int, [_u64, _vp, _vp, _sz, _u64, _vp, _vp, _vp]),
    "ronk_poly_divrem_dev": (_int, [_u64, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp]),
    "ronk_poly_divrem_full_dev": (_int, [_u64, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp]),
    "ronk_rs_decode_dev": (_int, [_u64, _vp, _vp, _sz, _vp, _vp, _vp]),
    "ronk_curve_msm_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "ronk_sharded_plan_create": (_int, [C.POINTER(_vp), C.c_uint32, _int, C.POINTER(_int), _int, _int]),
    "ronk_sharded_plan_create_ex": (_int, [C.POINTER(_vp), C.c_uint32, _int, C.POINTER(_int), _int, _int, _int]),
    "ronk_sharded_time_stages": (_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_float)]),
    "ronk_sharded_plan_create_p": (_int, [C.POINTER(_vp), _u64, _u64, C.c_uint32, _int, C.POINTER(_int), _int, _int, _int]),
    "ronk_sharded_plan_exchange": (_int, [_vp]),
    "ronk_sharded_plan_peer_access": (_int, [_vp, C.POINTER(_int), _int]),
    "ronk_sharded_plan_destroy": (_int, [_vp]),
    "ronk_sharded_plan_info": (_int, [_vp, _pu, _pu, _pu, C.POINTER(_int)]),
    "ronk_ntt_sharded_dev": (_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "ronk_sharded_sync": (_int, [_vp]),
    "ronk_ntt_sharded": (_int, [_vp, _vp, _vp]),
    "ronk_sharded_mul_plan_create_p": (_int, [C.POINTER(_vp), _u64, _u64, C.c_uint32, C.POINTER(_int), _int, _int, _int, _int]),
    "ronk_sharded_mul_plan_create": (_int, [C.POINTER(_vp), C.c_uint32, C.POINTER(_int), _int, _int, _int, _int]),
    "ronk_sharded_mul_plan_info": (_int, [_vp, _pu, _pu, _pu, C.POINTER(_int), C.POINTER(_int)]),
    "ronk_sharded_mul_plan_destroy": (_int, [_vp]),
    "ronk_poly_mul_sharded_dev": (_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "ronk_sharded_mul_sync": (_int, [_vp]),
    "ronk_poly_mul_sharded": (_int, [_vp, _vp, _sz, _vp, _sz, _vp]),
    "ronk_poseidon_create": (_int, [C.POINTER(_vp), _u64, C.c_uint32, _u64, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]),
    "ronk_poseidon_destroy": (_int, [_vp]),
    "ronk_poseidon_permute_dev": (_int, [_vp, _vp, _sz, _vp]),
    "ronk_poseidon_hash": (_int, [_vp, _vp, _sz, _vp]),
    "ronk_poseidon_sponge_dev": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp]),
    "ronk_merkle_tree_words": (_sz, [_sz, _sz]),
    "ronk_merkle_level_offset": (_sz, [_sz, _sz, _sz]),
    "ronk_merkle_commit_dev": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _sz, _vp, _vp]),
    "ronk_merkle_open_dev": (_int, [_vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp]),
    "ronk_merkle_verify_dev": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "ronk_merkle_commit": (_int, [_vp, _vp, _sz, _sz, _sz, _vp]),
    "ronk_merkle_open": (_int, [_vp, _sz, _sz, _vp, _sz, _vp, _vp]),
    "ronk_merkle_verify": (_int, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _vp, _vp]),
    "ronk_fri_check": (_int, [_u64, C.c_uint32, _u64, C.c_uint32, _u64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "ronk_fri_proof_words": (_sz, [C.c_uint32] * 5),
    "ronk_fri_workspace_words": (_sz, [C.c_uint32] * 5),
    "ronk_fri_create": (_int, [C.POINTER(_vp), _vp, _u64, C.c_uint32, _u64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "ronk_fri_destroy": (_int, [_vp]),
    "ronk_fri_fold_dev": (_int, [_vp, C.c_uint32, _vp, _vp, _vp, _vp]),
    "ronk_fri_prove_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "ronk_fri_verify_dev": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "ronk_fri_prove": (_int, [_vp, _vp, _vp, _vp]),
    "ronk_fri_verify": (_int, [_vp, _vp, _vp, C.POINTER(_int)]),
    "ronk_fri_check_ext": (_int, [_u64, C.c_uint32, _u64, _u64, C.c_uint32, _u64] + [C.c_uint32] * 6),
    "ronk_fri_proof_words_ext": (_sz, [C.c_uint32] * 6),
    "ronk_fri_workspace_words_ext": (_sz, [C.c_uint32] * 6),
    "ronk_fri_create_ext": (_int, [C.POINTER(_vp), _vp, _u64, _u64, C.c_uint32, _u64] + [C.c_uint32] * 6),
    "ronk_fri_query_indices_dev": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "ronk_pcs_check": (_int, [_u64, C.c_uint32, _u64, _u64, C.c_uint32, _u64] + [C.c_uint32] * 7),
    "ronk_pcs_proof_words": (_sz, [C.c_uint32] * 7),
    "ronk_pcs_workspace_words": (_sz, [C.c_uint32] * 7),
    "ronk_pcs_create": (_int, [C.POINTER(_vp), _vp, _u64, _u64, C.c_uint32, _u64] + [C.c_uint32] * 7),
    "ronk_pcs_destroy": (_int, [_vp]),
    "ronk_ext2_poly_eval_batch_dev": (_int, [_u64, _u64, _vp, C.c_uint32, _sz, _vp, C.c_uint32, _vp, _vp]),
    "ronk_ext2_poly_eval_batch": (_int, [_u64, _u64, _vp, C.c_uint32, _sz, _vp, C.c_uint32, _vp]),
    "ronk_deep_combine_dev": (_int, [_vp] * 8),
    "ronk_pcs_commit_dev": (_int, [_vp, _vp, _vp, _vp]),
    "ronk_pcs_open_dev": (_int, [_vp] * 10),
    "ronk_pcs_verify_dev": (_int, [_vp] * 7),
    "ronk_pcs_commit": (_int, [_vp, _vp, _vp]),
    "ronk_pcs_open": (_int, [_vp] * 7 + [C.POINTER(_int)]),
    "ronk_pcs_verify": (_int, [_vp] * 5 + [C.POINTER(_int)]),
    "ronk_pow_check": (_int, [_u64, C.c_uint32, _sz, C.c_uint32, C.c_uint32]),
    "ronk_pow_workspace_words": (_sz, []),
    "ronk_pow_grind_dev": (_int, [_vp, _vp, _sz, C.c_uint32, C.c_uint32, _sz, _vp, _vp, _vp]),
    "ronk_pow_verify_dev": (_int, [_vp, _vp, _sz, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "ronk_pow_grind": (_int, [_vp, _vp, _sz, C.c_uint32, C.c_uint32, _sz, _pu]),
    "ronk_pow_verify": (_int, [_vp, _vp, _sz, C.c_uint32, C.c_uint32, _u64, C.POINTER(_int)]),
    "ronk_fri_set_pow": (_int, [_vp, C.c_uint32, C.c_uint32]),
    "ronk_fri_handle_proof_words": (_sz, [_vp]),
    "ronk_fri_handle_workspace_words": (_sz, [_vp]),
    "ronk_pcs_set_pow": (_int, [_vp, C.c_uint32, C.c_uint32]),
    "ronk_pcs_handle_proof_words": (_sz, [_vp]),
    "ronk_pcs_handle_workspace_words": (_sz, [_vp]),
    "ronk_mpcs_check": (_int, [_u64, C.c_uint32, _u64, _u64, C.c_uint32, _u64] + [C.c_uint32] * 7 + [_vp, _vp]),
    "ronk_mpcs_proof_words": (_sz, [C.c_uint32] * 7 + [_vp, _vp]),
    "ronk_mpcs_workspace_words": (_sz, [C.c_uint32] * 7 + [_vp, _vp]),
    "ronk_mpcs_create": (_int, [C.POINTER(_vp), _vp, _u64, _u64, C.c_uint32, _u64] + [C.c_uint32] * 7 + [_vp, _vp]),
    "ronk_mpcs_destroy": (_int, [_vp]),
    "ronk_mpcs_set_pow": (_int, [_vp, C.c_uint32, C.c_uint32]),
    "ronk_mpcs_handle_proof_words": (_sz, [_vp]),
    "ronk_mpcs_handle_workspace_words": (_sz, [_vp]),
    "ronk_mpcs_commit_dev": (_int, [_vp, C.c_uint32, _vp, _vp, _vp]),
    "ronk_mpcs_combine_dev": (_int, [_vp] * 8),
    "ronk_mpcs_open_dev": (_int, [_vp] * 10),
    "ronk_mpcs_verify_dev": (_int, [_vp] * 7),
    "ronk_mpcs_commit": (_int, [_vp, C.c_uint32, _vp, _vp]),
    "ronk_mpcs_open": (_int, [_vp] * 7 + [C.POINTER(_int)]),
    "ronk_mpcs_verify": (_int, [_vp] * 5 + [C.POINTER(_int)]),
    "ronk_ext2_check": (_int, [_u64, _u64]),
    "ronk_ext2_vec_add_dev": (_int, [_u64, _u64, _vp, _vp, _vp, _sz, _vp]),
    "ronk_ext2_vec_sub_dev": (_int, [_u64, _u64, _vp, _vp, _vp, _sz, _vp]),
    "ronk_ext2_vec_mul_dev": (_int, [_u64, _u64, _vp, _vp, _vp, _sz, _vp]),
    "ronk_ext2_vec_neg_dev": (_int, [_u64, _u64, _vp, _vp, _sz, _vp]),
    "ronk_ext2_vec_mul_base_dev": (_int, [_u64, _u64, _vp, _vp, _vp, _sz, _vp]),
    "ronk_ext2_vec_pow_dev": (_int, [_u64, _u64, _vp, _u64, _vp, _sz, _vp]),
    "ronk_ext2_vec_inv_dev": (_int, [_u64, _u64, _vp, _vp, _sz, _vp, _vp]),
    "ronk_ext2_vec_add": (_int, [_u64, _u64, _vp, _vp, _vp, _sz]),
    "ronk_ext2_vec_sub": (_int, [_u64, _u64, _vp, _vp, _vp, _sz]),
    "ronk_ext2_vec_mul": (_int, [_u64, _u64, _vp, _vp, _vp, _sz]),
    "ronk_ext2_vec_neg": (_int, [_u64, _u64, _vp, _vp, _sz]),
    "ronk_ext2_vec_mul_base": (_int, [_u64, _u64, _vp, _vp, _vp, _sz]),
    "ronk_ext2_vec_pow": (_int, [_u64, _u64, _vp, _u64, _vp, _sz]),
    "ronk_ext2_vec_inv": (_int, [_u64, _u64, _vp, _vp, _sz]),
    "ronk_scan_workspace_words": (_sz, [_sz]),
    "ronk_vec_prefix_prod_dev": (_int, [_u64, _vp, _vp, _sz, _int, _vp, _vp, _vp]),
    "ronk_vec_prefix_sum_dev": (_int, [_u64, _vp, _vp, _sz, _int, _vp, _vp, _vp]),
    "ronk_ext2_vec_prefix_prod_dev": (_int, [_u64, _u64, _vp, _vp, _sz, _int, _vp, _vp, _vp]),
    "ronk_ext2_vec_prefix_sum_dev": (_int, [_u64, _u64, _vp, _vp, _sz, _int, _vp, _vp, _vp]),
    "ronk_accum_check": (_int, [_u64, _u64, C.c_uint32, _sz]),
    "ronk_perm_product_dev": (_int, [_u64, _u64, _vp, _vp, _vp, C.c_uint32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ronk_logup_sum_dev": (_int, [_u64, _u64, _vp, _vp, C.c_uint32, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ronk_vec_prefix_prod": (_int, [_u64, _vp, _vp, _sz, _int, _vp]),
    "ronk_vec_prefix_sum": (_int, [_u64, _vp, _vp, _sz, _int, _vp]),
    "ronk_ext2_vec_prefix_prod": (_int, [_u64, _u64, _vp, _vp, _sz, _int, _vp]),
    "ronk_ext2_vec_prefix_sum": (_int, [_u64, _u64, _vp, _vp, _sz, _int, _vp]),
    "ronk_perm_product": (_int, [_u64, _u64, _vp, _vp, _vp, C.c_uint32, _sz, _vp, _vp, _vp, _vp, C.POINTER(_int)]),
    "ronk_logup_sum": (_int, [_u64, _u64, _vp, _vp, C.c_uint32, _sz, _vp, _vp, _vp, C.POINTER(_int)]),
    "ronk_lookup_workspace_words": (_sz, [_sz]),
    "ronk_lookup_check": (_int, [_u64, _sz, C.c_uint32, _sz]),
    "ronk_lookup_mult_dev": (_int, [_u64, _vp, _sz, _vp, C.c_uint32, _sz, _int, _vp, _vp, _vp, _vp]),
    "ronk_lookup_mult": (_int, [_u64, _vp, _sz, _vp, C.c_uint32, _sz, _int, _vp, _vp]),
    "ronk_logup_quotient_dev": (_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ronk_logup_quotient": (_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "ronk_air_check": (_int, [C.c_uint32, C.c_uint32, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.c_uint32]),
    "ronk_air_create": (_int, [C.POINTER(_vp), _vp, C.c_uint32, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp,
                               C.c_uint32, _vp]),
    "ronk_air_destroy": (_int, [_vp]),
    "ronk_air_quotient_dev": (_int, [_vp] * 8),
    "ronk_air_quotient": (_int, [_vp] * 7),
    "ronk_air_cells": (C.c_uint32, [_vp, _vp, C.c_uint32]),
    "ronk_air_eval_point": (_int, [_vp] * 6),
    "ronk_stark_check": (_int, [_u64, C.c_uint32, _u64, _u64, C.c_uint32, C.c_uint32, _u64] + [C.c_uint32] * 5 + [_vp, _vp, C.c_uint32, _vp]
                         + [C.c_uint32] * 4 + [_vp, C.c_uint32]),
    "ronk_stark_create": (_int, [C.POINTER(_vp), _vp, _u64, _u64, C.c_uint32, C.c_uint32, _u64] + [C.c_uint32] * 5
                          + [_vp, _vp, C.c_uint32, _vp] + [C.c_uint32] * 4 + [_vp, C.c_uint32, _vp]),
    "ronk_stark_destroy": (_int, [_vp]),
    "ronk_stark_set_pow": (_int, [_vp, C.c_uint32, C.c_uint32]),
    "ronk_stark_proof_words": (_sz, [_vp]),
    "ronk_stark_workspace_words": (_sz, [_vp]),
    "ronk_stark_begin_dev": (_int, [_vp] * 5),
    "ronk_stark_commit_round_dev": (_int, [_vp, C.c_uint32, _vp, _vp, _vp]),
    "ronk_stark_challenges_dev": (_vp, [_vp, _vp]),
    "ronk_stark_finish_dev": (_int, [_vp] * 5),
    "ronk_stark_split_dev": (_int, [_vp] * 5),
    "ronk_stark_prove_dev": (_int, [_vp] * 8),
    "ronk_stark_verify_dev": (_int, [_vp] * 4 + [C.POINTER(_int), _vp]),
    "ronk_stark_prove": (_int, [_vp] * 5 + [C.POINTER(_int)]),
    "ronk_stark_verify": (_int, [_vp] * 4 + [C.POINTER(_int)]),
    "ronk_plonk_check": (_int, [_u64, _u64, _u64, C.c_uint32, C.c_uint32, _u64, _pu]),
    "ronk_plonk_create": (_int, [C.POINTER(_vp), _u64, _u64, _u64, C.c_uint32, C.c_uint32, _u64, _pu]),
    "ronk_plonk_destroy": (_int, [_vp]),
    "ronk_plonk_quotient_dev": (_int, [_vp] * 11),
    "ronk_plonk_quotient": (_int, [_vp] * 10),
    "ronk_dev_alloc": (_int, [C.POINTER(_vp), _sz]),
    "ronk_dev_free": (_int, [_vp]),
    "ronk_memcpy_h2d": (_int, [_vp, _vp, _sz]),
    "ronk_memcpy_d2h": (_int, [_vp, _vp, _sz]),
    "ronk_dev_sync": (_int, []),
    "ronk_set_device": (_int, [_int]),
    "ronk_get_device": (_int, [C.POINTER(_int)]),
    "ronk_trim_workspace": (_int, []),
}
# include/ronk_ntt_fixed.h: the periodic columns of a constraint program and the fixed round of the STARK
_SIG_FIXED = {
    "ronk_air_check_per": (_int, [C.c_uint32, C.c_uint32, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.c_uint32,
                                  C.c_uint32, _vp]),
    "ronk_air_create_per": (_int, [C.POINTER(_vp), _vp, C.c_uint32, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp,
                                   C.c_uint32, _vp, C.c_uint32, _vp, _vp]),
    "ronk_stark_check_fixed": (_int, [_u64, C.c_uint32, _u64, _u64, C.c_uint32, C.c_uint32, _u64] + [C.c_uint32] * 5
                               + [_vp, _vp, C.c_uint32, _vp] + [C.c_uint32] * 4 + [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp]),
    "ronk_stark_create_fixed": (_int, [C.POINTER(_vp), _vp, _u64, _u64, C.c_uint32, C.c_uint32, _u64] + [C.c_uint32] * 5
                                + [_vp, _vp, C.c_uint32, _vp] + [C.c_uint32] * 4 + [_vp, C.c_uint32, _vp, C.c_uint32, C.c_uint32, _vp, _vp]),
    "ronk_stark_fixed_words": (_sz, [_vp]),
    "ronk_stark_fixed_commit_dev": (_int, [_vp] * 4),
    "ronk_stark_fixed_root_dev": (_vp, [_vp, _vp]),
    "ronk_stark_set_fixed_dev": (_int, [_vp, _vp]),
    "ronk_stark_set_fixed_root_dev": (_int, [_vp, _vp]),
    "ronk_stark_fixed_commit": (_int, [_vp] * 3),
    "ronk_stark_set_fixed": (_int, [_vp, _vp, _int]),
}
for _name, (_res, _args) in list(_SIG.items()) + list(_SIG_FIXED.items()):
    if os.environ.get("RONK_LIB_PATH") and not hasattr(lib, _name):
        continue              # an older build in an A/B run may lack the newest entry points
    _f = getattr(lib, _name)  # AttributeError here = the library does not export a declared symbol
    _f.restype, _f.argtypes = _res, _args

EXPORTS = sorted(_SIG)                  # what include/ronk_ntt.h itself declares
EXPORTS_FIXED = sorted(_SIG_FIXED)      # what include/ronk_ntt_fixed.h declares


def check(rc, detail=""):
    if rc != 0:
        raise RonkPanic(rc, detail)


def device_count():
    n = _int(0)
    check(lib.ronk_device_count(C.byref(n)))
    return n.value


def arr(x):
    """canonical residues as a contiguous numpy uint64 array"""
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


def ptr(a):
    return a.ctypes.data_as(_vp)


def out_scalar(fn, *args):
    o = _u64(0)
    check(fn(*args, C.byref(o)))
    return o.value


class PlanOpts(C.Structure):
    """ronk_plan_opts (include/ronk_ntt.h)"""
    _fields_ = [("tile_log2_columns", _int), ("twiddle_matrix_log2_max", _int), ("in_flight", _int), ("split_log2_rows", _int),
                ("three_pass_from_log2", _int), ("reserved", _int * 3)]

    def __init__(self, tile_log2_columns=-1, twiddle_matrix_log2_max=-1, in_flight=-1):
        super().__init__(tile_log2_columns, twiddle_matrix_log2_max, in_flight)


class Plan:
    """RAII wrapper of ronk_plan: (p, g, n = 2^log2n, batch) on one device."""

    def __init__(self, p, g, log2n, batch=1, device=-1, tile_log2_columns=-1, twiddle_matrix_log2_max=-1, in_flight=-1):
        self.h = None
        h = _vp()
        if in_flight == -1 and not hasattr(lib, "ronk_plan_create_opts"):   # an older build in an A/B run
            check(lib.ronk_plan_create_tuned(C.byref(h), p, g, log2n, batch, device, tile_log2_columns,
                                             twiddle_matrix_log2_max))
        else:
            opts = PlanOpts(tile_log2_columns, twiddle_matrix_log2_max, in_flight)
            check(lib.ronk_plan_create_opts(C.byref(h), p, g, log2n, batch, device, C.byref(opts)))
        self.h, self.p, self.g, self.log2n, self.n, self.batch = h, p, g, log2n, 1 << log2n, batch

    def in_flight(self):
        """lanes the plan keeps in flight (ronk_plan_opts::in_flight resolved): 1 or 2"""
        return lib.ronk_plan_in_flight(self.h)

    def forward_many_dev(self, d_ins, d_outs, stream=0, inverse=False):
        """`len(d_ins)` independent [batch][n] device arrays in one call (ronk_ntt_forward_many_dev)"""
        k = len(d_ins)
        a = (_vp * k)(*d_ins)
        b = (_vp * k)(*d_outs)
        f = lib.ronk_ntt_inverse_many_dev if inverse else lib.ronk_ntt_forward_many_dev
        check(f(self.h, a, b, k, stream))

    def close(self):
        if getattr(self, "h", None):
            lib.ronk_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        if lib is not None:      # module globals are already torn down at interpreter exit
            self.close()

    def num_passes(self):
        return lib.ronk_plan_num_passes(self.h)

    def path(self):
        """1 = tiled Goldilocks kernels, 2 = the tile kernels over a Montgomery prime, 0 = generic radix-2 path (ronk_plan_path)"""
        return lib.ronk_plan_path(self.h)

    def forward(self, x, nodes=False):
        x = arr(x)
        assert x.size == self.n * self.batch
        out = np.empty_like(x)
        nd = np.empty(self.n, dtype=np.uint64) if nodes else None
        check(lib.ronk_ntt_forward(self.h, ptr(x), ptr(out), ptr(nd) if nodes else None))
        return (out, nd) if nodes else out

    def inverse(self, x):
        x = arr(x)
        assert x.size == self.n * self.batch
        out = np.empty_like(x)
        check(lib.ronk_ntt_inverse(self.h, ptr(x), ptr(out)))
        return out

    def forward_dev(self, d_in, d_out, stream=0):
        check(lib.ronk_ntt_forward_dev(self.h, d_in, d_out, stream))

    def inverse_dev(self, d_in, d_out, stream=0):
        check(lib.ronk_ntt_inverse_dev(self.h, d_in, d_out, stream))

    def rs_encode_batch_dev(self, d_msgs, k, d_ys, stream=0):
        """batched Message::encode::<N> (codes/reed_solomon.rs:42-52): [batch][k] messages -> [batch][n] y-coordinates"""
        check(lib.ronk_rs_encode_batch_dev(self.h, d_msgs, k, d_ys, stream))

    def rs_recover_batch_dev(self, k, d_erased, n_erased, d_ys, d_msgs, d_full, d_status, stream=0):
        """erasure recovery, the inverse of rs_encode_batch_dev (ronk_rs_recover_batch_dev): [batch][n] codewords with the same
        n_erased positions lost -> [batch][k] messages (d_full, may be None: the repaired codewords); d_status receives one int
        per row (0, ERR_NOT_CODEWORD, or the list's ERR_ZERO_INVERSE / ERR_INDEX in every entry)"""
        check(lib.ronk_rs_recover_batch_dev(self.h, k, d_erased, n_erased, d_ys, d_msgs, d_full, d_status, stream))

    def time_passes(self, d_in, d_out, inverse=False, iters=20, stream=0):
        np_ = self.num_passes()
        ms = (C.c_float * np_)()
        check(lib.ronk_plan_time_passes(self.h, d_in, d_out, int(inverse), iters, ms, stream))
        return [float(v) for v in ms]


class PoseidonHandle:
    """ronk_poseidon: one parameter set (p, width, alpha, rounds, rate, rc, mds) resident on the current device.  The _dev
    methods take raw device pointers (int) and enqueue on `stream`."""

    def __init__(self, p, width, alpha, num_p, num_f, rate, rc, mds):
        rc = arr([int(v) % p for v in rc])
        mds = arr([int(v) % p for row in mds for v in row])
        if rc.size != (num_p + num_f) * width or mds.size != width * width:
            raise RonkPanic(ERR_INVALID, "rc holds (num_f + num_p) * width words, mds width * width")
        self.h = _vp()
        check(lib.ronk_poseidon_create(C.byref(self.h), p, width, alpha, num_p, num_f, rate, ptr(rc), ptr(mds)))
        self.p, self.width, self.rate = p, width, rate

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            lib.ronk_poseidon_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def hash_state(self, values):
        """Poseidon::hash's final state for `values` padded with ZERO (word 1 is the reference's return value)"""
        v = arr([int(x) for x in values])
        out = np.empty(self.width, dtype=np.uint64)
        check(lib.ronk_poseidon_hash(self.h, ptr(v) if v.size else None, v.size, ptr(out)))
        return out

    def permute_dev(self, d_states, count, stream=0):
        check(lib.ronk_poseidon_permute_dev(self.h, d_states, count, stream))

    def sponge_dev(self, d_in, n_items, length, item_stride, elem_stride, d_out, n_out, stream=0):
        check(lib.ronk_poseidon_sponge_dev(self.h, d_in, n_items, length, item_stride, elem_stride, d_out, n_out, stream))

    def pow_grind_dev(self, d_seed, seed_len, bits, log2_limit, max_lanes, d_work, d_nonce, stream=0):
        check(lib.ronk_pow_grind_dev(self.h, d_seed, seed_len, bits, log2_limit, max_lanes, d_work, d_nonce, stream))

    def pow_verify_dev(self, d_seed, seed_len, bits, log2_limit, d_nonce, d_ok, stream=0):
        check(lib.ronk_pow_verify_dev(self.h, d_seed, seed_len, bits, log2_limit, d_nonce, d_ok, stream))

    def merkle_commit_dev(self, d_leaves, n_leaves, leaf_len, item_stride, elem_stride, digest_len, d_tree, stream=0):
        check(lib.ronk_merkle_commit_dev(self.h, d_leaves, n_leaves, leaf_len, item_stride, elem_stride, digest_len, d_tree, stream))

    def merkle_verify_dev(self, d_leaves, n_idx, leaf_len, item_stride, elem_stride, d_indices, d_paths, n_leaves, digest_len, d_root,
                          d_ok, stream=0):
        check(lib.ronk_merkle_verify_dev(self.h, d_leaves, n_idx, leaf_len, item_stride, elem_stride, d_indices, d_paths, n_leaves,
                                         digest_len, d_root, d_ok, stream))


def pow_default_limit(p, bits):
    """log2_limit when the caller gives none: bits + 6 (a search that long fails with probability e^-64), capped by the library's
    40 and by the field (2^log2_limit < p)"""
    return min(bits + 6, 40, (p - 1).bit_length() - 1)


def merkle_tree_words(n_leaves, digest_len):
    return lib.ronk_merkle_tree_words(n_leaves, digest_len)


def merkle_level_offset(n_leaves, digest_len, level):
    return lib.ronk_merkle_level_offset(n_leaves, digest_len, level)


def merkle_open_dev(d_tree, n_leaves, digest_len, d_indices, n_idx, d_paths, d_status, stream=0):
    check(lib.ronk_merkle_open_dev(d_tree, n_leaves, digest_len, d_indices, n_idx, d_paths, d_status, stream))


class FriHandle:
    """ronk_fri: one FRI instance (log2_n, coset shift, arity, final size, blowup, queries, digest length) on a PoseidonHandle,
    which it borrows.  The _dev methods take raw device pointers (int) and enqueue on `stream`.  With w (a quadratic non-residue)
    the challenges and the folded layers live in F_p[t] / (t^2 - w) (ronk_fri_create_ext): layers are planar [2][N], a challenge
    is two words, and input_ext says whether layer 0 is planar pairs too."""

    def __init__(self, pos, g, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, w=None, input_ext=False,
                 pow_bits=0, pow_log2_limit=None):
        self.h = _vp()
        self.pos = pos      # keeps the Poseidon handle alive
        self.ext, self.input_ext = w is not None, bool(input_ext)
        self.shape = (log2_n, log2_arity, log2_final, n_queries, digest_len)
        if w is None:
            if input_ext:
                raise RonkPanic(ERR_INVALID, "input_ext needs the extension's w")
            check(lib.ronk_fri_create(C.byref(self.h), pos.h, g, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries,
                                      digest_len))
            self.proof_words = lib.ronk_fri_proof_words(*self.shape)
            self.workspace_words = lib.ronk_fri_workspace_words(*self.shape)
        else:
            check(lib.ronk_fri_create_ext(C.byref(self.h), pos.h, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup,
                                          n_queries, digest_len, int(self.input_ext)))
            self.proof_words = lib.ronk_fri_proof_words_ext(*self.shape, int(self.input_ext))
            self.workspace_words = lib.ronk_fri_workspace_words_ext(*self.shape, int(self.input_ext))
        self.n, self.arity, self.digest_len = 1 << log2_n, 1 << log2_arity, digest_len
        self.input_words = self.n * (2 if self.input_ext else 1)
        self.pow_bits = 0
        if pow_bits:
            self.set_pow(pow_bits, pow_log2_limit)

    def set_pow(self, bits, log2_limit=None):
        """grinding between the commit and the query phase (ronk_fri_set_pow), before the handle is used; bits = 0: none"""
        if log2_limit is None:
            log2_limit = pow_default_limit(self.pos.p, bits)
        check(lib.ronk_fri_set_pow(self.h, bits, log2_limit))
        self.pow_bits, self.pow_log2_limit = bits, log2_limit
        self.proof_words = lib.ronk_fri_handle_proof_words(self.h)
        self.workspace_words = lib.ronk_fri_handle_workspace_words(self.h)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            lib.ronk_fri_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def fold_dev(self, layer, d_in, d_beta, d_out, stream=0):
        check(lib.ronk_fri_fold_dev(self.h, layer, d_in, d_beta, d_out, stream))

    def prove_dev(self, d_evals, d_seed, d_work, d_proof, stream=0):
        check(lib.ronk_fri_prove_dev(self.h, d_evals, d_seed, d_work, d_proof, stream))

    def verify_dev(self, d_proof, d_seed, d_status, stream=0):
        check(lib.ronk_fri_verify_dev(self.h, d_proof, d_seed, d_status, stream))

    def prove(self, evals, seed):
        evals, seed = arr(evals), arr(seed)
        if evals.size != self.input_words or seed.size != self.digest_len:
            raise RonkPanic(ERR_INVALID, "evals holds 2^log2_n words ([2][2^log2_n] with input_ext), seed digest_len")
        proof = np.empty(self.proof_words, dtype=np.uint64)
        check(lib.ronk_fri_prove(self.h, ptr(evals), ptr(seed), ptr(proof)))
        return proof

    def verify(self, proof, seed):
        proof, seed = arr(proof), arr(seed)
        if proof.size != self.proof_words or seed.size != self.digest_len:
            raise RonkPanic(ERR_INVALID, "proof holds ronk_fri_proof_words words, seed digest_len")
        st = _int(-1)
        check(lib.ronk_fri_verify(self.h, ptr(proof), ptr(seed), C.byref(st)))
        return st.value


class PcsHandle:
    """ronk_pcs: the batched FRI polynomial commitment with DEEP quotients (include/ronk_ntt.h) for a [n_columns][2^log2_n] matrix
    opened at n_points points of F_p[t] / (t^2 - w), on a PoseidonHandle, which it borrows.  The _dev methods take raw device
    pointers (int) and enqueue on `stream`; one call at a time per handle."""

    def __init__(self, pos, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, n_columns, n_points,
                 pow_bits=0, pow_log2_limit=None):
        self.h = _vp()
        self.pos = pos      # keeps the Poseidon handle alive
        check(lib.ronk_pcs_create(C.byref(self.h), pos.h, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries,
                                  digest_len, n_columns, n_points))
        self.shape = (log2_n, log2_arity, log2_final, n_queries, digest_len, n_columns, n_points)
        self.proof_words = lib.ronk_pcs_proof_words(*self.shape)
        self.workspace_words = lib.ronk_pcs_workspace_words(*self.shape)
        self.n, self.arity, self.digest_len = 1 << log2_n, 1 << log2_arity, digest_len
        self.columns, self.points, self.coeffs = n_columns, n_points, (1 << log2_n) >> log2_blowup
        self.tree_words = lib.ronk_merkle_tree_words(self.n >> log2_arity, digest_len)
        self.pow_bits = 0
        if pow_bits:
            self.set_pow(pow_bits, pow_log2_limit)

    def set_pow(self, bits, log2_limit=None):
        """grinding in the embedded FRI (ronk_pcs_set_pow), before the handle is used; bits = 0: none"""
        if log2_limit is None:
            log2_limit = pow_default_limit(self.pos.p, bits)
        check(lib.ronk_pcs_set_pow(self.h, bits, log2_limit))
        self.pow_bits, self.pow_log2_limit = bits, log2_limit
        self.proof_words = lib.ronk_pcs_handle_proof_words(self.h)
        self.workspace_words = lib.ronk_pcs_handle_workspace_words(self.h)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            lib.ronk_pcs_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def combine_dev(self, d_M, d_y, d_z, d_alpha, d_G, d_status, stream=0):
        check(lib.ronk_deep_combine_dev(self.h, d_M, d_y, d_z, d_alpha, d_G, d_status, stream))

    def commit_dev(self, d_M, d_tree, stream=0):
        check(lib.ronk_pcs_commit_dev(self.h, d_M, d_tree, stream))

    def open_dev(self, d_M, d_tree, d_coef, d_z, d_seed, d_work, d_proof, d_status, stream=0):
        check(lib.ronk_pcs_open_dev(self.h, d_M, d_tree, d_coef, d_z, d_seed, d_work, d_proof, d_status, stream))

    def verify_dev(self, d_root, d_z, d_seed, d_proof, d_status, stream=0):
        check(lib.ronk_pcs_verify_dev(self.h, d_root, d_z, d_seed, d_proof, d_status, stream))

    def _sized(self, what, a, words):
        a = arr(a)
        if a.size != words:
            raise RonkPanic(ERR_INVALID, "%s holds %d words" % (what, words))
        return a

    def commit(self, M):
        """host matrix [n_columns][2^log2_n] -> the tree (the root is its last digest_len words)"""
        M = self._sized("the matrix", M, self.columns * self.n)
        tree = np.empty(self.tree_words, dtype=np.uint64)
        check(lib.ronk_pcs_commit(self.h, ptr(M), ptr(tree)))
        return tree

    def open(self, M, tree, coef, z, seed):
        """-> (the proof, status 0 or 32); z: planar [2][n_points]"""
        M, tree = self._sized("the matrix", M, self.columns * self.n), self._sized("the tree", tree, self.tree_words)
        coef = self._sized("the coefficients", coef, self.columns * self.coeffs)
        z, seed = self._sized("the points", z, 2 * self.points), self._sized("the seed", seed, self.digest_len)
        proof = np.empty(self.proof_words, dtype=np.uint64)
        st = _int(-1)
        check(lib.ronk_pcs_open(self.h, ptr(M), ptr(tree), ptr(coef), ptr(z), ptr(seed), ptr(proof), C.byref(st)))
        return proof, st.value

    def verify(self, root, z, seed, proof):
        root, z = self._sized("the root", root, self.digest_len), self._sized("the points", z, 2 * self.points)
        seed, proof = self._sized("the seed", seed, self.digest_len), self._sized("the proof", proof, self.proof_words)
        st = _int(-1)
        check(lib.ronk_pcs_verify(self.h, ptr(root), ptr(z), ptr(seed), ptr(proof), C.byref(st)))
        return st.value


def _u32s(values):
    values = [int(v) for v in values]
    return (C.c_uint32 * max(len(values), 1))(*values)


def _ptrs(values):
    """a host array of pointers from ints (device pointers) or numpy arrays (host pointers)"""
    values = [v if isinstance(v, int) else ptr(v).value for v in values]
    return (C.c_void_p * max(len(values), 1))(*values)


class MpcsHandle:
    """ronk_mpcs: the multi-matrix polynomial commitment (include/ronk_ntt.h): len(n_columns) matrices of n_columns[r] columns,
    round r opened at the points whose bits are set in point_masks[r], one DEEP codeword, one FRI; on a PoseidonHandle, which it
    borrows.  The _dev methods take raw device pointers (int; lists of them for the matrices, trees and coefficients) and enqueue
    on `stream`; one call at a time per handle."""

    def __init__(self, pos, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries, digest_len, n_points, n_columns,
                 point_masks, pow_bits=0, pow_log2_limit=None):
        self.h = _vp()
        self.pos = pos      # keeps the Poseidon handle alive
        n_columns, point_masks = [int(c) for c in n_columns], [int(m) for m in point_masks]
        if len(n_columns) != len(point_masks):
            raise RonkPanic(ERR_INVALID, "one mask per round")
        self.rounds = len(n_columns)
        cs, ms = _u32s(n_columns), _u32s(point_masks)
        check(lib.ronk_mpcs_create(C.byref(self.h), pos.h, g, w, log2_n, coset_shift, log2_arity, log2_final, log2_blowup, n_queries,
                                   digest_len, n_points, self.rounds, cs, ms))
        shape = (log2_n, log2_arity, log2_final, n_queries, digest_len, n_points, self.rounds, cs, ms)
        self.proof_words = lib.ronk_mpcs_proof_words(*shape)
        self.workspace_words = lib.ronk_mpcs_workspace_words(*shape)
        self.n, self.arity, self.digest_len = 1 << log2_n, 1 << log2_arity, digest_len
        self.columns, self.masks, self.points, self.coeffs = n_columns, point_masks, n_points, (1 << log2_n) >> log2_blowup
        self.claims = sum(bin(m).count("1") * c for c, m in zip(n_columns, point_masks))
        self.tree_words = lib.ronk_merkle_tree_words(self.n >> log2_arity, digest_len)
        self.pow_bits = 0
        if pow_bits:
            self.set_pow(pow_bits, pow_log2_limit)

    def set_pow(self, bits, log2_limit=None):
        """grinding in the embedded FRI (ronk_mpcs_set_pow), before the handle is used; bits = 0: none"""
        if log2_limit is None:
            log2_limit = pow_default_limit(self.pos.p, bits)
        check(lib.ronk_mpcs_set_pow(self.h, bits, log2_limit))
        self.pow_bits, self.pow_log2_limit = bits, log2_limit
        self.proof_words = lib.ronk_mpcs_handle_proof_words(self.h)
        self.workspace_words = lib.ronk_mpcs_handle_workspace_words(self.h)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            lib.ronk_mpcs_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _each(self, what, a):
        a = list(a)
        if len(a) != self.rounds:
            raise RonkPanic(ERR_INVALID, "%s: one per round" % what)
        return a

    def combine_dev(self, d_M, d_y, d_z, d_alpha, d_G, d_status, stream=0):
        check(lib.ronk_mpcs_combine_dev(self.h, _ptrs(self._each("the matrices", d_M)), d_y, d_z, d_alpha, d_G, d_status, stream))

    def commit_dev(self, r, d_M, d_tree, stream=0):
        check(lib.ronk_mpcs_commit_dev(self.h, r, d_M, d_tree, stream))

    def open_dev(self, d_M, d_tree, d_coef, d_z, d_seed, d_work, d_proof, d_status, stream=0):
        check(lib.ronk_mpcs_open_dev(self.h, _ptrs(self._each("the matrices", d_M)), _ptrs(self._each("the trees", d_tree)),
                                     _ptrs(self._each("the coefficients", d_coef)), d_z, d_seed, d_work, d_proof, d_status, stream))

    def verify_dev(self, d_roots, d_z, d_seed, d_proof, d_status, stream=0):
        check(lib.ronk_mpcs_verify_dev(self.h, d_roots, d_z, d_seed, d_proof, d_status, stream))

    def _sized(self, what, a, words):
        a = arr(a)
        if a.size != words:
            raise RonkPanic(ERR_INVALID, "%s holds %d words" % (what, words))
        return a

    def commit(self, r, M):
        """host matrix [n_columns[r]][2^log2_n] of round r -> its tree (the root is its last digest_len words)"""
        if not 0 <= r < self.rounds:
            raise RonkPanic(ERR_INVALID, "no such round")
        M = self._sized("the matrix", M, self.columns[r] * self.n)
        tree = np.empty(self.tree_words, dtype=np.uint64)
        check(lib.ronk_mpcs_commit(self.h, r, ptr(M), ptr(tree)))
        return tree

    def open(self, M, tree, coef, z, seed):
        """lists of the rounds' matrices, trees and coefficients -> (the proof, status 0 or 32); z: planar [2][n_points]"""
        M = [self._sized("a matrix", a, c * self.n) for a, c in zip(self._each("the matrices", M), self.columns)]
        tree = [self._sized("a tree", a, self.tree_words) for a in self._each("the trees", tree)]
        coef = [self._sized("the coefficients", a, c * self.coeffs) for a, c in zip(self._each("the coefficients", coef), self.columns)]
        z, seed = self._sized("the points", z, 2 * self.points), self._sized("the seed", seed, self.digest_len)
        proof = np.empty(self.proof_words, dtype=np.uint64)
        st = _int(-1)
        check(lib.ronk_mpcs_open(self.h, _ptrs(M), _ptrs(tree), _ptrs(coef), ptr(z), ptr(seed), ptr(proof), C.byref(st)))
        return proof, st.value

    def verify(self, roots, z, seed, proof):
        """roots: [rounds][digest_len]"""
        roots, z = self._sized("the roots", roots, self.rounds * self.digest_len), self._sized("the points", z, 2 * self.points)
        seed, proof = self._sized("the seed", seed, self.digest_len), self._sized("the proof", proof, self.proof_words)
        st = _int(-1)
        check(lib.ronk_mpcs_verify(self.h, ptr(roots), ptr(z), ptr(seed), ptr(proof), C.byref(st)))
        return st.value


def ext2_poly_eval_batch(p, w, coef, z):
    """coef: [n_columns][d] base words, z: planar [2][n_points] -> planar [2][n_points n_columns] (ronk_ext2_poly_eval_batch)"""
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.uint64))
    z = arr(z)
    if coef.ndim != 2 or z.size % 2:
        raise RonkPanic(ERR_INVALID, "coef is [n_columns][d], z planar [2][n_points]")
    c, d, k = coef.shape[0], coef.shape[1], z.size // 2
    y = np.empty(2 * k * c, dtype=np.uint64)
    check(lib.ronk_ext2_poly_eval_batch(p, w, ptr(coef), c, d, ptr(z), k, ptr(y)))
    return y


class ShardedPlan:
    """ronk_sharded_plan: the four-step NTT sharded over `devices` inside the library (single process; peer copies over
    xGMI in column chunks).  Rank g = devices[g]; the same ordinal may appear several times (logical ranks sharing a GPU:
    how the single-GPU tests drive this path)."""

    def __init__(self, log2n, devices, inverse=False, chunks=0, exchange=EXCHANGE_MESH, p=None, g=None):
        """p, g: any odd prime with 2^log2n | p - 1 and a primitive element of it (ronk_sharded_plan_create_p); default Goldilocks"""
        self.h = None
        h = _vp()
        devs = (_int * len(devices))(*devices)
        if p is None:
            check(lib.ronk_sharded_plan_create_ex(C.byref(h), log2n, int(inverse), devs, len(devices), chunks, exchange))
        else:
            check(lib.ronk_sharded_plan_create_p(C.byref(h), int(p), int(g), log2n, int(inverse), devs, len(devices), chunks, exchange))
        self.exchange = exchange
        self.h, self.n, self.ndev = h, 1 << log2n, len(devices)
        r, c, per, ch = _u64(0), _u64(0), _u64(0), _int(0)
        check(lib.ronk_sharded_plan_info(h, C.byref(r), C.byref(c), C.byref(per), C.byref(ch)))
        self.R, self.C, self.per_rank, self.chunks = r.value, c.value, per.value, ch.value

    def peer_access(self):
        """(matrix, staged): matrix[g][h] in {0 same device, 1 direct peer access, 2 staged through the host}; staged = the
        number of rank pairs whose blocks do NOT travel peer-to-peer (ronk_sharded_plan_peer_access)"""
        w = self.ndev
        m = (_int * (w * w))()
        staged = lib.ronk_sharded_plan_peer_access(self.h, m, w * w)
        if staged < 0:
            check(staged)
        return [[m[g * w + h] for h in range(w)] for g in range(w)], staged

    def transform(self, x):
        """host natural-order vector -> natural-order result (ronk_ntt_sharded)"""
        x = arr(x)
        assert x.size == self.n
        out = np.empty_like(x)
        check(lib.ronk_ntt_sharded(self.h, ptr(x), ptr(out)))
        return out

    def time_stages(self, d_in, d_out):
        """one transform in three serialised stages (ronk_sharded_time_stages): [phase 1, exchange, phase 2] in ms, and the
        achieved GB/s per directed link of the exchange"""
        a = (_vp * self.ndev)(*d_in)
        b = (_vp * self.ndev)(*d_out)
        ms = (C.c_float * 3)()
        check(lib.ronk_sharded_time_stages(self.h, a, b, ms))
        t = [float(v) for v in ms]
        per_link = self.n * 8 / (self.ndev ** 2)
        return {"phase1_ms": t[0], "exchange_ms": t[1], "phase2_ms": t[2],
                "bytes_per_directed_link": per_link, "GBs_per_directed_link": per_link / (t[1] * 1e-3) / 1e9 if t[1] > 0 else None}

    def transform_dev(self, d_in, d_out):
        """device pointers per rank (lists of ints); asynchronous, see sync()"""
        a = (_vp * self.ndev)(*d_in)
        b = (_vp * self.ndev)(*d_out)
        check(lib.ronk_ntt_sharded_dev(self.h, a, b))

    def sync(self):
        check(lib.ronk_sharded_sync(self.h))

    def close(self):
        if getattr(self, "h", None):
            lib.ronk_sharded_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        if lib is not None:
            self.close()


SHARDED_MUL_UNFUSED, SHARDED_MUL_FUSED = 1, 2


class ShardedMulPlan:
    """ronk_sharded_mul_plan: a * b over `devices` (the polynomial product sharded like ShardedPlan's transform).  Operands and
    product share the [R][C/W] column-block layout per rank (dist.scatter_input); `fused_middle` says whether the plan runs the
    fused middle kernel (1) or the composed one (0).  unfused=True forces the composed middle (RONK_SHARDED_MUL_UNFUSED), fused=True
    the fused one wherever an instantiation matches (RONK_SHARDED_MUL_FUSED); default: the library's measured choice."""

    def __init__(self, log2n, devices, chunks=0, exchange=EXCHANGE_MESH, p=None, g=None, unfused=False, fused=False):
        self.h = None
        h = _vp()
        devs = (_int * len(devices))(*devices)
        flags = (SHARDED_MUL_UNFUSED if unfused else 0) | (SHARDED_MUL_FUSED if fused else 0)
        if p is None:
            check(lib.ronk_sharded_mul_plan_create(C.byref(h), log2n, devs, len(devices), chunks, exchange, flags))
        else:
            check(lib.ronk_sharded_mul_plan_create_p(C.byref(h), int(p), int(g), log2n, devs, len(devices), chunks, exchange, flags))
        self.exchange = exchange
        self.h, self.n, self.ndev = h, 1 << log2n, len(devices)
        r, c, per, ch, fu = _u64(0), _u64(0), _u64(0), _int(0), _int(0)
        check(lib.ronk_sharded_mul_plan_info(h, C.byref(r), C.byref(c), C.byref(per), C.byref(ch), C.byref(fu)))
        self.R, self.C, self.per_rank, self.chunks, self.fused_middle = r.value, c.value, per.value, ch.value, fu.value

    def mul(self, a, b):
        """host coefficient vectors of any lengths with len(a) + len(b) - 1 <= n -> their product (ronk_poly_mul_sharded)"""
        a, b = arr(a), arr(b)
        out = np.empty(a.size + b.size - 1, dtype=np.uint64)
        check(lib.ronk_poly_mul_sharded(self.h, ptr(a), a.size, ptr(b), b.size, ptr(out)))
        return out

    def mul_dev(self, d_a, d_b, d_out):
        """device pointers per rank (lists of ints), [R][C/W] blocks of the zero-padded n-point vectors; asynchronous, see sync()"""
        a = (_vp * self.ndev)(*d_a)
        b = (_vp * self.ndev)(*d_b)
        o = (_vp * self.ndev)(*d_out)
        check(lib.ronk_poly_mul_sharded_dev(self.h, a, b, o))

    def sync(self):
        check(lib.ronk_sharded_mul_sync(self.h))

    def close(self):
        if getattr(self, "h", None):
            lib.ronk_sharded_mul_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        if lib is not None:
            self.close()


class FrPlan:
    """ronk_fr_plan (include/ronk_ntt.h): a transform of 2^log2n elements of BN254's scalar field, 4 words each.
    max_log2_tile caps the rows of every pass (0: the default plan)."""

    def __init__(self, log2n, max_log2_tile=0):
        self.h = _vp()
        self.log2n = log2n
        check(lib.ronk_plan_create_bn254(C.byref(self.h), log2n, max_log2_tile))

    def info(self):
        """-> the log2 rows of every pass, in order"""
        n, rows = C.c_uint32(0), (C.c_uint32 * 4)()
        check(lib.ronk_plan_info_bn254(self.h, C.byref(n), rows))
        return [int(rows[i]) for i in range(n.value)]

    def reserve(self, batch):
        """scratch for `batch` rows per set of launches (allocates and synchronises; a larger batch still runs, in slices)"""
        check(lib.ronk_plan_reserve_bn254(self.h, batch))

    def forward_dev(self, d_in, d_out, batch=1, stream=None):
        check(lib.ronk_ntt_forward_bn254_dev(self.h, d_in, d_out, batch, stream))

    def inverse_dev(self, d_in, d_out, batch=1, stream=None):
        check(lib.ronk_ntt_inverse_bn254_dev(self.h, d_in, d_out, batch, stream))

    def close(self):
        if self.h:
            lib.ronk_plan_destroy_bn254(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
