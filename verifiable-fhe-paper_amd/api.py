"""ctypes binding of include/vpbs_prover.h (libvpbs_hip.so).  No compute happens in Python."""
import ctypes as C
import json
import math
import os
import subprocess
import weakref
from fractions import Fraction

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libvpbs_hip.so")
P = 0xFFFFFFFF00000001
POW_ANY = 0xFFFFFFFFFFFFFFFF
U64P = C.POINTER(C.c_uint64)
U32P = C.POINTER(C.c_uint32)
U8P = C.POINTER(C.c_uint8)
SZP = C.POINTER(C.c_size_t)


class VpbsError(RuntimeError):
    """status=: the library's status code, kept as .status where the caller is meant to tell the failures apart"""

    def __init__(self, *args, status=None):
        super().__init__(*args)
        if status is not None:
            self.status = status


ERR_WITNESS = -6   # VPBS_ERR_WITNESS


class WitnessError(VpbsError):
    """a checked step proof refused a witness that does not satisfy the circuit; str() is vpbs_check_witness's message"""
    status = ERR_WITNESS


class ChallengerStateC(C.Structure):
    _fields_ = [("sponge", C.c_uint64 * 12), ("input", C.c_uint64 * 8), ("output", C.c_uint64 * 8),
                ("input_len", C.c_uint32), ("output_len", C.c_uint32)]


class FriParams(C.Structure):
    _fields_ = [("rate_bits", C.c_uint), ("cap_height", C.c_uint), ("pow_bits", C.c_uint),
                ("num_query_rounds", C.c_uint), ("n_rounds", C.c_uint), ("arity_bits", C.c_uint * 16),
                ("mul_final_by_x", C.c_int)]


class CompatC(C.Structure):
    """vpbs_compat: the switch table of the unpinned plonky2 0.2.0 choices (include/vpbs_prover.h)"""
    _fields_ = [("fri_mul_final_by_x", C.c_int), ("bytes_pi_len_prefix", C.c_int), ("digest_domain_separator", C.c_int),
                ("pow_smallest_nonce", C.c_int)]


COMPAT_FIELDS = tuple(f[0] for f in CompatC._fields_)


def compat(**over):
    """vpbs_compat_default with the given switches changed, e.g. compat(bytes_pi_len_prefix=0)"""
    k = CompatC()
    lib().vpbs_compat_default(C.byref(k))
    for name, v in over.items():
        if name not in COMPAT_FIELDS:
            raise ValueError("no such switch: " + name)
        setattr(k, name, int(v))
    return k


def compat_dict(k=None):
    k = k if k is not None else compat()
    return {name: int(getattr(k, name)) for name in COMPAT_FIELDS}


class FriBatchInfoC(C.Structure):
    _fields_ = [("point", C.c_uint64 * 2), ("n_polys", C.c_size_t), ("oracle_index", U32P), ("poly_index", U32P)]


class FriInstanceC(C.Structure):
    _fields_ = [("batches", C.POINTER(FriBatchInfoC)), ("n_batches", C.c_size_t)]


class GateC(C.Structure):
    """vpbs_gate: kind + parameters, and the derived / layout fields filled by vpbs_gates_layout."""
    _fields_ = [("kind", C.c_uint), ("p0", C.c_uint), ("p1", C.c_uint), ("p2", C.c_uint),
                ("degree", C.c_uint), ("num_constraints", C.c_uint), ("num_constants", C.c_uint), ("num_wires", C.c_uint),
                ("selector_index", C.c_uint), ("group_start", C.c_uint), ("group_end", C.c_uint), ("index", C.c_uint)]


class GeneratorC(C.Structure):
    """vpbs_generator"""
    _fields_ = [("kind", C.c_uint), ("p0", C.c_uint), ("inp", U32P), ("n_in", C.c_uint), ("out", U32P), ("n_out", C.c_uint)]


GENERATOR_KINDS = ["equality", "base_sum", "wire_split", "quotient_ext", "copy", "low_high"]


class CircuitC(C.Structure):
    """vpbs_circuit"""
    _fields_ = [("log_n", C.c_uint), ("n_wires", C.c_uint), ("n_routed", C.c_uint), ("gates", C.POINTER(GateC)), ("n_gates", C.c_uint),
                ("num_selectors", C.c_uint), ("row_gate", U32P), ("constants", U64P), ("n_constants_cols", C.c_uint),
                ("copies", U32P), ("n_copies", C.c_size_t), ("generators", C.POINTER(GeneratorC)), ("n_generators", C.c_size_t)]


GATE_KINDS = ["noop", "constant", "public_input", "arithmetic", "base_sum", "poseidon", "poseidon_mds", "arithmetic_ext", "mul_ext",
              "reducing", "reducing_ext", "random_access", "exponentiation", "coset_interpolation"]
UNUSED_SELECTOR = 0xFFFFFFFF


class StepInputsC(C.Structure):
    _fields_ = [("log_n", C.c_uint), ("n_wires", C.c_uint), ("n_zs_partial_products", C.c_uint), ("n_quotient", C.c_uint),
                ("num_challenges", C.c_uint), ("inputs_on_device", C.c_int),
                ("wires_values", C.c_void_p), ("zs_pp_values", C.c_void_p), ("quotient_coeffs", C.c_void_p),
                ("constants_sigmas", C.c_void_p), ("circuit_digest", C.c_uint64 * 4),
                ("public_inputs", U64P), ("n_public_inputs", C.c_size_t), ("forced_pow", C.c_uint64),
                ("sigmas_values", C.c_void_p), ("n_routed", C.c_uint), ("quotient_degree_factor", C.c_uint),
                ("n_constants", C.c_uint), ("gates", C.POINTER(GateC)), ("n_gates", C.c_uint), ("num_selectors", C.c_uint),
                ("sigmas_on_device", C.c_int), ("on_section", C.c_void_p), ("on_section_user", C.c_void_p)]


class VerifyInputsC(C.Structure):
    _fields_ = [("log_n", C.c_uint), ("rate_bits", C.c_uint), ("cap_height", C.c_uint),
                ("n_constants_sigmas", C.c_uint), ("n_wires", C.c_uint), ("n_zs_partial_products", C.c_uint), ("n_quotient", C.c_uint),
                ("num_challenges", C.c_uint), ("constants_sigmas_cap", U64P), ("circuit_digest", C.c_uint64 * 4),
                ("public_inputs", U64P), ("n_public_inputs", C.c_size_t), ("fri_only", C.c_int),
                ("n_constants", C.c_uint), ("n_routed", C.c_uint), ("quotient_degree_factor", C.c_uint), ("gate_terms_zeta", U64P),
                ("gates", C.POINTER(GateC)), ("n_gates", C.c_uint), ("num_selectors", C.c_uint), ("compat", C.POINTER(CompatC))]


class VerifyPbsInputsC(C.Structure):
    _fields_ = [("circuit", C.POINTER(VerifyInputsC)), ("N", C.c_uint), ("K", C.c_uint), ("n_lwe", C.c_uint), ("ggsw_len", C.c_size_t),
                ("testv", U64P), ("out_ct", U64P), ("ct", U64P), ("bsk", U64P), ("ksk", U64P)]


class IvcCircuitC(C.Structure):
    _fields_ = [("circuit", C.POINTER(CircuitC)), ("preset_pos", U32P), ("n_preset", C.c_size_t), ("pi_pos", U32P), ("n_pi", C.c_size_t),
                ("proof_words", C.c_size_t)]


class IvcTimingC(C.Structure):
    _fields_ = [("seconds", C.c_double), ("steps", C.c_uint), ("base_proof_ms", C.c_double), ("late_witness_ms", C.c_double),
                ("late_rows_upload_ms", C.c_double), ("prove_step_ms", C.c_double), ("early_witness_ms", C.c_double),
                ("late_ahead_ms", C.c_double)]


class PbsRunStatsC(C.Structure):
    _fields_ = [("seconds", C.c_double), ("outputs_seconds", C.c_double), ("proofs", C.c_size_t), ("prepare_chain_ms", C.c_double),
                ("chain", IvcTimingC)]


class TfheParamsC(C.Structure):
    _fields_ = [("log_N", C.c_uint), ("K", C.c_uint), ("ELL", C.c_uint), ("LOGB", C.c_uint)]


class ProgramDescC(C.Structure):
    _fields_ = [("n_inputs", C.c_uint), ("n_gates", C.c_uint), ("n_luts", C.c_uint), ("n_terms", C.c_size_t), ("gate_first", U64P),
                ("term_src", C.POINTER(C.c_uint32)), ("term_coef", U64P), ("gate_const", U64P), ("gate_lut", C.POINTER(C.c_uint32))]


class KeygenParamsC(C.Structure):
    _fields_ = [("log_N", C.c_uint), ("K", C.c_uint), ("ELL", C.c_uint), ("LOGB", C.c_uint), ("n_lwe", C.c_uint), ("seed", C.c_uint64),
                ("sigma_glwe", C.c_double), ("sigma_lwe", C.c_double)]


class NoiseStatsC(C.Structure):
    _fields_ = [("count", C.c_uint64), ("failures", C.c_uint64), ("max_abs", C.c_uint64), ("sum_abs", C.c_uint64 * 2), ("sum_sq", C.c_uint64 * 3),
                ("sum_signed", C.c_uint64 * 2), ("hist", C.c_uint64 * 65)]


class StepSizesC(C.Structure):
    _fields_ = [("cap_words", C.c_size_t), ("openings_words", C.c_size_t), ("fri_words", C.c_size_t)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, U64P, C.c_size_t, U64P)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, U64P, C.c_size_t)
ALLGATHER_DEV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t)
IVC_STEP_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint)
IVC_CHECKPOINT_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint, C.POINTER(C.c_uint8), C.c_size_t)
PBS_PROOF_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t, C.c_char_p)
AGGREGATE_FN = C.CFUNCTYPE(None, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t, C.c_void_p)   # vpbs_aggregate_fn
AGGREGATE_TREE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t)   # vpbs_aggregate_tree_fn
PBS_CHECKPOINT_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_uint, C.POINTER(C.c_uint8), C.c_size_t)


class CommC(C.Structure):
    _fields_ = [("rank", C.c_uint), ("world", C.c_uint), ("allgather", ALLGATHER_FN), ("allreduce_sum", ALLREDUCE_FN),
                ("user", C.c_void_p), ("allgather_dev", ALLGATHER_DEV_FN), ("d_stage_local", C.c_void_p),
                ("d_stage_full", C.c_void_p), ("stage_capacity_words", C.c_size_t)]


# every symbol include/vpbs_prover.h declares: name -> (restype, argtypes)
_VP, _SZ, _UI, _U64, _I = C.c_void_p, C.c_size_t, C.c_uint, C.c_uint64, C.c_int
SIGNATURES = {
    "vpbs_ctx_create": (_I, [_I, _UI, _UI, _UI, C.POINTER(_VP)]),
    "vpbs_ctx_destroy": (None, [_VP]),
    "vpbs_last_error": (C.c_char_p, [_VP]),
    "vpbs_ctx_synchronize": (_I, [_VP]),
    "vpbs_k_poseidon_host": (_I, [U64P, _SZ]),
    "vpbs_k_clock_probe": (_I, [_VP, C.POINTER(C.c_double)]),
    "vpbs_ctx_set_gate_lanes": (_I, [_VP, _UI]),
    "vpbs_ctx_stream": (_VP, [_VP]),
    "vpbs_compat_default": (None, [C.POINTER(CompatC)]),
    "vpbs_ctx_set_compat": (_I, [_VP, C.POINTER(CompatC)]),
    "vpbs_ctx_get_compat": (_I, [_VP, C.POINTER(CompatC)]),
    "vpbs_ctx_set_option": (_I, [_VP, _I, _U64]),
    "vpbs_ctx_get_option": (_I, [_VP, _I, U64P]),
    "vpbs_host_set_poseidon_x8": (_I, [_I]),
    "vpbs_host_set_cpu_budget": (_I, [_UI]),
    "vpbs_host_cpu_budget": (_UI, []),
    "vpbs_hash_pad": (None, [U64P, _SZ, U64P]),
    "vpbs_circuit_digest": (_I, [C.POINTER(CompatC), U64P, _SZ, _UI, U64P]),
    "vpbs_ctx_rate_bits": (_UI, [_VP]),
    "vpbs_ctx_cap_height": (_UI, [_VP]),
    "vpbs_commit_values": (_I, [_VP, U64P, _UI, _UI, C.POINTER(_VP), U64P]),
    "vpbs_commit_coeffs": (_I, [_VP, U64P, _UI, _UI, C.POINTER(_VP), U64P]),
    "vpbs_commit_values_dev": (_I, [_VP, _VP, _UI, _UI, C.POINTER(_VP), U64P]),
    "vpbs_commit_coeffs_dev": (_I, [_VP, _VP, _UI, _UI, C.POINTER(_VP), U64P]),
    "vpbs_commit_sharded_dev": (_I, [_VP, _VP, _I, _UI, _UI, _UI, _UI, C.POINTER(_VP), U64P]),
    "vpbs_batch_free": (None, [_VP]),
    "vpbs_batch_ncols": (_UI, [_VP]),
    "vpbs_batch_log_n": (_UI, [_VP]),
    "vpbs_batch_cap": (_I, [_VP, U64P]),
    "vpbs_batch_coeffs": (_I, [_VP, U64P]),
    "vpbs_batch_lde_rows": (_I, [_VP, _SZ, _SZ, _SZ, U64P]),
    "vpbs_batch_eval_ext": (_I, [_VP, U64P, U64P]),
    "vpbs_batch_open": (_I, [_VP, _SZ, U64P, U64P]),
    "vpbs_challenger_init": (None, [C.POINTER(ChallengerStateC)]),
    "vpbs_challenger_observe": (None, [C.POINTER(ChallengerStateC), U64P, _SZ]),
    "vpbs_challenger_get": (_U64, [C.POINTER(ChallengerStateC)]),
    "vpbs_hash_no_pad": (None, [U64P, _SZ, U64P]),
    "vpbs_hash_chain": (_I, [U64P, _SZ, _SZ, U64P, U64P]),
    "vpbs_hash_chain_links": (_I, [U64P, C.POINTER(U64P), _SZ, _SZ, U64P]),
    "vpbs_fri_params_standard": (None, [_UI, C.POINTER(FriParams)]),
    "vpbs_fri_proof_words": (_SZ, [C.POINTER(FriParams), _UI, C.POINTER(_SZ), _SZ]),
    "vpbs_fri_prove": (_I, [_VP, C.POINTER(_VP), _SZ, C.POINTER(FriInstanceC), C.POINTER(FriParams),
                            C.POINTER(ChallengerStateC), _U64, U64P]),
    "vpbs_step_sizes_get": (_I, [_VP, C.POINTER(StepInputsC), C.POINTER(StepSizesC)]),
    "vpbs_prove_step": (_I, [_VP, C.POINTER(StepInputsC), U64P, U64P, U64P, C.POINTER(ChallengerStateC), U64P]),
    "vpbs_prove_step_sharded": (_I, [_VP, C.POINTER(StepInputsC), C.POINTER(CommC), U64P, U64P, U64P, C.POINTER(ChallengerStateC), U64P]),
    "vpbs_rccl_available": (_I, []),
    "vpbs_rccl_unique_id": (_I, [C.POINTER(C.c_uint8)]),
    "vpbs_comm_rccl_create": (_I, [_VP, C.POINTER(C.c_uint8), _UI, _UI, _SZ, C.POINTER(CommC)]),
    "vpbs_comm_rccl_destroy": (None, [C.POINTER(CommC)]),
    "vpbs_step_proof_to_bytes": (C.c_long, [_VP, C.POINTER(StepInputsC), _UI, U64P, U64P, U64P, C.POINTER(C.c_uint8), _SZ]),
    "vpbs_partial_products": (_I, [_VP, _VP, _VP, _I, _UI, _UI, U64P, U64P, _UI, _UI, _VP]),
    "vpbs_quotient_permutation": (_I, [_VP, _VP, _UI, _VP, _VP, _UI, U64P, U64P, U64P, _UI, _UI, _VP, _VP, _I]),
    "vpbs_gate_default_params": (_I, [C.POINTER(GateC)]),
    "vpbs_gates_layout": (_I, [C.POINTER(GateC), _UI, _UI, C.POINTER(_UI), C.POINTER(_UI)]),
    "vpbs_gate_id": (_I, [C.POINTER(GateC), C.c_char_p, _SZ]),
    "vpbs_gate_terms": (_I, [_VP, _VP, _VP, C.POINTER(GateC), _UI, _UI, U64P, U64P, _UI, _VP]),
    "vpbs_gate_terms_at": (_I, [C.POINTER(GateC), _UI, _UI, U64P, _UI, U64P, _UI, U64P, U64P, _UI, U64P]),
    "vpbs_gate_fill_row": (_I, [C.POINTER(GateC), U64P, U64P]),
    "vpbs_selector_columns": (_I, [C.POINTER(CircuitC), U64P]),
    "vpbs_sigma_values": (_I, [C.POINTER(CircuitC), U64P]),
    "vpbs_generate_witness": (_I, [C.POINTER(CircuitC), U32P, U64P, _SZ, U64P, C.c_char_p, _SZ]),
    "vpbs_witness_plan_create": (_I, [C.POINTER(CircuitC), U32P, _SZ, C.POINTER(C.c_void_p), C.c_char_p, _SZ]),
    "vpbs_witness_plan_run": (_I, [C.c_void_p, U64P, C.c_uint, U64P, C.c_char_p, _SZ]),
    "vpbs_step_proof_from_bytes": (C.c_long, [C.POINTER(VerifyInputsC), C.POINTER(C.c_uint8), _SZ, U64P, U64P, U64P, U64P, _SZ]),
    "vpbs_witness_plan_free": (None, [C.c_void_p]),
    "vpbs_witness_plan_split": (_I, [C.c_void_p, C.POINTER(C.c_uint8), C.c_char_p, _SZ]),
    "vpbs_witness_plan_run_early": (_I, [C.c_void_p, U64P, C.c_uint, U64P, C.POINTER(C.c_void_p), C.c_char_p, _SZ]),
    "vpbs_witness_plan_run_early_recycled": (_I, [C.c_void_p, U64P, C.c_uint, U64P, C.POINTER(C.c_void_p), C.c_char_p, _SZ]),
    "vpbs_witness_plan_run_late": (_I, [C.c_void_p, C.c_void_p, U64P, U64P, C.c_char_p, _SZ]),
    "vpbs_witness_state_free": (None, [C.c_void_p]),
    "vpbs_witness_plan_run_late_packed": (_I, [C.c_void_p, C.c_void_p, U64P, U64P, C.c_char_p, _SZ]),
    "vpbs_witness_plan_late_count": (_SZ, [C.c_void_p]),
    "vpbs_witness_plan_late_stages": (_UI, [C.c_void_p]),
    "vpbs_witness_plan_run_late_stage": (_I, [C.c_void_p, C.c_void_p, _UI, U64P, U64P, C.c_char_p, _SZ]),
    "vpbs_witness_plan_late_input_count": (_SZ, [C.c_void_p]),
    "vpbs_witness_plan_late_input_positions": (_I, [C.c_void_p, U32P]),
    "vpbs_witness_state_from_late_inputs": (_I, [C.c_void_p, U64P, C.POINTER(C.c_void_p)]),
    "vpbs_witness_plan_late_positions": (_I, [C.c_void_p, U32P]),
    "vpbs_witness_plan_stats": (_I, [C.c_void_p, U64P]),
    "vpbs_witness_device_create": (_I, [C.c_void_p, C.c_void_p, C.c_uint, C.POINTER(C.c_void_p)]),
    "vpbs_witness_device_create_early": (_I, [C.c_void_p, C.c_void_p, C.c_uint, C.POINTER(C.c_void_p)]),
    "vpbs_witness_device_read_late_inputs": (_I, [C.c_void_p, C.c_uint, U64P]),
    "vpbs_witness_device_run": (_I, [C.c_void_p, U64P, C.c_uint]),
    "vpbs_witness_device_wires": (_I, [C.c_void_p, C.c_uint, C.c_void_p]),
    "vpbs_witness_device_read": (_I, [C.c_void_p, C.c_uint, U32P, _SZ, U64P]),
    "vpbs_witness_device_free": (None, [C.c_void_p]),
    "vpbs_check_witness": (_I, [C.POINTER(CircuitC), U64P, U64P, C.c_char_p, _SZ]),
    "vpbs_verify_step": (_I, [C.POINTER(VerifyInputsC), U64P, U64P, U64P]),
    "vpbs_proof_verifier_create": (_I, [_VP, C.POINTER(VerifyInputsC), _SZ, _SZ, C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_proof_verifier_run": (C.c_long, [_VP, C.POINTER(C.c_uint8), C.POINTER(_SZ), _SZ, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "vpbs_proof_verifier_free": (None, [_VP]),
    "vpbs_ivc_create": (_I, [_VP, C.POINTER(IvcCircuitC), C.POINTER(IvcCircuitC), _UI, _UI, _SZ, C.POINTER(CommC), C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_ivc_free": (None, [_VP]),
    "vpbs_ivc_verifier_data": (_I, [_VP, U64P, U64P]),
    "vpbs_ivc_set_step_callback": (_I, [_VP, IVC_STEP_FN, _VP]),
    "vpbs_ivc_set_device_witness": (_I, [_VP, _UI, _UI, _UI, _I]),
    "vpbs_ivc_last_error": (C.c_char_p, [_VP]),
    "vpbs_prove_step_sharded_fail": (_I, [_VP, C.POINTER(StepInputsC), C.POINTER(CommC), _I]),
    "vpbs_comm_allgather_checked": (_I, [C.POINTER(CommC), U64P, _SZ, U64P, _I]),
    "vpbs_host_set_late_threads": (_I, [_UI]),
    "vpbs_host_set_early_threads": (_I, [_UI]),
    "vpbs_host_set_blocking_sync": (_I, [_I]),
    "vpbs_host_blocking_sync": (_I, []),
    "vpbs_host_set_sync_word": (_I, [_I]),
    "vpbs_witness_device_has_late": (_I, [_VP]),
    "vpbs_witness_device_run_late": (_I, [C.c_void_p, C.c_uint, U64P]),
    "vpbs_ctx_device": (_I, [_VP]),
    "vpbs_witness_checker_create": (_I, [_VP, C.POINTER(CircuitC), C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_witness_checker_free": (None, [_VP]),
    "vpbs_witness_checker_run": (_I, [_VP, _VP, _I, U64P, C.c_char_p, _SZ]),
    "vpbs_prove_step_checked": (_I, [_VP, _VP, C.POINTER(StepInputsC), U64P, U64P, U64P, C.POINTER(ChallengerStateC), U64P]),
    "vpbs_ivc_set_check_witness": (_I, [_VP, _I]),
    "vpbs_ivc_witness_checks": (_I, [_VP, U64P]),
    "vpbs_ivc_prove_pbs": (C.c_long, [_VP, U64P, U64P, U64P, U64P, _UI, _UI, C.POINTER(C.c_uint8), _SZ, C.POINTER(IvcTimingC), C.c_char_p, _SZ]),
    "vpbs_verify_pbs": (_I, [C.POINTER(VerifyPbsInputsC), C.POINTER(C.c_uint8), _SZ, C.c_char_p, _SZ]),
    "vpbs_verify_pbs_prefix": (_I, [C.POINTER(VerifyPbsInputsC), C.POINTER(C.c_uint8), _SZ, C.POINTER(_UI), C.c_char_p, _SZ]),
    "vpbs_ivc_set_checkpoint": (_I, [_VP, _UI, IVC_CHECKPOINT_FN, _VP]),
    "vpbs_ivc_resume_pbs": (C.c_long, [_VP, U64P, U64P, U64P, U64P, _UI, C.POINTER(C.c_uint8), _SZ, _UI, C.POINTER(C.c_uint8), _SZ,
                                       C.POINTER(IvcTimingC), C.c_char_p, _SZ]),
    "vpbs_pbs_key_hash": (_I, [U64P, U64P, _UI, _SZ, U64P]),
    "vpbs_pbs_reason_text": (C.c_char_p, [_I]),
    "vpbs_pbs_verifier_create": (_I, [_VP, C.POINTER(VerifyPbsInputsC), U64P, _SZ, C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_pbs_verifier_run": (C.c_long, [_VP, C.POINTER(C.c_uint8), C.POINTER(_SZ), _SZ, U64P, _I, U64P, U64P, C.POINTER(C.c_uint8),
                                         C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "vpbs_pbs_verifier_free": (None, [_VP]),
    "vpbs_ring_verifier_create": (_I, [_VP, C.POINTER(VerifyPbsInputsC), _UI, _SZ, C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_ring_verifier_set_key": (_I, [_VP, _UI, U64P]),
    "vpbs_ring_verifier_clear_key": (_I, [_VP, _UI]),
    "vpbs_ring_verifier_count": (C.c_long, [_VP]),
    "vpbs_ring_verifier_run": (C.c_long, [_VP, C.POINTER(C.c_uint8), C.POINTER(_SZ), _SZ, _VP, U64P, _SZ, _VP, U64P, U64P, C.POINTER(C.c_uint8),
                                          C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_char_p, _SZ]),
    "vpbs_ring_verifier_free": (None, [_VP]),
    "vpbs_blind_rotate_step": (_I, [_VP, C.POINTER(TfheParamsC), _UI, _VP, _VP, _VP, _I, _I, _I, _VP, _I]),
    "vpbs_pbs_accumulator_chain": (_I, [_VP, C.POINTER(TfheParamsC), _UI, U64P, U64P, U64P, U64P, U64P]),
    "vpbs_host_alloc": (_VP, [_SZ]),
    "vpbs_host_free": (None, [_VP]),
    "vpbs_device_alloc": (_I, [_VP, _SZ, C.POINTER(_VP)]),
    "vpbs_device_upload": (_I, [_VP, _VP, U64P, _SZ]),
    "vpbs_device_upload_bg": (_I, [_VP, _VP, _VP, _SZ]),
    "vpbs_device_upload_rows": (_I, [_VP, _VP, _VP, _UI, _SZ, _SZ, _SZ]),
    "vpbs_witness_plan_late_rows": (_I, [_VP, C.POINTER(_SZ)]),
    "vpbs_device_scatter": (_I, [_VP, _VP, _VP, _VP, _SZ, _VP]),
    "vpbs_device_free": (None, [_VP, _VP]),
    "vpbs_keygen": (_I, [_VP, C.POINTER(KeygenParamsC), U64P, U64P, U64P, _VP, _VP, _I]),
    "vpbs_lwe_encrypt": (_I, [C.POINTER(KeygenParamsC), U64P, _U64, _U64, U64P]),
    "vpbs_testv": (_I, [_UI, _UI, U64P, U64P]),
    "vpbs_glwe_decrypt": (_I, [_VP, _UI, _UI, U64P, U64P, U64P]),
    "vpbs_bootstrapper_create": (_I, [_VP, C.POINTER(TfheParamsC), _UI, _VP, _VP, _I, _SZ, C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_bootstrapper_run": (C.c_long, [_VP, _VP, _SZ, _VP, _I, _VP, _VP, _VP, _I]),
    "vpbs_bootstrapper_run_from": (C.c_long, [_VP, _VP, _SZ, _VP, _VP, _VP, _I, _VP, _VP, _VP, _I]),
    "vpbs_bootstrapper_free": (None, [_VP]),
    "vpbs_keyring_create": (_I, [_VP, C.POINTER(TfheParamsC), _UI, _SZ, _SZ, C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_keyring_add": (_I, [_VP, _VP, _VP, _I, C.POINTER(_UI)]),
    "vpbs_keyring_remove": (_I, [_VP, _UI]),
    "vpbs_keyring_count": (_SZ, [_VP]),
    "vpbs_keyring_run": (C.c_long, [_VP, _VP, _SZ, _VP, _VP, _I, _VP, _VP, _VP, _I]),
    "vpbs_keyring_run_from": (C.c_long, [_VP, _VP, _SZ, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _I]),
    "vpbs_keyring_free": (None, [_VP]),
    "vpbs_pbs_prover_create": (_I, [_I, C.POINTER(IvcCircuitC), C.POINTER(IvcCircuitC), C.POINTER(TfheParamsC), _UI, _VP, _VP, _I, _UI, _UI,
                                    C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_pbs_prover_run": (C.c_long, [_VP, U64P, _SZ, U64P, _I, _UI, U64P, U64P, PBS_PROOF_FN, _VP, C.c_char_p, _SZ]),
    "vpbs_pbs_prover_resume": (C.c_long, [_VP, U64P, _SZ, U64P, _I, _VP, _VP, _UI, U64P, U64P, PBS_PROOF_FN, _VP, C.c_char_p, _SZ]),
    "vpbs_pbs_prover_key_hash": (_I, [_VP, U64P]),
    "vpbs_pbs_prover_verifier_data": (_I, [_VP, U64P, U64P]),
    "vpbs_pbs_prover_set_check_witness": (_I, [_VP, _I]),
    "vpbs_pbs_prover_witness_checks": (_I, [_VP, U64P]),
    "vpbs_pbs_prover_set_checkpoint": (_I, [_VP, _UI, PBS_CHECKPOINT_FN, _VP]),
    "vpbs_pbs_prover_last_run": (_I, [_VP, C.POINTER(PbsRunStatsC)]),
    "vpbs_pbs_prover_free": (None, [_VP]),
    "vpbs_ring_prover_create": (_I, [_I, C.POINTER(IvcCircuitC), C.POINTER(IvcCircuitC), C.POINTER(TfheParamsC), _UI, _SZ, _UI, _UI, C.POINTER(_VP),
                                     C.c_char_p, _SZ]),
    "vpbs_ring_prover_add": (_I, [_VP, _VP, _VP, _I, C.POINTER(_UI), C.c_char_p, _SZ]),
    "vpbs_ring_prover_remove": (_I, [_VP, _UI, C.c_char_p, _SZ]),
    "vpbs_ring_prover_key_hash": (_I, [_VP, _UI, U64P]),
    "vpbs_ring_prover_keyring": (_VP, [_VP]),
    "vpbs_ring_prover_context": (_VP, [_VP]),
    "vpbs_ring_prover_run": (C.c_long, [_VP, U64P, _SZ, _VP, U64P, _I, _UI, U64P, U64P, PBS_PROOF_FN, _VP, C.c_char_p, _SZ]),
    "vpbs_ring_prover_resume": (C.c_long, [_VP, U64P, _SZ, _VP, U64P, _I, _VP, _VP, _UI, U64P, U64P, PBS_PROOF_FN, _VP, C.c_char_p, _SZ]),
    "vpbs_ring_prover_verifier_data": (_I, [_VP, U64P, U64P]),
    "vpbs_ring_prover_set_check_witness": (_I, [_VP, _I]),
    "vpbs_ring_prover_witness_checks": (_I, [_VP, U64P]),
    "vpbs_ring_prover_set_checkpoint": (_I, [_VP, _UI, PBS_CHECKPOINT_FN, _VP]),
    "vpbs_ring_prover_last_run": (_I, [_VP, C.POINTER(PbsRunStatsC)]),
    "vpbs_ring_prover_free": (None, [_VP]),
    "vpbs_program_create": (_I, [_VP, C.POINTER(ProgramDescC), C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_program_levels": (C.c_long, [_VP, C.POINTER(_UI)]),
    "vpbs_program_run": (C.c_long, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "vpbs_program_run_batch": (C.c_long, [_VP, _VP, _VP, _SZ, _VP, _VP, _VP, _VP, _VP, _I]),
    "vpbs_program_prove": (C.c_long, [_VP, _VP, U64P, U64P, _UI, U64P, U64P, PBS_PROOF_FN, _VP, C.c_char_p, _SZ]),
    "vpbs_program_prove_batch": (C.c_long, [_VP, _VP, U64P, _SZ, _VP, U64P, _UI, U64P, U64P, PBS_PROOF_FN, _VP, C.c_char_p, _SZ]),
    "vpbs_program_verify": (C.c_long, [_VP, _VP, U64P, U64P, U64P, C.POINTER(C.c_uint8), C.POINTER(_SZ), C.POINTER(C.c_uint8),
                                       C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "vpbs_program_verify_batch": (C.c_long, [_VP, _VP, U64P, _SZ, _VP, U64P, U64P, C.POINTER(C.c_uint8), C.POINTER(_SZ), C.POINTER(C.c_uint8),
                                             C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_char_p, _SZ]),
    "vpbs_program_free": (None, [_VP]),
    "vpbs_program_create_multi": (_I, [_VP, C.POINTER(ProgramDescC), C.POINTER(_UI), C.POINTER(_UI), C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_program_wires": (C.c_long, [_VP, C.POINTER(_UI)]),
    "vpbs_lwe_snap": (_I, [_VP, _UI, _UI, _VP, _SZ, _VP, _I]),
    "vpbs_lwe_extract_at": (_I, [_VP, _UI, _UI, _UI, _VP, _SZ, _VP, _VP, _SZ, _VP, _I]),
    "vpbs_lut_testv_multi": (_I, [_UI, _UI, _UI, U64P, _U64, U64P]),
    "vpbs_lwe_extract": (_I, [_VP, _UI, _UI, _UI, _VP, _SZ, _VP, _I]),
    "vpbs_lwe_decrypt": (_I, [U64P, U64P, _UI, U64P]),
    "vpbs_lwe_encrypt_batch": (_I, [_VP, C.POINTER(KeygenParamsC), _VP, _I, _VP, _SZ, _U64, _VP, _I]),
    "vpbs_lut_testv": (_I, [_UI, _UI, U64P, _U64, U64P]),
    "vpbs_lwe_decode_batch": (_I, [_VP, _VP, _I, _VP, _SZ, _UI, _U64, _U64, _VP, _VP, _VP, _VP, C.POINTER(NoiseStatsC), _I]),
    "vpbs_lwe_rotation_batch": (_I, [_VP, _VP, _I, _VP, _SZ, _UI, _UI, _UI, _UI, _VP, _VP, _VP, _VP, C.POINTER(NoiseStatsC), _I]),
    "vpbs_keygen_seeded": (_I, [_VP, C.POINTER(KeygenParamsC), _U64, _VP, _VP, U64P, U64P, U64P, _VP, _VP, _I]),
    "vpbs_key_expand": (_I, [_VP, C.POINTER(TfheParamsC), _UI, _U64, _VP, _VP, _I, _VP, _VP, _I]),
    "vpbs_lwe_encrypt_seeded_batch": (_I, [_VP, C.POINTER(KeygenParamsC), _U64, _VP, _I, _VP, _SZ, _U64, _VP, _I]),
    "vpbs_lwe_expand_batch": (_I, [_VP, _UI, _U64, _U64, _VP, _SZ, _VP, _I]),
    "vpbs_keyring_add_seeded": (_I, [_VP, _U64, _VP, _VP, _I, C.POINTER(_UI)]),
    "vpbs_ring_prover_add_seeded": (_I, [_VP, _U64, _VP, _VP, _I, C.POINTER(_UI), C.c_char_p, _SZ]),
    "vpbs_k_poseidon_batch": (_I, [_VP, U64P, _SZ]),
    "vpbs_k_hash_rows": (_I, [_VP, U64P, _SZ, _UI, U64P]),
    "vpbs_k_intt": (_I, [_VP, U64P, _UI, _UI, U64P]),
    "vpbs_k_coset_lde": (_I, [_VP, U64P, _UI, _UI, _UI, _U64, U64P]),
    "vpbs_k_merkle_cap": (_I, [_VP, U64P, _SZ, _UI, _UI, U64P]),
    "vpbs_k_negacyclic_ntt": (_I, [_VP, U64P, _UI, _UI, _I]),
    "vpbs_ntt_params": (_I, [_UI, U64P, U64P, U64P]),
    "vpbs_timing_enable": (_I, [_VP, _I]),
    "vpbs_timing_report": (_I, [_VP, C.c_char_p, _SZ]),
    "vpbs_timing_shader_clock": (_I, [_VP, C.POINTER(C.c_double), C.POINTER(_UI)]),
    "vpbs_aggregate_reason_text": (C.c_char_p, [_I]),
    "vpbs_aggregate_root": (_I, [_UI, _UI, _UI, U64P, _SZ, U64P, _SZ, _VP, U64P, U64P, U64P, _SZ, _VP, U64P]),
    "vpbs_verify_aggregate": (_I, [_VP, _SZ, U64P, _SZ, _VP, U64P, U64P, U64P, _SZ, _VP, C.POINTER(C.c_uint8), _SZ, C.POINTER(_I), C.c_char_p, _SZ]),
    "vpbs_aggregator_create": (_I, [_VP, _VP, _SZ, _VP, _UI, C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_aggregator_verifier_data": (_I, [_VP, U64P]),
    "vpbs_aggregator_run": (C.c_long, [_VP, C.POINTER(C.c_uint8), C.POINTER(_SZ), _SZ, C.POINTER(C.c_uint8), _SZ, _VP, C.c_char_p, _SZ]),
    "vpbs_aggregator_last_run": (_I, [_VP, _VP]),
    "vpbs_aggregator_free": (None, [_VP]),
    "vpbs_aggregator_set_device_witness": (_I, [_VP, _UI, C.c_char_p, _SZ]),
    "vpbs_aggregator_device_stats": (_I, [_VP, U64P]),
    "vpbs_aggregate_level_jobs": (_I, [C.POINTER(_SZ), _SZ, _UI, _VP, _VP, _VP, _SZ]),
    "vpbs_aggregator_run_many": (C.c_long, [_VP, C.POINTER(C.c_uint8), C.POINTER(_SZ), C.POINTER(_SZ), _SZ, AGGREGATE_TREE_FN, _VP, C.c_char_p, _SZ]),
    "vpbs_aggregate_verifier_create": (_I, [_VP, _VP, _SZ, C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_aggregate_verifier_run": (_I, [_VP, C.POINTER(C.c_uint8), _SZ, _SZ, _VP, _SZ, _VP, _VP, _VP, _VP, _SZ, _VP, _I, C.POINTER(_I),
                                         C.c_char_p, _SZ]),
    "vpbs_aggregate_verifier_root": (_I, [_VP, _SZ, _VP, _SZ, _VP, _VP, _VP, _VP, _SZ, _VP, _I, U64P, C.c_char_p, _SZ]),
    "vpbs_aggregate_verifier_free": (None, [_VP]),
    "vpbs_aggregate_verifier_create_many": (_I, [_VP, _VP, _SZ, _SZ, C.POINTER(_VP), C.c_char_p, _SZ]),
    "vpbs_aggregate_verifier_run_many": (C.c_long, [_VP, C.POINTER(C.c_uint8), C.POINTER(_SZ), _SZ, C.POINTER(_SZ), _VP, _SZ, _VP, _VP, _VP, _VP, _SZ,
                                                    _VP, _I, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_char_p, _SZ]),
    "vpbs_aggregate_verifier_roots_many": (_I, [_VP, _SZ, C.POINTER(_SZ), _VP, _SZ, _VP, _VP, _VP, _VP, _SZ, _VP, _I, U64P, C.POINTER(C.c_uint8),
                                                C.c_char_p, _SZ]),
    "vpbs_program_gate_inputs": (_I, [_VP, _UI, _UI, _UI, U64P, _SZ, U64P, U64P, C.c_char_p, _SZ]),
    "vpbs_program_aggregate_root": (_I, [_VP, _UI, _UI, _UI, U64P, U64P, U64P, U64P, U64P, U64P, C.c_char_p, _SZ]),
    "vpbs_program_verify_aggregate": (_I, [_VP, _VP, U64P, U64P, U64P, U64P, C.POINTER(C.c_uint8), _SZ, C.POINTER(_I), C.c_char_p, _SZ]),
    "vpbs_program_prove_aggregate": (C.c_long, [_VP, _VP, _VP, U64P, U64P, U64P, U64P, C.POINTER(C.c_uint8), _SZ, _VP, PBS_PROOF_FN, _VP, C.c_char_p,
                                                _SZ]),
    "vpbs_program_prove_aggregate_batch": (C.c_long, [_VP, _VP, _VP, U64P, _SZ, _VP, U64P, U64P, U64P, AGGREGATE_FN, PBS_PROOF_FN, _VP, C.c_char_p,
                                                      _SZ]),
    "vpbs_program_verify_aggregate_batch": (C.c_long, [_VP, _VP, U64P, _SZ, _VP, U64P, _SZ, U64P, U64P, C.POINTER(C.c_uint8), C.POINTER(_SZ),
                                                       C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_char_p, _SZ]),
}

# test entries (csrc/test_entries.h): exported for the suite, not part of the C ABI
INTERNAL_SIGNATURES = {
    "vpbs_test_ivc_preset_matrix": (_I, [_SZ, _SZ, _SZ, _SZ, _UI, _UI, _UI, U64P, U64P, U64P, U64P, U64P, U64P, U64P, U64P]),
    "vpbs_test_pbs_prover_preset_matrix": (_I, [_VP, U64P, U64P, _UI, _UI, U64P]),
    "vpbs_test_pbs_prover_preset_words": (_SZ, [_VP]),
    "vpbs_test_pbs_prover_dummy_proof": (_I, [_VP, U64P]),
    "vpbs_test_aggregator_preset_matrix": (_I, [_VP, _UI, U64P, _SZ, _VP, _UI, U64P]),
    "vpbs_test_stream_counts": (_I, [_I, C.POINTER(_UI)]),
}

_lib = None


def build_library(force=False):
    """Compile the HIP library in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    args = ["make", "-C", os.path.join(PKG_DIR, "csrc"), "-j4"]
    if force:
        subprocess.check_call(args + ["clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    """The loaded HIP library.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VpbsError("libvpbs_hip.so is missing: run __graft_entry__.build() (make -C verifiable-fhe-paper_amd/csrc). "
                            "There is no CPU fallback for the proving path.")
        # PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.so.1.  Two HSA runtimes in one
        # process cannot both own the GPU, so when torch is present it is imported FIRST: the dynamic loader then
        # resolves this library's DT_NEEDED libamdhip64.so.7 to the copy torch already mapped (same soname).
        if os.environ.get("VPBS_HIP_RUNTIME", "torch") == "torch":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(INTERNAL_SIGNATURES.items()):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def _u64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


# ---- the pointer vocabulary: every array or device address reaches the library through one of these four ----
def _ptr(a):
    """a contiguous uint64 array that is known not to be empty -> U64P"""
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(U64P)


def _keep_ptr(a):
    """a uint64 array -> U64P, a valid pointer for an empty array too (the pointer keeps what it points to alive); None stays None"""
    return None if a is None else _ptr(a if a.size else np.zeros(1, np.uint64))


def _keep_u32(a):
    """the same for a uint32 array -> U32P"""
    if a is None:
        return None
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return (a if a.size else np.zeros(1, np.uint32)).ctypes.data_as(U32P)


def _dev(x):
    """a device address (an integer) -> c_void_p; None or 0 -> None"""
    return C.c_void_p(int(x)) if x else None


def _cts_testv(who, N, n_lwe, cts, testv):
    """the shapes every bootstrapping call checks: cts [count][n + 1] and testv [N] shared or [count][N] -> (cts, testv), contiguous uint64"""
    c, tv = _u64(cts), _u64(testv)
    if c.ndim != 2 or c.shape[1] != n_lwe + 1 or tv.shape not in ((N,), (c.shape[0], N)):
        raise ValueError("%s: expected cts [count][%d] and testv [%d] or [count][%d]" % (who, n_lwe + 1, N, N))
    return c, tv


def _packed(proofs, offsets=None, shape=None, outputs=0):
    """the serialised proofs of one call -- a list of them, or with `offsets` the (buf, offsets) of pack_proofs -- as the C ABI takes them
    -> (count, bytes pointer, size_t offsets pointer, `outputs` np.uint8 arrays of `shape` ([count] unless given) for the verdicts and
    reasons, their pointers)"""
    buf, offs = pack_proofs(proofs) if offsets is None else (proofs, offsets)
    buf, offs = np.ascontiguousarray(buf, dtype=np.uint8), np.ascontiguousarray(offs, dtype=np.uint64)
    count = offs.size - 1
    outs = tuple(np.zeros(max(count, 0) if shape is None else shape, np.uint8) for _ in range(outputs))
    data = buf.ctypes.data_as(U8P) if buf.size else (C.c_uint8 * 1)()
    return count, data, offs.ctypes.data_as(SZP), outs, [o.ctypes.data_as(U8P) for o in outs]


class _Handle:
    """The lifecycle of every object that wraps a C handle whose entry points are named <_prefix>_*: h is the handle (None once freed),
    ctx the Context it lives on (None for an object without one).  An object on a context registers with it (_created): it must not
    outlive the context, so Context.close() closes the survivors first -- in any order: no destructor of the library reaches into another
    registered object, only into the context and into what the object itself made.  Closing again, or after the context, does nothing."""
    _prefix = None
    _owns = True   # False: a view of a handle that another object frees (RingProver.keyring) -- close() only forgets it
    h = ctx = None

    def _entry(self, name):
        return getattr(lib(), "%s_%s" % (self._prefix, name))

    @staticmethod
    def _fail(what, rc, text=None):
        """the VpbsError of a failed call, with .status: "<what>: status <rc>: <text>" (no what, no text: that part is left out)"""
        return VpbsError("%sstatus %d%s" % (what + ": " if what else "", rc, "" if text is None else ": " + text), status=rc)

    def _construct(self, ctx, *args, entry="create", what=None, status=False):
        """<_prefix>_<entry>(*args, &handle, err, 512), then _created(ctx).  A status other than 0 raises VpbsError "<what>: status <rc>:
        <the library's message>" (what: the entry point unless given; status: with .status)"""
        h, err = C.c_void_p(), C.create_string_buffer(512)
        rc = self._entry(entry)(*args, C.byref(h), err, 512)
        if rc:
            e = self._fail("%s_%s" % (self._prefix, entry) if what is None else what, rc, err.value.decode())
            raise e if status else VpbsError(str(e))
        self.h = h
        self._created(ctx)

    def _created(self, ctx):
        self.ctx = ctx
        if ctx is not None:
            ctx._batches.add(self)

    def _release(self):
        """<_prefix>_free(h); a subclass lets go first of what goes with the handle (RingProver: its view)"""
        self._entry("free")(self.h)

    def close(self):
        if self.h:
            try:
                if self._owns:
                    self._release()
            finally:
                self.h = None
                if self.ctx is not None:
                    self.ctx._batches.discard(self)

    free = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ChallengerState:
    """Host Challenger (plonky2 iop/challenger.rs) of the product library."""

    def __init__(self):
        self.c = ChallengerStateC()
        lib().vpbs_challenger_init(C.byref(self.c))

    def clone(self):
        o = ChallengerState()
        C.memmove(C.byref(o.c), C.byref(self.c), C.sizeof(ChallengerStateC))
        return o

    def observe(self, elems):
        e = _u64(elems).reshape(-1)
        lib().vpbs_challenger_observe(C.byref(self.c), _ptr(e), e.size)

    def get(self):
        return int(lib().vpbs_challenger_get(C.byref(self.c)))

    def get_n(self, n):
        return [self.get() for _ in range(n)]

    def get_ext(self):
        return np.array(self.get_n(2), np.uint64)

    def state_words(self):
        c = self.c
        return (list(c.sponge), list(c.input)[:c.input_len], list(c.output)[:c.output_len])


def hash_no_pad(x):
    x = _u64(x).reshape(-1)
    out = np.zeros(4, np.uint64)
    lib().vpbs_hash_no_pad(_ptr(x), x.size, _ptr(out))
    return out


def host_set_poseidon_x8(on):
    """vpbs_host_set_poseidon_x8: the host's eight-permutations-per-AVX-512-register Poseidon on / off (process-wide) -> what is in force"""
    return bool(lib().vpbs_host_set_poseidon_x8(1 if on else 0))


def host_set_cpu_budget(cpus):
    """vpbs_host_set_cpu_budget: the CPUs this process may use for the witness-generation pools (0 = the default: affinity and cgroup quota)"""
    lib().vpbs_host_set_cpu_budget(int(cpus))
    return lib().vpbs_host_cpu_budget()


def host_cpu_budget():
    """vpbs_host_cpu_budget: the CPUs this process may use (affinity, cgroup quota, vpbs_host_set_cpu_budget), without changing anything"""
    return lib().vpbs_host_cpu_budget()


def host_set_late_threads(threads):
    """vpbs_host_set_late_threads: threads of the late witness phase's pool for plans split afterwards (0 = default).  A host that runs ONE
    IVC chain and has 16 CPUs asks for 14: the last late stage of the in-circuit verifier is 28 independent FRI queries."""
    lib().vpbs_host_set_late_threads(int(threads))


def host_set_early_threads(threads):
    """vpbs_host_set_early_threads: threads of the early witness phase's pool for pools created afterwards (0 = default)"""
    lib().vpbs_host_set_early_threads(int(threads))


def early_threads_for(chains, cpus=None):
    """what the tools ask for: ONE thread per chain's early phase from four chains per process on -- the phase runs ahead of the proof and
    has `chains` proof times to finish in, a pool only spins between its levels (eight chains on 16 CPUs: the same throughput with 42
    instead of 78 CPU-ms per proof) -- the default (a pool of half the CPUs, at most 8) for fewer chains, where the early phase of the next
    step can be what the chain waits for"""
    return 1 if chains >= 4 else 0


def late_threads_for(chains, cpus=None):
    """what the tools ask for: 14 for a single chain on a host with at least 16 CPUs for this process (its latency is the late phase's); 4
    from four chains per process on (round 5: eight chains on 16 CPUs prove 7.0 ms per chained proof with 4 or 8 late threads each, at 34-38
    instead of 40-47 CPU-ms per proof -- tools/experiments/ivc_matrix.sh VPBS_LATE_THREADS=4:16:8:0:200); the default otherwise"""
    cpus = host_cpu_budget() if cpus is None else cpus
    if chains == 1 and cpus >= 16:
        return 14
    return 4 if chains >= 4 and cpus >= 8 else 0      # fewer CPUs: the default (half the CPUs: one thread at 2 CPUs) is already below 4


def hash_pad(x=()):
    """PoseidonHash::hash_pad (pad10*1, then hash_no_pad)"""
    x = _u64(x).reshape(-1)
    out = np.zeros(4, np.uint64)
    lib().vpbs_hash_pad(_ptr(x) if x.size else None, x.size, _ptr(out))
    return out


def circuit_digest(cs_cap, log_n, k=None):
    """vpbs_circuit_digest: verifier_only.circuit_digest as CircuitBuilder::build derives it (formula: compat.digest_domain_separator)"""
    cap = _u64(cs_cap).reshape(-1)
    out = np.zeros(4, np.uint64)
    rc = lib().vpbs_circuit_digest(C.byref(k) if k is not None else None, _ptr(cap), cap.size, log_n, _ptr(out))
    if rc:
        raise VpbsError("vpbs_circuit_digest: malformed cap")
    return out


class GateSet:
    """The gate set of a circuit, laid out like CircuitBuilder::build + selector_polynomials (vpbs_gates_layout).
    spec: list of (kind name, p0, p1, p2) with zeros meaning the *_from_config defaults."""

    def __init__(self, spec, max_degree=9):  # CircuitBuilder::build: selector_polynomials(.., quotient_degree_factor + 1)
        arr = (GateC * len(spec))()
        for g, item in zip(arr, spec):
            name, *ps = item if isinstance(item, (tuple, list)) else (item,)
            ps = list(ps) + [0] * (3 - len(ps))
            g.kind, g.p0, g.p1, g.p2 = GATE_KINDS.index(name), ps[0], ps[1], ps[2]
            if lib().vpbs_gate_default_params(C.byref(g)):
                raise VpbsError("unsupported gate parameters: %r" % (item,))
        ns, ngc = C.c_uint(), C.c_uint()
        if lib().vpbs_gates_layout(arr, len(spec), max_degree, C.byref(ns), C.byref(ngc)):
            raise VpbsError("vpbs_gates_layout failed")
        self.arr, self.n = arr, len(spec)
        self.num_selectors, self.num_gate_constraints = ns.value, ngc.value
        self.num_constants = max(g.num_constants for g in arr)

    def __iter__(self):
        return iter(self.arr)

    def by_kind(self, name):
        return next(g for g in self.arr if g.kind == GATE_KINDS.index(name))

    def ids(self):
        out = []
        for g in self.arr:
            buf = C.create_string_buffer(4096)
            if lib().vpbs_gate_id(C.byref(g), buf, 4096) < 0:
                raise VpbsError("vpbs_gate_id failed")
            out.append(buf.value.decode())
        return out

    def selector_values(self, gate):
        """the value of every selector polynomial on a row that holds `gate` (selector_polynomials)"""
        return [gate.index if s == gate.selector_index else UNUSED_SELECTOR for s in range(self.num_selectors)]

    def terms_at(self, constants_at, wires_at, pi_hash, alphas):
        """vpbs_gate_terms_at: folded gate constraints at one GF(p^2) point from openings [..][2] -> [nc][2]"""
        c, w, h, a = _u64(constants_at), _u64(wires_at), _u64(pi_hash), _u64(alphas)
        out = np.zeros((a.size, 2), np.uint64)
        rc = lib().vpbs_gate_terms_at(self.arr, self.n, self.num_selectors, _ptr(c), c.shape[0], _ptr(w), w.shape[0], _ptr(h), _ptr(a),
                                      a.size, _ptr(out))
        if rc:
            raise VpbsError("vpbs_gate_terms_at failed: %d" % rc)
        return out

    @staticmethod
    def fill_row(gate, constants, row):
        """vpbs_gate_fill_row: run the gate's generators on one trace row (in place on a uint64 array)"""
        c = _u64(constants if constants is not None and len(constants) else [0])
        assert row.dtype == np.uint64 and row.flags["C_CONTIGUOUS"]
        rc = lib().vpbs_gate_fill_row(C.byref(gate), _ptr(c), _ptr(row))
        if rc:
            raise VpbsError("vpbs_gate_fill_row failed: %d" % rc)
        return row


class Circuit:
    """vpbs_circuit: gate instance per row, constants columns, copy constraints (host-side description of a circuit)."""

    def __init__(self, gates, log_n, row_gate, constants, copies, n_wires=135, n_routed=80, generators=()):
        """generators: [(kind name, p0, [input positions (column, row)], [output positions]), ...] gadget-level generators"""
        n = 1 << log_n
        self.gates, self.log_n, self.n, self.n_wires, self.n_routed = gates, log_n, n, n_wires, n_routed
        self.row_gate = np.ascontiguousarray(row_gate, dtype=np.uint32)
        self.constants = _u64(constants)
        self.copies = np.ascontiguousarray(np.asarray(copies, dtype=np.uint32).reshape(-1, 2))
        assert self.row_gate.shape == (n,) and self.constants.shape[1] == n
        c = CircuitC()
        c.log_n, c.n_wires, c.n_routed = log_n, n_wires, n_routed
        c.gates, c.n_gates, c.num_selectors = gates.arr, gates.n, gates.num_selectors
        c.row_gate = self.row_gate.ctypes.data_as(U32P)
        c.constants, c.n_constants_cols = _ptr(self.constants), self.constants.shape[0]
        c.copies, c.n_copies = self.copies.ctypes.data_as(U32P), self.copies.shape[0]
        self._gen_keep = []
        self.generator_list = list(generators)
        if generators:
            arr = (GeneratorC * len(generators))()
            for g, (kind, p0, ins, outs) in zip(arr, generators):
                i = np.array([cc * n + rr for cc, rr in ins], dtype=np.uint32)
                o = np.array([cc * n + rr for cc, rr in outs], dtype=np.uint32)
                self._gen_keep += [i, o]
                g.kind, g.p0 = GENERATOR_KINDS.index(kind), p0
                g.inp, g.n_in, g.out, g.n_out = i.ctypes.data_as(U32P), i.size, o.ctypes.data_as(U32P), o.size
            c.generators, c.n_generators = arr, len(generators)
            self._gen_keep.append(arr)
        self.c = c

    def selector_columns(self):
        out = np.zeros((self.gates.num_selectors, self.n), np.uint64)
        if lib().vpbs_selector_columns(C.byref(self.c), _ptr(out)):
            raise VpbsError("vpbs_selector_columns failed")
        return out

    def sigma_values(self):
        out = np.zeros((self.n_routed, self.n), np.uint64)
        if lib().vpbs_sigma_values(C.byref(self.c), _ptr(out)):
            raise VpbsError("vpbs_sigma_values failed")
        return out

    def check_witness(self, wires, pi_hash):
        """vpbs_check_witness -> (ok, message of the first violation)"""
        w, h = _u64(wires), _u64(pi_hash)
        assert w.shape == (self.n_wires, self.n)
        err = C.create_string_buffer(512)
        rc = lib().vpbs_check_witness(C.byref(self.c), _ptr(w), _ptr(h), err, 512)
        if rc < 0:
            raise VpbsError("vpbs_check_witness: " + err.value.decode())
        return rc == 1, err.value.decode()

    def generate_witness(self, presets):
        """presets: {(column, row): value} (the PartialWitness) -> wires [n_wires][n]"""
        pos = np.array([c * self.n + r for (c, r) in presets], dtype=np.uint32)
        val = _u64([int(v) for v in presets.values()])
        out = np.zeros((self.n_wires, self.n), np.uint64)
        err = C.create_string_buffer(512)
        rc = lib().vpbs_generate_witness(C.byref(self.c), pos.ctypes.data_as(U32P), _ptr(val) if val.size else None, pos.size, _ptr(out), err, 512)
        if rc:
            raise VpbsError("vpbs_generate_witness: " + err.value.decode())
        return out


    def witness_plan(self, positions):
        """vpbs_witness_plan_create for a PartialWitness that sets `positions` [(column, row), ...] -> WitnessPlan"""
        return WitnessPlan(self, positions)


class WitnessPlan(_Handle):
    """vpbs_witness_plan: the compiled witness generator of one circuit (create once, run per PartialWitness)."""
    _prefix = "vpbs_witness_plan"

    def __init__(self, circuit, positions):
        self.circuit = circuit
        pos = np.array([c * circuit.n + r for (c, r) in positions], dtype=np.uint32)
        self.n_preset, self.positions = pos.size, pos
        h, err = C.c_void_p(), C.create_string_buffer(512)
        rc = lib().vpbs_witness_plan_create(C.byref(circuit.c), pos.ctypes.data_as(U32P), pos.size, C.byref(h), err, 512)
        if rc:
            raise VpbsError("vpbs_witness_plan_create: " + err.value.decode())
        self.h = h

    def run(self, values, threads=0, out=None):
        """values in the order of the positions given at creation -> wires [n_wires][n]"""
        val = _u64(values)
        assert val.size == self.n_preset
        if out is None:
            out = np.empty((self.circuit.n_wires, self.circuit.n), np.uint64)
        err = C.create_string_buffer(512)
        rc = lib().vpbs_witness_plan_run(self.h, _ptr(val) if val.size else None, threads, _ptr(out), err, 512)
        if rc:
            raise VpbsError("vpbs_witness_plan_run: " + err.value.decode())
        return out

    def split(self, late):
        """vpbs_witness_plan_split: late[i] marks preset i (creation order) as arriving late -> run_early / run_late"""
        m = np.ascontiguousarray(np.asarray(late, dtype=np.uint8))
        assert m.size == self.n_preset
        err = C.create_string_buffer(512)
        if lib().vpbs_witness_plan_split(self.h, m.ctypes.data_as(C.POINTER(C.c_uint8)), err, 512):
            raise VpbsError("vpbs_witness_plan_split: " + err.value.decode())

    def run_early(self, values, out, threads=0, recycled=False):
        """everything that does not depend on the late presets -> opaque state for run_late (out: the [n_wires][n] matrix, filled).
        recycled: `out` still holds the result of an earlier run of this plan -- only the positions that carry values are rewritten"""
        val = _u64(values)
        assert val.size == self.n_preset and out.dtype == np.uint64 and out.flags["C_CONTIGUOUS"]
        st, err = C.c_void_p(), C.create_string_buffer(512)
        fn = lib().vpbs_witness_plan_run_early_recycled if recycled else lib().vpbs_witness_plan_run_early
        if fn(self.h, _ptr(val), threads, _ptr(out), C.byref(st), err, 512):
            raise VpbsError("vpbs_witness_plan_run_early: " + err.value.decode())
        return st

    def run_late(self, state, values, out):
        """the late presets and what depends on them, into the same matrix; consumes the state"""
        val = _u64(values)
        assert val.size == self.n_preset
        err = C.create_string_buffer(512)
        if lib().vpbs_witness_plan_run_late(self.h, state, _ptr(val), _ptr(out), err, 512):
            raise VpbsError("vpbs_witness_plan_run_late: " + err.value.decode())
        return out

    def late_stages(self):
        """vpbs_witness_plan_late_stages: stages of the late phase (split() with stage numbers 1, 2, ..)"""
        return int(lib().vpbs_witness_plan_late_stages(self.h))

    def run_late_stage(self, state, stage, values, packed_out=None):
        """one late stage ahead of run_late (stages once each, ascending); the state is kept.  packed_out: the uint64 [late_count] array a
        later run_late_packed(.., out=packed_out) completes -- the stage writes its share of the packed wires at once"""
        val = _u64(values)
        assert val.size == self.n_preset
        err = C.create_string_buffer(512)
        if lib().vpbs_witness_plan_run_late_stage(self.h, state, stage, _ptr(val), _ptr(packed_out) if packed_out is not None else None, err, 512):
            raise VpbsError("vpbs_witness_plan_run_late_stage: " + err.value.decode())

    def run_late_packed(self, state, values, out=None):
        """the late phase without the matrix -> the values of late_positions(), in that order; consumes the state"""
        val = _u64(values)
        assert val.size == self.n_preset
        if out is None:
            out = np.zeros(int(lib().vpbs_witness_plan_late_count(self.h)), np.uint64)
        err = C.create_string_buffer(512)
        if lib().vpbs_witness_plan_run_late_packed(self.h, state, _ptr(val), _ptr(out), err, 512):
            raise VpbsError("vpbs_witness_plan_run_late_packed: " + err.value.decode())
        return out

    def late_input_positions(self):
        """-> uint32 wire positions, one per early-known copy class the late phase touches (vpbs_witness_plan_late_input_positions)"""
        out = np.zeros(int(lib().vpbs_witness_plan_late_input_count(self.h)), np.uint32)
        if lib().vpbs_witness_plan_late_input_positions(self.h, out.ctypes.data_as(U32P)):
            raise VpbsError("vpbs_witness_plan_late_input_positions: the plan is not split")
        return out

    def state_from_late_inputs(self, values):
        """a late-phase state seeded with the values of late_input_positions() (an early phase that ran elsewhere) -> state for run_late"""
        val = _u64(values)
        assert val.size == int(lib().vpbs_witness_plan_late_input_count(self.h))
        st = C.c_void_p()
        if lib().vpbs_witness_state_from_late_inputs(self.h, _ptr(val), C.byref(st)):
            raise VpbsError("vpbs_witness_state_from_late_inputs failed (plan not split, or a non-canonical value)")
        return st

    def late_positions(self):
        """-> uint32 wire positions (column * n + row) the late phase writes (vpbs_witness_plan_late_positions)"""
        out = np.zeros(int(lib().vpbs_witness_plan_late_count(self.h)), np.uint32)
        if lib().vpbs_witness_plan_late_positions(self.h, out.ctypes.data_as(U32P)):
            raise VpbsError("vpbs_witness_plan_late_positions: the plan is not split")
        return out

    def late_rows(self):
        """-> (row_lo, row_hi): the rows run_late writes (vpbs_witness_plan_late_rows)"""
        out = (C.c_size_t * 2)()
        if lib().vpbs_witness_plan_late_rows(self.h, out):
            raise VpbsError("vpbs_witness_plan_late_rows: the plan is not split")
        return int(out[0]), int(out[1])

    def stats(self):
        """-> dict(slots, generators, levels, positions)"""
        out = np.zeros(4, np.uint64)
        if lib().vpbs_witness_plan_stats(self.h, _ptr(out)):
            raise VpbsError("vpbs_witness_plan_stats failed")
        return dict(zip(("slots", "generators", "levels", "positions"), (int(x) for x in out)))


class WitnessChecker(_Handle):
    """vpbs_witness_checker: vpbs_check_witness on the device (same verdict, same message); the circuit's tables are uploaded once."""
    _prefix = "vpbs_witness_checker"

    def __init__(self, ctx, circuit):
        self.circuit = circuit
        self._construct(ctx, ctx.h, C.byref(circuit.c))

    def check(self, wires, pi_hash):
        """wires: a host matrix [n_wires][n] or a device pointer (int) to one -> (ok, message of the first violation)"""
        h = _u64(pi_hash)
        assert h.size == 4
        err = C.create_string_buffer(512)
        if isinstance(wires, int):
            rc = lib().vpbs_witness_checker_run(self.h, wires, 1, _ptr(h), err, 512)
        else:
            w = _u64(wires)
            assert w.shape == (self.circuit.n_wires, self.circuit.n)
            rc = lib().vpbs_witness_checker_run(self.h, w.ctypes.data, 0, _ptr(h), err, 512)
        if rc < 0:
            raise VpbsError("vpbs_witness_checker_run: status %d: %s" % (rc, err.value.decode()))
        return rc == 1, err.value.decode()


class WitnessDevice(_Handle):
    """vpbs_witness_device: the plan's schedule replayed on the device for a batch of PartialWitnesses (create once per circuit)."""
    _prefix = "vpbs_witness_device"

    def __init__(self, ctx, plan, max_batch, early=False):
        """early: the early phase of a split plan alone (vpbs_witness_device_create_early); the late presets' rows of `values` are ignored"""
        self.plan, self.max_batch = plan, max_batch   # the plan is kept: the device object replays it
        h = C.c_void_p()
        ctx._check(self._entry("create_early" if early else "create")(ctx.h, plan.h, max_batch, C.byref(h)))
        self.h = h
        self._created(ctx)

    def run_late(self, instance, values):
        """the late phase of one instance of the last batch on top of its early values (values: [n_preset], the late entries are read)"""
        v = _u64(values)
        assert v.size == self.plan.n_preset
        self.ctx._check(lib().vpbs_witness_device_run_late(self.h, instance, _ptr(v)))

    def read_late_inputs(self, instance):
        """the early values the host's late phase needs of one instance, in the order of plan.late_input_positions()"""
        out = np.zeros(int(lib().vpbs_witness_plan_late_input_count(self.plan.h)), np.uint64)
        self.ctx._check(lib().vpbs_witness_device_read_late_inputs(self.h, instance, _ptr(out)))
        return out

    def run(self, values):
        """values: [n_preset][batch] (rows in the order of the plan's positions)"""
        v = _u64(values)
        assert v.ndim == 2 and v.shape[0] == self.plan.n_preset and 1 <= v.shape[1] <= self.max_batch
        self.batch = v.shape[1]
        self.ctx._check(lib().vpbs_witness_device_run(self.h, _ptr(v), v.shape[1]))

    def wires(self, instance, d_wires_ptr):
        """gather one instance into a device [n_wires][n] matrix (pointer as int)"""
        self.ctx._check(lib().vpbs_witness_device_wires(self.h, instance, d_wires_ptr))

    def read(self, instance, positions):
        """values at wire positions [(column, row), ...] of one instance -> numpy uint64"""
        n = self.plan.circuit.n
        pos = np.array([c * n + r for (c, r) in positions], dtype=np.uint32)
        out = np.zeros(pos.size, np.uint64)
        self.ctx._check(lib().vpbs_witness_device_read(self.h, instance, pos.ctypes.data_as(U32P), pos.size, _ptr(out)))
        return out


def hash_chain(items, claimed=None):
    """verify_hash_output of the reference (ivc_based_vpbs.rs:64-78): -> (chain hash, matches claimed)"""
    it = _u64(items)
    out = np.zeros(4, np.uint64)
    cl = _u64(claimed) if claimed is not None else None
    rc = lib().vpbs_hash_chain(_ptr(it), it.shape[0], it.shape[1], _ptr(cl) if cl is not None else None, _ptr(out))
    if rc < 0:
        raise VpbsError("vpbs_hash_chain failed")
    return out, rc == 1


def hash_chain_links(prefix, items):
    """links of a hash chain from `prefix` on: out[k] = hash_no_pad(h_{k-1} || items[k]) -> [n_links][4] (vpbs_hash_chain_links: concurrent
    callers of the same shape share AVX-512 lanes when the process is short of CPUs)"""
    it = _u64(items)
    pre = _u64(prefix)
    out = np.zeros((it.shape[0], 4), np.uint64)
    ptrs = (U64P * it.shape[0])(*[_ptr(it[k]) for k in range(it.shape[0])])
    if lib().vpbs_hash_chain_links(_ptr(pre), ptrs, it.shape[0], it.shape[1], _ptr(out)) != 0:
        raise VpbsError("vpbs_hash_chain_links failed")
    return out


def verify_step(proof, cs_cap, ncols, circuit_digest, public_inputs, log_n, num_challenges=2, check_permutation=True, n_constants=0,
                n_routed=0, quotient_degree_factor=8, gate_terms_zeta=None, rate_bits=3, cap_height=4, gates=None, compat=None):
    """Host-side verifier of the product library (plonky2 `verify`: transcript, vanishing identity at zeta -- permutation argument and the
    gate constraints, the PublicInputGate binding among them -- then verify_fri_proof).  True = accepted.  The full check is the default and
    needs the circuit's shape: n_constants, n_routed and its gates (or gate_terms_zeta, or neither for a circuit of NoopGates only).
    check_permutation=False (= verify_step_fri_only) checks the transcript, PoW, Merkle paths and the low-degree test ONLY: it accepts a
    proof over unsatisfied wires, so it is a statement about the commitments, never about the circuit."""
    if check_permutation and n_routed == 0:
        raise ValueError("verify_step: the full check needs n_constants / n_routed (and the gates); for transcript + FRI only call "
                         "verify_step_fri_only explicitly")
    v = VerifyInputsC()
    v.log_n, v.rate_bits, v.cap_height = log_n, rate_bits, cap_height
    v.n_constants_sigmas, v.n_wires, v.n_zs_partial_products, v.n_quotient = ncols
    v.num_challenges = num_challenges
    cap = _u64(cs_cap)
    v.constants_sigmas_cap = _ptr(cap)
    for i in range(4):
        v.circuit_digest[i] = int(circuit_digest[i])
    pi = _u64(public_inputs).reshape(-1)
    v.public_inputs = _ptr(pi)
    v.n_public_inputs = pi.size
    v.fri_only = 0 if check_permutation else 1
    v.n_constants, v.n_routed, v.quotient_degree_factor = n_constants, n_routed, quotient_degree_factor
    gt = _u64(gate_terms_zeta) if gate_terms_zeta is not None else None
    v.gate_terms_zeta = _ptr(gt) if gt is not None else None
    if gates is not None:
        v.gates, v.n_gates, v.num_selectors = gates.arr, gates.n, gates.num_selectors
    if compat is not None:
        v.compat = C.pointer(compat)
    caps, openings, fri = _u64(proof["caps"]), _u64(proof["openings"]), _u64(proof["fri"])
    rc = lib().vpbs_verify_step(C.byref(v), _ptr(caps), _ptr(openings), _ptr(fri))
    if rc < 0:
        raise VpbsError("vpbs_verify_step: malformed arguments (%d)" % rc)
    return rc == 1


VERIFY_OK, VERIFY_MALFORMED, VERIFY_VANISHING, VERIFY_POW, VERIFY_FRI, VERIFY_MERKLE = range(6)   # vpbs_proof_verifier reasons


def pack_proofs(blobs):
    """serialised proofs -> (one uint8 buffer, offsets [count + 1] as size_t): the input of vpbs_proof_verifier_run"""
    lens = np.fromiter((len(b) for b in blobs), dtype=np.uint64, count=len(blobs))
    offsets = np.zeros(len(blobs) + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    buf = np.frombuffer(b"".join(bytes(b) for b in blobs), dtype=np.uint8) if blobs else np.zeros(0, np.uint8)
    return buf, offsets


class ProofVerifier(_Handle):
    """vpbs_proof_verifier: vpbs_step_proof_from_bytes + vpbs_verify_step for a batch of serialised step proofs on the device, with the host's
    verdict for every one of them.  The parameters mirror verify_step (each proof carries its own public inputs); max_public_inputs is the
    parser's public_inputs_capacity.  Every proof slot on the device holds the proof's words and max_public_inputs more, max_batch slots:
    size both to the proofs at hand (the defaults, 256 proofs of up to 8192 public inputs, take ~200 MB for a paper-size step proof)."""
    _prefix = "vpbs_proof_verifier"

    def __init__(self, ctx, cs_cap, ncols, circuit_digest, log_n, num_challenges=2, check_permutation=True, n_constants=0, n_routed=0,
                 quotient_degree_factor=8, gates=None, compat=None, rate_bits=3, cap_height=4, max_batch=256, max_public_inputs=1 << 13,
                 gate_terms_zeta=None):
        if check_permutation and n_routed == 0:
            raise ValueError("ProofVerifier: the full check needs n_constants / n_routed (and the gates); check_permutation=False for "
                             "transcript + FRI only")
        self.max_batch = max_batch
        v = VerifyInputsC()
        v.log_n, v.rate_bits, v.cap_height = log_n, rate_bits, cap_height
        v.n_constants_sigmas, v.n_wires, v.n_zs_partial_products, v.n_quotient = ncols
        v.num_challenges = num_challenges
        self._cap = _u64(cs_cap)
        v.constants_sigmas_cap = _ptr(self._cap)
        for i in range(4):
            v.circuit_digest[i] = int(circuit_digest[i])
        v.fri_only = 0 if check_permutation else 1
        v.n_constants, v.n_routed, v.quotient_degree_factor = n_constants, n_routed, quotient_degree_factor
        self._gt = _u64(gate_terms_zeta) if gate_terms_zeta is not None else None
        v.gate_terms_zeta = _ptr(self._gt) if self._gt is not None else None
        if gates is not None:
            v.gates, v.n_gates, v.num_selectors = gates.arr, gates.n, gates.num_selectors
        if compat is not None:
            self._compat = compat
            v.compat = C.pointer(compat)
        self._construct(ctx, ctx.h, C.byref(v), max_batch, max_public_inputs)

    def verify_packed(self, buf, offsets):
        """buf: uint8 buffer, offsets: [count + 1] (pack_proofs) -> (verdicts, reasons), np.uint8 each"""
        count, data, offs, results, ptrs = _packed(buf, offsets, outputs=2)
        rc = lib().vpbs_proof_verifier_run(self.h, data, offs, count, *ptrs)
        if rc < 0:
            raise VpbsError("vpbs_proof_verifier_run: status %d" % rc)
        return results

    def verify(self, blobs):
        """list of ProofWithPublicInputs byte strings -> (verdicts, reasons), np.uint8 each"""
        return self.verify_packed(*pack_proofs(blobs))


def _ivc_circuit(d, proof_words, keep):
    """IvcCircuitC of a circuit_file.CircuitDescription; `keep` takes what its pointers refer to and must outlive the call that reads it"""
    c = IvcCircuitC()
    pre = np.ascontiguousarray(d.preset_flat, dtype=np.uint32)
    pi = np.ascontiguousarray(d.pi_flat, dtype=np.uint32)
    keep.extend([pre, pi, d])
    c.circuit = C.pointer(d.circuit.c)
    c.preset_pos, c.n_preset = pre.ctypes.data_as(U32P), pre.size
    c.pi_pos, c.n_pi = pi.ctypes.data_as(U32P), pi.size
    c.proof_words = proof_words
    return c


class Ivc(_Handle):
    """vpbs_ivc: one verifiable PBS as one call -- the IVC chain of verified_pbs (ivc_based_vpbs.rs:159-386) driven inside the library.
    cyclic / dummy: circuit_file.CircuitDescription of the exported cyclic step circuit and its dummy circuit."""
    _prefix = "vpbs_ivc"

    def __init__(self, ctx, cyclic, dummy, N, K, ggsw_len, comm=None):
        """comm: a CommC (sharding.make_comm / make_comm_rccl) -> every step proof coset-sharded over the ranks; every rank builds its own Ivc"""
        self._keep = [comm]
        cy, du = _ivc_circuit(cyclic, cyclic.meta["proof_words"], self._keep), _ivc_circuit(dummy, 0, self._keep)
        h, err = C.c_void_p(), C.create_string_buffer(512)
        if lib().vpbs_ivc_create(ctx.h, C.byref(cy), C.byref(du), N, K, ggsw_len, C.byref(comm) if comm is not None else None, C.byref(h),
                                 err, 512):
            raise VpbsError("vpbs_ivc_create: " + err.value.decode())
        self.h = h
        self._created(ctx)
        self.vk_words = 4 + (4 << 4)
        self.max_bytes = 8 * (cyclic.meta["proof_words"] + len(cyclic.pi_pos)) + (1 << 16)

    def verifier_data(self):
        """-> (cyclic circuit: digest [4] + cap, dummy circuit: the same)"""
        a, b = np.zeros(self.vk_words, np.uint64), np.zeros(self.vk_words, np.uint64)
        lib().vpbs_ivc_verifier_data(self.h, _ptr(a), _ptr(b))
        return a, b

    def set_device_witness(self, ELL, LOGB, batch, late_on_device=False):
        """vpbs_ivc_set_device_witness: the early witness phases of `batch` steps at a time on the device (0: back to the host pipeline);
        late_on_device: the late phase there as well (the host generates no witness)"""
        rc = lib().vpbs_ivc_set_device_witness(self.h, ELL, LOGB, batch, 1 if late_on_device else 0)
        if rc != 0:
            raise VpbsError("vpbs_ivc_set_device_witness: status %d: %s" % (rc, lib().vpbs_ivc_last_error(self.h).decode()))

    def set_check_witness(self, on=True):
        """vpbs_ivc_set_check_witness: every witness of later chains (base proof and steps) checked on the device before it is proven; a
        violation stops prove_pbs with VpbsError "... step k: <message>".  Resets the counters of witness_checks()."""
        rc = lib().vpbs_ivc_set_check_witness(self.h, 1 if on else 0)
        if rc != 0:
            raise VpbsError("vpbs_ivc_set_check_witness: status %d: %s" % (rc, lib().vpbs_ivc_last_error(self.h).decode()))

    def witness_checks(self):
        """-> (witnesses checked, violations found) since the last set_check_witness"""
        out = np.zeros(2, np.uint64)
        lib().vpbs_ivc_witness_checks(self.h, _ptr(out))
        return int(out[0]), int(out[1])

    def on_step(self, fn):
        """vpbs_ivc_set_step_callback: fn(done) runs on the proving thread with done = 0 after the base proof and 1 .. steps after each
        chained step proof (None removes it).  An exception raised by fn is kept and re-raised by prove_pbs."""
        self._step_error = None
        if fn is None:
            self._step_cb = None
            lib().vpbs_ivc_set_step_callback(self.h, C.cast(None, IVC_STEP_FN), None)
            return

        def trampoline(_user, done):
            try:
                if self._step_error is None:
                    fn(int(done))
            except BaseException as e:   # noqa: BLE001 -- must not unwind through the C frames
                self._step_error = e
        self._step_cb = IVC_STEP_FN(trampoline)
        lib().vpbs_ivc_set_step_callback(self.h, self._step_cb, None)

    def on_checkpoint(self, every, fn):
        """vpbs_ivc_set_checkpoint: fn(done, bytes) runs on the proving thread after every chained step `done` that is a multiple of `every`
        and below the call's last step; bytes are what prove_pbs(..., steps=done) returns -- a checkpoint resume_pbs takes.  every = 0 or
        fn = None turns it off.  An exception raised by fn is kept and re-raised by prove_pbs / resume_pbs."""
        self._ckpt_error = None
        if fn is None or not every:
            self._ckpt_cb = None
            lib().vpbs_ivc_set_checkpoint(self.h, 0, C.cast(None, IVC_CHECKPOINT_FN), None)
            return

        def trampoline(_user, done, data, n):
            try:
                if self._ckpt_error is None:
                    fn(int(done), C.string_at(data, n))
            except BaseException as e:   # noqa: BLE001 -- must not unwind through the C frames
                self._ckpt_error = e
        self._ckpt_cb = IVC_CHECKPOINT_FN(trampoline)
        lib().vpbs_ivc_set_checkpoint(self.h, every, self._ckpt_cb, None)

    def _raise_callback_errors(self):
        for name in ("_step_error", "_ckpt_error"):
            e = getattr(self, name, None)
            if e is not None:
                setattr(self, name, None)
                raise e

    def prove_pbs(self, testv, ct, bsk, ksk, steps=0):
        """-> (ProofWithPublicInputs bytes of the LAST proof of the chain, timing dict)"""
        tv, c, ks = _u64(testv).reshape(-1), _u64(ct).reshape(-1), _u64(ksk).reshape(-1)
        bs = _u64(bsk).reshape(-1) if c.size > 1 else None
        buf, t, err = (C.c_uint8 * self.max_bytes)(), IvcTimingC(), C.create_string_buffer(512)
        n = lib().vpbs_ivc_prove_pbs(self.h, _ptr(tv), _ptr(c), _ptr(bs) if bs is not None else None, _ptr(ks), c.size - 1, steps, buf,
                                     self.max_bytes, C.byref(t), err, 512)
        self._raise_callback_errors()
        if n < 0:
            raise VpbsError("vpbs_ivc_prove_pbs: " + err.value.decode())
        return bytes(buf[:n]), {f: getattr(t, f) for f, _ in IvcTimingC._fields_}

    def resume_pbs(self, checkpoint, testv, ct, bsk, ksk, steps=0):
        """vpbs_ivc_resume_pbs: the chain from a checkpoint (the bytes of a prefix of k steps) to `steps` (0: the whole chain) -> (the bytes
        prove_pbs(testv, ct, bsk, ksk, steps) returns, timing dict of the steps proven here).  A checkpoint that does not verify against this
        object's verifier data, these keys and this ciphertext raises VpbsError "... checkpoint: <why>"."""
        tv, c, ks = _u64(testv).reshape(-1), _u64(ct).reshape(-1), _u64(ksk).reshape(-1)
        bs = _u64(bsk).reshape(-1) if c.size > 1 else None
        cp = bytes(checkpoint)
        src = (C.c_uint8 * max(1, len(cp))).from_buffer_copy(cp or b"\0")
        buf, t, err = (C.c_uint8 * self.max_bytes)(), IvcTimingC(), C.create_string_buffer(512)
        n = lib().vpbs_ivc_resume_pbs(self.h, _ptr(tv), _ptr(c), _ptr(bs) if bs is not None else None, _ptr(ks), c.size - 1, src, len(cp),
                                      steps, buf, self.max_bytes, C.byref(t), err, 512)
        self._raise_callback_errors()
        if n < 0:
            raise VpbsError("vpbs_ivc_resume_pbs: " + err.value.decode())
        return bytes(buf[:n]), {f: getattr(t, f) for f, _ in IvcTimingC._fields_}


def verify_pbs(blob, cs_cap, ncols, circuit_digest, log_n, n_constants, n_routed, gates, N, K, testv, ct, bsk, ksk, out_ct, num_challenges=2,
               quotient_degree_factor=8, rate_bits=3, cap_height=4, compat=None):
    """vpbs_verify_pbs = the reference's verify_pbs (ivc_based_vpbs.rs:388-489) on the serialised LAST proof of an IVC chain:
    -> (accepted, reason of the first failing check).  bsk: [n][ggsw_len] (NTT domain, flattened), ksk: [ggsw_len], ct: [n + 1]; out_ct [K][N]
    is the bootstrapped ciphertext the caller holds -- required, as in the reference (:440-442); None raises VpbsError."""
    v = VerifyInputsC()
    v.log_n, v.rate_bits, v.cap_height = log_n, rate_bits, cap_height
    v.n_constants_sigmas, v.n_wires, v.n_zs_partial_products, v.n_quotient = ncols
    v.num_challenges = num_challenges
    cap = _u64(cs_cap)
    v.constants_sigmas_cap = _ptr(cap)
    for i in range(4):
        v.circuit_digest[i] = int(circuit_digest[i])
    v.n_constants, v.n_routed, v.quotient_degree_factor = n_constants, n_routed, quotient_degree_factor
    v.gates, v.n_gates, v.num_selectors = gates.arr, gates.n, gates.num_selectors
    if compat is not None:
        v.compat = C.pointer(compat)
    p = VerifyPbsInputsC()
    p.circuit = C.pointer(v)
    ct_a, tv, ks = _u64(ct).reshape(-1), _u64(testv).reshape(-1), _u64(ksk).reshape(-1)
    bs = _u64(bsk).reshape(-1) if bsk is not None and len(bsk) else None
    oc = _u64(out_ct).reshape(-1) if out_ct is not None else None
    p.N, p.K, p.n_lwe, p.ggsw_len = N, K, ct_a.size - 1, ks.size
    p.testv, p.ct, p.ksk = _ptr(tv), _ptr(ct_a), _ptr(ks)
    p.bsk = _ptr(bs) if bs is not None else None
    p.out_ct = _ptr(oc) if oc is not None else None
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
    why = C.create_string_buffer(256)
    rc = lib().vpbs_verify_pbs(C.byref(p), buf, len(blob), why, 256)
    if rc < 0:
        raise VpbsError("vpbs_verify_pbs: " + why.value.decode())
    return rc == 1, why.value.decode()


def verify_pbs_prefix(blob, cs_cap, ncols, circuit_digest, log_n, n_constants, n_routed, gates, N, K, testv, ct, bsk, ksk, out_ct=None,
                      num_challenges=2, quotient_degree_factor=8, rate_bits=3, cap_height=4, compat=None):
    """vpbs_verify_pbs_prefix: verify_pbs's checks on the last proof of a chain of k = counter proofs (a checkpoint), k in 1 .. n + 2, the hash
    chains over the first k keys and masks; out_ct optional -> (accepted, k, reason of the first failing check).  Arguments as verify_pbs."""
    v = VerifyInputsC()
    v.log_n, v.rate_bits, v.cap_height = log_n, rate_bits, cap_height
    v.n_constants_sigmas, v.n_wires, v.n_zs_partial_products, v.n_quotient = ncols
    v.num_challenges = num_challenges
    cap = _u64(cs_cap)
    v.constants_sigmas_cap = _ptr(cap)
    for i in range(4):
        v.circuit_digest[i] = int(circuit_digest[i])
    v.n_constants, v.n_routed, v.quotient_degree_factor = n_constants, n_routed, quotient_degree_factor
    v.gates, v.n_gates, v.num_selectors = gates.arr, gates.n, gates.num_selectors
    if compat is not None:
        v.compat = C.pointer(compat)
    p = VerifyPbsInputsC()
    p.circuit = C.pointer(v)
    ct_a, tv, ks = _u64(ct).reshape(-1), _u64(testv).reshape(-1), _u64(ksk).reshape(-1)
    bs = _u64(bsk).reshape(-1) if bsk is not None and len(bsk) else None
    oc = _u64(out_ct).reshape(-1) if out_ct is not None else None
    p.N, p.K, p.n_lwe, p.ggsw_len = N, K, ct_a.size - 1, ks.size
    p.testv, p.ct, p.ksk = _ptr(tv), _ptr(ct_a), _ptr(ks)
    p.bsk = _ptr(bs) if bs is not None else None
    p.out_ct = _ptr(oc) if oc is not None else None
    buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(bytes(blob) or b"\0")
    why, done = C.create_string_buffer(256), C.c_uint(0)
    rc = lib().vpbs_verify_pbs_prefix(C.byref(p), buf, len(blob), C.byref(done), why, 256)
    if rc < 0:
        raise VpbsError("vpbs_verify_pbs_prefix: " + why.value.decode())
    return rc == 1, int(done.value), why.value.decode()


(PBS_OK, PBS_MALFORMED, PBS_TESTV_MASK, PBS_TESTV, PBS_COUNTER, PBS_OUT_CT, PBS_PROOF, PBS_VERIFIER_DATA, PBS_KEY_HASH,
 PBS_LWE_HASH) = range(10)   # vpbs_pbs_verifier reasons, in vpbs_verify_pbs's order


def pbs_reason_text(reason):
    """vpbs_pbs_reason_text: the `why` vpbs_verify_pbs writes when that check fails ("" for PBS_OK)"""
    t = lib().vpbs_pbs_reason_text(int(reason))
    if t is None:
        raise ValueError("no vPBS verifier reason %r" % (reason,))
    return t.decode()


def pbs_key_hash(bsk, ksk):
    """vpbs_pbs_key_hash: the key hash chain of verify_pbs over [zeros, bsk_0 .. bsk_{n-1}, ksk] (host) -> [4].  bsk: [n][ggsw_len]"""
    ks = _u64(ksk).reshape(-1)
    if ks.size == 0:
        raise VpbsError("vpbs_pbs_key_hash: an empty ksk (ggsw_len = 0)")
    bs = _u64(bsk).reshape(-1, ks.size) if bsk is not None and len(bsk) else np.zeros((0, ks.size), np.uint64)
    out = np.zeros(4, np.uint64)
    if lib().vpbs_pbs_key_hash(_ptr(bs) if bs.size else None, _ptr(ks), bs.shape[0], ks.size, _ptr(out)) != 0:
        raise VpbsError("vpbs_pbs_key_hash: malformed arguments")
    return out


def _verify_pbs_shape(cs_cap, ncols, circuit_digest, log_n, n_constants, n_routed, gates, N, K, n_lwe, ggsw_len, num_challenges, quotient_degree_factor,
                      rate_bits, cap_height, compat):
    """the vpbs_verify_pbs_inputs a device verifier is created from (no testv, ct, out_ct or keys) -> (struct, what it points to)"""
    v = VerifyInputsC()
    v.log_n, v.rate_bits, v.cap_height = log_n, rate_bits, cap_height
    v.n_constants_sigmas, v.n_wires, v.n_zs_partial_products, v.n_quotient = ncols
    v.num_challenges = num_challenges
    cap = _u64(cs_cap)
    v.constants_sigmas_cap = _ptr(cap)
    for i in range(4):
        v.circuit_digest[i] = int(circuit_digest[i])
    v.n_constants, v.n_routed, v.quotient_degree_factor = n_constants, n_routed, quotient_degree_factor
    v.gates, v.n_gates, v.num_selectors = gates.arr, gates.n, gates.num_selectors
    if compat is not None:
        v.compat = C.pointer(compat)
    p = VerifyPbsInputsC()
    p.circuit = C.pointer(v)
    p.N, p.K, p.n_lwe, p.ggsw_len = N, K, n_lwe, ggsw_len
    return p, (v, cap, gates, compat)


class _PbsVerify(_Handle):
    """What PbsVerifier and RingVerifier share: the creation from _verify_pbs_shape and the run over packed proofs.  A subclass gives
    _statement(count, ...): its own arguments checked and turned into what <_prefix>_run takes between the proofs and the verdicts."""
    _run_err = False   # <_prefix>_run ends in (err, err_len) and its failures carry .status

    def _create(self, ctx, shape, N, K, n_lwe, max_batch, *create_args):
        """shape: _verify_pbs_shape's leading arguments; create_args: what <_prefix>_create takes between the shape and max_batch"""
        self.max_batch, self.N, self.K, self.n_lwe = max_batch, N, K, n_lwe
        p, self._keep = _verify_pbs_shape(*shape)
        self._construct(ctx, ctx.h, C.byref(p), *create_args, max_batch)

    def _verify(self, buf, offsets, *statement):
        count, data, offs, results, ptrs = _packed(buf, offsets, outputs=3)
        args = self._statement(count, *statement)
        what, err = self._prefix + "_run", C.create_string_buffer(512)
        rc = self._entry("run")(self.h, data, offs, count, *args, *ptrs, *((err, 512) if self._run_err else ()))
        if rc < 0:
            raise self._fail(what, rc, err.value.decode() or None) if self._run_err else VpbsError("%s: status %d" % (what, rc))
        return results


class PbsVerifier(_PbsVerify):
    """vpbs_pbs_verifier: vpbs_verify_pbs for a batch of vPBS proofs (the serialised last proofs of IVC chains) on the device, all under the
    key set whose hash is key_hash (pbs_key_hash).  The parameters mirror verify_pbs; every proof brings its own ct and out_ct."""
    _prefix = "vpbs_pbs_verifier"

    def __init__(self, ctx, cs_cap, ncols, circuit_digest, log_n, n_constants, n_routed, gates, N, K, n_lwe, ggsw_len, key_hash, max_batch=64,
                 num_challenges=2, quotient_degree_factor=8, rate_bits=3, cap_height=4, compat=None):
        shape = (cs_cap, ncols, circuit_digest, log_n, n_constants, n_routed, gates, N, K, n_lwe, ggsw_len, num_challenges, quotient_degree_factor,
                 rate_bits, cap_height, compat)
        self._create(ctx, shape, N, K, n_lwe, max_batch, _ptr(_u64(key_hash).reshape(-1)))

    def _statement(self, count, testv, cts, out_cts):
        tv = _u64(testv)
        per_proof = tv.ndim == 2
        tv, c, o = tv.reshape(-1), _u64(cts).reshape(-1), _u64(out_cts).reshape(-1)
        if c.size != count * (self.n_lwe + 1) or o.size != count * self.K * self.N or tv.size != (count if per_proof else 1) * self.N:
            raise ValueError("PbsVerifier.verify: expected testv [N] or [%d][N], cts [%d][n + 1] and out_cts [%d][K][N]" % (count, count, count))
        return _keep_ptr(tv), 1 if per_proof else 0, _keep_ptr(c), _keep_ptr(o)

    def verify_packed(self, buf, offsets, testv, cts, out_cts):
        """buf, offsets: pack_proofs; testv: [N] shared or [count][N]; cts: [count][n + 1]; out_cts: [count][K][N]
        -> (verdicts, reasons, proof_reasons), np.uint8 each"""
        return self._verify(buf, offsets, testv, cts, out_cts)

    def verify(self, blobs, testv, cts, out_cts):
        """list of serialised vPBS proofs -> (verdicts, reasons, proof_reasons), np.uint8 each"""
        return self.verify_packed(*pack_proofs(blobs), testv, cts, out_cts)


def verify_step_fri_only(proof, cs_cap, ncols, circuit_digest, public_inputs, log_n, num_challenges=2, rate_bits=3, cap_height=4):
    """Transcript + PoW + Merkle paths + FRI low-degree test only (vpbs_verify_inputs.fri_only = 1): for proofs over synthetic columns
    whose constraints are not meant to hold.  NOT a sound accept of a circuit."""
    return verify_step(proof, cs_cap, ncols, circuit_digest, public_inputs, log_n, num_challenges=num_challenges, check_permutation=False,
                       rate_bits=rate_bits, cap_height=cap_height)


def step_proof_from_bytes(blob, ncols, log_n, n_constants, num_challenges=2, rate_bits=3, cap_height=4, max_public_inputs=1 << 16, compat=None):
    """vpbs_step_proof_from_bytes: ProofWithPublicInputs bytes -> ({"caps", "openings", "fri"}, public inputs)"""
    v = VerifyInputsC()
    v.log_n, v.rate_bits, v.cap_height = log_n, rate_bits, cap_height
    v.n_constants_sigmas, v.n_wires, v.n_zs_partial_products, v.n_quotient = ncols
    v.num_challenges, v.n_constants = num_challenges, n_constants
    if compat is not None:
        v.compat = C.pointer(compat)
    # the FRI words of this shape: the rounds follow rate_bits and cap_height, as the parser's own FriParams::standard does
    p = fri_params(log_n, rate_bits=rate_bits, cap_height=cap_height, arity_bits=standard_arity_bits(log_n, rate_bits, cap_height))
    sizes = (C.c_size_t * 4)(*ncols)
    fri_words = lib().vpbs_fri_proof_words(C.byref(p), log_n, sizes, 4)
    if fri_words == 0:
        raise VpbsError("vpbs_step_proof_from_bytes: not a step proof of this shape")
    caps = np.zeros((3, 1 << cap_height, 4), np.uint64)
    openings = np.zeros((sum(ncols) + num_challenges, 2), np.uint64)
    fri = np.zeros(fri_words, np.uint64)
    pis = np.zeros(max_public_inputs, np.uint64)
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
    n = lib().vpbs_step_proof_from_bytes(C.byref(v), buf, len(blob), _ptr(caps), _ptr(openings), _ptr(fri), _ptr(pis), pis.size)
    if n < 0:
        raise VpbsError("vpbs_step_proof_from_bytes: not a step proof of this shape")
    return {"caps": caps, "openings": openings, "fri": fri}, pis[:n].copy()


def lwe_encrypt(params, s_lwe, message, nonce=0):
    """vpbs_lwe_encrypt (host): lwe::encrypt(s_lwe, message, sigma_lwe) with the seeded mask / noise streams of `nonce` -> ct [n + 1]"""
    s = _u64(s_lwe).reshape(-1)
    ct = np.zeros(s.size + 1, np.uint64)
    if lib().vpbs_lwe_encrypt(C.byref(params), _ptr(s), int(message), int(nonce), _ptr(ct)) != 0:
        raise VpbsError("vpbs_lwe_encrypt: bad arguments")
    return ct


def testv(N, p=2):
    """get_testv(p, get_delta(2 p)) -> (testv [N], delta)"""
    t, d = np.zeros(N, np.uint64), np.zeros(1, np.uint64)
    if lib().vpbs_testv(N.bit_length() - 1, p, _ptr(t), _ptr(d)) != 0:
        raise VpbsError("vpbs_testv: bad arguments")
    return t, int(d[0])


def lwe_decrypt(s_lwe, ct):
    """vpbs_lwe_decrypt (host): lwe::decrypt (crypto/lwe.rs:62-69) = body - <s, mask>; ct [n + 1] -> int, or [count][n + 1] -> [count]"""
    s, c = _u64(s_lwe).reshape(-1), _u64(ct)
    if c.shape[-1] != s.size + 1:
        raise ValueError("lwe_decrypt: ct must be [.., n + 1] for a key of n words")
    rows = c.reshape(-1, s.size + 1)
    out = np.zeros(rows.shape[0], np.uint64)
    for i in range(rows.shape[0]):
        if lib().vpbs_lwe_decrypt(_ptr(s), _ptr(np.ascontiguousarray(rows[i])), s.size, _ptr(out[i:i + 1])) != 0:
            raise VpbsError("vpbs_lwe_decrypt: bad arguments")
    return int(out[0]) if c.ndim == 1 else out


def lut_testv(N, p, table, delta=None):
    """vpbs_lut_testv: the test vector of a lookup table over [0, p): block i holds table[i] * delta (entries below 2 p; delta defaults to
    get_delta(2 p), with which the identity table gives testv(N, p)).  A message in [p, 2 p) bootstraps to the NEGATED entry -> (testv [N], delta)"""
    t = _u64(table).reshape(-1)
    if t.size != p:
        raise ValueError("lut_testv: the table must have p = %d entries" % p)
    if delta is None:
        d = np.zeros(1, np.uint64)
        if lib().vpbs_testv(N.bit_length() - 1, p, None, _ptr(d)) != 0:
            raise VpbsError("vpbs_lut_testv: bad arguments")
        delta = int(d[0])
    out = np.zeros(N, np.uint64)
    if lib().vpbs_lut_testv(N.bit_length() - 1, p, _ptr(t), int(delta), _ptr(out)) != 0:
        raise VpbsError("vpbs_lut_testv: bad arguments (p a power of two, p <= N, entries below 2 p)")
    return out, int(delta)


class NoiseStats:
    """vpbs_noise_stats: exact integer statistics of the decoding errors err_i that lwe_decode_batch calls have added so far."""

    def __init__(self):
        self.c = NoiseStatsC()

    @staticmethod
    def _words(w, signed=False):
        v = sum(int(x) << (64 * i) for i, x in enumerate(w))
        return v - (1 << (64 * len(w))) if signed and v >> (64 * len(w) - 1) else v

    count = property(lambda self: int(self.c.count))
    failures = property(lambda self: int(self.c.failures))
    max_abs = property(lambda self: int(self.c.max_abs))
    sum_abs = property(lambda self: self._words(self.c.sum_abs))
    sum_sq = property(lambda self: self._words(self.c.sum_sq))
    sum_signed = property(lambda self: self._words(self.c.sum_signed, signed=True))
    hist = property(lambda self: [int(x) for x in self.c.hist])

    def mean(self):
        return float(Fraction(self.sum_signed, self.count)) if self.count else 0.0

    def mean_abs(self):
        return float(Fraction(self.sum_abs, self.count)) if self.count else 0.0

    def std(self):
        """sqrt(E[err^2] - E[err]^2), the variance formed in exact rationals before the one rounding to a float"""
        if not self.count:
            return 0.0
        return math.sqrt(Fraction(self.count * self.sum_sq - self.sum_signed ** 2, self.count ** 2))

    @staticmethod
    def _ln_erfc(x):
        """ln erfc(x); beyond x = 25, where erfc nears the smallest doubles, its asymptotic series (next term below 1e-11 there)"""
        if x < 25.0:
            return math.log(math.erfc(x))
        y = 1.0 / (2.0 * x * x)
        return -x * x - math.log(x * math.sqrt(math.pi)) + math.log1p(-y + 3.0 * y * y - 15.0 * y ** 3 + 105.0 * y ** 4)

    def tail_log2(self, bound):
        """log2 of P(|X| > bound) for X Gaussian with the exact mean and variance of this struct: a MODEL of the tail, not a measurement of
        it.  What the struct holds decides how far the model can be trusted: a sum of bounded roundings (the rotation error of
        lwe_rotation_batch at sigma 0: n + 1 terms, each within half a step) has LIGHTER tails than a Gaussian of its variance, so there
        the figure is pessimistic; the ciphertext's own noise (lwe_decode_batch's err, and its share of dev) IS Gaussian, so there it is
        the tail.  Stable for large arguments (erfc's asymptotic series in logarithms): finite wherever the variance is not zero.  With
        zero variance: 0.0 if |mean| > bound, else -inf."""
        if not self.count:
            raise ValueError("NoiseStats.tail_log2: an empty struct")
        m, s, b = self.mean(), self.std(), float(bound)
        if s == 0.0:
            return 0.0 if abs(m) > b else -math.inf
        hi, lo = self._ln_erfc((b - m) / (s * math.sqrt(2.0))), self._ln_erfc((b + m) / (s * math.sqrt(2.0)))
        top = max(hi, lo)
        return (top + math.log(math.exp(hi - top) + math.exp(lo - top)) - math.log(2.0)) / math.log(2.0)

    def as_dict(self):
        return {"count": self.count, "failures": self.failures, "max_abs": self.max_abs, "sum_abs": self.sum_abs, "sum_sq": self.sum_sq,
                "sum_signed": self.sum_signed, "hist": self.hist}


def _is_dev(x):
    return isinstance(x, (int, np.integer))


def _lwe_encrypt_batch(ctx, params, s_lwe, messages, nonce0, out_dev_ptr, count, mask_seed=None):
    """vpbs_lwe_encrypt_batch, or with mask_seed vpbs_lwe_encrypt_seeded_batch: the same arguments, [count] bodies instead of [count][n + 1] rows"""
    name = "vpbs_lwe_encrypt_batch" if mask_seed is None else "vpbs_lwe_encrypt_seeded_batch"
    h = ctx.h if ctx is not None else None
    n = int(params.n_lwe)
    key = None if _is_dev(s_lwe) else _u64(s_lwe).reshape(-1)
    if key is not None and key.size != n:
        raise ValueError("lwe_encrypt_batch: the key must have n_lwe = %d words" % n)
    msgs = None if _is_dev(messages) else _u64(messages).reshape(-1)
    if msgs is None and (count is None or out_dev_ptr is None):
        raise ValueError("lwe_encrypt_batch: messages on the device need count and out_dev_ptr")
    count = msgs.size if msgs is not None else int(count)
    keep = np.zeros(1, np.uint64)   # a valid pointer for an empty batch
    pkey = int(s_lwe) if key is None else key.ctypes.data
    tmp, out = None, None
    try:
        if out_dev_ptr is None:
            out = np.zeros((count, n + 1) if mask_seed is None else count, np.uint64)
            pm, po, on_device = _keep_ptr(msgs), _keep_ptr(out), 0
        else:
            if msgs is not None:
                tmp = ctx.device_upload_new(msgs if count else keep)
            pm, po, on_device = (tmp if msgs is not None else int(messages)), int(out_dev_ptr), 1
        if mask_seed is None:
            rc = lib().vpbs_lwe_encrypt_batch(h, C.byref(params), pkey, 1 if key is None else 0, pm, count, int(nonce0), po, on_device)
        else:
            rc = lib().vpbs_lwe_encrypt_seeded_batch(h, C.byref(params), int(mask_seed), pkey, 1 if key is None else 0, pm, count, int(nonce0), po,
                                                     on_device)
    finally:
        if tmp is not None:
            ctx.device_free(tmp)
    if rc:
        if h:
            text = lib().vpbs_last_error(h).decode()
        else:   # no context to hold the text: name the first offending index here
            bad = np.nonzero(msgs >= np.uint64(P))[0]
            text = ("message %d is not below p" % bad[0] if bad.size else
                    "nonce0 + count exceeds 2^24" if int(nonce0) + count > 1 << 24 else "bad arguments")
        raise VpbsError("%s: status %d: %s" % (name, rc, text))
    return out


def _lwe_expand_batch(ctx, n_lwe, mask_seed, bodies, nonce0, out_dev_ptr, count):
    h = ctx.h if ctx is not None else None
    b = None if _is_dev(bodies) else _u64(bodies).reshape(-1)
    if b is None and (count is None or out_dev_ptr is None):
        raise ValueError("lwe_expand_batch: bodies on the device need count and out_dev_ptr")
    count = b.size if b is not None else int(count)
    keep = np.zeros(1, np.uint64)   # a valid pointer for an empty batch
    tmp, out = None, None
    try:
        if out_dev_ptr is None:
            out = np.zeros((count, int(n_lwe) + 1), np.uint64)
            pb, po, on_device = _keep_ptr(b), _keep_ptr(out), 0
        else:
            if b is not None:
                tmp = ctx.device_upload_new(b if count else keep)
            pb, po, on_device = (tmp if b is not None else int(bodies)), int(out_dev_ptr), 1
        rc = lib().vpbs_lwe_expand_batch(h, int(n_lwe), int(mask_seed), int(nonce0), pb, count, po, on_device)
    finally:
        if tmp is not None:
            ctx.device_free(tmp)
    if rc:
        text = (lib().vpbs_last_error(h).decode() if h else
                "nonce0 + count exceeds 2^24" if int(nonce0) + count > 1 << 24 else "n_lwe must be 1 .. 2^24 - 1, or a null pointer")
        raise VpbsError("vpbs_lwe_expand_batch: status %d: %s" % (rc, text))
    return out


def seeded_key_shapes(N, K, ELL, n_lwe):
    """words of one key set (bsk and ksk together) as vpbs_keygen_seeded ships it and as vpbs_key_expand rebuilds it -> (bodies words, full
    words): the bodies are the last of the K polynomials of every GLWE, 1 / K of the key set"""
    glwes = (n_lwe + 1) * K * ELL
    return glwes * N, glwes * K * N


def key_expand_args(N, K, ELL, n_lwe, bsk_bodies, ksk_bodies):
    """shapes of the host form of Context.key_expand / KeyRing.add_seeded / RingProver.add_seeded, checked without a device: bsk_bodies
    [n_lwe][K*ELL*N], ksk_bodies [K*ELL*N] (keygen_seeded's layout; either may be None) -> (bsk_bodies, ksk_bodies), contiguous uint64"""
    g = K * ELL * N
    b = None if bsk_bodies is None else _u64(bsk_bodies)
    k = None if ksk_bodies is None else _u64(ksk_bodies).reshape(-1)
    if (b is not None and b.shape != (n_lwe, g)) or (k is not None and k.size != g):
        raise ValueError("key_expand: expected bsk_bodies [%d][%d] and ksk_bodies [%d]" % (n_lwe, g, g))
    return b, k


def _seeded_add_args(obj, bsk_bodies, ksk_bodies, bodies_on_device):
    if bodies_on_device:
        return C.c_void_p(int(bsk_bodies)), C.c_void_p(int(ksk_bodies)), None
    b, k = key_expand_args(obj.N, obj.K, obj.ELL, obj.n_lwe, bsk_bodies, ksk_bodies)
    if b is None or k is None:
        raise ValueError("add_seeded: both bsk_bodies and ksk_bodies are needed")
    return C.c_void_p(b.ctypes.data), C.c_void_p(k.ctypes.data), (b, k)


DECODE_OUTPUTS = ("phase", "msg", "err")
ROTATION_OUTPUTS = ("rot", "idx", "dev")


def _lwe_rows_batch(who, names, call, host_text, ctx, s_lwe, cts, expected, count, stats, want, n_lwe):
    """the body of the two calls that turn rows [count][n + 1] into three words per row and a tally (vpbs_lwe_decode_batch,
    vpbs_lwe_rotation_batch): names are the three outputs (the last one signed), call(h, key pointer, key_on_device, cts, count, n, expected,
    the three output pointers, stats, where) the entry point; host_text(key) words the refusal of a call without a context"""
    h = ctx.h if ctx is not None else None
    key = None if _is_dev(s_lwe) else _u64(s_lwe).reshape(-1)
    n = key.size if key is not None else n_lwe
    if n is None:
        raise ValueError("%s: a key on the device needs n_lwe" % who)
    if any(w not in names for w in want):
        raise ValueError("%s: want names any of %r" % (who, names))
    rows = None if _is_dev(cts) else _u64(cts)
    if rows is not None:
        if rows.ndim != 2 or rows.shape[1] != n + 1 or (count is not None and count != rows.shape[0]):
            raise ValueError("%s: expected cts [count][%d]" % (who, n + 1))
        count = rows.shape[0]
    elif count is None:
        raise ValueError("%s: ciphertexts on the device need count" % who)
    if isinstance(want, dict) and rows is not None:
        raise ValueError("%s: device outputs need device ciphertexts" % who)
    exp = None if expected is None or _is_dev(expected) else _u64(expected).reshape(-1)
    if exp is not None and exp.size != count:
        raise ValueError("%s: expected must have count = %d entries" % (who, count))
    keep = np.zeros(1, np.uint64)
    tmp, outs = None, {}
    try:
        if rows is not None:
            where, pc, pe = 0, _keep_ptr(rows), _keep_ptr(exp)
        else:
            where, pc = (1 if isinstance(want, dict) else 2), int(cts)
            if exp is not None:
                tmp = ctx.device_upload_new(exp if count else keep)
            pe = None if expected is None else tmp if exp is not None else int(expected)
        if where == 1:
            po = [int(want[w]) if w in want else None for w in names]
        else:
            outs = {w: np.zeros(count, np.uint64) for w in want}
            po = [_keep_ptr(outs.get(w)) for w in names]
        rc = call(h, int(s_lwe) if key is None else key.ctypes.data, 1 if key is None else 0, pc, count, n, pe, po,
                  C.byref(stats.c) if stats is not None else None, where)
    finally:
        if tmp is not None:
            ctx.device_free(tmp)
    if rc:
        raise VpbsError("vpbs_%s: status %d: %s" % (who, rc, lib().vpbs_last_error(h).decode() if h else host_text(key)))
    if where == 1:
        return None
    if names[2] in outs:
        outs[names[2]] = outs[names[2]].view(np.int64)
    return outs


def _lwe_decode_batch(ctx, s_lwe, cts, delta, modulus, expected, count, stats, want, n_lwe):
    def call(h, pkey, key_dev, pc, count, n, pe, po, pstats, where):
        return lib().vpbs_lwe_decode_batch(h, pkey, key_dev, pc, count, n, int(delta), int(modulus), pe, po[0], po[1], po[2], pstats, where)
    return _lwe_rows_batch("lwe_decode_batch", DECODE_OUTPUTS, call, lambda key: "bad arguments", ctx, s_lwe, cts, expected, count, stats, want,
                           n_lwe)


def _lwe_rotation_batch(ctx, s_lwe, cts, N, p, log_slots, expected, count, stats, want, n_lwe):
    N = int(N)
    if N < 2 or N & (N - 1):
        raise ValueError("lwe_rotation_batch: N must be a power of two, 2 .. 2^16")

    def call(h, pkey, key_dev, pc, count, n, pe, po, pstats, where):
        return lib().vpbs_lwe_rotation_batch(h, pkey, key_dev, pc, count, n, N.bit_length() - 1, int(log_slots), int(p), pe, po[0], po[1], po[2],
                                             pstats, where)

    def host_text(key):   # no context to hold the text: name the first offending index here
        bad = np.nonzero(key % np.uint64(P) > 1)[0] if key is not None else ()
        return "key word %d is neither 0 nor 1" % bad[0] if len(bad) else "bad arguments"
    return _lwe_rows_batch("lwe_rotation_batch", ROTATION_OUTPUTS, call, host_text, ctx, s_lwe, cts, expected, count, stats, want, n_lwe)


def lwe_encrypt_batch(params, s_lwe, messages, nonce0=0):
    """vpbs_lwe_encrypt_batch on the host (null context): row i = lwe_encrypt(params, s_lwe, messages[i], nonce0 + i) -> cts [count][n + 1]"""
    return _lwe_encrypt_batch(None, params, s_lwe, messages, nonce0, None, None)


def lwe_encrypt_seeded_batch(params, mask_seed, s_lwe, messages, nonce0=0):
    """vpbs_lwe_encrypt_seeded_batch on the host (null context): bodies [count], the last word of lwe_encrypt_batch's rows when the mask
    streams are keyed by mask_seed and the noise by params.seed (mask_seed == params.seed: of lwe_encrypt_batch's rows themselves)"""
    return _lwe_encrypt_batch(None, params, s_lwe, messages, nonce0, None, None, mask_seed=mask_seed)


def lwe_expand_batch(n_lwe, mask_seed, bodies, nonce0=0):
    """vpbs_lwe_expand_batch on the host (null context): row i = the n_lwe mask words of nonce nonce0 + i under mask_seed, then bodies[i]
    -> cts [count][n + 1]"""
    return _lwe_expand_batch(None, n_lwe, mask_seed, bodies, nonce0, None, None)


def lwe_decode_batch(s_lwe, cts, delta, modulus, expected=None, stats=None, want=("msg",)):
    """vpbs_lwe_decode_batch on the host (null context); see Context.lwe_decode_batch"""
    return _lwe_decode_batch(None, s_lwe, cts, delta, modulus, expected, None, stats, want, None)


def lwe_rotation_batch(s_lwe, cts, N, p, log_slots=0, expected=None, stats=None, want=("idx",)):
    """vpbs_lwe_rotation_batch on the host (null context); see Context.lwe_rotation_batch"""
    return _lwe_rotation_batch(None, s_lwe, cts, N, p, log_slots, expected, None, stats, want, None)


def lut_expect(testv, mu, j=0):
    """the prediction contract of vpbs_lwe_rotation_batch, stated once: E(mu + j), the phase of coefficient j of the output GLWE of a
    bootstrap with rotation mu ("rot") under test vector testv [N] when the keys are noise-free and the decomposition exact; indices mod 2N,
    E(x) = testv[x] for x < N and -testv[x - N] otherwise.  mu a number -> int, an array -> np.uint64 array"""
    tv = _u64(testv).reshape(-1)
    n = tv.size
    x = (np.asarray(mu).astype(np.int64) + int(j)) % (2 * n)
    v = tv[x % n] % np.uint64(P)
    out = np.where(x >= n, (np.uint64(P) - v) % np.uint64(P), v)
    return int(out) if out.ndim == 0 else out


def _lwe_snap(ctx, N, log_slots, words, count=None, out_dev_ptr=None):
    h = ctx.h if ctx is not None else None
    if out_dev_ptr is not None:
        rc = lib().vpbs_lwe_snap(h, N.bit_length() - 1, log_slots, _dev(words), count, _dev(out_dev_ptr), 1)
        out = None
    else:
        w = _u64(words)
        out = np.zeros(w.shape, np.uint64)
        rc = lib().vpbs_lwe_snap(h, N.bit_length() - 1, log_slots, _keep_ptr(w), w.size, _keep_ptr(out), 0)
    if rc:
        raise VpbsError("vpbs_lwe_snap: status %d: %s" % (rc, lib().vpbs_last_error(h).decode() if h else "bad arguments (log_slots <= log_N <= 11)"))
    return out


def _lwe_extract_at(ctx, glwe, n_lwe, index, src, count=None, N=None, K=None, out_dev_ptr=None):
    h = ctx.h if ctx is not None else None
    ix, sr = (np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (index, src))
    if ix.size != sr.size:
        raise ValueError("lwe_extract_at: index and src must have one entry per output row")
    rows = ix.size
    pi, ps = _keep_u32(ix), _keep_u32(sr)
    if out_dev_ptr is not None:
        rc = lib().vpbs_lwe_extract_at(h, N.bit_length() - 1, K, n_lwe, C.c_void_p(int(glwe)), count, pi, ps, rows, C.c_void_p(int(out_dev_ptr)), 1)
        out = None
    else:
        g = _u64(glwe)
        g3 = g.reshape((1,) + g.shape) if g.ndim == 2 else g
        cnt, K_, N_ = g3.shape
        out = np.zeros((rows, n_lwe + 1), np.uint64)
        rc = lib().vpbs_lwe_extract_at(h, N_.bit_length() - 1, K_, n_lwe, _keep_ptr(g3), cnt, pi, ps, rows, _keep_ptr(out), 0)
    if rc:
        raise VpbsError("vpbs_lwe_extract_at: status %d: %s" % (rc, lib().vpbs_last_error(h).decode() if h else
                                                                "bad arguments (index below N, src below count, 1 <= n_lwe <= (K - 1) N)"))
    return out


def lwe_snap(N, log_slots, words):
    """vpbs_lwe_snap on the host (null context): every word rounded to a multiple of 2^(64 - log2(2N) + log_slots) -- then the mod switch of
    every word, and of any sum of them, is a multiple of 2^log_slots.  log_slots = 0 only reduces below p.  -> array of the shape of words"""
    return _lwe_snap(None, N, log_slots, words)


def lwe_extract_at(glwe, n_lwe, index, src):
    """vpbs_lwe_extract_at on the host (null context): row i = sample extraction of coefficient index[i] of glwe[src[i]] (glwe [count][K][N], or
    one [K][N]) -> [rows][n_lwe + 1]; index 0 is Context.lwe_extract"""
    return _lwe_extract_at(None, glwe, n_lwe, index, src)


def lut_testv_multi(N, p, tables, delta=None):
    """vpbs_lut_testv_multi: tables [s][p], s a power of two with s * 2 p <= N, interleaved in groups of s coefficients: coefficient j < s of
    the bootstrap of a ciphertext snapped with log_slots = log2(s) carries tables[j][m] * delta -> (testv [N], delta)"""
    t = _u64(tables)
    if t.ndim != 2 or t.shape[1] != p or t.shape[0] < 1 or t.shape[0] & (t.shape[0] - 1):
        raise ValueError("lut_testv_multi: expected tables [s][%d] with s a power of two" % p)
    if delta is None:
        d = np.zeros(1, np.uint64)
        if lib().vpbs_testv(N.bit_length() - 1, p, None, _ptr(d)) != 0:
            raise VpbsError("vpbs_lut_testv_multi: bad arguments")
        delta = int(d[0])
    out = np.zeros(N, np.uint64)
    if lib().vpbs_lut_testv_multi(N.bit_length() - 1, p, t.shape[0].bit_length() - 1, _ptr(t.reshape(-1)), int(delta), _ptr(out)) != 0:
        raise VpbsError("vpbs_lut_testv_multi: bad arguments (p a power of two, entries below 2 p, s * 2 p <= N)")
    return out, int(delta)


def _key_args(who, bsk, ksk, K, ELL, N, n_lwe, keys_on_device):
    """the key set of a bootstrapping object: bsk [n][K*ELL*K*N] and ksk [K*ELL*K*N] as host arrays (keygen's layout), or device
    pointers (integers) with keys_on_device -> (bsk pointer, ksk pointer, N, n_lwe, what the pointers refer to).  N and n_lwe are the
    shape the keys must have; None: the shape is read off the host arrays, and device keys are refused."""
    if keys_on_device:
        if N is None or n_lwe is None:
            raise ValueError("%s: device keys need N and n_lwe" % who)
        return C.c_void_p(int(bsk)), C.c_void_p(int(ksk)), N, n_lwe, None
    b, k = _u64(bsk), _u64(ksk).reshape(-1)
    if N is None or n_lwe is None:
        n_lwe, N = b.shape[0], k.size // (K * ELL * K)
        want = "bsk [n][K*ELL*K*N] and ksk [K*ELL*K*N]"
    else:
        want = "bsk [%d][%d] and ksk [%d]" % (n_lwe, K * ELL * K * N, K * ELL * K * N)
    if b.shape != (n_lwe, K * ELL * K * N) or k.size != K * ELL * K * N:
        raise ValueError("%s: expected %s" % (who, want))
    return C.c_void_p(b.ctypes.data), C.c_void_p(k.ctypes.data), N, n_lwe, (b, k)


class _ChainRun(_Handle):
    """The run methods of Bootstrapper and KeyRing: one body each for run, run_from and run_device; key_of (the ring's slots) is
    checked and passed on only by the ring (_ring).  The object has N, K, n_lwe and, for key_of, max_keys."""
    _ring = False

    def _run_fail(self, name, rc, status=True):
        e = self._fail("%s_%s" % (self._prefix, name), rc, lib().vpbs_last_error(self.ctx.h).decode())
        return e if status else VpbsError(str(e))

    def _outputs(self, count):
        return np.zeros((count, self.K, self.N), np.uint64), np.zeros((count, self.n_lwe + 1), np.uint64)

    def _run(self, cts, testv, accumulators, key_of=None):
        ring, who = self._ring, type(self).__name__ + ".run"
        c, tv = _cts_testv(who, self.N, self.n_lwe, cts, testv)
        count = c.shape[0]
        ko = [_keep_u32(keyring_key_of(key_of, count, self.max_keys))] if ring else []
        out_ct, lwe_out = self._outputs(count)
        accs = np.zeros((count, self.n_lwe + 2, self.K, self.N), np.uint64) if accumulators else None
        rc = self._entry("run")(self.h, _keep_ptr(c), count, *ko, _keep_ptr(tv), 1 if tv.ndim == 2 else 0, _keep_ptr(out_ct), _keep_ptr(lwe_out),
                                _keep_ptr(accs), 0)
        if rc != count:
            raise self._run_fail("run", rc, status=ring)
        return (out_ct, lwe_out, accs) if accumulators else (out_ct, lwe_out)

    def _run_from(self, cts, start, acc_in, testv, accumulators, key_of=None):
        who = type(self).__name__ + ".run_from"
        c, st, acc, tv = run_from_args(self.N, self.K, self.n_lwe, cts, start, acc_in, testv, who)
        count = c.shape[0]
        ko = [_keep_u32(keyring_key_of(key_of, count, self.max_keys))] if self._ring else []
        out_ct, lwe_out = self._outputs(count)
        accs = _accs_out(accumulators, count, self.n_lwe, self.K, self.N, who)
        rc = self._entry("run_from")(self.h, _keep_ptr(c), count, *ko, _keep_u32(st), _keep_ptr(acc), _keep_ptr(tv), 1 if tv.ndim == 2 else 0,
                                     _keep_ptr(out_ct), _keep_ptr(lwe_out), _keep_ptr(accs), 0)
        if rc != count:
            raise self._run_fail("run_from", rc)
        return (out_ct, lwe_out) if accs is None else (out_ct, lwe_out, accs)

    def _run_device(self, d_cts, count, d_testv, testv_per_ct, d_out_ct, d_lwe_out, d_accs, key_of=None):
        ko = [_keep_u32(keyring_key_of(key_of, count, self.max_keys))] if self._ring else []
        rc = self._entry("run")(self.h, _dev(d_cts), count, *ko, _dev(d_testv), 1 if testv_per_ct else 0, _dev(d_out_ct), _dev(d_lwe_out),
                                _dev(d_accs), 1)
        if rc != count:
            raise self._run_fail("run", rc, status=self._ring)


class Bootstrapper(_ChainRun):
    """vpbs_bootstrapper: the whole PBS (accumulator chain of verified_pbs + partial_sample_extract) for batches of LWE ciphertexts in one
    launch, under a key set that stays on the device.  bsk [n][K*ELL*K*N], ksk [K*ELL*K*N] (keygen's layout): host arrays, or device
    pointers (integers) with keys_on_device=True, N and n_lwe given -- they must stay allocated while the object lives."""
    _prefix = "vpbs_bootstrapper"

    def __init__(self, ctx, bsk, ksk, K, ELL, LOGB, max_batch=64, N=None, n_lwe=None, keys_on_device=False):
        if not keys_on_device:
            N = n_lwe = None   # host keys say their own shape
        pb, pk, N, n_lwe, _keep = _key_args("Bootstrapper", bsk, ksk, K, ELL, N, n_lwe, keys_on_device)
        self.N, self.K, self.ELL, self.LOGB, self.n_lwe, self.max_batch = N, K, ELL, LOGB, n_lwe, max_batch
        prm = TfheParamsC(N.bit_length() - 1, K, ELL, LOGB)
        self._construct(ctx, ctx.h, C.byref(prm), n_lwe, pb, pk, 1 if keys_on_device else 0, max_batch)

    def run(self, cts, testv, accumulators=False):
        """cts [count][n + 1]; testv [N] shared or [count][N] -> (out_ct [count][K][N], lwe_out [count][n + 1]) and, with accumulators=True,
        every intermediate accumulator [count][n + 2][K][N] (Context.pbs_accumulator_chain for each ciphertext)"""
        return self._run(cts, testv, accumulators)

    def run_from(self, cts, start, acc_in, testv, accumulators=False):
        """run with a start step per row (vpbs_bootstrapper_run_from): start [count] (0: from the test vector, as run; k in 1 .. n + 2: from
        acc_in[i] [K][N], the accumulator after step k - 1, running steps k .. n + 1); acc_in [count][K][N], or None when every start is 0.
        accumulators: True for a fresh array, or an array [count][n + 2][K][N] to write into -- slots below k - 1 of a resumed row keep
        what they held.  A start above n + 2 raises VpbsError with the library's message, which names the row; nothing is launched."""
        return self._run_from(cts, start, acc_in, testv, accumulators)

    def run_device(self, d_cts, count, d_testv, testv_per_ct=False, d_out_ct=None, d_lwe_out=None, d_accs=None):
        """the same on device pointers (integers; None = output not wanted); returns when the outputs are in place"""
        self._run_device(d_cts, count, d_testv, testv_per_ct, d_out_ct, d_lwe_out, d_accs)


def run_from_args(N, K, n_lwe, cts, start, acc_in, testv, who="run_from"):
    """shapes of a run_from call, checked without a device: cts [count][n + 1], start [count] non-negative integers (their upper bound is
    the library's refusal, which names the row), acc_in [count][K][N] or None, testv [N] or [count][N] -> (cts, start as uint32, acc_in,
    testv), contiguous"""
    c, tv = _cts_testv(who, N, n_lwe, cts, testv)
    st = np.asarray(start)
    if st.shape == (0,):
        st = st.astype(np.uint32)
    if st.dtype.kind not in "iu" or st.shape != (c.shape[0],):
        raise ValueError("%s: expected start [%d], one integer step per ciphertext" % (who, c.shape[0]))
    for i, v in enumerate(st.tolist()):
        if v < 0 or v > 0xFFFFFFFF:
            raise ValueError("%s: start[%d] = %d is not a step" % (who, i, v))
    acc = None
    if acc_in is not None:
        acc = _u64(acc_in)
        if acc.shape != (c.shape[0], K, N):
            raise ValueError("%s: expected acc_in [%d][%d][%d], got shape %s" % (who, c.shape[0], K, N, acc.shape))
    elif st.any():
        raise ValueError("%s: a row with start > 0 needs acc_in" % who)
    return c, np.ascontiguousarray(st, dtype=np.uint32), acc, tv


def _accs_out(accumulators, count, n_lwe, K, N, who):
    """the accumulators argument of run_from: False / None -> None, True -> a zeroed array, an array -> itself (written in place)"""
    if accumulators is None or accumulators is False:
        return None
    if accumulators is True:
        return np.zeros((count, n_lwe + 2, K, N), np.uint64)
    a = accumulators
    if not isinstance(a, np.ndarray) or a.dtype != np.uint64 or not a.flags["C_CONTIGUOUS"] or a.shape != (count, n_lwe + 2, K, N):
        raise ValueError("%s: accumulators must be True or a contiguous uint64 array [%d][%d][%d][%d]" % (who, count, n_lwe + 2, K, N))
    return a


def resume_args(N, n_lwe, cts, testv, checkpoints, steps=0, key_of=None, max_keys=None):
    """shapes of a PbsProver.resume / RingProver.resume call, checked without a device: cts [count][n + 1], testv [N] or [count][N],
    checkpoints a list of `count` entries, each bytes (non-empty) or None, steps 0 .. n + 2 and, for the ring prover (max_keys given), key_of
    [count] slots below max_keys -> (cts, testv, checkpoints as a list, key_of as uint32 or None)"""
    who = "RingProver.resume" if max_keys is not None else "PbsProver.resume"
    c, tv = _cts_testv(who, N, n_lwe, cts, testv)
    if int(steps) != steps or steps < 0 or steps > n_lwe + 2:
        raise ValueError("%s: steps must be 0 .. n_lwe + 2 = %d, got %r" % (who, n_lwe + 2, steps))
    if isinstance(checkpoints, (bytes, bytearray, memoryview)) or not hasattr(checkpoints, "__len__"):
        raise ValueError("%s: checkpoints must be a list of bytes or None, one entry per ciphertext" % who)
    cps = list(checkpoints)
    if len(cps) != c.shape[0]:
        raise ValueError("%s: expected %d checkpoints, one entry (bytes or None) per ciphertext, got %d" % (who, c.shape[0], len(cps)))
    for i, b in enumerate(cps):
        if b is None:
            continue
        if not isinstance(b, (bytes, bytearray)):
            raise ValueError("%s: checkpoints[%d] must be bytes or None, not %s" % (who, i, type(b).__name__))
        if len(b) == 0:
            raise ValueError("%s: checkpoints[%d] is empty; pass None for a chain that starts at step 0" % (who, i))
        cps[i] = bytes(b)
    ko = keyring_key_of(key_of, c.shape[0], max_keys) if max_keys is not None else None
    return c, tv, cps, ko


def _checkpoint_arrays(cps):
    """the checkpoints of resume_args as the C ABI wants them: (uint8_t* [count], size_t [count], what keeps the bytes alive)"""
    count = max(1, len(cps))
    ptrs, lens = (C.c_void_p * count)(), (C.c_size_t * count)()
    keep = [C.create_string_buffer(b, len(b)) if b is not None else None for b in cps]
    for i, k in enumerate(keep):
        ptrs[i] = C.addressof(k) if k is not None else None
        lens[i] = len(cps[i]) if k is not None else 0
    return ptrs, lens, keep


def keyring_key_of(key_of, count, max_keys):
    """the key_of argument of KeyRing.run as the C ABI wants it: a contiguous uint32 array [count] of slots below max_keys.  Refused here,
    before any device call: a non-integer dtype, a shape other than [count], a negative slot or one at or above max_keys."""
    k = np.asarray(key_of)
    if k.shape == (0,):   # an empty list has no dtype of its own
        k = k.astype(np.uint32)
    if k.dtype.kind not in "iu":
        raise ValueError("KeyRing: key_of must hold integers, not %s" % k.dtype)
    if k.shape != (count,):
        raise ValueError("KeyRing: expected key_of [%d], one slot per ciphertext, got shape %s" % (count, k.shape))
    for i, v in enumerate(k.tolist()):
        if v < 0 or v >= max_keys:
            raise ValueError("KeyRing: key_of[%d] = %d is not a slot of a ring of %d (max_keys)" % (i, v, max_keys))
    return np.ascontiguousarray(k, dtype=np.uint32)


def keyring_run_args(N, n_lwe, max_keys, cts, key_of, testv):
    """shapes of a KeyRing.run call, checked without a device: cts [count][n + 1], key_of [count], testv [N] or [count][N]"""
    c, tv = _cts_testv("KeyRing.run", N, n_lwe, cts, testv)
    return c, keyring_key_of(key_of, c.shape[0], max_keys), tv


def program_batch_args(n_inputs, n_lwe, N, n_luts, max_keys, inputs, key_of, testvs, gate_outputs=None):
    """shapes of a Program.run_batch call, checked without a device: inputs [instances][n_inputs][n + 1], key_of [instances] slots below
    max_keys (any integer dtype; the offending index is named), testvs [n_luts][N] -> (inputs, key_of as uint32, testvs), contiguous.
    With gate_outputs [n_gates] (a program with multi-output gates; 1 per plain gate) the shape of wires_out comes fourth:
    (instances, n_inputs + sum gate_outputs, n + 1)."""
    if gate_outputs is not None:
        x, ko, tv = program_batch_args(n_inputs, n_lwe, N, n_luts, max_keys, inputs, key_of, testvs)
        m = np.asarray(gate_outputs, dtype=np.int64).reshape(-1)
        if (m < 1).any():
            raise ValueError("Program.run_batch: gate %d has no output" % int(np.argmax(m < 1)))
        return x, ko, tv, (x.shape[0], n_inputs + int(m.sum()), n_lwe + 1)
    x, tv = _u64(inputs), _u64(testvs)
    if x.ndim != 3 or x.shape[1:] != (n_inputs, n_lwe + 1):
        raise ValueError("Program.run_batch: expected inputs [instances][%d][%d], got shape %s" % (n_inputs, n_lwe + 1, x.shape))
    if tv.shape != (n_luts, N):
        raise ValueError("Program.run_batch: expected testvs [%d][%d], got shape %s" % (n_luts, N, tv.shape))
    return x, keyring_key_of(key_of, x.shape[0], max_keys), tv


class _KeySlots:
    """The slots of a key ring as KeyRing and RingProver fill them: add, add_seeded, remove.  The object is a _Handle with N, K, ELL and
    n_lwe; _slot_err says whether its entries end in (err, err_len) -- the ring prover's do; the ring's leave the text with the context."""
    _slot_err = False

    def _slot_call(self, name, *args):
        err = C.create_string_buffer(512)
        rc = self._entry(name)(self.h, *args, *((err, 512) if self._slot_err else ()))
        if rc:
            raise self._fail("%s_%s" % (self._prefix, name), rc, (err.value if self._slot_err else lib().vpbs_last_error(self.ctx.h)).decode())

    def add(self, bsk, ksk, keys_on_device=False):
        """bsk [n][K*ELL*K*N], ksk [K*ELL*K*N] (keygen's layout) uploaded once, or device pointers (integers) adopted with
        keys_on_device=True -- they must stay allocated until the slot is removed.  Returns the slot: the lowest free number.  The ring
        prover also walks the key hash chain of the key set once, on the host."""
        pb, pk, _, _, _keep = _key_args(type(self).__name__ + ".add", bsk, ksk, self.K, self.ELL, self.N, self.n_lwe, keys_on_device)
        slot = C.c_uint()
        self._slot_call("add", pb, pk, 1 if keys_on_device else 0, C.byref(slot))
        return slot.value

    def add_seeded(self, mask_seed, bsk_bodies, ksk_bodies, bodies_on_device=False):
        """<_prefix>_add_seeded: the key set of Context.key_expand(mask_seed, bodies), expanded on the device into memory the ring owns
        (remove frees it).  bsk_bodies [n][K*ELL*N], ksk_bodies [K*ELL*N] (keygen_seeded's layout, 1 / K of the key set), or device pointers
        (integers) with bodies_on_device=True -- they are read during the call only.  Returns the slot: the lowest free number.  The ring
        prover downloads the expanded key set once for its key hash chain, as add does for keys that are on the device only."""
        pb, pk, _keep = _seeded_add_args(self, bsk_bodies, ksk_bodies, bodies_on_device)
        slot = C.c_uint()
        self._slot_call("add_seeded", int(mask_seed), pb, pk, 1 if bodies_on_device else 0, C.byref(slot))
        return slot.value

    def remove(self, slot):
        self._slot_call("remove", int(slot))


class KeyRing(_KeySlots, _ChainRun):
    """vpbs_keyring: up to max_keys key sets of one shape resident on the device, and the whole PBS of a MIXED batch -- ciphertext i under
    the key set of slot key_of[i] -- in one launch.  Row i of every output is what Bootstrapper(key set key_of[i]).run gives for it."""
    _prefix = "vpbs_keyring"
    _ring = True

    def __init__(self, ctx, K, ELL, LOGB, N, n_lwe, max_keys, max_batch=64):
        self.N, self.K, self.ELL, self.LOGB, self.n_lwe = N, K, ELL, LOGB, n_lwe
        self.max_keys, self.max_batch = max_keys, max_batch
        prm = TfheParamsC(N.bit_length() - 1, K, ELL, LOGB)
        self._construct(ctx, ctx.h, C.byref(prm), n_lwe, max_keys, max_batch)

    @classmethod
    def _view(cls, h, ctx, N, K, ELL, LOGB, n_lwe, max_keys, max_batch):
        """a KeyRing on a handle that another object owns and frees (RingProver.keyring): close() forgets the handle, nothing more"""
        ring = cls.__new__(cls)
        ring.h, ring.ctx, ring._owns = h, ctx, False
        ring.N, ring.K, ring.ELL, ring.LOGB, ring.n_lwe, ring.max_keys, ring.max_batch = N, K, ELL, LOGB, n_lwe, max_keys, max_batch
        return ring

    def count(self):
        return lib().vpbs_keyring_count(self.h)

    def run(self, cts, key_of, testv, accumulators=False):
        """cts [count][n + 1]; key_of [count] slots; testv [N] shared or [count][N] -> (out_ct [count][K][N], lwe_out [count][n + 1]) and,
        with accumulators=True, every intermediate accumulator [count][n + 2][K][N]"""
        return self._run(cts, testv, accumulators, key_of)

    def run_from(self, cts, key_of, start, acc_in, testv, accumulators=False):
        """Bootstrapper.run_from under the key set of slot key_of[i] (vpbs_keyring_run_from)"""
        return self._run_from(cts, start, acc_in, testv, accumulators, key_of)

    def run_device(self, d_cts, count, key_of, d_testv, testv_per_ct=False, d_out_ct=None, d_lwe_out=None, d_accs=None):
        """the same on device pointers (integers; None = output not wanted); key_of stays a host array; returns when the outputs are in place"""
        self._run_device(d_cts, count, d_testv, testv_per_ct, d_out_ct, d_lwe_out, d_accs, key_of)


def ivc_preset_matrix_for_tests(proof_words, n_lwe, first, pis, ct, bsk, ksk, cyclic_vk, dummy_vk, dummy_proof):
    """vpbs_test_ivc_preset_matrix (host, a test entry): the early-phase preset matrix [n_preset][count] of chain steps [first, first + count) as the
    device-witness pipeline's host loop builds it.  pis [count][n_pi]: the public inputs of the predecessors of those steps."""
    q, c, ks = _u64(pis), _u64(ct).reshape(-1), _u64(ksk).reshape(-1)
    bs = _u64(bsk).reshape(-1) if n_lwe else None
    cv, dv, dp = _u64(cyclic_vk).reshape(-1), _u64(dummy_vk).reshape(-1), _u64(dummy_proof).reshape(-1)
    count, n_pi = q.shape
    out = np.zeros((2 * (proof_words + n_pi) + 1 + ks.size + 1 + 2 * cv.size, count), np.uint64)
    rc = lib().vpbs_test_ivc_preset_matrix(proof_words, n_pi, ks.size, cv.size, n_lwe, first, count, _ptr(q), _ptr(c), _ptr(bs) if bs is not None else None,
                                      _ptr(ks), _ptr(cv), _ptr(dv), _ptr(dp), _ptr(out))
    if rc != 0:
        raise VpbsError("vpbs_test_ivc_preset_matrix: status %d" % rc)
    return out


class PbsProveError(VpbsError):
    """PbsProver.prove: some chains failed.  failures {index: message}; proofs (None at those indices), out_ct, lwe_out: what the others gave"""

    def __init__(self, failures, proofs, out_ct, lwe_out):
        super().__init__("vpbs_pbs_prover_run: " + "; ".join("ciphertext %d: %s" % f for f in sorted(failures.items())))
        self.failures, self.proofs, self.out_ct, self.lwe_out = failures, proofs, out_ct, lwe_out


class _BatchProver(_Handle):
    """What PbsProver and RingProver share: the chains' settings, the checkpoint callback, the run behind prove and resume, and the
    statistics of the last run.  The object lives on a device, not on a Context of the caller's."""

    def _create(self, device, cyclic, dummy, N, K, ELL, LOGB, *create_args):
        """create_args: what <_prefix>_create takes behind (device, cyclic, dummy, TFHE parameters)"""
        keep = []
        cy, du = _ivc_circuit(cyclic, cyclic.meta["proof_words"], keep), _ivc_circuit(dummy, 0, keep)
        prm = TfheParamsC(N.bit_length() - 1, K, ELL, LOGB)
        self._construct(None, device, C.byref(cy), C.byref(du), C.byref(prm), *create_args, status=True)
        self.vk_words = 4 + (4 << 4)
        self._proof_words = cyclic.meta["proof_words"]
        self._ckpt_cb = self._ckpt_error = None

    def verifier_data(self):
        """-> (cyclic circuit: digest [4] + cap, dummy circuit: the same)"""
        a, b = np.zeros(self.vk_words, np.uint64), np.zeros(self.vk_words, np.uint64)
        self._entry("verifier_data")(self.h, _ptr(a), _ptr(b))
        return a, b

    def set_check_witness(self, on=True):
        """every witness of later chains checked on the device before it is proven (Ivc.set_check_witness on every chain); resets the counters"""
        rc = self._entry("set_check_witness")(self.h, 1 if on else 0)
        if rc != 0:
            raise VpbsError("%s_set_check_witness: status %d" % (self._prefix, rc))

    def witness_checks(self):
        """-> (witnesses checked, violations found), summed over the chains, since the last set_check_witness"""
        out = np.zeros(2, np.uint64)
        self._entry("witness_checks")(self.h, _ptr(out))
        return int(out[0]), int(out[1])

    def on_checkpoint(self, every, fn):
        """fn(index, done, bytes) after every chained step `done` of ciphertext `index` that is a multiple of `every` and below the chain's
        last step (Ivc.on_checkpoint with the ciphertext index); never two calls at once.  every = 0 or fn = None turns it off.  An
        exception raised by fn is kept and re-raised by prove.  A chain resumed at step k (resume) counts its `every` from k -- after
        steps k + every, k + 2 every, .. -- and `done` stays the number of chain steps."""
        self._ckpt_error = None
        if fn is None or not every:
            self._ckpt_cb = None
            self._entry("set_checkpoint")(self.h, 0, C.cast(None, PBS_CHECKPOINT_FN), None)
            return

        def trampoline(_user, index, done, data, n):
            try:
                if self._ckpt_error is None:
                    fn(int(index), int(done), C.string_at(data, n))
            except BaseException as e:   # noqa: BLE001 -- must not unwind through the C frames
                self._ckpt_error = e
        self._ckpt_cb = PBS_CHECKPOINT_FN(trampoline)
        self._entry("set_checkpoint")(self.h, every, self._ckpt_cb, None)

    def _run(self, c, tv, cps, steps, on_proof, key_of=None, out_ct=None, lwe_out=None):
        """<_prefix>_run, or _resume with the checkpoints cps; key_of: the ring prover's slots -> (proofs, out_ct, lwe_out, errors)"""
        count = c.shape[0]
        out_ct = np.zeros((count, self.K, self.N), np.uint64) if out_ct is None else out_ct
        lwe_out = np.zeros((count, self.n_lwe + 1), np.uint64) if lwe_out is None else lwe_out
        if out_ct.shape != (count, self.K, self.N) or lwe_out.shape != (count, self.n_lwe + 1):
            raise ValueError("%s.prove: expected out_ct [count][K][N] and lwe_out [count][n + 1]" % type(self).__name__)
        proofs, failures, raised, errors = [None] * count, [], [], [None] * count

        def trampoline(_user, index, data, n, error):
            try:
                if not data:
                    text = (error or b"").decode()
                    if cps is not None and text.startswith("checkpoint: "):
                        errors[index] = text   # a refused checkpoint: reported, not raised
                    else:
                        failures.append((int(index), text))
                    return
                proofs[index] = C.string_at(data, n)
                if on_proof is not None and not raised:
                    on_proof(int(index), proofs[index])
            except BaseException as e:   # noqa: BLE001 -- must not unwind through the C frames
                raised.append(e)
        cb, err = PBS_PROOF_FN(trampoline), C.create_string_buffer(512)
        args = [self.h, _keep_ptr(c), count] + ([] if key_of is None else [_keep_u32(key_of)])
        args += [_keep_ptr(tv), 1 if tv.ndim == 2 else 0]
        what = self._prefix + "_run"
        if cps is not None:
            what = self._prefix + "_resume"
            ptrs, lens, alive = _checkpoint_arrays(cps)
            args += [C.addressof(ptrs), C.addressof(lens)]
        n = getattr(lib(), what)(*args, steps, _keep_ptr(out_ct), _keep_ptr(lwe_out), cb, None, err, 512)
        if raised:
            raise raised[0]
        e, self._ckpt_error = self._ckpt_error, None
        if e is not None:
            raise e
        if n < 0:
            raise self._fail(what, n, err.value.decode())
        if failures:
            raise PbsProveError(dict(failures), proofs, out_ct, lwe_out)
        return proofs, out_ct, lwe_out, errors

    def last_run(self):
        """<_prefix>_last_run -> dict: seconds, outputs_seconds (call until out_ct / lwe_out were complete), proofs, prepare_chain_ms
        (per chain: waiting for its public inputs) and chain = the mean vpbs_ivc_timing of the delivered chains"""
        st = PbsRunStatsC()
        self._entry("last_run")(self.h, C.byref(st))
        return {"seconds": st.seconds, "outputs_seconds": st.outputs_seconds, "proofs": st.proofs, "prepare_chain_ms": st.prepare_chain_ms,
                "chain": {f: getattr(st.chain, f) for f, _ in IvcTimingC._fields_}}


class PbsProver(_BatchProver):
    """vpbs_pbs_prover: the bootstraps of a batch of LWE ciphertexts AND their vPBS proofs under one key set that stays on the device.
    cyclic / dummy: circuit_file.CircuitDescription of the exported cyclic step circuit and its dummy circuit.  bsk [n][K*ELL*K*N], ksk
    [K*ELL*K*N] (keygen's layout): host arrays, or device pointers (integers) with keys_on_device=True and n_lwe given -- they must stay
    allocated while the object lives.  `chains` IVC chains run side by side, each in the device-witness pipeline with `witness_batch` steps
    per batch."""
    _prefix = "vpbs_pbs_prover"

    def __init__(self, device, cyclic, dummy, bsk, ksk, K, ELL, LOGB, chains=8, witness_batch=64, keys_on_device=False, N=None, n_lwe=None):
        if not keys_on_device:
            N = n_lwe = None   # host keys say their own shape
        pb, pk, N, n_lwe, _keep = _key_args("PbsProver", bsk, ksk, K, ELL, N, n_lwe, keys_on_device)
        self.N, self.K, self.ELL, self.LOGB, self.n_lwe, self.chains = N, K, ELL, LOGB, n_lwe, chains
        self._create(device, cyclic, dummy, N, K, ELL, LOGB, n_lwe, pb, pk, 1 if keys_on_device else 0, chains, witness_batch)

    def key_hash(self):
        """the end of the key hash chain walked at creation: what PbsVerifier takes (= pbs_key_hash(bsk, ksk))"""
        out = np.zeros(4, np.uint64)
        lib().vpbs_pbs_prover_key_hash(self.h, _ptr(out))
        return out

    def prove(self, cts, testv, steps=0, on_proof=None):
        """cts [count][n + 1]; testv [N] shared or [count][N] -> (proofs: list of bytes in the order of cts, out_ct [count][K][N], lwe_out
        [count][n + 1]).  on_proof(index, bytes) is called as each proof completes (completion order, never two calls at once); an exception
        it raises is re-raised here after the run has drained.  A chain that fails does not stop the others: after the run PbsProveError is
        raised, naming the failed indices, with .failures {index: message} and .proofs (None at the failed indices), .out_ct, .lwe_out --
        everything the chains that succeeded delivered."""
        c, tv = _cts_testv("PbsProver.prove", self.N, self.n_lwe, cts, testv)
        return self._run(c, tv, None, steps, on_proof)[:3]

    def resume(self, cts, testv, checkpoints, steps=0, on_proof=None):
        """prove, with a checkpoint per ciphertext (vpbs_pbs_prover_resume): checkpoints is a list of bytes (what on_checkpoint's fn received
        for that ciphertext: the proof after chain steps 0 .. k - 1) or None (an ordinary chain from step 0) -> (proofs, out_ct, lwe_out,
        errors).  A resumed chain goes on at step k and delivers the proof of the uninterrupted chain, byte for byte; steps = k returns the
        checkpoint itself.  A checkpoint the prover refuses (it does not verify, belongs to another ciphertext or key set, or lies beyond
        `steps`) raises nothing: the row is None in proofs and errors[i] is the message ("checkpoint: ..."); errors is None elsewhere, and
        out_ct / lwe_out are complete for every row.  Chains that fail for another reason raise PbsProveError as in prove."""
        c, tv, cps, _ = resume_args(self.N, self.n_lwe, cts, testv, checkpoints, steps)
        return self._run(c, tv, cps, steps, on_proof)

    def dummy_proof_for_tests(self):
        """vpbs_test_pbs_prover_dummy_proof: the dummy proof [proof_words] as the object's vpbs_ivc holds it on the host"""
        out = np.zeros(self._proof_words, np.uint64)
        if lib().vpbs_test_pbs_prover_dummy_proof(self.h, _ptr(out)) != 0:
            raise VpbsError("vpbs_test_pbs_prover_dummy_proof failed")
        return out

    def preset_matrix(self, ct, testv, first, count):
        """vpbs_test_pbs_prover_preset_matrix (a test entry): the early-phase preset matrix [n_preset][count] of steps [first, first + count) of the chain of
        `ct`, assembled on the device by the kernels the chains use"""
        c, tv = _u64(ct).reshape(-1), _u64(testv).reshape(-1)
        out = np.zeros((lib().vpbs_test_pbs_prover_preset_words(self.h), count), np.uint64)
        rc = lib().vpbs_test_pbs_prover_preset_matrix(self.h, _ptr(c), _ptr(tv), first, count, _ptr(out))
        if rc != 0:
            raise VpbsError("vpbs_test_pbs_prover_preset_matrix: status %d" % rc)
        return out


def ring_prove_args(N, n_lwe, max_keys, cts, key_of, testv, steps=0):
    """shapes of a RingProver.prove call, checked without a device: cts [count][n + 1], key_of [count] slots below max_keys (any integer
    dtype; the offending index is named), testv [N] or [count][N], steps 0 .. n + 2 -> (cts, key_of as uint32, testv), contiguous"""
    c, tv = _cts_testv("RingProver.prove", N, n_lwe, cts, testv)
    if int(steps) != steps or steps < 0 or steps > n_lwe + 2:
        raise ValueError("RingProver.prove: steps must be 0 .. n_lwe + 2 = %d, got %r" % (n_lwe + 2, steps))
    return c, keyring_key_of(key_of, c.shape[0], max_keys), tv


class _RingContext:
    """the context of a RingProver's ring, as far as KeyRing and Program.run_batch need one: the handle (for vpbs_last_error)"""

    def __init__(self, h):
        self.h, self._batches = h, set()


class RingProver(_KeySlots, _BatchProver):
    """vpbs_ring_prover: ONE prover for all clients of a key ring.  The object owns a KeyRing of max_keys slots, `chains` IVC chains in the
    device-witness pipeline and the key hash chain of every slot; prove() bootstraps and proves ciphertext i under the key set of slot
    key_of[i], and its proof is byte for byte what a PbsProver of that key set gives.  cyclic / dummy, chains, witness_batch: as PbsProver.
    .keyring is a KeyRing view of the owned ring (KeyRing.run and Program.run_batch evaluate on the same resident keys; it is not closed
    by the caller, and its add / remove are refused: key sets come and go through this object, which keeps their key links)."""
    _prefix = "vpbs_ring_prover"
    _slot_err = True
    keyring = None

    def __init__(self, device, cyclic, dummy, K, ELL, LOGB, N, n_lwe, max_keys, chains=8, witness_batch=64):
        self.N, self.K, self.ELL, self.LOGB, self.n_lwe, self.chains, self.max_keys = N, K, ELL, LOGB, n_lwe, chains, max_keys
        self._create(device, cyclic, dummy, N, K, ELL, LOGB, n_lwe, max_keys, chains, witness_batch)
        self.keyring = KeyRing._view(C.c_void_p(lib().vpbs_ring_prover_keyring(self.h)), _RingContext(C.c_void_p(lib().vpbs_ring_prover_context(self.h))),
                                     N, K, ELL, LOGB, n_lwe, max_keys, 256)

    def key_hash(self, slot):
        """the end of the slot's key hash chain: what the PbsVerifier of that client takes (= pbs_key_hash(bsk, ksk))"""
        out = np.zeros(4, np.uint64)
        rc = lib().vpbs_ring_prover_key_hash(self.h, int(slot), _ptr(out))
        if rc:
            raise self._fail("vpbs_ring_prover_key_hash", rc, "slot %d holds no key set" % slot)
        return out

    def prove(self, cts, key_of, testv, steps=0, on_proof=None, out_ct=None, lwe_out=None):
        """cts [count][n + 1]; key_of [count] slots; testv [N] shared or [count][N] -> (proofs: list of bytes in the order of cts, out_ct
        [count][K][N], lwe_out [count][n + 1]); on_proof, failures (PbsProveError) and `steps` as in PbsProver.prove.  A key_of entry that
        names an empty slot raises VpbsError (.status = VPBS_ERR_INVALID) with the ring's message before anything runs.  out_ct / lwe_out:
        arrays to write into instead of fresh ones."""
        c, ko, tv = ring_prove_args(self.N, self.n_lwe, self.max_keys, cts, key_of, testv, steps)
        return self._run(c, tv, None, steps, on_proof, ko, out_ct, lwe_out)[:3]

    def resume(self, cts, key_of, testv, checkpoints, steps=0, on_proof=None, out_ct=None, lwe_out=None):
        """PbsProver.resume under the key set of slot key_of[i] (vpbs_ring_prover_resume) -> (proofs, out_ct, lwe_out, errors).  A
        checkpoint presented under another slot than the one it was made under is refused with "checkpoint: the key hash chain does not
        match"."""
        c, tv, cps, ko = resume_args(self.N, self.n_lwe, cts, testv, checkpoints, steps, key_of, self.max_keys)
        return self._run(c, tv, cps, steps, on_proof, ko, out_ct, lwe_out)

    def _release(self):
        if self.keyring is not None:
            self.keyring.close()   # the view first: its handle goes with the prover's
        super()._release()


def ring_verify_args(N, K, n_lwe, max_keys, max_batch, count, key_of, testvs, cts, out_cts, testv_of=None):
    """shapes of a RingVerifier.verify call, checked without a device: key_of [count] slots below max_keys (any integer dtype; the offending
    index is named), testvs [N] or [n_testv][N], cts [count][n + 1], out_cts [count][K][N] (or [count][K N]), testv_of [count] indices below
    n_testv -- or None with n_testv == count (proof i takes testvs[i]) or n_testv == 1 -> (key_of as uint32, testvs [n_testv][N], cts,
    out_cts [count][K N], testv_of as uint32 or None), contiguous"""
    if count > max_batch:
        raise ValueError("RingVerifier.verify: %d proofs exceed max_batch %d" % (count, max_batch))
    tv, c, o = _u64(testvs), _u64(cts), _u64(out_cts)
    if tv.ndim == 1:
        tv = tv.reshape(1, -1)
    if tv.ndim != 2 or tv.shape[1] != N or tv.shape[0] > max_batch:
        raise ValueError("RingVerifier.verify: expected testvs [%d] or [n_testv][%d] with n_testv <= max_batch %d, got shape %s" % (N, N, max_batch, tv.shape))
    if c.shape != (count, n_lwe + 1) or o.size != count * K * N or (count and o.shape[0] != count):
        raise ValueError("RingVerifier.verify: expected cts [%d][%d] and out_cts [%d][%d][%d], got shapes %s and %s" % (count, n_lwe + 1, count, K, N,
                                                                                                                     c.shape, o.shape))
    ko = keyring_key_of(key_of, count, max_keys)
    n_testv = tv.shape[0]
    if testv_of is None:
        if n_testv not in (count, 1):
            raise ValueError("RingVerifier.verify: without testv_of, testvs must be [%d][N] (one per proof) or one shared vector, got %d" % (count, n_testv))
        to = None
    else:
        to = np.asarray(testv_of)
        if to.shape == (0,):
            to = to.astype(np.uint32)
        if to.dtype.kind not in "iu" or to.shape != (count,):
            raise ValueError("RingVerifier.verify: expected testv_of [%d] of integers, got %s %s" % (count, to.dtype, to.shape))
        for i, t in enumerate(to.tolist()):
            if t < 0 or t >= n_testv:
                raise ValueError("RingVerifier.verify: testv_of[%d] = %d is not below n_testv %d" % (i, t, n_testv))
        to = np.ascontiguousarray(to, dtype=np.uint32)
    return ko, tv, c, np.ascontiguousarray(o.reshape(count, K * N)), to


class RingVerifier(_PbsVerify):
    """vpbs_ring_verifier: ONE device verifier of whole vPBS proofs for the clients of a key ring.  Slot s holds the key hash of a key set
    (pbs_key_hash, or RingProver.key_hash(s): the caller chooses the slot, so the slots can be the ring prover's); verify() checks proof i
    against slot key_of[i] and gives it what a PbsVerifier made from that slot's key hash gives.  The parameters mirror PbsVerifier."""
    _prefix = "vpbs_ring_verifier"
    _run_err = True

    def __init__(self, ctx, cs_cap, ncols, circuit_digest, log_n, n_constants, n_routed, gates, N, K, n_lwe, ggsw_len, max_keys, max_batch=512,
                 num_challenges=2, quotient_degree_factor=8, rate_bits=3, cap_height=4, compat=None):
        self.max_keys = max_keys
        shape = (cs_cap, ncols, circuit_digest, log_n, n_constants, n_routed, gates, N, K, n_lwe, ggsw_len, num_challenges, quotient_degree_factor,
                 rate_bits, cap_height, compat)
        self._create(ctx, shape, N, K, n_lwe, max_batch, max_keys)

    def set_key(self, slot, key_hash):
        """fills or replaces a slot with a key hash [4]"""
        kh = np.ascontiguousarray(_u64(key_hash).reshape(-1))
        if kh.size != 4:
            raise ValueError("RingVerifier.set_key: a key hash is 4 words, got %d" % kh.size)
        rc = lib().vpbs_ring_verifier_set_key(self.h, int(slot), _ptr(kh))
        if rc:
            raise self._fail("vpbs_ring_verifier_set_key", rc, "slot %d of %d" % (slot, self.max_keys))

    def clear_key(self, slot):
        rc = lib().vpbs_ring_verifier_clear_key(self.h, int(slot))
        if rc:
            raise self._fail("vpbs_ring_verifier_clear_key", rc, "slot %d is empty or out of range" % slot)

    def count(self):
        return int(lib().vpbs_ring_verifier_count(self.h))

    def _statement(self, count, key_of, testvs, cts, out_cts, testv_of):
        ko, tv, c, o, to = ring_verify_args(self.N, self.K, self.n_lwe, self.max_keys, self.max_batch, count, key_of, testvs, cts, out_cts, testv_of)
        return _keep_u32(ko), _keep_ptr(tv.reshape(-1)), tv.shape[0], _keep_u32(to), _keep_ptr(c.reshape(-1)), _keep_ptr(o.reshape(-1))

    def verify_packed(self, buf, offsets, key_of, testvs, cts, out_cts, testv_of=None):
        """buf, offsets: pack_proofs; the rest as verify"""
        return self._verify(buf, offsets, key_of, testvs, cts, out_cts, testv_of)

    def verify(self, blobs, key_of, testvs, cts, out_cts, testv_of=None):
        """blobs: list of serialised vPBS proofs; key_of [count] slots; testvs [N] shared, [count][N], or a table [n_testv][N] addressed by
        testv_of [count]; cts [count][n + 1]; out_cts [count][K][N] -> (verdicts, reasons, proof_reasons), np.uint8 each.  A key_of entry
        that names an empty slot raises VpbsError (.status = VPBS_ERR_INVALID) before anything runs."""
        return self.verify_packed(*pack_proofs(blobs), key_of, testvs, cts, out_cts, testv_of)


# ---- aggregation: the vPBS proofs of a batch folded into one proof (csrc/aggregate.hip) ----
AGG_OK, AGG_MALFORMED, AGG_VERIFIER_DATA, AGG_PROOF, AGG_ROOT = range(5)   # vpbs_aggregate_reason, in vpbs_verify_aggregate's order
AGG_VK_WORDS = 68


class AggregateShapeC(C.Structure):
    _fields_ = [("N", C.c_uint), ("K", C.c_uint), ("n_lwe", C.c_uint), ("levels", C.c_uint), ("level_shapes", C.POINTER(VerifyInputsC)),
                ("vks", U64P)]


class AggregateStatsC(C.Structure):
    _fields_ = [("seconds", C.c_double), ("check_leaves_ms", C.c_double), ("witness_ms", C.c_double), ("prove_ms", C.c_double),
                ("nodes", C.c_uint), ("depth", C.c_uint)]


def aggregate_reason_text(reason):
    """vpbs_aggregate_reason_text: the `why` vpbs_verify_aggregate writes when that check fails ("" for AGG_OK)"""
    t = lib().vpbs_aggregate_reason_text(int(reason))
    if t is None:
        raise ValueError("no aggregate verifier reason %r" % (reason,))
    return t.decode()


def aggregate_depth(count):
    """d = max(1, ceil(log2 count)): the level whose circuit proves the root over `count` leaves"""
    if count < 1:
        raise ValueError("aggregate_depth: count must be at least 1")
    return max(1, (int(count) - 1).bit_length())


def _circuit_shape(v, d):
    """fills a VerifyInputsC from a circuit (circuit_file.CircuitDescription, or what a circuit builder's build() returns): degree, column
    counts, gates; cap, digest and public inputs stay empty"""
    n_constants = getattr(d, "n_constants", None)
    if n_constants is None:
        n_constants = d.constants.shape[0]
    n_routed, n_wires = getattr(d, "n_routed", 80), getattr(d, "n_wires", 135)
    v.log_n, v.rate_bits, v.cap_height = d.log_n, 3, 4
    v.n_constants_sigmas, v.n_wires, v.n_zs_partial_products, v.n_quotient = n_constants + n_routed, n_wires, 20, 16
    v.num_challenges = 2
    v.n_constants, v.n_routed, v.quotient_degree_factor = n_constants, n_routed, 8
    v.gates, v.n_gates, v.num_selectors = d.gates.arr, d.gates.n, d.gates.num_selectors


class AggregateShape:
    """vpbs_aggregate_shape: what a verifier of aggregates holds -- the ring (N, K, n_lwe), the level circuits A_1 .. A_levels (each an
    object with log_n, gates and n_constants or constants: a loaded circuit file or a built circuit) and vks [levels + 1][68]: vk_0 of the
    cyclic step circuit, then vk_l of A_l (Aggregator.verifier_data())."""

    def __init__(self, N, K, n_lwe, vks, level_circuits):
        self.N, self.K, self.n_lwe, self.levels = N, K, n_lwe, len(level_circuits)
        self.vks = np.ascontiguousarray(_u64(vks).reshape(-1, AGG_VK_WORDS))
        if self.levels < 1 or self.vks.shape[0] != self.levels + 1:
            raise ValueError("AggregateShape: %d level circuits need vks [%d][68], got %s" % (self.levels, self.levels + 1, self.vks.shape))
        self._shapes = (VerifyInputsC * self.levels)()
        self._keep = list(level_circuits)
        for v, d in zip(self._shapes, level_circuits):
            _circuit_shape(v, d)
        self.c = AggregateShapeC(N, K, n_lwe, self.levels, self._shapes, _ptr(self.vks))


def _aggregate_args(who, N, K, n_lwe, testvs, cts, out_cts, key_hashes, key_of, testv_of):
    """the statement arrays of an aggregate, shapes checked -> (count, testvs [n_testv][N], cts [count][n + 1], out_cts [count][K N],
    key_hashes [n_keys][4], key_of uint32 [count] or None, testv_of uint32 [count] or None)"""
    tv, c, o, kh = _u64(testvs), _u64(cts), _u64(out_cts), _u64(key_hashes)
    if tv.ndim == 1:
        tv = tv.reshape(1, -1)
    if kh.ndim == 1:
        kh = kh.reshape(1, -1)
    c = c.reshape(-1, n_lwe + 1)
    count = c.shape[0]
    if tv.ndim != 2 or tv.shape[1] != N or kh.ndim != 2 or kh.shape[1] != 4 or o.size != count * K * N:
        raise ValueError("%s: expected testvs [n_testv][%d], cts [count][%d], out_cts [count][%d][%d] and key_hashes [n_keys][4]; got %s, %s, %s, %s" %
                         (who, N, n_lwe + 1, K, N, tv.shape, c.shape, o.shape, kh.shape))

    def index(a, name):
        if a is None:
            return None
        a = np.asarray(a)
        if a.size and a.dtype.kind not in "iu" or a.shape != (count,):
            raise ValueError("%s: expected %s [%d] of integers, got %s %s" % (who, name, count, a.dtype, a.shape))
        if a.size and (int(a.min()) < 0 or int(a.max()) >= 1 << 32):
            raise ValueError("%s: %s holds an entry that is no uint32" % (who, name))
        return np.ascontiguousarray(a, dtype=np.uint32)
    return (count, np.ascontiguousarray(tv), np.ascontiguousarray(c), np.ascontiguousarray(o.reshape(count, K * N)), np.ascontiguousarray(kh),
            index(key_of, "key_of"), index(testv_of, "testv_of"))


def _aggregate_ptrs(tv, c, o, kh, ko, to):
    """the statement arrays of _aggregate_args in the order every aggregate entry point takes them"""
    return (_keep_ptr(tv), tv.shape[0], _keep_u32(to), _keep_ptr(c), _keep_ptr(o), _keep_ptr(kh), kh.shape[0], _keep_u32(ko))


def aggregate_root(N, K, n_lwe, vk0, testvs, cts, out_cts, key_hashes, key_of=None, testv_of=None):
    """vpbs_aggregate_root (host): the root of the aggregate's statement over the leaves (testvs[testv_of[i]], cts[i], out_cts[i],
    key_hashes[key_of[i]]) under the cyclic circuit's verifier data vk0 [68] -> [4].  VpbsError for no leaves, an index out of range, or a
    raw word of testvs / out_cts / key_hashes / vk0 at or above p (no proof has such a statement)."""
    count, tv, c, o, kh, ko, to = _aggregate_args("aggregate_root", N, K, n_lwe, testvs, cts, out_cts, key_hashes, key_of, testv_of)
    vk = _u64(vk0).reshape(-1)
    if vk.size != AGG_VK_WORDS:
        raise ValueError("aggregate_root: vk0 is 68 words (digest, cap), got %d" % vk.size)
    out = np.zeros(4, np.uint64)
    rc = lib().vpbs_aggregate_root(N, K, n_lwe, _ptr(vk), count, *_aggregate_ptrs(tv, c, o, kh, ko, to), _ptr(out))
    if rc == 1:
        raise VpbsError("vpbs_aggregate_root: a word of the statement is not a field element (at or above p): no proof has this statement")
    if rc:
        raise VpbsError("vpbs_aggregate_root: malformed arguments (count = %d; indices below n_testv = %d and n_keys = %d)" %
                        (count, tv.shape[0], kh.shape[0]))
    return out


def verify_aggregate(shape, blob, count, testvs, cts, out_cts, key_hashes, key_of=None, testv_of=None):
    """vpbs_verify_aggregate (host): ONE proof for `count` bootstraps -> (accepted, reason), reason one of AGG_* in the order of the checks
    (aggregate_reason_text).  shape: an AggregateShape; the statement arrays as aggregate_root; count must be their number of leaves."""
    n, tv, c, o, kh, ko, to = _aggregate_args("verify_aggregate", shape.N, shape.K, shape.n_lwe, testvs, cts, out_cts, key_hashes, key_of, testv_of)
    if n != count:
        raise ValueError("verify_aggregate: count = %d but the statement has %d leaves" % (count, n))
    buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(bytes(blob) or b"\0")
    why, reason = C.create_string_buffer(256), C.c_int(0)
    rc = lib().vpbs_verify_aggregate(C.byref(shape.c), count, *_aggregate_ptrs(tv, c, o, kh, ko, to), buf, len(blob), C.byref(reason), why, 256)
    if rc < 0:
        raise VpbsError("vpbs_verify_aggregate: " + why.value.decode())
    return rc == 1, int(reason.value)


# ---- one proof per program instance: the gates of a program as the leaves of one aggregate (csrc/program.hip) ----
def program_aggregate_args(who, n_inputs, n_gates, n_luts, N, K, n_lwe, inputs, out_cts, testvs=None, key_hash=None, instances=None):
    """shapes of a program statement, checked without a device: inputs [n_inputs][n + 1] and out_cts [n_gates][K][N] -- with a leading
    instance axis when `instances` is not None (True: taken from inputs) -- testvs [n_luts][N] and key_hash [4] where given
    -> (inputs, out_cts, testvs or None, key_hash or None), contiguous uint64"""
    x, o = _u64(inputs), _u64(out_cts)
    lead = () if instances is None else (x.shape[0] if instances is True and x.ndim == 3 else instances,)
    if x.shape != lead + (n_inputs, n_lwe + 1):
        raise ValueError("%s: expected inputs %s, got shape %s" % (who, "".join("[%d]" % d for d in lead + (n_inputs, n_lwe + 1)), x.shape))
    if o.size != int(np.prod(lead + (n_gates, K, N))) or (instances is not None and o.shape[:1] != lead):
        raise ValueError("%s: expected out_cts %s, got shape %s" % (who, "".join("[%d]" % d for d in lead + (n_gates, K, N)), o.shape))
    tv = kh = None
    if testvs is not None:
        tv = _u64(testvs)
        if tv.shape != (n_luts, N):
            raise ValueError("%s: expected testvs [%d][%d], got shape %s" % (who, n_luts, N, tv.shape))
    if key_hash is not None:
        kh = _u64(key_hash).reshape(-1)
        if kh.size != 4:
            raise ValueError("%s: a key hash is 4 words, got %d" % (who, kh.size))
    c = np.ascontiguousarray
    return c(x), c(o.reshape(lead + (n_gates, K * N))), None if tv is None else c(tv), None if kh is None else c(kh)


def program_gate_inputs(prog, N, K, n_lwe, inputs, out_cts):
    """vpbs_program_gate_inputs (host; a host-only Program will do): the gate inputs c_g a verifier recomputes from the program inputs and the
    CLAIMED outputs -- the extraction of every claimed output, the gate's combination, its snap -> [n_gates][n + 1], or
    [instances][n_gates][n + 1] for inputs [instances][n_inputs][n + 1] and out_cts [instances][n_gates][K][N]"""
    batched = _u64(inputs).ndim == 3
    x, o, _, _ = program_aggregate_args("program_gate_inputs", prog.n_inputs, prog.n_gates, prog.n_luts, N, K, n_lwe, inputs, out_cts,
                                        instances=True if batched else None)
    B = x.shape[0] if batched else 1
    out = np.zeros(((B,) if batched else ()) + (prog.n_gates, n_lwe + 1), np.uint64)
    err = C.create_string_buffer(512)
    rc = lib().vpbs_program_gate_inputs(prog.h, N, K, n_lwe, _keep_ptr(x.reshape(-1)), B, _keep_ptr(o.reshape(-1)), _keep_ptr(out.reshape(-1)), err, 512)
    if rc:
        raise VpbsError("status %d: %s" % (rc, err.value.decode()))
    return out


def program_aggregate_root(prog, N, K, n_lwe, vk0, inputs, testvs, out_cts, key_hash):
    """vpbs_program_aggregate_root (host): the root of the aggregate of one program instance -- one leaf per gate, in gate order: leaf g is
    (testvs[gate_lut[g]], c_g of program_gate_inputs, out_cts[g], key_hash) -> [4]; aggregate_root's errors"""
    x, o, tv, kh = program_aggregate_args("program_aggregate_root", prog.n_inputs, prog.n_gates, prog.n_luts, N, K, n_lwe, inputs, out_cts, testvs,
                                          key_hash)
    vk = _u64(vk0).reshape(-1)
    if vk.size != AGG_VK_WORDS:
        raise ValueError("program_aggregate_root: vk0 is 68 words (digest, cap), got %d" % vk.size)
    out, err = np.zeros(4, np.uint64), C.create_string_buffer(512)
    rc = lib().vpbs_program_aggregate_root(prog.h, N, K, n_lwe, _ptr(vk), _keep_ptr(x.reshape(-1)), _keep_ptr(tv.reshape(-1)), _keep_ptr(o.reshape(-1)),
                                           _ptr(kh), _ptr(out), err, 512)
    if rc == 1:
        raise VpbsError("vpbs_program_aggregate_root: a word of the statement is not a field element (at or above p): no proof has this statement")
    if rc:
        raise VpbsError("status %d: %s" % (rc, err.value.decode()))
    return out


def program_verify_aggregate(prog, shape, blob, inputs, testvs, out_cts, key_hash):
    """vpbs_program_verify_aggregate (host): the client's check of ONE proof for its program instance, without a GPU -> (accepted, reason),
    verify_aggregate's reasons in its order.  shape: an AggregateShape; prog may be host-only."""
    x, o, tv, kh = program_aggregate_args("program_verify_aggregate", prog.n_inputs, prog.n_gates, prog.n_luts, shape.N, shape.K, shape.n_lwe, inputs,
                                          out_cts, testvs, key_hash)
    buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(bytes(blob) or b"\0")
    why, reason = C.create_string_buffer(512), C.c_int(0)
    rc = lib().vpbs_program_verify_aggregate(prog.h, C.byref(shape.c), _keep_ptr(x.reshape(-1)), _keep_ptr(tv.reshape(-1)), _keep_ptr(o.reshape(-1)),
                                             _ptr(kh), buf, len(blob), C.byref(reason), why, 512)
    if rc < 0:
        raise VpbsError("status %d: %s" % (rc, why.value.decode()))
    return rc == 1, int(reason.value)


def aggregate_many_args(counts, max_leaves=None, max_aggregates=None, levels=None):
    """the trees of a many-run, checked without a device: counts [n_agg] leaf counts, each 1 .. 2^levels, n_agg <= max_aggregates, their sum
    <= max_leaves (a limit that is None is not checked) -> leaf_first [n_agg + 1] as the C ABI wants it (size_t)"""
    c = np.asarray(counts)
    if c.ndim != 1 or c.size == 0 or c.dtype.kind not in "iu":
        raise ValueError("aggregate_many_args: counts is a non-empty list of integers, one leaf count per aggregate")
    for a, n in enumerate(c.tolist()):
        if n < 1:
            raise ValueError("aggregate_many_args: tree %d is empty" % a)
        if levels is not None and n > 1 << levels:
            raise ValueError("aggregate_many_args: tree %d: %d leaves exceed 2^levels = %d" % (a, n, 1 << levels))
    if max_aggregates is not None and c.size > max_aggregates:
        raise ValueError("aggregate_many_args: %d aggregates exceed max_aggregates %d" % (c.size, max_aggregates))
    if max_leaves is not None and int(c.sum()) > max_leaves:
        raise ValueError("aggregate_many_args: %d leaves exceed max_leaves %d" % (int(c.sum()), max_leaves))
    return np.concatenate([[0], np.cumsum(c)]).astype(np.uint64)


def aggregate_level_jobs(counts, level):
    """vpbs_aggregate_level_jobs (host only): the distinct nodes of `level` over trees of counts[t] leaves, tree by tree -> (tree, left,
    right), np.uint32 [nodes] each; left / right index the list of level - 1 (level 1: the leaves of all trees, concatenated).  The padding
    rule of Aggregator.aggregate and aggregate_many, stated once."""
    aggregate_many_args(counts)
    if int(level) < 1:
        raise ValueError("aggregate_level_jobs: level is at least 1, got %r" % (level,))
    c = np.asarray(counts).astype(np.uint64)
    cp = c.ctypes.data_as(C.POINTER(C.c_size_t))
    n = lib().vpbs_aggregate_level_jobs(cp, c.size, int(level), None, None, None, 0)
    if n < 0:
        raise VpbsError("vpbs_aggregate_level_jobs: status %d" % n)
    tree, left, right = (np.zeros(max(n, 1), np.uint32) for _ in range(3))
    lib().vpbs_aggregate_level_jobs(cp, c.size, int(level), tree.ctypes.data, left.ctypes.data, right.ctypes.data, n)
    return tree[:n], left[:n], right[:n]


class Aggregator(_Handle):
    """vpbs_aggregator: folds serialised vPBS proofs into one proof.  leaf: the cyclic step circuit (a loaded circuit file) with its
    verifier data leaf_vk [68] (digest, cap: PbsProver / RingProver.verifier_data()[0]); level_circuits: A_1 .. A_levels as loaded circuit
    files (circuit_file.find_aggregate_circuits) -- up to 2^levels leaves."""
    _prefix = "vpbs_aggregator"

    def __init__(self, ctx, leaf, leaf_vk, level_circuits):
        self.levels = len(level_circuits)
        self._vk0 = _u64(leaf_vk).reshape(-1).copy()
        if self._vk0.size != AGG_VK_WORDS:
            raise ValueError("Aggregator: leaf_vk is 68 words (digest, cap), got %d" % self._vk0.size)
        v = VerifyInputsC()
        _circuit_shape(v, leaf)
        v.constants_sigmas_cap = C.cast(self._vk0[4:].ctypes.data, U64P)
        for i in range(4):
            v.circuit_digest[i] = int(self._vk0[i])
        self._keep = [leaf, v]
        arr = (IvcCircuitC * self.levels)(*[_ivc_circuit(d, d.meta["proof_words"], self._keep) for d in level_circuits])
        self._construct(ctx, ctx.h, C.byref(v), len(leaf.pi_pos), arr, self.levels, what="")
        top = level_circuits[-1]
        self.max_bytes = 8 * (top.circuit.n_wires * 64 + (1 << 17)) + 8 * len(top.pi_pos)

    def verifier_data(self):
        """-> [levels + 1][68]: vk_0 (the cyclic circuit's) .. vk_levels, what an AggregateShape takes"""
        out = np.zeros((self.levels + 1, AGG_VK_WORDS), np.uint64)
        lib().vpbs_aggregator_verifier_data(self.h, _ptr(out))
        return out

    def aggregate(self, blobs):
        """serialised vPBS proofs (1 .. 2^levels of them) -> the aggregate proof's bytes.  A leaf that does not parse, does not verify or
        carries other verifier data raises VpbsError("... leaf i: ...") before anything is proven (last_run()["nodes"] == 0)."""
        count, data, offs, _, _ = _packed(blobs)
        out, err = np.zeros(self.max_bytes, np.uint8), C.create_string_buffer(512)
        n = lib().vpbs_aggregator_run(self.h, data, offs, count, out.ctypes.data_as(U8P), out.size, None, err, 512)
        if n < 0:
            raise self._fail("", n, err.value.decode())
        return out[:n].tobytes()

    def last_run(self):
        s = AggregateStatsC()
        lib().vpbs_aggregator_last_run(self.h, C.byref(s))
        return {k: getattr(s, k) for k, _ in AggregateStatsC._fields_}

    def set_device_witness(self, max_nodes):
        """vpbs_aggregator_set_device_witness: max_nodes >= 1 -- the node witnesses of a tree level in device batches of at most max_nodes
        (the same bytes as the host path); 0 -- back to the host path, the default.  A level circuit without a device form, or memory that is
        not there, raises VpbsError and leaves the host path on."""
        if int(max_nodes) < 0:
            raise ValueError("Aggregator.set_device_witness: max_nodes is 0 (the host path) or a batch size, got %r" % (max_nodes,))
        err = C.create_string_buffer(512)
        rc = lib().vpbs_aggregator_set_device_witness(self.h, int(max_nodes), err, 512)
        if rc:
            raise VpbsError("status %d: %s" % (rc, err.value.decode()))

    def device_stats(self):
        """vpbs_aggregator_device_stats of the last run: nodes whose witness came from the device, witness batches, device-witness
        microseconds (HIP events around the batches), microseconds of reading public inputs and gathering wires"""
        out = np.zeros(4, np.uint64)
        lib().vpbs_aggregator_device_stats(self.h, _ptr(out))
        return dict(zip(("nodes", "batches", "witness_us", "gather_us"), (int(v) for v in out)))

    def aggregate_many(self, blob_lists, on_aggregate=None):
        """vpbs_aggregator_run_many: one list of serialised vPBS proofs per tree -> the aggregates, in tree order; aggregate t is byte for
        byte aggregate(blob_lists[t]).  All leaves are checked first: a bad one raises VpbsError("... tree t, leaf i: ...") before anything is
        proven.  With the device witness on, the level-l nodes of ALL trees share the device batches.  on_aggregate(t, bytes) as they are made."""
        counts = [len(b) for b in blob_lists]
        aggregate_many_args(counts, levels=self.levels)
        _, data, offs, _, _ = _packed([b for blobs in blob_lists for b in blobs])
        cnt = np.asarray(counts, np.uint64)
        out, raised = [None] * len(counts), []

        def take(_, tree, data, n):
            try:
                out[tree] = C.string_at(data, n)
                if on_aggregate is not None and not raised:
                    on_aggregate(int(tree), out[tree])
            except BaseException as e:   # never through the C frames
                raised.append(e)
        cb = AGGREGATE_TREE_FN(take)
        err = C.create_string_buffer(512)
        n = lib().vpbs_aggregator_run_many(self.h, data, offs, cnt.ctypes.data_as(SZP), len(counts), cb, None, err, 512)
        if raised:
            raise raised[0]
        if n < 0:
            raise self._fail("", n, err.value.decode())
        return out

    def test_preset_matrix(self, level, rows, pairs):
        """vpbs_test_aggregator_preset_matrix (a test entry): rows [n_rows][row_words] child proofs flat | pis, pairs [batch][2] -> the preset
        matrix [n_preset][batch] of that chunk of level-`level` nodes as the device path assembles it"""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        n_preset = 2 * r.shape[1] + AGG_VK_WORDS * level
        out = np.zeros((n_preset, pr.shape[0]), np.uint64)
        rc = lib().vpbs_test_aggregator_preset_matrix(self.h, level, _ptr(r.reshape(-1)), r.shape[0], pr.ctypes.data, pr.shape[0], _ptr(out.reshape(-1)))
        if rc:
            raise VpbsError("vpbs_test_aggregator_preset_matrix: status %d" % rc)
        return out


class AggregateVerifier(_Handle):
    """vpbs_aggregate_verifier: verify_aggregate on the device -- leaf statements, LWE chains and the fold as kernels, the root proof through
    the batch verifier's stages -> the host's verdict and reason.  With on_device=True testvs, cts, out_cts and key_hashes are device pointers
    (ints) and n_testv / n_keys say how many rows the tables have; key_of and testv_of are host arrays in every mode.
    max_aggregates > 1 (vpbs_aggregate_verifier_create_many): verify_many / roots_many take up to that many aggregates -- max_leaves leaves
    in all -- in ONE device run, whose latency-bound chain is as long as that of one aggregate."""
    _prefix = "vpbs_aggregate_verifier"

    def __init__(self, ctx, shape, max_leaves, max_aggregates=1):
        self.shape, self.max_leaves, self.max_aggregates = shape, max_leaves, max_aggregates
        self._construct(ctx, ctx.h, C.byref(shape.c), max_leaves, max_aggregates, entry="create_many", what="")

    def _statement(self, who, count, testvs, cts, out_cts, key_hashes, key_of, testv_of, on_device, n_testv, n_keys):
        """-> (the number of leaves, the statement as every entry point of the verifier takes it)"""
        s = self.shape
        if not on_device:
            n, tv, c, o, kh, ko, to = _aggregate_args(who, s.N, s.K, s.n_lwe, testvs, cts, out_cts, key_hashes, key_of, testv_of)
            if count is not None and n != count:
                raise ValueError("%s: count = %d but the statement has %d leaves" % (who, count, n))
            return n, _aggregate_ptrs(tv, c, o, kh, ko, to) + (0,)
        if count is None or n_testv is None or n_keys is None:
            raise ValueError("%s: device pointers need count, n_testv and n_keys" % who)
        ko, to = (None if a is None else np.ascontiguousarray(np.asarray(a), dtype=np.uint32) for a in (key_of, testv_of))
        for a in (ko, to):
            if a is not None and a.shape != (count,):
                raise ValueError("%s: key_of and testv_of are host arrays of %d entries" % (who, count))
        return count, (int(testvs), n_testv, _keep_u32(to), int(cts), int(out_cts), int(key_hashes), n_keys, _keep_u32(ko), 1)

    def root(self, testvs, cts, out_cts, key_hashes, key_of=None, testv_of=None, on_device=False, count=None, n_testv=None, n_keys=None):
        """aggregate_root computed on the device -> [4]"""
        count, a = self._statement("AggregateVerifier.root", count, testvs, cts, out_cts, key_hashes, key_of, testv_of, on_device, n_testv, n_keys)
        out, err = np.zeros(4, np.uint64), C.create_string_buffer(512)
        rc = lib().vpbs_aggregate_verifier_root(self.h, count, *a, _ptr(out), err, 512)
        if rc == 1:
            raise VpbsError("vpbs_aggregate_verifier_root: a word of the statement is not a field element (at or above p)")
        if rc:
            raise VpbsError("status %d: %s" % (rc, err.value.decode()))
        return out

    def verify(self, blob, count, testvs, cts, out_cts, key_hashes, key_of=None, testv_of=None, on_device=False, n_testv=None, n_keys=None):
        """-> (verdict, reason): verify_aggregate's, for the same arguments"""
        count, a = self._statement("AggregateVerifier.verify", count, testvs, cts, out_cts, key_hashes, key_of, testv_of, on_device, n_testv, n_keys)
        buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(bytes(blob) or b"\0")
        err, reason = C.create_string_buffer(512), C.c_int(0)
        rc = lib().vpbs_aggregate_verifier_run(self.h, buf, len(blob), count, *a, C.byref(reason), err, 512)
        if rc < 0:
            raise VpbsError("status %d: %s" % (rc, err.value.decode()))
        return rc == 1, int(reason.value)

    def _many(self, who, counts, testvs, cts, out_cts, key_hashes, key_of, testv_of, on_device, n_testv, n_keys):
        first = aggregate_many_args(counts, self.max_leaves, self.max_aggregates, min(self.shape.levels, aggregate_depth(self.max_leaves)))
        _, a = self._statement(who, int(first[-1]), testvs, cts, out_cts, key_hashes, key_of, testv_of, on_device, n_testv, n_keys)
        return first.size - 1, first.ctypes.data_as(SZP), a

    def roots_many(self, counts, testvs, cts, out_cts, key_hashes, key_of=None, testv_of=None, on_device=False, n_testv=None, n_keys=None):
        """the statement stages of many trees in one run: tree a owns the next counts[a] leaves of the per-leaf arrays -> (roots
        [n_agg][4], raw_bad uint8 [n_agg]: 1 where a raw word of that tree's statement is at or above p and its root means nothing)"""
        n_agg, first, a = self._many("AggregateVerifier.roots_many", counts, testvs, cts, out_cts, key_hashes, key_of, testv_of, on_device,
                                           n_testv, n_keys)
        out, bad, err = np.zeros((n_agg, 4), np.uint64), np.zeros(n_agg, np.uint8), C.create_string_buffer(512)
        rc = lib().vpbs_aggregate_verifier_roots_many(self.h, n_agg, first, *a, _ptr(out.reshape(-1)), bad.ctypes.data_as(U8P), err, 512)
        if rc:
            raise VpbsError("status %d: %s" % (rc, err.value.decode()))
        return out, bad

    def verify_many(self, blobs, counts, testvs, cts, out_cts, key_hashes, key_of=None, testv_of=None, on_device=False, n_testv=None, n_keys=None):
        """many aggregates in one run: blobs[a] over the next counts[a] leaves -> (verdicts, reasons), np.uint8 [n_agg] each; entry a is
        verify_aggregate's (and verify's) verdict and reason for that blob on its slice of the statement"""
        if len(blobs) != len(counts):
            raise ValueError("AggregateVerifier.verify_many: %d blobs for %d leaf counts" % (len(blobs), len(counts)))
        n_agg, first, a = self._many("AggregateVerifier.verify_many", counts, testvs, cts, out_cts, key_hashes, key_of, testv_of, on_device,
                                           n_testv, n_keys)
        _, data, offs, results, ptrs = _packed(blobs, outputs=2)
        err = C.create_string_buffer(512)
        rc = lib().vpbs_aggregate_verifier_run_many(self.h, data, offs, n_agg, first, *a, *ptrs, err, 512)
        if rc < 0:
            raise VpbsError("status %d: %s" % (rc, err.value.decode()))
        return results


class Program(_Handle):
    """vpbs_program: a netlist of bootstraps on resident keys.  Wire w < n_inputs is input w, wire n_inputs + g the output of gate g; gate g
    bootstraps const * (0, .., 0, 1) + sum coef * wire[src] with test vector testvs[lut].  gates: a list of (terms=[(src, coef), ..], const, lut)
    in topological order, or the CSR arrays as a dict {gate_first, term_src, term_coef, gate_const, gate_lut}.  ctx=None gives a host-only
    object (validated and levelised: levels()); an invalid description raises VpbsError with a message that names the gate.
    Multi-output gates: a gate may be a 5-tuple (terms, const, lut, log_slots, outputs) -- its input is snapped with log_slots (lwe_snap), it
    has `outputs` <= 2^log_slots output wires (the extractions of coefficients 0 .. outputs - 1 of its output GLWE, lwe_extract_at) and
    testvs[lut] is a packed test vector (lut_testv_multi); a 3-tuple is (.., 0, 1).  The CSR dict takes gate_log_slots and gate_outputs.
    Output j of gate g is wire n_inputs + out_first[g] + j (wires()); every per-gate result stays per gate: one proof for all its outputs."""
    _prefix = "vpbs_program"

    def __init__(self, ctx, n_inputs, gates, n_luts):
        if isinstance(gates, dict):
            first = np.ascontiguousarray(gates["gate_first"], dtype=np.uint64).reshape(-1)
            src = np.ascontiguousarray(gates["term_src"], dtype=np.uint32).reshape(-1)
            coef, const = _u64(gates["term_coef"]).reshape(-1), _u64(gates["gate_const"]).reshape(-1)
            lut = np.ascontiguousarray(gates["gate_lut"], dtype=np.uint32).reshape(-1)
            multi = "gate_log_slots" in gates or "gate_outputs" in gates
            slots = np.ascontiguousarray(gates.get("gate_log_slots", np.zeros(lut.size)), dtype=np.uint32).reshape(-1)
            outs = np.ascontiguousarray(gates.get("gate_outputs", np.ones(lut.size)), dtype=np.uint32).reshape(-1)
        else:
            gates = [tuple(g) for g in gates]
            first = np.cumsum([0] + [len(g[0]) for g in gates]).astype(np.uint64)
            src = np.array([t[0] for g in gates for t in g[0]], np.uint32)
            coef = np.array([int(t[1]) for g in gates for t in g[0]], np.uint64)
            const, lut = np.array([int(g[1]) for g in gates], np.uint64), np.array([g[2] for g in gates], np.uint32)
            if any(len(g) not in (3, 5) for g in gates):
                raise ValueError("Program: a gate is (terms, const, lut) or (terms, const, lut, log_slots, outputs)")
            multi = any(len(g) == 5 for g in gates)
            slots = np.array([g[3] if len(g) == 5 else 0 for g in gates], np.uint32)
            outs = np.array([g[4] if len(g) == 5 else 1 for g in gates], np.uint32)
        if src.size != coef.size or const.size != lut.size or first.size != const.size + 1 or slots.size != lut.size or outs.size != lut.size:
            raise ValueError("Program: expected gate_first [n_gates + 1], term_src / term_coef [n_terms], gate_const / gate_lut "
                             "(/ gate_log_slots / gate_outputs) [n_gates]")
        self.n_inputs, self.n_gates, self.n_luts = n_inputs, int(const.size), n_luts
        self.gate_log_slots, self.gate_outputs = slots, outs
        self.n_wires = n_inputs + self.n_gates   # until the object says otherwise
        self.gate_first, self.term_src, self.term_coef, self.gate_const, self.gate_lut = first, src, coef, const, lut
        d = ProgramDescC(n_inputs, self.n_gates, n_luts, src.size, _ptr(first), src.ctypes.data_as(C.POINTER(C.c_uint32)), _ptr(coef), _ptr(const),
                         lut.ctypes.data_as(C.POINTER(C.c_uint32)))
        if multi:
            self._construct(ctx, ctx.h if ctx is not None else None, C.byref(d), _keep_u32(slots), _keep_u32(outs), entry="create_multi")
        else:
            self._construct(ctx, ctx.h if ctx is not None else None, C.byref(d))
        self.n_wires = self.wires()[1]

    def levels(self):
        """-> (level of every gate in the caller's order, np.uint32 [n_gates]; number of levels)"""
        out = np.zeros(max(self.n_gates, 1), np.uint32)
        n = lib().vpbs_program_levels(self.h, out.ctypes.data_as(C.POINTER(C.c_uint)))
        if n < 0:
            raise VpbsError("vpbs_program_levels: status %d" % n)
        return out[:self.n_gates], int(n)

    def wires(self):
        """-> (out_first np.uint32 [n_gates + 1]: output j of gate g is wire n_inputs + out_first[g] + j; the number of wires)"""
        out = np.zeros(self.n_gates + 1, np.uint32)
        n = lib().vpbs_program_wires(self.h, out.ctypes.data_as(C.POINTER(C.c_uint)))
        if n < 0:
            raise VpbsError("vpbs_program_wires: status %d" % n)
        return out, int(n)

    def _host_args(self, who, n_lwe, N, inputs, testvs):
        x, tv = _u64(inputs).reshape(-1, n_lwe + 1), _u64(testvs).reshape(-1, N)
        if x.shape[0] != self.n_inputs or tv.shape[0] != self.n_luts:
            raise ValueError("Program.%s: expected inputs [%d][%d] and testvs [%d][%d]" % (who, self.n_inputs, n_lwe + 1, self.n_luts, N))
        return x, tv

    def run(self, bootstrapper, inputs, testvs, gate_cts=True, out_cts=True):
        """inputs [n_inputs][n + 1], testvs [n_luts][N] -> (wires [n_inputs + n_gates][n + 1], gate_cts [n_gates][n + 1], out_cts
        [n_gates][K][N]), all in the caller's gate order; the number of levels is levels()[1].  gate_cts=False / out_cts=False: that
        output is not downloaded (None in its place)."""
        b = bootstrapper
        x, tv = self._host_args("run", b.n_lwe, b.N, inputs, testvs)
        wires = np.zeros((self.n_wires, b.n_lwe + 1), np.uint64)
        cts = np.zeros((self.n_gates, b.n_lwe + 1), np.uint64) if gate_cts else None
        out = np.zeros((self.n_gates, b.K, b.N), np.uint64) if out_cts else None
        p = _keep_ptr
        rc = lib().vpbs_program_run(self.h, b.h, p(x), p(tv), p(wires), p(cts), p(out), 0)
        if rc < 0:
            raise VpbsError("vpbs_program_run: status %d: %s" % (rc, lib().vpbs_last_error(b.ctx.h).decode()))
        return wires, cts, out

    def margins(self, ctx, s_lwe, gate_cts, p_of_lut, expected=None, *, N, n_lwe=None, stats=None):
        """lwe_rotation_batch over the gate inputs of a run: gate_cts [n_gates][n + 1] as run() returns them (a host array, or a device
        pointer as run_device() fills it), p_of_lut [n_luts] the p of every test vector, expected [n_gates] table positions or None ->
        (mu, idx, dev, stats_per_level): three arrays [n_gates] in the caller's gate order (dev int64) and one NoiseStats per level of
        levels().  The rows are already snapped, so every call passes log_slots 0; one call per level and p over host rows, per run of
        consecutive gates of one level and p over a device pointer.  ctx None: on the host (host arrays only).  N: the ring size of the
        bootstraps, which the program itself does not know; n_lwe: for a key on the device; stats: the list of an earlier call, added to
        (a survey over many instances)."""
        p_of_lut = [int(v) for v in p_of_lut]
        if len(p_of_lut) != self.n_luts:
            raise ValueError("Program.margins: p_of_lut must have n_luts = %d entries" % self.n_luts)
        level, n_levels = self.levels()
        dev_rows = _is_dev(gate_cts)
        n = int(n_lwe) if _is_dev(s_lwe) else _u64(s_lwe).size
        rows = None if dev_rows else _u64(gate_cts).reshape(self.n_gates, n + 1)
        exp = None if expected is None else _u64(expected).reshape(-1)
        if exp is not None and exp.size != self.n_gates:
            raise ValueError("Program.margins: expected must have n_gates = %d entries" % self.n_gates)
        p_of_gate = np.array([p_of_lut[l] for l in self.gate_lut], np.int64)
        out = {w: np.zeros(self.n_gates, np.uint64) for w in ROTATION_OUTPUTS}
        stats = [NoiseStats() for _ in range(n_levels)] if stats is None else stats
        if len(stats) != n_levels:
            raise ValueError("Program.margins: stats must hold one NoiseStats per level, %d" % n_levels)
        for lv in range(1, n_levels + 1):
            for p in sorted(set(p_of_gate[level == lv].tolist())):
                pick = np.nonzero((level == lv) & (p_of_gate == p))[0]
                # a device pointer: runs of consecutive gates; host rows: the whole group, gathered
                groups = np.split(pick, np.nonzero(np.diff(pick) != 1)[0] + 1) if dev_rows else [pick]
                for g in groups:
                    cts = int(gate_cts) + 8 * (n + 1) * int(g[0]) if dev_rows else rows[g]
                    got = _lwe_rotation_batch(ctx, s_lwe, cts, N, p, 0, None if exp is None else exp[g], g.size if dev_rows else None,
                                              stats[lv - 1], ROTATION_OUTPUTS, n)
                    for w in ROTATION_OUTPUTS:
                        out[w][g] = got[w].view(np.uint64)
        return out["rot"], out["idx"], out["dev"].view(np.int64), stats

    def run_device(self, bootstrapper, d_inputs, d_testvs, d_wires=None, d_gate_cts=None, d_out_cts=None):
        """the same on device pointers (integers; None = output not wanted); returns the number of levels when the outputs are in place"""
        rc = lib().vpbs_program_run(self.h, bootstrapper.h, _dev(d_inputs), _dev(d_testvs), _dev(d_wires), _dev(d_gate_cts), _dev(d_out_cts), 1)
        if rc < 0:
            raise VpbsError("vpbs_program_run: status %d: %s" % (rc, lib().vpbs_last_error(bootstrapper.ctx.h).decode()))
        return rc

    def _batch_fail(self, ring, rc):
        return self._fail("vpbs_program_run_batch", rc, lib().vpbs_last_error(ring.ctx.h).decode())

    def run_batch(self, ring, inputs, key_of, testvs, gate_cts=True, out_cts=True):
        """ONE program for many input sets on a KeyRing: inputs [instances][n_inputs][n + 1], key_of [instances] slots, testvs [n_luts][N]
        shared -> (wires [instances][n_inputs + n_gates][n + 1], gate_cts [instances][n_gates][n + 1], out_cts [instances][n_gates][K][N]);
        slice b is run(Bootstrapper of the key set in slot key_of[b], inputs[b], testvs), word for word.  Level l of all instances goes
        into launches of the ring's max_batch rows.  gate_cts=False / out_cts=False: that output is not downloaded (None in its place)."""
        if self.ctx is None:
            raise VpbsError("Program.run_batch: a host-only program (made without a context) cannot be evaluated")
        if ring is None or not ring.h:
            raise VpbsError("Program.run_batch: no ring (None, or a closed KeyRing)")
        r = ring
        x, ko, tv = program_batch_args(self.n_inputs, r.n_lwe, r.N, self.n_luts, r.max_keys, inputs, key_of, testvs)
        count = x.shape[0]
        wires = np.zeros((count, self.n_wires, r.n_lwe + 1), np.uint64)
        cts = np.zeros((count, self.n_gates, r.n_lwe + 1), np.uint64) if gate_cts else None
        out = np.zeros((count, self.n_gates, r.K, r.N), np.uint64) if out_cts else None
        p = _keep_ptr
        rc = lib().vpbs_program_run_batch(self.h, r.h, p(x), count, _keep_u32(ko), p(tv), p(wires), p(cts), p(out), 0)
        if rc < 0:
            raise self._batch_fail(r, rc)
        return wires, cts, out

    def run_batch_device(self, ring, d_inputs, instances, key_of, d_testvs, d_wires=None, d_gate_cts=None, d_out_cts=None):
        """the same on device pointers (integers; None = output not wanted); key_of stays a host array; returns the number of levels when
        the outputs are in place"""
        if self.ctx is None:
            raise VpbsError("Program.run_batch_device: a host-only program (made without a context) cannot be evaluated")
        if ring is None or not ring.h:
            raise VpbsError("Program.run_batch_device: no ring (None, or a closed KeyRing)")
        ko = keyring_key_of(key_of, instances, ring.max_keys)
        rc = lib().vpbs_program_run_batch(self.h, ring.h, _dev(d_inputs), instances, _keep_u32(ko), _dev(d_testvs), _dev(d_wires), _dev(d_gate_cts),
                                          _dev(d_out_cts), 1)
        if rc < 0:
            raise self._batch_fail(ring, rc)
        return rc

    @staticmethod
    def _gate_proof_fn(on_proof, raised, proofs=None, failures=None, index=int):
        """the PBS_PROOF_FN of a proving call: proof i into proofs[i] and a failing row into failures (where kept), on_proof(index(i), bytes)
        until a callback raises -- the exception goes into `raised`, never through the C frames"""
        def trampoline(_user, i, data, n, error):
            try:
                if not data:
                    if failures is not None:
                        failures.append((int(i), (error or b"").decode()))
                    return
                if proofs is None and on_proof is None:
                    return
                blob = C.string_at(data, n)
                if proofs is not None:
                    proofs[i] = blob
                if on_proof is not None and not raised:
                    on_proof(index(int(i)), blob)
            except BaseException as e:   # noqa: BLE001 -- must not unwind through the C frames
                raised.append(e)
        return PBS_PROOF_FN(trampoline)

    @staticmethod
    def _proving_done(name, prover, n, err, raised, failed=None):
        """after a proving call: the callback's exception, the checkpoint callback's, a negative status (VpbsError with .status), failing
        rows (failed = (failures, proofs, out_cts, wires) -> PbsProveError)"""
        if raised:
            raise raised[0]
        e, prover._ckpt_error = prover._ckpt_error, None
        if e is not None:
            raise e
        if n < 0:
            raise _Handle._fail(name, n, err.value.decode())
        if failed is not None and failed[0]:
            raise PbsProveError(dict(failed[0]), *failed[1:])

    def prove(self, pbs_prover, inputs, testvs, steps=0, on_proof=None):
        """-> (proofs: list of bytes in the caller's gate order, wires, out_cts).  Proof g is PbsProver.prove(gate_cts[g], testvs[lut_g])[0];
        on_proof(gate, bytes), failures (PbsProveError, with .out_ct = out_cts and .lwe_out = wires) and `steps` as in PbsProver.prove."""
        pp = pbs_prover
        x, tv = self._host_args("prove", pp.n_lwe, pp.N, inputs, testvs)
        wires, out = np.zeros((self.n_wires, pp.n_lwe + 1), np.uint64), np.zeros((self.n_gates, pp.K, pp.N), np.uint64)
        proofs, failures, raised = [None] * self.n_gates, [], []
        cb, err, p = self._gate_proof_fn(on_proof, raised, proofs, failures), C.create_string_buffer(512), _keep_ptr
        n = lib().vpbs_program_prove(self.h, pp.h, p(x), p(tv), steps, p(wires), p(out), cb, None, err, 512)
        self._proving_done("vpbs_program_prove", pp, n, err, raised, (failures, proofs, out, wires))
        return proofs, wires, out

    def prove_batch(self, ring_prover, inputs, key_of, testvs, steps=0, on_proof=None):
        """ONE program for many input sets, evaluated AND proven on a RingProver: inputs [instances][n_inputs][n + 1], key_of [instances]
        slots, testvs [n_luts][N] -> (proofs[b][g]: bytes, wires [instances][n_inputs + n_gates][n + 1], out_cts
        [instances][n_gates][K][N]).  wires and out_cts are run_batch's on the prover's ring; proof (b, g) is byte for byte
        prove(PbsProver of the key set in slot key_of[b], inputs[b], testvs)[0][g].  on_proof((b, g), bytes); failures: PbsProveError with
        .failures keyed by b * n_gates + g.  verify_batch() checks all instances on one RingVerifier filled from key_hash(slot); a client
        verifies its own instance with verify() and a PbsVerifier made from key_hash(slot)."""
        if self.ctx is None:
            raise VpbsError("Program.prove_batch: a host-only program (made without a context) cannot be evaluated")
        rp = ring_prover
        if rp is None or not rp.h:
            raise VpbsError("Program.prove_batch: no ring prover (None, or a closed RingProver)")
        x, ko, tv = program_batch_args(self.n_inputs, rp.n_lwe, rp.N, self.n_luts, rp.max_keys, inputs, key_of, testvs)
        B, G = x.shape[0], self.n_gates
        wires, out = np.zeros((B, self.n_wires, rp.n_lwe + 1), np.uint64), np.zeros((B, G, rp.K, rp.N), np.uint64)
        flat, failures, raised = [None] * (B * G), [], []
        cb = self._gate_proof_fn(on_proof, raised, flat, failures, index=lambda i: divmod(i, G))
        err, p = C.create_string_buffer(512), _keep_ptr
        n = lib().vpbs_program_prove_batch(self.h, rp.h, p(x), B, _keep_u32(ko), p(tv), steps, p(wires), p(out), cb, None, err, 512)
        self._proving_done("vpbs_program_prove_batch", rp, n, err, raised, (failures, flat, out, wires))
        return [flat[b * G:(b + 1) * G] for b in range(B)], wires, out

    def verify(self, pbs_verifier, inputs, testvs, out_cts, proofs):
        """out_cts [n_gates][K][N]: the claimed output GLWEs; proofs: list of bytes in gate order -> (verdicts, reasons, proof_reasons),
        np.uint8 [n_gates] each.  The program is proven iff every verdict is 1."""
        v = pbs_verifier
        x, tv = self._host_args("verify", v.n_lwe, v.N, inputs, testvs)
        o = _u64(out_cts).reshape(-1)
        if o.size != self.n_gates * v.K * v.N or len(proofs) != self.n_gates:
            raise ValueError("Program.verify: expected out_cts [%d][K][N] and %d proofs" % (self.n_gates, self.n_gates))
        _, data, offs, results, ptrs = _packed(proofs, shape=self.n_gates, outputs=3)
        p = _keep_ptr
        rc = lib().vpbs_program_verify(self.h, v.h, p(x), p(tv), p(o), data, offs, *ptrs)
        if rc < 0:
            raise VpbsError("vpbs_program_verify: status %d: %s" % (rc, lib().vpbs_last_error(v.ctx.h).decode()))
        return results

    def verify_batch(self, ring_verifier, inputs, key_of, testvs, out_cts, proofs):
        """verify for many instances on ONE RingVerifier: inputs [instances][n_inputs][n + 1], key_of [instances] slots, testvs [n_luts][N],
        out_cts [instances][n_gates][K][N] (claimed), proofs[b][g] as prove_batch returns them -> (verdicts, reasons, proof_reasons), np.uint8
        [instances][n_gates] each; row (b, g) is verify(PbsVerifier of slot key_of[b]'s key hash, inputs[b], testvs, out_cts[b], proofs[b])[.][g].
        The rows reach the verifier in chunks of its max_batch that may straddle instances."""
        if self.ctx is None:
            raise VpbsError("Program.verify_batch: a host-only program (made without a context) cannot be verified")
        rv = ring_verifier
        if rv is None or not rv.h:
            raise VpbsError("Program.verify_batch: no ring verifier (None, or a closed RingVerifier)")
        x, ko, tv = program_batch_args(self.n_inputs, rv.n_lwe, rv.N, self.n_luts, rv.max_keys, inputs, key_of, testvs)
        B, G = x.shape[0], self.n_gates
        o = _u64(out_cts).reshape(-1)
        if o.size != B * G * rv.K * rv.N or len(proofs) != B or any(len(row) != G for row in proofs):
            raise ValueError("Program.verify_batch: expected out_cts [%d][%d][K][N] and proofs [%d][%d]" % (B, G, B, G))
        _, data, offs, results, ptrs = _packed([blob for row in proofs for blob in row], shape=(B, G), outputs=3)
        err, p = C.create_string_buffer(512), _keep_ptr
        rc = lib().vpbs_program_verify_batch(self.h, rv.h, p(x), B, _keep_u32(ko), p(tv), p(o), data, offs, *ptrs, err, 512)
        if rc < 0:
            raise self._fail("vpbs_program_verify_batch", rc, err.value.decode())
        return results

    def prove_aggregate(self, pbs_prover, aggregator, inputs, testvs, on_proof=None):
        """ONE proof for the program instance: prove(), then Aggregator.aggregate over the gate proofs in gate order -> (blob, wires,
        out_cts); the bytes are that composition's.  on_proof(gate, bytes) still sees every gate proof.  A program of more than
        2^levels gates (or none) is refused before anything is proven: VpbsError, on_proof never called."""
        pp = pbs_prover
        x, tv = self._host_args("prove_aggregate", pp.n_lwe, pp.N, inputs, testvs)
        wires, out = np.zeros((self.n_wires, pp.n_lwe + 1), np.uint64), np.zeros((self.n_gates, pp.K, pp.N), np.uint64)
        raised = []
        cb, err, p = self._gate_proof_fn(on_proof, raised), C.create_string_buffer(512), _keep_ptr
        blob = np.zeros(aggregator.max_bytes, np.uint8)
        n = lib().vpbs_program_prove_aggregate(self.h, pp.h, aggregator.h, p(x), p(tv), p(wires), p(out), blob.ctypes.data_as(U8P),
                                               blob.size, None, cb, None, err, 512)
        self._proving_done("vpbs_program_prove_aggregate", pp, n, err, raised)
        return blob[:n].tobytes(), wires, out

    def prove_aggregate_batch(self, ring_prover, aggregator, inputs, key_of, testvs, on_aggregate=None):
        """one aggregate PER INSTANCE on a RingProver: prove_batch(), then instance by instance Aggregator.aggregate over its gate proofs
        -> (blobs [instances], wires, out_cts); blobs[b] is byte for byte prove_aggregate on a PbsProver of the key set in slot
        key_of[b], and a client verifies its own with program_verify_aggregate.  on_aggregate(b, bytes) as they are made.  With the
        aggregator's device witness on (Aggregator.set_device_witness) all instances are ONE run of the aggregator (aggregate_many's)."""
        if self.ctx is None:
            raise VpbsError("Program.prove_aggregate_batch: a host-only program (made without a context) cannot be evaluated")
        rp = ring_prover
        if rp is None or not rp.h:
            raise VpbsError("Program.prove_aggregate_batch: no ring prover (None, or a closed RingProver)")
        x, ko, tv = program_batch_args(self.n_inputs, rp.n_lwe, rp.N, self.n_luts, rp.max_keys, inputs, key_of, testvs)
        B, G = x.shape[0], self.n_gates
        wires, out = np.zeros((B, self.n_wires, rp.n_lwe + 1), np.uint64), np.zeros((B, G, rp.K, rp.N), np.uint64)
        blobs, raised = [None] * B, []

        def trampoline(instance, data, n, _user):
            try:
                blobs[instance] = C.string_at(data, n)
                if on_aggregate is not None and not raised:
                    on_aggregate(int(instance), blobs[instance])
            except BaseException as e:   # noqa: BLE001 -- must not unwind through the C frames
                raised.append(e)
        cb, none, err, p = AGGREGATE_FN(trampoline), PBS_PROOF_FN(), C.create_string_buffer(512), _keep_ptr
        n = lib().vpbs_program_prove_aggregate_batch(self.h, rp.h, aggregator.h, p(x), B, _keep_u32(ko), p(tv), p(wires), p(out), cb, none, None, err, 512)
        self._proving_done("vpbs_program_prove_aggregate_batch", rp, n, err, raised)
        return blobs, wires, out

    def verify_aggregate_batch(self, agg_verifier, inputs, key_of, key_hashes, testvs, out_cts, blobs):
        """the aggregates of many instances on ONE AggregateVerifier (made with max_aggregates > 1 to take several per run): inputs
        [instances][n_inputs][n + 1], key_of [instances] indices into key_hashes [n_keys][4], testvs [n_luts][N], out_cts
        [instances][n_gates][K][N] (claimed), blobs [instances] -> (verdicts, reasons), np.uint8 [instances]; entry b is
        program_verify_aggregate(blobs[b], inputs[b], testvs, out_cts[b], key_hashes[key_of[b]]).  The gate inputs are recomputed on the
        device and stay there."""
        if self.ctx is None:
            raise VpbsError("Program.verify_aggregate_batch: a host-only program (made without a context) cannot be verified on the device")
        av = agg_verifier
        if av is None or not av.h:
            raise VpbsError("Program.verify_aggregate_batch: no aggregate verifier (None, or a closed AggregateVerifier)")
        s = av.shape
        kh = _u64(key_hashes)
        kh = np.ascontiguousarray(kh.reshape(1, -1) if kh.ndim == 1 else kh)
        if kh.ndim != 2 or kh.shape[1] != 4:
            raise ValueError("Program.verify_aggregate_batch: expected key_hashes [n_keys][4], got shape %s" % (kh.shape,))
        x, ko, tv = program_batch_args(self.n_inputs, s.n_lwe, s.N, self.n_luts, kh.shape[0], inputs, key_of, testvs)
        B = x.shape[0]
        _, o, _, _ = program_aggregate_args("Program.verify_aggregate_batch", self.n_inputs, self.n_gates, self.n_luts, s.N, s.K, s.n_lwe, x, out_cts,
                                            instances=B)
        if len(blobs) != B:
            raise ValueError("Program.verify_aggregate_batch: %d blobs for %d instances" % (len(blobs), B))
        _, data, offs, results, ptrs = _packed(blobs, shape=B, outputs=2)
        err, p = C.create_string_buffer(512), _keep_ptr
        rc = lib().vpbs_program_verify_aggregate_batch(self.h, av.h, p(x), B, _keep_u32(ko), p(kh), kh.shape[0], p(tv), p(o), data, offs, *ptrs, err, 512)
        if rc < 0:
            raise self._fail("vpbs_program_verify_aggregate_batch", rc, err.value.decode())
        return results


ERR_INVALID = -1   # VPBS_ERR_INVALID


def set_arity_bits(p, arity_bits):
    """the reduction rounds of a FriParams from a list: n_rounds = its length, the rest of arity_bits[16] zero.  A list the array cannot hold
    keeps its length in n_rounds (the library refuses it) and its first 16 entries."""
    bits = [int(a) for a in arity_bits]
    p.n_rounds = len(bits)
    for i in range(len(p.arity_bits)):
        p.arity_bits[i] = bits[i] if i < len(bits) else 0
    return p


def standard_arity_bits(degree_bits, rate_bits=3, cap_height=4):
    """FriReductionStrategy::ConstantArityBits(4, 5) under a FriConfig of this rate and cap height (FriParams::standard of the library)"""
    bits, d = [], degree_bits
    while d > 5 and d + rate_bits >= cap_height + 4:
        bits.append(4)
        d -= 4
    return bits


def fri_params(degree_bits, **over):
    """vpbs_fri_params_standard with the given fields changed; arity_bits=[...] (a list) sets the reduction rounds"""
    p = FriParams()
    lib().vpbs_fri_params_standard(degree_bits, C.byref(p))
    for k, v in over.items():
        if k == "arity_bits":
            set_arity_bits(p, v)
        else:
            setattr(p, k, v)
    return p


def ntt_params(log_n):
    n = 1 << log_n
    roots, inv, ninv = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(1, np.uint64)
    rc = lib().vpbs_ntt_params(log_n, _ptr(roots), _ptr(inv), _ptr(ninv))
    if rc:
        raise VpbsError("vpbs_ntt_params failed: %d" % rc)
    return roots, inv, int(ninv[0])


class Batch(_Handle):
    """Device-resident PolynomialBatch handle (fri/oracle.rs).  A batch must not outlive its context (Context.close() frees the
    survivors); one that did is only forgotten: vpbs_batch_free reaches into the context."""
    _prefix = "vpbs_batch"
    _owns = property(lambda self: bool(self.ctx.h))

    def __init__(self, ctx, handle):
        self.h = handle
        self.ncols = lib().vpbs_batch_ncols(handle)
        self.log_n = lib().vpbs_batch_log_n(handle)
        self.n = 1 << self.log_n
        self._created(ctx)

    def cap(self):
        out = np.zeros((1 << self.ctx.cap_height, 4), np.uint64)
        self.ctx._check(lib().vpbs_batch_cap(self.h, _ptr(out)))
        return out

    def coeffs(self):
        out = np.zeros((self.ncols, self.n), np.uint64)
        self.ctx._check(lib().vpbs_batch_coeffs(self.h, _ptr(out)))
        return out

    def lde_rows(self, row_start, nrows, step=1):
        out = np.zeros((nrows, self.ncols), np.uint64)
        self.ctx._check(lib().vpbs_batch_lde_rows(self.h, row_start, nrows, step, _ptr(out)))
        return out

    def eval_ext(self, zeta):
        z = _u64(zeta)
        out = np.zeros((self.ncols, 2), np.uint64)
        self.ctx._check(lib().vpbs_batch_eval_ext(self.h, _ptr(z), _ptr(out)))
        return out

    def open(self, leaf_index):
        """(leaf, siblings) for a GLOBAL leaf index (must lie in this batch's shard when it is sharded)."""
        nsib = self.log_n + self.ctx.rate_bits - self.ctx.cap_height
        leaf, sib = np.zeros(self.ncols, np.uint64), np.zeros((nsib, 4), np.uint64)
        self.ctx._check(lib().vpbs_batch_open(self.h, leaf_index, _ptr(leaf), _ptr(sib)))
        return leaf, sib


class Context:
    """One device + one HIP stream (vpbs_ctx).  Not re-entrant: one Context per host thread."""

    def __init__(self, device=0, log_n_max=16, rate_bits=3, cap_height=4):
        self.h = C.c_void_p()
        self.rate_bits, self.cap_height = rate_bits, cap_height
        self._batches = weakref.WeakSet()
        rc = lib().vpbs_ctx_create(device, log_n_max, rate_bits, cap_height, C.byref(self.h))
        if rc:
            self.h = None
            raise VpbsError("vpbs_ctx_create(device=%d) failed with status %d (no MI355X visible?)" % (device, rc))

    def close(self):
        if self.h:
            for b in list(self._batches):   # every _Handle made on this context that is still open
                b.close()
            lib().vpbs_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise _Handle._fail("", rc, lib().vpbs_last_error(self.h).decode())

    def synchronize(self):
        self._check(lib().vpbs_ctx_synchronize(self.h))

    def set_gate_lanes(self, lanes):
        """1 (default): the gate-constraint stage on the context's stream (right for the LDS-tile gate kernel); 3: three streams (the
        per-gate launches of VPBS_OPT_GATES_FUSED = 0)"""
        self._check(lib().vpbs_ctx_set_gate_lanes(self.h, lanes))

    OPTIONS = {"gate_lanes": 0, "gates_fused": 1, "gate_items": 2, "wide_threshold": 3, "merkle_climb": 4, "gates_tile": 5}

    def set_option(self, name, value):
        """vpbs_ctx_set_option: a launch heuristic of this context (never changes a result); names: Context.OPTIONS"""
        if lib().vpbs_ctx_set_option(self.h, self.OPTIONS[name], int(value)):
            raise VpbsError("vpbs_ctx_set_option(%s, %r): not a valid value" % (name, value))

    def get_option(self, name):
        v = C.c_uint64()
        self._check(lib().vpbs_ctx_get_option(self.h, self.OPTIONS[name], C.byref(v)))
        return int(v.value)

    def set_compat(self, k=None, **over):
        """the context proves and serialises under this switch table (vpbs_ctx_set_compat); set_compat() restores the defaults"""
        k = k if k is not None else compat(**over)
        if lib().vpbs_ctx_set_compat(self.h, C.byref(k)):
            raise VpbsError("vpbs_ctx_set_compat: a position this build does not implement: %r" % (compat_dict(k),))
        return k

    def get_compat(self):
        k = CompatC()
        self._check(lib().vpbs_ctx_get_compat(self.h, C.byref(k)))
        return k

    @property
    def stream(self):
        return lib().vpbs_ctx_stream(self.h)

    # ---- commits ----
    def _commit(self, fn, data, ncols=None, log_n=None, want_cap=True):
        out = C.c_void_p()
        cap = np.zeros((1 << self.cap_height, 4), np.uint64) if want_cap else None
        cap_p = _ptr(cap) if want_cap else None
        if isinstance(data, np.ndarray):
            data = _u64(data)
            ncols, n = data.shape
            log_n = n.bit_length() - 1
            assert 1 << log_n == n
            self._check(fn(self.h, _ptr(data), ncols, log_n, C.byref(out), cap_p))
        else:  # device pointer (int)
            self._check(fn(self.h, C.c_void_p(int(data)), ncols, log_n, C.byref(out), cap_p))
        b = Batch(self, out)
        b.cap_at_commit = cap
        return b

    def commit_values(self, values):
        return self._commit(lib().vpbs_commit_values, values)

    def commit_coeffs(self, coeffs):
        return self._commit(lib().vpbs_commit_coeffs, coeffs)

    def commit_values_dev(self, dptr, ncols, log_n, want_cap=True):
        return self._commit(lib().vpbs_commit_values_dev, dptr, ncols, log_n, want_cap)

    def commit_coeffs_dev(self, dptr, ncols, log_n, want_cap=True):
        return self._commit(lib().vpbs_commit_coeffs_dev, dptr, ncols, log_n, want_cap)

    def commit_sharded_dev(self, dptr, ncols, log_n, shard, n_shards, is_values=True):
        """One rank's share of a coset-sharded commitment (device pointer in).  Returns (batch, local cap entries)."""
        out = C.c_void_p()
        cap = np.zeros(((1 << self.cap_height) // n_shards, 4), np.uint64)
        self._check(lib().vpbs_commit_sharded_dev(self.h, C.c_void_p(int(dptr)), 1 if is_values else 0, ncols, log_n, shard, n_shards,
                                                  C.byref(out), _ptr(cap)))
        b = Batch(self, out)
        b.shard, b.n_shards = shard, n_shards
        return b, cap

    # ---- FRI ----
    def fri_prove(self, oracles, batches, challenger, params, forced_pow=POW_ANY, proof_out=None):
        """batches: [(point(2), [(oracle_index, poly_index), ...]), ...] -> flat FriProof words.
        proof_out: the caller's own buffer (contiguous uint64, at least vpbs_fri_proof_words long) instead of a new one; vpbs_fri_prove is
        then called with it whatever the parameters are."""
        degree_bits = oracles[0].log_n
        ncols = (C.c_size_t * len(oracles))(*[o.ncols for o in oracles])
        if proof_out is None:
            words = lib().vpbs_fri_proof_words(C.byref(params), degree_bits, ncols, len(oracles))
            if words == 0:   # parameters the library refuses as a whole: nothing to size a proof by
                raise _Handle._fail("", ERR_INVALID, "vpbs_fri_proof_words refuses these FRI parameters at degree 2^%d (rounds, arities, cap "
                                    "height, query rounds or tree count)" % degree_bits)
            proof = np.zeros(words, np.uint64)
        else:
            proof = proof_out
        handles = (C.c_void_p * len(oracles))(*[o.h for o in oracles])
        infos = (FriBatchInfoC * len(batches))()
        keep = []
        for i, (point, polys) in enumerate(batches):
            oi = np.array([p[0] for p in polys], np.uint32)
            pi = np.array([p[1] for p in polys], np.uint32)
            keep += [oi, pi]
            infos[i].point[0], infos[i].point[1] = int(point[0]), int(point[1])
            infos[i].n_polys = len(polys)
            infos[i].oracle_index = oi.ctypes.data_as(U32P)
            infos[i].poly_index = pi.ctypes.data_as(U32P)
        inst = FriInstanceC(infos, len(batches))
        self._check(lib().vpbs_fri_prove(self.h, handles, len(oracles), C.byref(inst), C.byref(params),
                                         C.byref(challenger.c), forced_pow, _ptr(proof)))
        return proof

    # ---- step proof ----
    def make_step_inputs(self, log_n, wires, zs_pp, quotient, constants_sigmas, circuit_digest, public_inputs,
                         num_challenges=2, forced_pow=POW_ANY, on_device=False, shapes=None, sigmas=None, n_routed=0,
                         quotient_degree_factor=8, n_constants=0, gates=None):
        """wires/zs_pp/quotient: numpy matrices [ncols][n] (host) or device pointers with shapes=(nw, nz, nq).
        zs_pp=None: the Z / partial-product matrix is computed on the device from `sigmas` ([n_routed][n] values, same
        residency as the other matrices); shapes[1] / n_zs then must equal num_challenges * ceil(n_routed / 8).
        quotient=None: the 8 * num_challenges quotient chunks are evaluated on the device for the permutation argument
        (sigma LDE columns are taken from constants_sigmas[n_constants : n_constants + n_routed])."""
        si = StepInputsC()
        si.log_n = log_n
        keep = []
        n_zs_auto = num_challenges * ((n_routed + quotient_degree_factor - 1) // quotient_degree_factor) if n_routed else 0
        if on_device:
            nw, nz, nq = shapes
            si.wires_values = int(wires)
            si.quotient_coeffs = int(quotient) if quotient is not None else None
            si.zs_pp_values = int(zs_pp) if zs_pp is not None else None
            if sigmas is not None:
                si.sigmas_values = int(sigmas)
        else:
            wires = _u64(wires)
            keep.append(wires)
            nw = wires.shape[0]
            si.wires_values = wires.ctypes.data
            if quotient is not None:
                quotient = _u64(quotient)
                keep.append(quotient)
                nq = quotient.shape[0]
                si.quotient_coeffs = quotient.ctypes.data
            else:
                nq = 8 * num_challenges
                si.quotient_coeffs = None
            if zs_pp is not None:
                zs_pp = _u64(zs_pp)
                keep.append(zs_pp)
                nz = zs_pp.shape[0]
                si.zs_pp_values = zs_pp.ctypes.data
            else:
                nz = n_zs_auto
                si.zs_pp_values = None
            if sigmas is not None and isinstance(sigmas, int):   # a device pointer: circuit data uploaded once
                si.sigmas_values, si.sigmas_on_device = sigmas, 1
            elif sigmas is not None:
                sigmas = _u64(sigmas)
                keep.append(sigmas)
                si.sigmas_values = sigmas.ctypes.data
        si.n_routed = n_routed
        si.quotient_degree_factor = quotient_degree_factor
        si.n_constants = n_constants
        if gates is not None:  # a GateSet: the gate constraints join the quotient (quotient=None only)
            si.gates, si.n_gates, si.num_selectors = gates.arr, gates.n, gates.num_selectors
            keep.append(gates)
        si.n_wires, si.n_zs_partial_products, si.n_quotient = nw, nz, nq
        si.num_challenges = num_challenges
        si.inputs_on_device = 1 if on_device else 0
        si.constants_sigmas = constants_sigmas.h
        for i in range(4):
            si.circuit_digest[i] = int(circuit_digest[i])
        pi = _u64(public_inputs).reshape(-1)
        keep.append(pi)
        si.public_inputs = _ptr(pi)
        si.n_public_inputs = pi.size
        si.forced_pow = forced_pow
        si._keep = keep
        return si

    def prove_step(self, si, comm=None):
        """comm: a CommC (sharding.make_comm) -> vpbs_prove_step_sharded, every rank returns the complete proof."""
        sizes = StepSizesC()
        self._check(lib().vpbs_step_sizes_get(self.h, C.byref(si), C.byref(sizes)))
        caps = np.zeros((3, sizes.cap_words // 4, 4), np.uint64)
        openings = np.zeros((sizes.openings_words // 2, 2), np.uint64)
        fri = np.zeros(sizes.fri_words, np.uint64)
        ch = ChallengerState()
        chal = np.zeros(3 * si.num_challenges + 2, np.uint64)
        if comm is None:
            self._check(lib().vpbs_prove_step(self.h, C.byref(si), _ptr(caps), _ptr(openings), _ptr(fri), C.byref(ch.c), _ptr(chal)))
        else:
            self._check(lib().vpbs_prove_step_sharded(self.h, C.byref(si), C.byref(comm), _ptr(caps), _ptr(openings), _ptr(fri),
                                                      C.byref(ch.c), _ptr(chal)))
        return {"caps": caps, "openings": openings, "fri": fri, "challenger": ch, "challenges": chal}

    def prove_step_checked(self, si, checker):
        """vpbs_prove_step_checked: prove_step with the witness checked on the device first (checker: a WitnessChecker of the circuit on
        this context's device).  A violated witness raises WitnessError with vpbs_check_witness's message; the context stays usable."""
        sizes = StepSizesC()
        self._check(lib().vpbs_step_sizes_get(self.h, C.byref(si), C.byref(sizes)))
        caps = np.zeros((3, sizes.cap_words // 4, 4), np.uint64)
        openings = np.zeros((sizes.openings_words // 2, 2), np.uint64)
        fri = np.zeros(sizes.fri_words, np.uint64)
        ch = ChallengerState()
        chal = np.zeros(3 * si.num_challenges + 2, np.uint64)
        rc = lib().vpbs_prove_step_checked(self.h, checker.h, C.byref(si), _ptr(caps), _ptr(openings), _ptr(fri), C.byref(ch.c), _ptr(chal))
        if rc == ERR_WITNESS:
            raise WitnessError(lib().vpbs_last_error(self.h).decode())
        self._check(rc)
        return {"caps": caps, "openings": openings, "fri": fri, "challenger": ch, "challenges": chal}

    def step_proof_to_bytes(self, si, n_constants, proof):
        cap = 8 * (proof["caps"].size + proof["openings"].size + proof["fri"].size + si.n_public_inputs + 8) + 4096
        buf = (C.c_uint8 * cap)()
        n = lib().vpbs_step_proof_to_bytes(self.h, C.byref(si), n_constants, _ptr(proof["caps"]), _ptr(proof["openings"]),
                                           _ptr(proof["fri"]), buf, cap)
        if n < 0:
            raise VpbsError("vpbs_step_proof_to_bytes failed: %d" % n)
        return bytes(buf[:n])

    def partial_products(self, wires, sigmas, betas, gammas, max_degree=8):
        """all_wires_permutation_partial_products on host matrices -> [nc * chunks][n] (Z's first)."""
        w, sg = _u64(wires), _u64(sigmas)
        n_routed, n = sg.shape
        nc = len(betas)
        chunks = (n_routed + max_degree - 1) // max_degree
        out = np.zeros((nc * chunks, n), np.uint64)
        b, g = _u64(betas), _u64(gammas)
        self._check(lib().vpbs_partial_products(self.h, w.ctypes.data, sg.ctypes.data, 0, n_routed, n.bit_length() - 1, _ptr(b), _ptr(g), nc,
                                                max_degree, out.ctypes.data))
        return out

    def quotient_permutation(self, cs_batch, n_constants, wires_batch, zs_batch, n_routed, betas, gammas, alphas, max_degree=8,
                             gate_terms_dev=None):
        """compute_quotient_polys (permutation part) from committed batches -> [nc * 8][n] coefficient chunks (host)."""
        nc = len(betas)
        out = np.zeros((nc * 8, wires_batch.n), np.uint64)
        b, g, a = _u64(betas), _u64(gammas), _u64(alphas)
        self._check(lib().vpbs_quotient_permutation(self.h, cs_batch.h, n_constants, wires_batch.h, zs_batch.h, n_routed, _ptr(b), _ptr(g),
                                                    _ptr(a), nc, max_degree, C.c_void_p(gate_terms_dev) if gate_terms_dev else None,
                                                    out.ctypes.data, 0))
        return out

    def gate_terms(self, cs_batch, wires_batch, gates, pi_hash, alphas, out_dev_ptr):
        """vpbs_gate_terms: folded gate constraints on the LDE coset -> device buffer [nc][8n] (leaf order)."""
        h, a = _u64(pi_hash), _u64(alphas)
        self._check(lib().vpbs_gate_terms(self.h, cs_batch.h, wires_batch.h, gates.arr, gates.n, gates.num_selectors, _ptr(h), _ptr(a), a.size,
                                          C.c_void_p(int(out_dev_ptr))))

    def blind_rotate_step(self, acc_in, masks, ggsw, K, ELL, LOGB, first_step=False, last_step=False):
        """One vPBS step on a batch of accumulators (host arrays): acc_in [B][K][N], masks [B], ggsw [K*ELL*K*N] shared or
        [B][K*ELL*K*N] per instance (NTT domain, Ggsw::flatten order) -> acc_out [B][K][N]."""
        acc = _u64(acc_in)
        B, K_, N = acc.shape
        assert K_ == K
        m = _u64(masks).reshape(-1)
        prm = TfheParamsC(N.bit_length() - 1, K, ELL, LOGB)
        out = np.zeros_like(acc)
        g = _u64(ggsw) if ggsw is not None else None
        per_instance = 1 if (g is not None and g.ndim == 2) else 0
        self._check(lib().vpbs_blind_rotate_step(self.h, C.byref(prm), B, acc.ctypes.data, m.ctypes.data,
                                                 g.ctypes.data if g is not None else None, per_instance, 1 if first_step else 0,
                                                 1 if last_step else 0, out.ctypes.data, 0))
        return out

    def pbs_accumulator_chain(self, acc_init, lwe_ct, bsk, ksk, K, ELL, LOGB):
        """All n + 2 accumulators of one PBS (verified_pbs order): acc_init [K][N], lwe_ct [n+1], bsk [n][K*ELL*K*N], ksk."""
        acc = _u64(acc_init)
        K_, N = acc.shape
        ct, b, k = _u64(lwe_ct).reshape(-1), _u64(bsk), _u64(ksk).reshape(-1)
        n = ct.size - 1
        assert K_ == K and b.shape == (n, K * ELL * K * N)
        prm = TfheParamsC(N.bit_length() - 1, K, ELL, LOGB)
        out = np.zeros((n + 2, K, N), np.uint64)
        self._check(lib().vpbs_pbs_accumulator_chain(self.h, C.byref(prm), n, _ptr(acc), _ptr(ct), _ptr(b), _ptr(k), _ptr(out)))
        return out

    def keygen(self, N, K, ELL, LOGB, n_lwe, seed, sigma_glwe=0.0, sigma_lwe=0.0, want_bsk=True, want_ksk=True):
        """vpbs_keygen: every key of one PBS from one seed (main.rs:40-46 with the RNGs seeded) -> dict(params, s_lwe [n], s_glwe [K-1][N],
        s_to [K][N], bsk [n][K*ELL*K*N], ksk [K*ELL*K*N]); bsk / ksk in the NTT domain, Ggsw::flatten order."""
        prm = KeygenParamsC(N.bit_length() - 1, K, ELL, LOGB, n_lwe, seed, sigma_glwe, sigma_lwe)
        s_lwe, s_glwe, s_to = np.zeros(n_lwe, np.uint64), np.zeros((K - 1, N), np.uint64), np.zeros((K, N), np.uint64)
        g = K * ELL * K * N
        bsk = np.zeros((n_lwe, g), np.uint64) if want_bsk else None
        ksk = np.zeros(g, np.uint64) if want_ksk else None
        self._check(lib().vpbs_keygen(self.h, C.byref(prm), _ptr(s_lwe), _ptr(s_glwe), _ptr(s_to), bsk.ctypes.data if want_bsk else None,
                                      ksk.ctypes.data if want_ksk else None, 0))
        return {"params": prm, "s_lwe": s_lwe, "s_glwe": s_glwe, "s_to": s_to, "bsk": bsk, "ksk": ksk}

    def keygen_device(self, N, K, ELL, LOGB, n_lwe, seed, sigma_glwe=0.0, sigma_lwe=0.0):
        """vpbs_keygen with keys_on_device = 1: the same keys, bsk / ksk left in device memory -> dict(params, s_lwe, s_glwe, s_to host
        arrays; d_bsk, d_ksk device pointers for Bootstrapper(keys_on_device=True), to be released with device_free)"""
        prm = KeygenParamsC(N.bit_length() - 1, K, ELL, LOGB, n_lwe, seed, sigma_glwe, sigma_lwe)
        s_lwe, s_glwe, s_to = np.zeros(n_lwe, np.uint64), np.zeros((K - 1, N), np.uint64), np.zeros((K, N), np.uint64)
        g = K * ELL * K * N
        d_bsk, d_ksk = C.c_void_p(), C.c_void_p()
        self._check(lib().vpbs_device_alloc(self.h, n_lwe * g, C.byref(d_bsk)))
        self._check(lib().vpbs_device_alloc(self.h, g, C.byref(d_ksk)))
        self._check(lib().vpbs_keygen(self.h, C.byref(prm), _ptr(s_lwe), _ptr(s_glwe), _ptr(s_to), d_bsk, d_ksk, 1))
        return {"params": prm, "s_lwe": s_lwe, "s_glwe": s_glwe, "s_to": s_to, "d_bsk": d_bsk.value, "d_ksk": d_ksk.value}

    def keygen_seeded(self, N, K, ELL, LOGB, n_lwe, seed, mask_seed, sigma_glwe=0.0, sigma_lwe=0.0, s_lwe=None, s_glwe=None, on_device=False):
        """vpbs_keygen_seeded: keygen under the split generator -- the mask streams from the public mask_seed, the secrets and the noise
        from the private seed -- handing out only the last polynomial of every GLWE: 1 / K of the key set.  s_lwe [n] and s_glwe [K-1][N]
        (both or neither) are the caller's OWN binary secrets; without them the secrets are those of keygen(seed).  -> dict(params,
        mask_seed, s_lwe, s_glwe, s_to host arrays; bsk_bodies [n][K*ELL*N], ksk_bodies [K*ELL*N] host arrays, or with on_device=True
        d_bsk_bodies, d_ksk_bodies device pointers to be released with device_free).  With mask_seed == seed the bodies are those of
        keygen's bsk / ksk.  mix64 is not a cryptographic generator: keys for benchmarking and integration, not for production."""
        prm = KeygenParamsC(N.bit_length() - 1, K, ELL, LOGB, n_lwe, seed, sigma_glwe, sigma_lwe)
        if (s_lwe is None) != (s_glwe is None):
            raise ValueError("keygen_seeded: s_lwe and s_glwe are given together or not at all")
        own = s_lwe is not None
        if own:
            sl_in, sg_in = _u64(s_lwe).reshape(-1), _u64(s_glwe).reshape(-1)
            if sl_in.size != n_lwe or sg_in.size != (K - 1) * N:
                raise ValueError("keygen_seeded: expected s_lwe [%d] and s_glwe [%d][%d]" % (n_lwe, K - 1, N))
        o_lwe, o_glwe, o_to = np.zeros(n_lwe, np.uint64), np.zeros((K - 1, N), np.uint64), np.zeros((K, N), np.uint64)
        g = K * ELL * N
        out = {"params": prm, "mask_seed": mask_seed, "s_lwe": o_lwe, "s_glwe": o_glwe, "s_to": o_to}
        if on_device:
            d_b, d_k = C.c_void_p(), C.c_void_p()
            self._check(lib().vpbs_device_alloc(self.h, n_lwe * g, C.byref(d_b)))
            self._check(lib().vpbs_device_alloc(self.h, g, C.byref(d_k)))
            pb, pk = d_b, d_k
        else:
            out["bsk_bodies"], out["ksk_bodies"] = np.zeros((n_lwe, g), np.uint64), np.zeros(g, np.uint64)
            pb, pk = out["bsk_bodies"].ctypes.data, out["ksk_bodies"].ctypes.data
        rc = lib().vpbs_keygen_seeded(self.h, C.byref(prm), int(mask_seed), sl_in.ctypes.data if own else None, sg_in.ctypes.data if own else None,
                                      _ptr(o_lwe), _ptr(o_glwe), _ptr(o_to), pb, pk, 1 if on_device else 0)
        if rc and on_device:
            self.device_free(d_b.value)
            self.device_free(d_k.value)
        self._check(rc)
        if on_device:
            out["d_bsk_bodies"], out["d_ksk_bodies"] = d_b.value, d_k.value
        return out

    def key_expand(self, N, K, ELL, n_lwe, mask_seed, bsk_bodies, ksk_bodies, on_device=False, d_bsk=None, d_ksk=None):
        """vpbs_key_expand: the full keys in keygen's layout from mask_seed and the bodies of keygen_seeded, word for word; the mask
        polynomials are regenerated and transformed on the device, the bodies copied in.  Host-array form: bsk_bodies [n][K*ELL*N] and
        ksk_bodies [K*ELL*N] (either may be None).  Device-pointer form: integers (None to skip one).  -> dict(bsk [n][K*ELL*K*N], ksk
        [K*ELL*K*N]) host arrays, or with on_device=True dict(d_bsk, d_ksk) device pointers for Bootstrapper / PbsProver / KeyRing.add with
        keys_on_device=True, to be released with device_free; or, with d_bsk / d_ksk (16-byte aligned device pointers of the caller's), the
        keys written there and nothing returned."""
        prm = TfheParamsC(N.bit_length() - 1, K, ELL, 0)   # the gadget base plays no part in the masks
        g = K * ELL * K * N
        bodies_dev = _is_dev(bsk_bodies) or _is_dev(ksk_bodies)
        if bodies_dev:
            pb, pk = (None if x is None else C.c_void_p(int(x)) for x in (bsk_bodies, ksk_bodies))
        else:
            b, k = key_expand_args(N, K, ELL, n_lwe, bsk_bodies, ksk_bodies)
            pb, pk = (None if x is None else C.c_void_p(x.ctypes.data) for x in (b, k))
        want_b, want_k = bsk_bodies is not None, ksk_bodies is not None
        if d_bsk is not None or d_ksk is not None:   # the caller's device buffers
            if (d_bsk is not None) != want_b or (d_ksk is not None) != want_k:
                raise ValueError("key_expand: d_bsk goes with bsk_bodies and d_ksk with ksk_bodies")
            rc = lib().vpbs_key_expand(self.h, C.byref(prm), n_lwe, int(mask_seed), pb, pk, 1 if bodies_dev else 0,
                                       C.c_void_p(int(d_bsk)) if want_b else None, C.c_void_p(int(d_ksk)) if want_k else None, 1)
            self._check(rc)
            return None
        if on_device:
            d_b, d_k = C.c_void_p(), C.c_void_p()
            if want_b:
                self._check(lib().vpbs_device_alloc(self.h, n_lwe * g, C.byref(d_b)))
            if want_k:
                self._check(lib().vpbs_device_alloc(self.h, g, C.byref(d_k)))
            ob, ok = (d_b if want_b else None), (d_k if want_k else None)
        else:
            bsk = np.zeros((n_lwe, g), np.uint64) if want_b else None
            ksk = np.zeros(g, np.uint64) if want_k else None
            ob, ok = (C.c_void_p(bsk.ctypes.data) if want_b else None), (C.c_void_p(ksk.ctypes.data) if want_k else None)
        rc = lib().vpbs_key_expand(self.h, C.byref(prm), n_lwe, int(mask_seed), pb, pk, 1 if bodies_dev else 0, ob, ok, 1 if on_device else 0)
        if rc and on_device:
            for d in (d_b, d_k):
                if d.value:
                    self.device_free(d.value)
        self._check(rc)
        if on_device:
            return {"d_bsk": d_b.value, "d_ksk": d_k.value}
        return {"bsk": bsk, "ksk": ksk}

    def lwe_encrypt_seeded_batch(self, params, mask_seed, s_lwe, messages, nonce0=0, out_dev_ptr=None, count=None):
        """vpbs_lwe_encrypt_seeded_batch on the device: bodies [count], the last word of lwe_encrypt_batch's rows under the split generator
        (mask streams from mask_seed, noise from params.seed).  s_lwe, messages, out_dev_ptr and count as in lwe_encrypt_batch."""
        return _lwe_encrypt_batch(self, params, s_lwe, messages, nonce0, out_dev_ptr, count, mask_seed=mask_seed)

    def lwe_expand_batch(self, n_lwe, mask_seed, bodies, nonce0=0, out_dev_ptr=None, count=None):
        """vpbs_lwe_expand_batch on the device: row i = the n_lwe mask words of nonce nonce0 + i under mask_seed, then bodies[i].  bodies is a
        host array or a device pointer (an integer; then count and out_dev_ptr are needed).  Without out_dev_ptr the rows come back,
        [count][n + 1]; with it they are left at that device pointer -- for KeyRing.run_device and the like -- and nothing is returned."""
        return _lwe_expand_batch(self, n_lwe, mask_seed, bodies, nonce0, out_dev_ptr, count)

    def device_free(self, d_ptr):
        lib().vpbs_device_free(self.h, C.c_void_p(int(d_ptr)))

    def device_upload_new(self, host):
        """a fresh device buffer holding the words of `host` -> device pointer (to be released with device_free)"""
        a = _u64(host).reshape(-1)
        d = C.c_void_p()
        self._check(lib().vpbs_device_alloc(self.h, max(a.size, 1), C.byref(d)))
        if a.size:
            self._check(lib().vpbs_device_upload(self.h, d, _ptr(a), a.size))
        return d.value

    def lwe_encrypt_batch(self, params, s_lwe, messages, nonce0=0, out_dev_ptr=None, count=None):
        """vpbs_lwe_encrypt_batch on the device: row i = lwe_encrypt(params, s_lwe, messages[i], nonce0 + i), word for word.  s_lwe and messages
        are host arrays or device pointers (integers; messages on the device need count and out_dev_ptr).  Without out_dev_ptr the rows come
        back, [count][n + 1]; with it they are left at that device pointer and nothing is returned."""
        return _lwe_encrypt_batch(self, params, s_lwe, messages, nonce0, out_dev_ptr, count)

    def lwe_decode_batch(self, s_lwe, cts_or_dev_ptr, delta, modulus, expected=None, count=None, stats=None, want=("msg",), n_lwe=None):
        """vpbs_lwe_decode_batch on the device.  cts [count][n + 1] host array, or a device pointer with count (then expected may be a device
        pointer too; a key on the device needs n_lwe).  want: names among "phase", "msg", "err" -> dict of host arrays [count] (err as int64);
        or, for device ciphertexts, a dict name -> device pointer, filled in place (returns None).  stats: a NoiseStats that is ADDED to;
        expected makes err relative to expected * delta and counts msg != expected mod modulus as a failure."""
        return _lwe_decode_batch(self, s_lwe, cts_or_dev_ptr, delta, modulus, expected, count, stats, want, n_lwe)

    def lwe_rotation_batch(self, s_lwe, cts_or_dev_ptr, N, p, log_slots=0, expected=None, count=None, stats=None, want=("idx",), n_lwe=None):
        """vpbs_lwe_rotation_batch on the device: what a bootstrap of each row will look up, without running it.  The arguments
        are lwe_decode_batch's, with the ring size N, the p of lut_testv and the gate's log_slots (0 for rows that are already snapped) in
        the place of delta and modulus.  want: names among "rot" (mu: coefficient j of the output's phase is lut_expect(testv, mu, j)),
        "idx" (the table position read; [p, 2p) is the negated half), "dev" (int64: positions between mu and the centre of the block of
        expected, or of idx) -> dict of host arrays [count]; or, for device ciphertexts, a dict name -> device pointer, filled in place
        (returns None).  stats: a NoiseStats that is ADDED to, over dev; expected counts idx != expected mod 2p as a failure.  The key's
        words must be 0 or 1."""
        return _lwe_rotation_batch(self, s_lwe, cts_or_dev_ptr, N, p, log_slots, expected, count, stats, want, n_lwe)

    def lwe_extract(self, glwe, n_lwe, count=None, N=None, K=None, out_dev_ptr=None):
        """vpbs_lwe_extract: Glwe::partial_sample_extract(n_lwe) of GLWEs [count][K][N] (or one [K][N]) -> [count][n_lwe + 1] (or [n_lwe + 1]).
        With out_dev_ptr, glwe is a device pointer too (count, N, K given) and nothing is returned."""
        if out_dev_ptr is not None:
            self._check(lib().vpbs_lwe_extract(self.h, N.bit_length() - 1, K, n_lwe, C.c_void_p(int(glwe)), count, C.c_void_p(int(out_dev_ptr)), 1))
            return None
        g = _u64(glwe)
        one = g.ndim == 2
        g3 = g.reshape((1,) + g.shape) if one else g
        cnt, K_, N_ = g3.shape
        out = np.zeros((cnt, n_lwe + 1), np.uint64)
        self._check(lib().vpbs_lwe_extract(self.h, N_.bit_length() - 1, K_, n_lwe, g3.ctypes.data, cnt, out.ctypes.data, 0))
        return out[0] if one else out

    def lwe_snap(self, N, log_slots, words, count=None, out_dev_ptr=None):
        """vpbs_lwe_snap on the device (see api.lwe_snap).  With out_dev_ptr, words is a device pointer of count words and nothing is returned."""
        return _lwe_snap(self, N, log_slots, words, count, out_dev_ptr)

    def lwe_extract_at(self, glwe, n_lwe, index, src, count=None, N=None, K=None, out_dev_ptr=None):
        """vpbs_lwe_extract_at on the device (see api.lwe_extract_at); index and src stay host arrays.  With out_dev_ptr, glwe is a device
        pointer too (count, N, K given) and nothing is returned."""
        return _lwe_extract_at(self, glwe, n_lwe, index, src, count, N, K, out_dev_ptr)

    def timing_shader_clock(self):
        """-> (MHz sustained under the leaf-hash kernel while timing was on, launches sampled)"""
        mhz, n = C.c_double(), C.c_uint()
        self._check(lib().vpbs_timing_shader_clock(self.h, C.byref(mhz), C.byref(n)))
        return mhz.value, n.value

    def clock_probe(self):
        """shader clock in MHz, measured on the context's stream after the work queued so far"""
        out = C.c_double()
        self._check(lib().vpbs_k_clock_probe(self.h, C.byref(out)))
        return out.value

    def upload_bg(self, d_dst, host, words):
        """vpbs_device_upload_bg: host (pinned) -> device pointer on the upload stream the contexts of a device share; callable from a
        second thread while a prover call runs on the context"""
        if lib().vpbs_device_upload_bg(self.h, C.c_void_p(int(d_dst)), C.c_void_p(int(host)), int(words)):
            raise VpbsError("vpbs_device_upload_bg failed")

    def upload_rows(self, d_dst, host, n_cols, n, row_lo, row_hi):
        """vpbs_device_upload_rows: rows [row_lo, row_hi) of every column of a column-major [n_cols][n] matrix"""
        self._check(lib().vpbs_device_upload_rows(self.h, C.c_void_p(int(d_dst)), C.c_void_p(int(host)), n_cols, n, row_lo, row_hi))

    def scatter(self, d_dst, d_positions, host_values, count, d_stage):
        """vpbs_device_scatter: d_dst[positions[i]] = host_values[i] (pointers as integers)"""
        self._check(lib().vpbs_device_scatter(self.h, C.c_void_p(int(d_dst)), C.c_void_p(int(d_positions)), C.c_void_p(int(host_values)), count,
                                              C.c_void_p(int(d_stage))))

    def glwe_decrypt(self, s, ct):
        """Glwe::decrypt: s [K-1][N] (or [K][N]: the leading K-1 polynomials are used), ct [K][N] -> m [N]"""
        ct = _u64(ct)
        K, N = ct.shape
        s = np.ascontiguousarray(_u64(s)[:K - 1])
        out = np.zeros(N, np.uint64)
        self._check(lib().vpbs_glwe_decrypt(self.h, N.bit_length() - 1, K, _ptr(s), _ptr(ct), _ptr(out)))
        return out

    # ---- kernel-level hooks ----
    def poseidon_batch(self, states):
        s = _u64(states).copy()
        self._check(lib().vpbs_k_poseidon_batch(self.h, _ptr(s), s.shape[0]))
        return s

    def hash_rows(self, rows):
        r = _u64(rows)
        out = np.zeros((r.shape[0], 4), np.uint64)
        self._check(lib().vpbs_k_hash_rows(self.h, _ptr(r), r.shape[0], r.shape[1], _ptr(out)))
        return out

    def intt(self, values):
        v = _u64(values)
        out = np.zeros_like(v)
        self._check(lib().vpbs_k_intt(self.h, _ptr(v), v.shape[0], v.shape[1].bit_length() - 1, _ptr(out)))
        return out

    def coset_lde(self, coeffs, rate_bits=3, shift=7):
        c = _u64(coeffs)
        out = np.zeros((c.shape[0], c.shape[1] << rate_bits), np.uint64)
        self._check(lib().vpbs_k_coset_lde(self.h, _ptr(c), c.shape[0], c.shape[1].bit_length() - 1, rate_bits, shift, _ptr(out)))
        return out

    def merkle_cap(self, leaves, cap_height):
        l = _u64(leaves)
        out = np.zeros((1 << cap_height, 4), np.uint64)
        self._check(lib().vpbs_k_merkle_cap(self.h, _ptr(l), l.shape[0], l.shape[1], cap_height, _ptr(out)))
        return out

    def negacyclic_ntt(self, data, inverse=False):
        d = _u64(data).copy()
        self._check(lib().vpbs_k_negacyclic_ntt(self.h, _ptr(d), d.shape[0], d.shape[1].bit_length() - 1, 1 if inverse else 0))
        return d

    # ---- timing ----
    def timing_enable(self, on=1):
        """0 off, 1 every kernel group, 2 only the dominant kernel (leaf_hash)."""
        self._check(lib().vpbs_timing_enable(self.h, int(on)))

    def timing_report(self):
        buf = C.create_string_buffer(8192)
        self._check(lib().vpbs_timing_report(self.h, buf, 8192))
        return json.loads(buf.value.decode())
