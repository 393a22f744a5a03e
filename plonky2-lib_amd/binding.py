"""ctypes binding of libglprover.so (C ABI: include/glp.h).

Mirrors the plonky2 objects the reference touches on the prove() path:
  Batch            <-> `PolynomialBatch`       (fri/oracle.rs)   from_values / from_coeffs / cap / prove / get
  Context.fft/ifft <-> `PolynomialCoeffs::fft`, `PolynomialValues::ifft`
Errors surface as GlpError carrying glp_last_error(), the analogue of the `anyhow::Error` that
`data.prove(pw)` returns [REF src/ecdsa/gadgets/ecdsa.rs:349].
"""
import ctypes as C
import os
import re
import subprocess
import weakref

import numpy as np

P = 0xFFFFFFFF00000001
_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SO = os.path.join(_HERE, "libglprover.so")
_lib = None


class GlpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("glp error %d: %s" % (code, msg))
        self.code = code


class _Gate(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("type", "selector_index", "group_start", "group_end", "row",
                                          "num_constraints", "p0", "p1")]


class _CircuitDesc(C.Structure):
    _fields_ = ([(f, C.c_uint32) for f in ("degree_bits", "num_wires", "num_routed_wires", "num_constants",
                                           "num_selectors", "num_challenges", "quotient_degree_factor",
                                           "num_partial_products", "num_gate_constraints", "rate_bits", "cap_height",
                                           "proof_of_work_bits", "num_query_rounds", "num_reductions")] +
                [("reduction_arity_bits", C.c_uint32 * 16), ("num_gates", C.c_uint32), ("num_public_inputs", C.c_uint32),
                 ("gates", C.POINTER(_Gate)), ("k_is", C.c_void_p), ("circuit_digest", C.c_uint64 * 4),
                 ("constants", C.c_void_p), ("sigmas", C.c_void_p), ("hasher", C.c_uint32)])


class _FriRange(C.Structure):
    _fields_ = [("oracle", C.c_uint32), ("col_begin", C.c_uint32), ("num_cols", C.c_uint32)]


class _FriPoint(C.Structure):
    _fields_ = [("point", C.c_uint64 * 2), ("num_ranges", C.c_uint32), ("ranges", C.POINTER(_FriRange))]


class _FriDesc(C.Structure):
    _fields_ = [("num_oracles", C.c_uint32), ("oracles", C.POINTER(C.c_void_p)), ("num_points", C.c_uint32),
                ("points", C.POINTER(_FriPoint)), ("num_reductions", C.c_uint32), ("reduction_arity_bits", C.c_uint32 * 16),
                ("proof_of_work_bits", C.c_uint32), ("num_query_rounds", C.c_uint32)]


class _FriOracleShape(C.Structure):
    _fields_ = [("num_cols", C.c_uint32), ("salted", C.c_uint32), ("shared", C.c_uint32)]


class _FriVerifyDesc(C.Structure):
    _fields_ = [("num_oracles", C.c_uint32), ("oracles", C.POINTER(_FriOracleShape)), ("log_n", C.c_uint32), ("rate_bits", C.c_uint32),
                ("cap_height", C.c_uint32), ("hasher", C.c_uint32), ("num_points", C.c_uint32), ("points", C.POINTER(_FriPoint)),
                ("num_reductions", C.c_uint32), ("reduction_arity_bits", C.c_uint32 * 16), ("proof_of_work_bits", C.c_uint32),
                ("num_query_rounds", C.c_uint32)]


class _PermDesc(C.Structure):
    _fields_ = [("log_n", C.c_uint32), ("num_wires", C.c_uint32), ("num_routed_wires", C.c_uint32), ("num_challenges", C.c_uint32),
                ("chunk_size", C.c_uint32), ("k_is", C.c_void_p)]


class _GateProgramDesc(C.Structure):
    _fields_ = [("code", C.c_void_p), ("num_instructions", C.c_uint32), ("pool", C.c_void_p), ("num_pool", C.c_uint32), ("num_regs", C.c_uint32),
                ("num_params", C.c_uint32), ("num_oracles", C.c_uint32), ("oracle_cols", C.c_void_p)]


class _ExtOpenings(C.Structure):
    _fields_ = [("at", C.c_void_p), ("at_next", C.c_void_p), ("proof_stride", C.c_size_t)]


class _WitnessReport(C.Structure):
    _fields_ = [("failed_constraints", C.c_uint64), ("failed_rows", C.c_uint64), ("failed_copies", C.c_uint64), ("row", C.c_uint64),
                ("gate", C.c_uint32), ("constraint", C.c_uint32), ("value", C.c_uint64), ("copy_row", C.c_uint64), ("copy_col", C.c_uint32),
                ("to_col", C.c_uint32), ("to_row", C.c_uint64), ("copy_value", C.c_uint64), ("to_value", C.c_uint64)]


class _WitnessPlanInfo(C.Structure):
    _fields_ = [("num_waves", C.c_uint32), ("num_units", C.c_uint64), ("num_stuck_units", C.c_uint64), ("num_copies", C.c_uint64),
                ("num_cells_known", C.c_uint64), ("widest_wave_units", C.c_uint64), ("stuck_row", C.c_uint64), ("stuck_gate", C.c_uint32),
                ("stuck_unit", C.c_uint32)]


class _WitnessFreeUnit(C.Structure):          # glp_witness_free_unit
    _fields_ = [("kind", C.c_uint32), ("modulus", C.c_uint32), ("cell_begin", C.c_uint32), ("len", C.c_uint16 * 6)]


class _WitnessProgramDesc(C.Structure):      # glp_witness_program_desc
    _fields_ = [("code", C.c_void_p), ("num_instructions", C.c_uint32), ("pool", C.c_void_p), ("num_pool", C.c_uint32), ("num_regs", C.c_uint32),
                ("num_inputs", C.c_uint32), ("num_outputs", C.c_uint32)]


class _WitnessPlanFreeInfo(C.Structure):
    _fields_ = [("num_free_units", C.c_uint64), ("num_stuck_free_units", C.c_uint64), ("first_stuck_free_unit", C.c_uint64),
                ("widest_wave_free_units", C.c_uint64)]


# GLP_WGEN_* of include/glp.h: the kinds of free units, their largest operand, the output cell that is not written
(WGEN_EQUALITY, WGEN_NONNATIVE_ADD, WGEN_NONNATIVE_MULTI_ADD, WGEN_NONNATIVE_SUB, WGEN_NONNATIVE_MUL, WGEN_NONNATIVE_INV, WGEN_BIGUINT_DIV_REM,
 WGEN_GLV_SECP256K1) = range(1, 9)
WGEN_PROGRAM = 9                               # a unit program: modulus = its index in programs, len = num_inputs, num_outputs
WGEN_MAX_LIMBS = 18
WGEN_NO_CELL = 0xFFFFFFFFFFFFFFFF
FREE_UNIT_DTYPE = np.dtype([("kind", np.uint32), ("modulus", np.uint32), ("cell_begin", np.uint32), ("len", np.uint16, (6,))])


# GLP_GATE_* of include/glp.h and the names of the gate types (19 is unassigned)
(GATE_NOOP, GATE_CONSTANT, GATE_PUBLIC_INPUT, GATE_ARITHMETIC, GATE_POSEIDON, GATE_U32_INTERLEAVE, GATE_UNINTERLEAVE_U32, GATE_UNINTERLEAVE_B32,
 GATE_U32_ARITHMETIC, GATE_U32_ADD_MANY, GATE_U32_SUBTRACTION, GATE_U32_RANGE_CHECK, GATE_COMPARISON, GATE_BASE_SUM, GATE_RANDOM_ACCESS,
 GATE_ARITHMETIC_EXTENSION, GATE_MUL_EXTENSION, GATE_REDUCING, GATE_REDUCING_EXTENSION) = range(19)
GATE_EXPONENTIATION, GATE_COSET_INTERPOLATION, GATE_POSEIDON_MDS = 20, 21, 22
GATE_PROGRAM = 23                              # a caller-defined gate: p0 = its program (Circuit(programs=...)); it has no name, reports give its number
GATE_PROGRAM_MAX_CONSTRAINTS = 4096            # GLP_GATE_PROGRAM_MAX_CONSTRAINTS
GATE_TYPE_NAMES = {
    GATE_NOOP: "NoopGate", GATE_CONSTANT: "ConstantGate", GATE_PUBLIC_INPUT: "PublicInputGate", GATE_ARITHMETIC: "ArithmeticGate",
    GATE_POSEIDON: "PoseidonGate", GATE_U32_INTERLEAVE: "U32InterleaveGate", GATE_UNINTERLEAVE_U32: "UninterleaveToU32Gate",
    GATE_UNINTERLEAVE_B32: "UninterleaveToB32Gate", GATE_U32_ARITHMETIC: "U32ArithmeticGate", GATE_U32_ADD_MANY: "U32AddManyGate",
    GATE_U32_SUBTRACTION: "U32SubtractionGate", GATE_U32_RANGE_CHECK: "U32RangeCheckGate", GATE_COMPARISON: "ComparisonGate",
    GATE_BASE_SUM: "BaseSumGate", GATE_RANDOM_ACCESS: "RandomAccessGate", GATE_ARITHMETIC_EXTENSION: "ArithmeticExtensionGate",
    GATE_MUL_EXTENSION: "MulExtensionGate", GATE_REDUCING: "ReducingGate", GATE_REDUCING_EXTENSION: "ReducingExtensionGate",
    GATE_EXPONENTIATION: "ExponentiationGate", GATE_COSET_INTERPOLATION: "CosetInterpolationGate", GATE_POSEIDON_MDS: "PoseidonMdsGate",
}
LDE_ROW_MAJOR, LDE_COL_MAJOR = 0, 1     # GLP_LDE_* of glp_batch_lde_values
RUN_SUM, RUN_PRODUCT = 0, 1             # GLP_RUN_* of glp_running_columns


def library_path():
    return _SO


def build_library(force=False):
    """Compile every HIP translation unit for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return _SO


def exported_symbols():
    """Function names declared in include/glp.h."""
    hdr = open(os.path.join(_ROOT, "include", "glp.h")).read()
    return re.findall(r"GLP_API [^;(]*?(glp_\w+)\(", hdr)


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise GlpError(-4, "libglprover.so is not built (run __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(_SO)
    vp, u32, u64, sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t
    L.glp_last_error.restype = C.c_char_p
    L.glp_version.restype = C.c_char_p
    L.glp_ctx_stream.restype = vp
    L.glp_ctx_stream.argtypes = [vp]
    L.glp_batch_num_digests.restype = sz
    L.glp_batch_num_digests.argtypes = [vp]
    sigs = {
        "glp_ctx_create": [C.c_int, C.POINTER(vp)],
        "glp_ctx_destroy": [vp],
        "glp_ctx_synchronize": [vp],
        "glp_ctx_set_profiling": [vp, C.c_int],
        "glp_ctx_stage_reset": [vp],
        "glp_ctx_stage_count": [vp],
        "glp_ctx_stage_get": [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(C.c_double)],
        "glp_poseidon_permute": [vp, vp, sz],
        "glp_fill_random_device": [vp, vp, sz, u64],
        "glp_fft": [vp, vp, u32, u32],
        "glp_ifft": [vp, vp, u32, u32],
        "glp_lde": [vp, vp, u32, u32, u32, u64, vp],
        "glp_batch_from_values": [vp, vp, u32, u32, u32, u32, C.POINTER(vp)],
        "glp_batch_from_values_device": [vp, vp, u32, u32, u32, u32, C.POINTER(vp)],
        "glp_batch_from_coeffs": [vp, vp, u32, u32, u32, u32, C.POINTER(vp)],
        "glp_batch_from_coeffs_device": [vp, vp, u32, u32, u32, u32, C.POINTER(vp)],
        "glp_batch_from_values_h": [vp, vp, u32, u32, u32, u32, u32, C.POINTER(vp)],
        "glp_batch_from_coeffs_h": [vp, vp, u32, u32, u32, u32, u32, C.POINTER(vp)],
        "glp_keccak256": [vp, vp, sz, sz, vp],
        "glp_batch_free": [vp],
        "glp_batch_info": [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)],
        "glp_batch_cap": [vp, vp],
        "glp_batch_coeffs": [vp, u32, u32, vp],
        "glp_batch_leaf": [vp, u64, vp],
        "glp_batch_merkle_proof": [vp, u64, vp],
        "glp_batch_digests": [vp, vp],
        "glp_batch_from_values_salted": [vp, vp, u32, u32, u32, u32, u32, vp, C.POINTER(vp)],
        "glp_ctx_set_salt_seed": [vp, vp],
    }
    L.glp_batch_leaf_len.restype = u32
    L.glp_batch_leaf_len.argtypes = [vp]
    L.glp_perm_num_polys.restype = u32
    L.glp_perm_num_polys.argtypes = [C.POINTER(_PermDesc)]
    for name in ("glp_batch_num_proofs", "glp_fri_num_proofs"):
        getattr(L, name).restype = u32
        getattr(L, name).argtypes = [vp]
    L.glp_proof_words.restype = sz
    L.glp_proof_words.argtypes = [vp]
    L.glp_proof_bytes_len.restype = sz
    L.glp_proof_bytes_len.argtypes = [vp]
    sigs.update({
        "glp_circuit_create": [vp, C.POINTER(_CircuitDesc), C.POINTER(vp)],
        "glp_circuit_create_ex": [vp, C.POINTER(_CircuitDesc), u32, C.POINTER(vp)],
        "glp_circuit_create_prog": [vp, C.POINTER(_CircuitDesc), u32, C.POINTER(_GateProgramDesc), u32, C.POINTER(vp)],
        "glp_gate_program_circuit_check": [C.POINTER(_GateProgramDesc), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)],
        "glp_circuit_zero_knowledge": [vp],
        "glp_circuit_free": [vp],
        "glp_circuit_digest": [vp, vp],
        "glp_circuit_constants_sigmas_cap": [vp, vp],
        "glp_prove": [vp, vp, vp, vp, vp],
        "glp_proof_to_bytes": [vp, vp, vp, sz],
        "glp_proof_from_bytes": [vp, vp, sz, vp],
        "glp_prove_device": [vp, vp, vp, vp, vp],
        "glp_session_begin": [vp, vp, vp, C.c_int, vp, C.POINTER(vp), vp, vp],
        "glp_session_partial_products": [vp, vp, vp, vp],
        "glp_session_quotient": [vp, vp, vp],
        "glp_session_open": [vp, vp, vp],
        "glp_session_fri_combine": [vp, vp],
        "glp_session_fri_commit": [vp, vp],
        "glp_session_fri_fold": [vp, vp],
        "glp_session_fri_final_poly": [vp, vp],
        "glp_pow_search": [vp, vp, vp, C.c_uint32, C.c_uint32, vp],
        "glp_pow_search_h": [vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, vp],
        "glp_session_queries": [vp, C.c_uint64, vp, C.c_uint32],
        "glp_session_proof": [vp, vp],
        "glp_session_end": [vp],
        "glp_session_oracle": [vp, u32, C.POINTER(vp)],
        "glp_fri_begin": [vp, C.POINTER(_FriDesc), C.POINTER(vp)],
        "glp_fri_open": [vp, vp],
        "glp_fri_combine": [vp, vp],
        "glp_fri_commit": [vp, vp],
        "glp_fri_fold": [vp, vp],
        "glp_fri_final_poly": [vp, vp],
        "glp_fri_queries": [vp, C.c_uint64, vp, C.c_uint32],
        "glp_fri_proof": [vp, vp],
        "glp_fri_end": [vp],
        "glp_fri_prove": [vp, C.POINTER(_FriDesc), vp, vp, u32, vp, vp],
        "glp_batch_many_from_values": [vp, vp, C.c_int, u32, u32, u32, u32, u32, u32, vp, C.POINTER(vp)],
        "glp_batch_many_from_coeffs": [vp, vp, C.c_int, u32, u32, u32, u32, u32, u32, vp, C.POINTER(vp)],
        "glp_batch_member": [vp, u32, C.POINTER(vp)],
        "glp_batch_caps": [vp, vp],
        "glp_batch_lde_values": [vp, u32, u32, u32, u64, u64, u32, vp, C.c_int],
        "glp_coset_ifft": [vp, vp, u32, u32, u64],
        "glp_batch_from_coset_values": [vp, vp, C.c_int, u32, u32, u32, u32, u32, u32, u32, vp, C.POINTER(vp)],
        "glp_perm_zs_commit": [vp, C.POINTER(_PermDesc), u32, vp, C.c_int, vp, C.c_int, vp, vp, u32, u32, u32, vp, C.POINTER(vp)],
        "glp_perm_quotient_values": [vp, C.POINTER(_PermDesc), u32, vp, u32, vp, vp, u32, vp, vp, vp, vp, C.c_int, vp, C.c_int],
        "glp_gate_program_check": [C.POINTER(_GateProgramDesc), C.POINTER(u32)],
        "glp_gate_program_create": [vp, C.POINTER(_GateProgramDesc), C.POINTER(vp)],
        "glp_gate_program_free": [vp],
        "glp_gate_program_sums": [vp, vp, u32, C.POINTER(vp), u32, u32, vp, vp, vp, C.c_int],
        "glp_gate_program_eval_ext": [vp, vp, u32, u32, vp, C.POINTER(_ExtOpenings), C.c_int, vp, vp, vp, C.c_int],
        "glp_gate_program_rows": [vp, vp, u32, u32, C.POINTER(vp), C.POINTER(u32), C.c_int, vp, vp, C.c_int],
        "glp_running_columns": [vp, u32, u32, u32, u32, u32, vp, vp, sz, C.c_int, vp, C.c_int, vp],
        "glp_perm_check_zeta": [vp, C.POINTER(_PermDesc), u32, u32, vp, C.POINTER(_ExtOpenings), C.POINTER(_ExtOpenings), C.POINTER(_ExtOpenings),
                                C.POINTER(_ExtOpenings), C.c_int, vp, vp, vp, vp, C.c_int, vp, vp],
        "glp_fri_begin_many": [vp, C.POINTER(_FriDesc), u32, vp, C.POINTER(vp)],
        "glp_fri_queries_many": [vp, vp, vp],
        "glp_pow_search_many": [vp, u32, u32, vp, vp, u32, u32, vp],
        "glp_fri_prove_many": [vp, C.POINTER(_FriDesc), u32, vp, vp, vp, u32, vp, vp],
        "glp_fri_verify_many": [vp, C.POINTER(_FriVerifyDesc), u32, vp, C.POINTER(vp), vp, vp, vp, vp, u32, vp, vp],
        "glp_fri_verify_queries_many": [vp, C.POINTER(_FriVerifyDesc), u32, vp, C.POINTER(vp), vp, vp, vp, vp, vp, vp, vp],
        "glp_fri_verify": [vp, C.POINTER(_FriVerifyDesc), C.POINTER(vp), vp, vp, vp, vp, u32],
        "glp_verify": [vp, vp],
        "glp_verify_n": [vp, vp, sz],
        "glp_prove_batch": [vp, vp, u32, vp, C.c_int, vp, vp],
        "glp_verify_batch": [vp, vp, u32, vp, vp, vp],
        "glp_witness_fill": [vp, vp, vp, C.c_int],
        "glp_witness_check": [vp, vp, u32, vp, C.c_int, vp, C.POINTER(_WitnessReport), vp],
        "glp_witness_columns": [vp, u32, vp],
        "glp_witness_unit_columns": [vp, u32, u32, vp],
        "glp_witness_plan_create": [vp, vp, vp, u32, C.POINTER(vp)],
        "glp_witness_plan_create_ex": [vp, vp, vp, u32, vp, u32, vp, sz, vp, u32, C.POINTER(vp)],
        "glp_witness_plan_create_prog": [vp, vp, vp, u32, vp, u32, vp, sz, vp, u32, vp, u32, C.POINTER(vp)],
        "glp_witness_plan_create_rand": [vp, vp, vp, u32, vp, u32, vp, u32, vp, sz, vp, u32, vp, u32, C.POINTER(vp)],
        "glp_witness_program_check": [C.POINTER(_WitnessProgramDesc)],
        "glp_witness_plan_free_info": [vp, C.POINTER(_WitnessPlanFreeInfo)],
        "glp_witness_plan_info": [vp, C.POINTER(_WitnessPlanInfo)],
        "glp_witness_plan_cell_waves": [vp, vp],
        "glp_witness_plan_free": [vp],
        "glp_witness_generate": [vp, vp, u32, vp, vp, u32],
        "glp_witness_read_cells": [vp, vp, u32, vp, vp, u32, vp],
        "glp_host_alloc": [vp, sz, C.POINTER(vp)],
        "glp_host_free": [vp, vp],
        "glp_witness_stage": [vp, vp, vp, u32, C.POINTER(vp)],
        "glp_prove_staged": [vp, vp, vp, vp, vp],
        "glp_witness_free": [vp],
        "glp_dev_alloc": [vp, sz, C.POINTER(vp)],
        "glp_dev_free": [vp, vp],
        "glp_dev_upload": [vp, vp, vp, sz],
        "glp_dev_download": [vp, vp, vp, sz],
    })
    sigs.update({
        "glp_circuit_file_write": [C.c_char_p, C.POINTER(_CircuitDesc), vp, vp],
        "glp_circuit_file_open": [C.c_char_p, C.c_int, C.POINTER(vp)],
        "glp_circuit_file_close": [vp],
    })
    L.glp_circuit_file_desc.restype = C.POINTER(_CircuitDesc)
    L.glp_circuit_file_desc.argtypes = [vp]
    for name in ("glp_circuit_file_wires", "glp_circuit_file_public_inputs"):
        getattr(L, name).restype = vp
        getattr(L, name).argtypes = [vp]
    for name in ("glp_num_openings", "glp_final_poly_len"):
        getattr(L, name).restype = sz
        getattr(L, name).argtypes = [vp]
    for name in ("glp_fri_num_openings", "glp_fri_final_poly_len", "glp_fri_proof_words"):
        getattr(L, name).restype = sz
        getattr(L, name).argtypes = [vp]
    for name in ("glp_fri_verify_proof_words", "glp_fri_verify_num_openings"):
        getattr(L, name).restype = sz
        getattr(L, name).argtypes = [C.POINTER(_FriVerifyDesc)]
    for name, argtypes in sigs.items():
        getattr(L, name).argtypes = argtypes
    L.glp_fri_end.restype = None
    L.glp_ctx_destroy.restype = None
    L.glp_batch_free.restype = None
    L.glp_circuit_free.restype = None
    L.glp_session_end.restype = None
    L.glp_circuit_file_close.restype = None
    L.glp_witness_free.restype = None
    L.glp_witness_plan_free.restype = None
    L.glp_witness_num_units.restype = u32
    L.glp_witness_num_units.argtypes = [vp, u32]
    L.glp_witness_plan_num_random.restype = u32
    L.glp_witness_plan_num_random.argtypes = [vp]
    L.glp_gate_program_free.restype = None
    _lib = L
    return L


def splitmix_field(seed, count, offset=0):
    """numpy twin of glp_fill_random_device (same values for the same seed)."""
    with np.errstate(over="ignore"):
        i = np.arange(offset + 1, offset + count + 1, dtype=np.uint64)
        z = np.uint64(seed) + i * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        return np.where(z >= np.uint64(P), z - np.uint64(P), z)


def _chk(rc):
    if rc != 0:
        raise GlpError(rc, load_library().glp_last_error().decode())


def _a(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """One GPU + one HIP stream (glp_ctx)."""

    def __init__(self, device=0):
        L = load_library()
        self._h = C.c_void_p()
        _chk(L.glp_ctx_create(int(device), C.byref(self._h)))
        self.device = device
        self._plans = weakref.WeakSet()    # witness plans: a glp_witness_plan must be freed before its context, host tables and all

    def close(self):
        if getattr(self, "_h", None):
            for plan in list(getattr(self, "_plans", ())):
                plan.free()
            load_library().glp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def synchronize(self):
        _chk(load_library().glp_ctx_synchronize(self._h))

    @property
    def stream(self):
        return load_library().glp_ctx_stream(self._h)

    # -- stage timers
    def set_profiling(self, on=True):
        _chk(load_library().glp_ctx_set_profiling(self._h, 1 if on else 0))

    def stage_reset(self):
        _chk(load_library().glp_ctx_stage_reset(self._h))

    def stages(self):
        L = load_library()
        out = []
        for i in range(L.glp_ctx_stage_count(self._h)):
            name, ms, by = C.c_char_p(), C.c_float(), C.c_double()
            _chk(L.glp_ctx_stage_get(self._h, i, C.byref(name), C.byref(ms), C.byref(by)))
            out.append((name.value.decode(), ms.value, by.value))
        return out

    # -- primitives
    def poseidon_permute(self, states):
        s = _a(states).reshape(-1, 12).copy()
        _chk(load_library().glp_poseidon_permute(self._h, _p(s), s.shape[0]))
        return s

    def fft(self, cols):
        a = np.atleast_2d(_a(cols)).copy()
        _chk(load_library().glp_fft(self._h, _p(a), a.shape[0], int(a.shape[1]).bit_length() - 1))
        return a

    def ifft(self, cols):
        a = np.atleast_2d(_a(cols)).copy()
        _chk(load_library().glp_ifft(self._h, _p(a), a.shape[0], int(a.shape[1]).bit_length() - 1))
        return a

    def lde(self, coeffs, rate_bits=3, shift=7):
        a = np.atleast_2d(_a(coeffs))
        out = np.empty((a.shape[0], a.shape[1] << rate_bits), np.uint64)
        _chk(load_library().glp_lde(self._h, _p(a), a.shape[0], int(a.shape[1]).bit_length() - 1, rate_bits, shift, _p(out)))
        return out

    def coset_ifft(self, cols, shift=7):
        """PolynomialValues::coset_ifft(shift) (glp_coset_ifft): natural-order values on shift * <w> -> natural-order coefficients"""
        a = np.atleast_2d(_a(cols)).copy()
        _chk(load_library().glp_coset_ifft(self._h, _p(a), a.shape[0], int(a.shape[1]).bit_length() - 1, int(shift)))
        return a

    def dev_alloc(self, nbytes):
        """Device buffer from the context's pool (for the *_device entry points); returns the pointer as an int."""
        p = C.c_void_p()
        _chk(load_library().glp_dev_alloc(self._h, int(nbytes), C.byref(p)))
        return p.value

    def dev_free(self, ptr):
        _chk(load_library().glp_dev_free(self._h, C.c_void_p(ptr)))

    def dev_upload(self, ptr, array):
        a = np.ascontiguousarray(array)
        _chk(load_library().glp_dev_upload(self._h, C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def dev_download(self, ptr, array):
        _chk(load_library().glp_dev_download(self._h, array.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), array.nbytes))

    def host_alloc(self, shape):
        """Page-locked host memory (glp_host_alloc) as a uint64 numpy array of `shape`: what witness generation should write into
        so that glp_witness_stage's copy overlaps the proof in flight.  Free with host_free(array)."""
        n = int(np.prod(shape))
        p = C.c_void_p()
        _chk(load_library().glp_host_alloc(self._h, max(n, 1) * 8, C.byref(p)))
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(max(n, 1),))[:n].reshape(shape)
        self.__dict__.setdefault("_pinned", {})[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr):
        p = self.__dict__.get("_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None and getattr(self, "_h", None):
            _chk(load_library().glp_host_free(self._h, C.c_void_p(p)))

    def fill_random_device(self, dev_ptr, count, seed):
        _chk(load_library().glp_fill_random_device(self._h, C.c_void_p(dev_ptr), count, seed))

    # -- PolynomialBatch
    def batch_from_values(self, values, rate_bits=3, cap_height=4, hasher=0):
        return Batch._make(self, "glp_batch_from_values_h", values, rate_bits, cap_height, hasher)

    def batch_from_values_salted(self, values, seed, rate_bits=3, cap_height=4, hasher=0):
        """PolynomialBatch::from_values(.., blinding = true): 4 salt columns after the polynomials, salts from `seed` (glp.h)"""
        a = _a(values)
        if a.ndim != 2 or a.shape[1] & (a.shape[1] - 1) or a.shape[1] == 0:
            raise GlpError(-1, "expected a [ncols][n] array, n a power of two")
        sd = _a(seed)
        if sd.size != 4:
            raise GlpError(-1, "the salt seed is 4 words")
        ncols, n = a.shape
        h = C.c_void_p()
        _chk(load_library().glp_batch_from_values_salted(self._h, _p(a), ncols, n.bit_length() - 1, rate_bits, cap_height, int(hasher),
                                                         _p(sd), C.byref(h)))
        b = Batch(self, h, ncols, n.bit_length() - 1, rate_bits, cap_height)
        b.hasher = int(hasher)
        return b

    def set_salt_seed(self, seed=None):
        """glp_ctx_set_salt_seed: a fixed seed for the salts of zero-knowledge proofs (tests, reproducibility), None = a fresh OS seed
        per call (the default).  Reusing a fixed seed across witnesses breaks hiding."""
        if seed is None:
            _chk(load_library().glp_ctx_set_salt_seed(self._h, None))
            return
        sd = _a(seed)
        if sd.size != 4:
            raise GlpError(-1, "the salt seed is 4 words")
        _chk(load_library().glp_ctx_set_salt_seed(self._h, _p(sd)))

    def batch_from_coeffs(self, coeffs, rate_bits=3, cap_height=4, hasher=0):
        return Batch._make(self, "glp_batch_from_coeffs_h", coeffs, rate_bits, cap_height, hasher)

    def batch_many_from_values(self, values, rate_bits=3, cap_height=4, hasher=0, seed=None):
        """glp_batch_many_from_values: values [num_proofs][ncols][n] -> one Batch of num_proofs members; seed (4 words): member k is
        salted with seed3 + k"""
        return Batch._make_many(self, "glp_batch_many_from_values", values, rate_bits, cap_height, hasher, seed)

    def batch_many_from_coeffs(self, coeffs, rate_bits=3, cap_height=4, hasher=0, seed=None):
        return Batch._make_many(self, "glp_batch_many_from_coeffs", coeffs, rate_bits, cap_height, hasher, seed)

    def batch_from_coset_values(self, values, sub_bits, rate_bits=3, cap_height=4, hasher=0, seed=None, dev_ptr=None, shape=None):
        """glp_batch_from_coset_values: values [num_polys][M] (or [num_proofs][num_polys][M] for K proofs), natural order on the
        coset 7 <W_M>, M = n << sub_bits -> the Batch of the num_polys << sub_bits chunk polynomials.  dev_ptr (with shape): the
        values are already in HBM at that pointer."""
        if dev_ptr is None:
            a = _a(values)
            shape = a.shape
        if len(shape) not in (2, 3) or shape[-1] & (shape[-1] - 1) or shape[-1] < (1 << sub_bits):
            raise GlpError(-1, "expected a [num_polys][M] or [num_proofs][num_polys][M] array, M = n << sub_bits a power of two")
        K, num_polys, M = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
        log_n = M.bit_length() - 1 - sub_bits
        sd = None if seed is None else _a(seed)
        if sd is not None and sd.size != 4:
            raise GlpError(-1, "the salt seed is 4 words")
        h = C.c_void_p()
        _chk(load_library().glp_batch_from_coset_values(self._h, _p(a) if dev_ptr is None else C.c_void_p(dev_ptr), 0 if dev_ptr is None else 1,
                                                        K, num_polys, log_n, int(sub_bits), rate_bits, cap_height, int(hasher),
                                                        None if sd is None else _p(sd), C.byref(h)))
        b = Batch(self, h, num_polys << sub_bits, log_n, rate_bits, cap_height)
        b.hasher = int(hasher)
        return b

    def perm_zs_commit(self, desc, wires, sigmas, betas, gammas, rate_bits=3, cap_height=4, hasher=0, seed=None, wires_dev_ptr=None,
                       sigmas_dev_ptr=None):
        """glp_perm_zs_commit: Z and the partial products of the permutation argument, committed.  desc: the attributes perm_desc()
        reads.  betas, gammas [num_challenges] with wires [num_wires][n] for one proof, or [num_proofs][num_challenges] with wires
        [num_proofs][num_wires][n]; sigmas [num_routed_wires][n].  *_dev_ptr: that array is already in HBM at the pointer (the host
        argument is ignored).  Returns the Batch of num_proofs members, perm_num_polys(desc) columns each."""
        d, keep = perm_desc(desc)
        b, g = _a(betas), _a(gammas)
        K = b.shape[0] if b.ndim == 2 else 1
        w = None if wires_dev_ptr is not None else _a(wires)
        sg = None if sigmas_dev_ptr is not None else _a(sigmas)
        n = 1 << d.log_n
        if w is not None and w.size != K * d.num_wires * n:
            raise GlpError(-1, "wires has %d elements, expected num_proofs * num_wires * n = %d" % (w.size, K * d.num_wires * n))
        if sg is not None and sg.size != d.num_routed_wires * n:
            raise GlpError(-1, "sigmas has %d elements, expected num_routed_wires * n = %d" % (sg.size, d.num_routed_wires * n))
        if b.size != K * d.num_challenges or g.size != b.size:
            raise GlpError(-1, "betas and gammas are [num_challenges] or [num_proofs][num_challenges]")
        sd = None if seed is None else _a(seed)
        if sd is not None and sd.size != 4:
            raise GlpError(-1, "the salt seed is 4 words")
        L = load_library()
        h = C.c_void_p()
        _chk(L.glp_perm_zs_commit(self._h, C.byref(d), K, C.c_void_p(wires_dev_ptr) if w is None else _p(w), 0 if w is not None else 1,
                                  C.c_void_p(sigmas_dev_ptr) if sg is None else _p(sg), 0 if sg is not None else 1, _p(b), _p(g), rate_bits,
                                  cap_height, int(hasher), None if sd is None else _p(sd), C.byref(h)))
        out = Batch(self, h, int(L.glp_perm_num_polys(C.byref(d))), d.log_n, rate_bits, cap_height)
        out.hasher = int(hasher)
        return out

    def perm_quotient_values(self, desc, sigmas_oracle, sigma_col_begin, wires_oracle, zs_oracle, sub_bits, betas, gammas, alphas,
                             gate_sums=None, gate_sums_dev_ptr=None, out_dev_ptr=None):
        """glp_perm_quotient_values: the permutation terms of the vanishing polynomial (plus alpha^T gate_sums) over Z_H on the coset
        7 <W_M>, M = n << sub_bits, natural order: [num_challenges][M] for challenges [num_challenges], [num_proofs][num_challenges][M]
        for [num_proofs][num_challenges] -- what batch_from_coset_values takes.  gate_sums: None, or an array of the result's shape
        (gate_sums_dev_ptr: already in HBM).  out_dev_ptr: the values go to that HBM pointer and None is returned."""
        d, keep = perm_desc(desc)
        b, g, al = _a(betas), _a(gammas), _a(alphas)
        K = b.shape[0] if b.ndim == 2 else 1
        if b.size != K * d.num_challenges or g.size != b.size or al.size != b.size:
            raise GlpError(-1, "betas, gammas and alphas are [num_challenges] or [num_proofs][num_challenges]")
        M = 1 << (d.log_n + int(sub_bits))
        shape = (K, d.num_challenges, M) if b.ndim == 2 else (d.num_challenges, M)
        gs = None if gate_sums is None or gate_sums_dev_ptr is not None else _a(gate_sums)
        if gs is not None and gs.size != K * d.num_challenges * M:
            raise GlpError(-1, "gate_sums has %d elements, expected num_proofs * num_challenges * M = %d" % (gs.size, K * d.num_challenges * M))
        gs_arg = C.c_void_p(gate_sums_dev_ptr) if gate_sums_dev_ptr is not None else (None if gs is None else _p(gs))
        out = None if out_dev_ptr is not None else np.empty(shape, np.uint64)
        _chk(load_library().glp_perm_quotient_values(self._h, C.byref(d), K, sigmas_oracle._h, int(sigma_col_begin), wires_oracle._h, zs_oracle._h,
                                                     int(sub_bits), _p(b), _p(g), _p(al), gs_arg, 0 if gate_sums_dev_ptr is None else 1,
                                                     C.c_void_p(out_dev_ptr) if out is None else _p(out), 0 if out is not None else 1))
        return out

    def perm_check_zeta(self, desc, num_quotient_chunks, zetas, sigmas, wires, zs, zs_next, quotient, betas, gammas, alphas, gate_sums=None,
                        gate_sums_dev_ptr=None, reasons=False):
        """glp_perm_check_zeta: the vanishing identity at zeta of num_proofs proofs, the gate terms taken from the caller.  desc: the
        attributes perm_desc() reads.  sigmas, wires, zs, zs_next, quotient: ExtOpenings (plonk_ext_openings() slices them out of a
        fri_verify_many openings array); zs_next shares zs's stride.  zetas [num_proofs][2]; betas, gammas, alphas [num_challenges]
        for one proof or [num_proofs][num_challenges].  gate_sums: None, or [num_proofs][num_challenges][2] (gate_sums_dev_ptr: in HBM,
        the out_dev_ptr of GateProgram.eval_ext).  With ExtOpenings over HBM zetas is an HBM pointer too.  Returns status [num_proofs]
        int32 (0 accepted, -5 rejected), with reasons=True (status, [num_proofs] str)."""
        d, keep = perm_desc(desc)
        b, g, al = _a(betas), _a(gammas), _a(alphas)
        K = b.shape[0] if b.ndim == 2 else 1
        if b.size != K * d.num_challenges or g.size != b.size or al.size != b.size:
            raise GlpError(-1, "betas, gammas and alphas are [num_challenges] or [num_proofs][num_challenges]")
        if zs_next is not None and (zs_next.proof_stride != zs.proof_stride or zs_next.on_device != zs.on_device):
            raise GlpError(-1, "zs_next has another proof_stride or memory than zs")
        parts = [sigmas, wires, zs, quotient]
        on_dev = _ext_on_device(parts)
        z = zetas if on_dev else _a(zetas)
        if not on_dev and z.size != 2 * K:
            raise GlpError(-1, "zetas has %d words, expected 2 * num_proofs = %d" % (z.size, 2 * K))
        cs = [o._c() for o in parts]
        if zs_next is not None:
            cs[2].at_next = zs_next._c().at
        gs = None if gate_sums is None or gate_sums_dev_ptr is not None else _a(gate_sums)
        if gs is not None and gs.size != 2 * K * d.num_challenges:
            raise GlpError(-1, "gate_sums has %d words, expected 2 * num_proofs * num_challenges = %d" % (gs.size, 2 * K * d.num_challenges))
        gs_arg = C.c_void_p(gate_sums_dev_ptr) if gate_sums_dev_ptr is not None else (None if gs is None else _p(gs))
        status = np.zeros(K, np.int32)
        buf = C.create_string_buffer(K * 160) if reasons else None
        _chk(load_library().glp_perm_check_zeta(self._h, C.byref(d), K, int(num_quotient_chunks), C.c_void_p(z) if on_dev else _p(z), C.byref(cs[0]),
                                                C.byref(cs[1]), C.byref(cs[2]), C.byref(cs[3]), 1 if on_dev else 0, _p(b), _p(g), _p(al), gs_arg,
                                                0 if gate_sums_dev_ptr is None else 1, status.ctypes.data_as(C.c_void_p), buf))
        del keep
        if not reasons:
            return status
        return status, [buf.raw[160 * k:160 * (k + 1)].split(b"\0", 1)[0].decode() for k in range(K)]

    def gate_program(self, prog):
        """glp_gate_program_create: prog is what gate_program.Assembler.assemble() returns (or anything gate_program_desc() takes).
        Returns the GateProgram, resident in HBM until free()."""
        d, keep = gate_program_desc(prog)
        h = C.c_void_p()
        _chk(load_library().glp_gate_program_create(self._h, C.byref(d), C.byref(h)))
        g = GateProgram(self, h, int(d.num_params), int(d.num_oracles))
        g.num_out = gate_program_check(prog)                     # columns of GateProgram.rows: the EMITs of a single-gate program
        return g

    def running_columns(self, kind, nums, dens, num_proofs=None, num_args=None, num_terms=None, log_n=None, in_proof_stride=None,
                        nums_dev_ptr=None, dens_dev_ptr=None, out_dev_ptr=None):
        """glp_running_columns: the helper columns nums / dens and the running column of kind RUN_SUM (logUp) or RUN_PRODUCT (grand
        product).  dens (and nums, or None for all ones): [num_terms][n] for one argument of one proof, [num_args][num_terms][n], or
        [num_proofs][num_args][num_terms][n]; the result has dens's leading dimensions: out [..][num_terms + 1][n] (the helper columns,
        then Z) and totals [num_proofs][num_args] (0 for a closed sum, 1 for a closed product).  dens_dev_ptr / nums_dev_ptr: the
        inputs are in HBM at these pointers (both or neither; nums_dev_ptr None: all ones) and num_proofs, num_args, num_terms, log_n
        and, unless the proofs are packed, in_proof_stride (words between proofs) say how.  out_dev_ptr: the columns go to that HBM
        pointer and (None, totals) is returned.  A zero denominator is GlpError -5 naming proof, argument, term and row."""
        if dens_dev_ptr is None:
            d = _a(dens)
            if not 2 <= d.ndim <= 4:
                raise GlpError(-1, "dens is [num_terms][n], [num_args][num_terms][n] or [num_proofs][num_args][num_terms][n]")
            lead = d.shape[:-2]
            K, A = ((1, 1), (1, d.shape[0]), d.shape[:2])[d.ndim - 2]
            T, n = d.shape[-2:]
            if n & (n - 1) or n == 0:
                raise GlpError(-1, "n must be a power of two")
            log_n = n.bit_length() - 1
            nm = None if nums is None else _a(nums)
            if nm is not None and nm.shape != d.shape:
                raise GlpError(-1, "nums has another shape than dens")
            stride = A * T * n
            d_arg, n_arg, on_dev = _p(d), None if nm is None else _p(nm), 0
        else:
            K, A, T, n = int(num_proofs), int(num_args), int(num_terms), 1 << int(log_n)
            lead = (K, A)
            stride = A * T * n if in_proof_stride is None else int(in_proof_stride)
            d_arg, n_arg, on_dev = C.c_void_p(dens_dev_ptr), None if nums_dev_ptr is None else C.c_void_p(nums_dev_ptr), 1
        out = None if out_dev_ptr is not None else np.empty(lead + (T + 1, n), np.uint64)
        totals = np.zeros((K, A), np.uint64)
        _chk(load_library().glp_running_columns(self._h, int(kind), K, A, T, int(log_n), n_arg, d_arg, stride, on_dev,
                                                C.c_void_p(out_dev_ptr) if out is None else _p(out), 0 if out is not None else 1, _p(totals)))
        return out, totals

    def pow_search_many(self, hasher, sponge_states, pending_inputs, bits):
        """glp_pow_search_many: sponge_states [K][12], pending_inputs [K][num_pending] (num_pending < 8) -> the K smallest witnesses"""
        st = _a(sponge_states).reshape(-1, 12)
        pend = _a(pending_inputs)
        pend = pend.reshape(st.shape[0], pend.size // max(st.shape[0], 1))
        out = np.zeros(st.shape[0], np.uint64)
        _chk(load_library().glp_pow_search_many(self._h, int(hasher), st.shape[0], _p(st), _p(pend) if pend.size else None, pend.shape[1],
                                                int(bits), _p(out)))
        return out

    def keccak256(self, msgs):
        """Keccak-256 of equal-length byte strings on the GPU (glp_keccak256): list of bytes -> list of 32-byte digests."""
        msgs = [bytes(m) for m in msgs]
        if not msgs:
            return []
        n = len(msgs[0])
        if any(len(m) != n for m in msgs):
            raise GlpError(-1, "glp_keccak256 takes messages of one length")
        buf = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8)
        out = np.zeros((len(msgs), 32), np.uint8)
        _chk(load_library().glp_keccak256(self._h, buf.ctypes.data_as(C.c_void_p), len(msgs), n, out.ctypes.data_as(C.c_void_p)))
        return [bytes(r) for r in out]

    def batch_from_values_device(self, dev_ptr, ncols, log_n, rate_bits=3, cap_height=4):
        return Batch._make_dev(self, "glp_batch_from_values_device", dev_ptr, ncols, log_n, rate_bits, cap_height)

    def batch_from_coeffs_device(self, dev_ptr, ncols, log_n, rate_bits=3, cap_height=4):
        return Batch._make_dev(self, "glp_batch_from_coeffs_device", dev_ptr, ncols, log_n, rate_bits, cap_height)


class Batch:
    """plonky2 `PolynomialBatch` resident on the GPU."""

    def __init__(self, ctx, handle, ncols, log_n, rate_bits, cap_height, owner=None, parent=None):
        self.ctx, self._h = ctx, handle
        self.ncols, self.log_n, self.rate_bits, self.cap_height = ncols, log_n, rate_bits, cap_height
        self._owner = owner        # a borrowed handle (Session.oracle): the owner frees it, and is kept alive meanwhile
        self._parent = parent      # a member view (Batch.member): freed like any batch, its device memory is the parent's
        self._views = weakref.WeakSet()    # views handed out by member(): they end with this batch
        self.hasher = 0                    # GLP_HASH_* of the tree; the constructors that take a hasher set it

    @classmethod
    def _make_many(cls, ctx, fn, arr, rate_bits, cap_height, hasher, seed):
        a = _a(arr)
        if a.ndim != 3 or a.shape[2] & (a.shape[2] - 1) or a.shape[2] == 0:
            raise GlpError(-1, "expected a [num_proofs][ncols][n] array, n a power of two")
        sd = None if seed is None else _a(seed)
        if sd is not None and sd.size != 4:
            raise GlpError(-1, "the salt seed is 4 words")
        K, ncols, n = a.shape
        h = C.c_void_p()
        _chk(getattr(load_library(), fn)(ctx._h, _p(a), 0, K, ncols, n.bit_length() - 1, rate_bits, cap_height, int(hasher),
                                         None if sd is None else _p(sd), C.byref(h)))
        b = cls(ctx, h, ncols, n.bit_length() - 1, rate_bits, cap_height)
        b.hasher = int(hasher)
        return b

    @property
    def num_proofs(self):
        """members of a many-proof batch (1 for every other batch)"""
        return int(load_library().glp_batch_num_proofs(self._h))

    def member(self, k):
        """glp_batch_member: member k as a Batch of its own, a view into this one.  The view keeps this batch alive; free() of this
        batch ends its views first (their handles become None, so a later use is a GlpError, not a stale pointer)"""
        h = C.c_void_p()
        _chk(load_library().glp_batch_member(self._h, int(k), C.byref(h)))
        v = Batch(self.ctx, h, self.ncols, self.log_n, self.rate_bits, self.cap_height, parent=self)
        v.hasher = self.hasher
        self._views.add(v)
        return v

    def caps(self):
        """every member's cap: [num_proofs][2^cap_height][4]"""
        out = np.empty((self.num_proofs, 1 << self.cap_height, 4), np.uint64)
        _chk(load_library().glp_batch_caps(self._h, _p(out)))
        return out

    @classmethod
    def _make(cls, ctx, fn, arr, rate_bits, cap_height, hasher=0):
        a = _a(arr)
        if a.ndim != 2:
            raise GlpError(-1, "expected a [ncols][n] array")
        ncols, n = a.shape
        if n & (n - 1) or n == 0:
            raise GlpError(-1, "n must be a power of two")
        h = C.c_void_p()
        _chk(getattr(load_library(), fn)(ctx._h, _p(a), ncols, n.bit_length() - 1, rate_bits, cap_height, int(hasher), C.byref(h)))
        b = cls(ctx, h, ncols, n.bit_length() - 1, rate_bits, cap_height)
        b.hasher = int(hasher)
        return b

    @classmethod
    def _make_dev(cls, ctx, fn, dev_ptr, ncols, log_n, rate_bits, cap_height):
        h = C.c_void_p()
        _chk(getattr(load_library(), fn)(ctx._h, C.c_void_p(dev_ptr), ncols, log_n, rate_bits, cap_height, C.byref(h)))
        return cls(ctx, h, ncols, log_n, rate_bits, cap_height)

    def free(self):
        if self._h:
            for v in list(self._views):
                v.free()
            if self._parent is not None:                                  # a view: only its host struct, no context needed
                load_library().glp_batch_free(self._h)
            elif self._owner is None and getattr(self.ctx, "_h", None):   # never touch a handle whose context is already gone
                load_library().glp_batch_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    @property
    def num_leaves(self):
        return 1 << (self.log_n + self.rate_bits)

    def cap(self):
        out = np.empty((1 << self.cap_height, 4), np.uint64)
        _chk(load_library().glp_batch_cap(self._h, _p(out)))
        return out

    def coeffs(self, col_begin=0, ncols=None):
        ncols = self.ncols - col_begin if ncols is None else ncols
        out = np.empty((ncols, 1 << self.log_n), np.uint64)
        _chk(load_library().glp_batch_coeffs(self._h, col_begin, ncols, _p(out)))
        return out

    def lde_values(self, col_begin, num_cols, sub_bits, row_begin=0, num_rows=None, layout=LDE_ROW_MAJOR, dev_ptr=None):
        """glp_batch_lde_values: rows [row_begin, row_begin + num_rows) of the coset 7 <W_M>, M = n << sub_bits, for columns
        [col_begin, col_begin + num_cols): row i is `get_lde_values(i, 2^(rate_bits - sub_bits))`.  Returns [num_rows][num_cols]
        (LDE_ROW_MAJOR) or [num_cols][num_rows] (LDE_COL_MAJOR), with a leading [num_proofs] for a many-proof batch.  dev_ptr: the
        values go to that HBM pointer instead (asynchronous on the ctx stream) and None is returned."""
        if num_rows is None:
            num_rows = (1 << (self.log_n + sub_bits)) - row_begin
        L = load_library()
        if dev_ptr is not None:
            _chk(L.glp_batch_lde_values(self._h, col_begin, num_cols, sub_bits, row_begin, num_rows, layout, C.c_void_p(dev_ptr), 1))
            return None
        K = self.num_proofs if self._h else 1
        inner = (max(num_rows, 0), num_cols) if layout == LDE_ROW_MAJOR else (num_cols, max(num_rows, 0))
        out = np.empty(((K,) + inner) if K > 1 else inner, np.uint64)
        _chk(L.glp_batch_lde_values(self._h, col_begin, num_cols, sub_bits, row_begin, num_rows, layout, _p(out if out.size else np.empty(1, np.uint64)), 0))   # an empty window is the library's error to name
        return out

    @property
    def leaf_len(self):
        """words of one Merkle leaf: ncols, + 4 salts for a salted batch"""
        return int(load_library().glp_batch_leaf_len(self._h))

    def leaf(self, index):
        out = np.empty(self.leaf_len, np.uint64)
        _chk(load_library().glp_batch_leaf(self._h, int(index), _p(out)))
        return out

    def prove(self, index):
        depth = self.log_n + self.rate_bits - self.cap_height
        out = np.empty((depth, 4), np.uint64)
        _chk(load_library().glp_batch_merkle_proof(self._h, int(index), _p(out)))
        return out

    def digests(self):
        n = load_library().glp_batch_num_digests(self._h)
        out = np.empty((n, 4), np.uint64)
        _chk(load_library().glp_batch_digests(self._h, _p(out)))
        return out


def gate_program_desc(prog, **fields):
    """attribute bag (code, pool, num_regs, num_params, oracle_cols: a gate_program.Program) -> (glp_gate_program_desc, the arrays that
    must stay alive while it is used).  fields: struct fields set afterwards, for descriptions the library is meant to refuse."""
    code, pool, cols = _a(prog.code), _a(prog.pool), np.ascontiguousarray(prog.oracle_cols, np.uint32)
    d = _GateProgramDesc(code.ctypes.data if code.size else None, code.size, pool.ctypes.data if pool.size else None, pool.size, int(prog.num_regs),
                         int(prog.num_params), cols.size, cols.ctypes.data if cols.size else None)
    for k, v in fields.items():
        setattr(d, k, v)
    return d, (code, pool, cols)


def gate_program_check(prog, **fields):
    """glp_gate_program_check (host only, no context): the largest number of EMITs in one gate, or GlpError naming the instruction
    and the field"""
    d, _keep = gate_program_desc(prog, **fields)
    out = C.c_uint32()
    _chk(load_library().glp_gate_program_check(C.byref(d), C.byref(out)))
    return int(out.value)


def gate_program_circuit_check(prog, **fields):
    """glp_gate_program_circuit_check (host only, no context): the rules a program is held to as a gate of a circuit (GATE_PROGRAM,
    Circuit(programs=...)) -> (num_constraints, degree, wires_used, consts_used), or GlpError naming the instruction and the field"""
    d, _keep = prog if isinstance(prog, tuple) else gate_program_desc(prog, **fields)
    out = [C.c_uint32() for _ in range(4)]
    _chk(load_library().glp_gate_program_circuit_check(C.byref(d), *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def witness_program_desc(prog, **fields):
    """attribute bag (code, pool, num_regs, num_inputs, num_outputs: a witness_program.WitnessProgram) -> (glp_witness_program_desc, the
    arrays that must stay alive while it is used).  fields: struct fields set afterwards, for descriptions the library is meant to refuse."""
    code, pool = _a(prog.code), _a(prog.pool)
    counts = [int(prog.num_regs), int(prog.num_inputs), int(prog.num_outputs)]
    if min(counts) < 0 or max(counts + [code.size, pool.size]) >= 1 << 32:
        raise GlpError(-1, "witness program: a count does not fit a uint32")
    d = _WitnessProgramDesc(code.ctypes.data if code.size else None, code.size, pool.ctypes.data if pool.size else None, pool.size, *counts)
    for k, v in fields.items():
        setattr(d, k, v)
    return d, (code, pool)


def witness_program_descs(programs):
    """a list of such bags -> (a C array of glp_witness_program_desc, what must stay alive)"""
    pairs = [witness_program_desc(p) for p in programs]
    arr = (_WitnessProgramDesc * max(len(pairs), 1))(*[d for d, _ in pairs])
    return arr, [k for _, k in pairs]


def witness_program_check(prog, **fields):
    """glp_witness_program_check (host only, no context): GlpError naming the instruction and the field, or the description's field"""
    d, _keep = witness_program_desc(prog, **fields)
    _chk(load_library().glp_witness_program_check(C.byref(d)))


class GateProgram:
    """A gate program resident on the GPU (glp_gate_program_create)."""

    def __init__(self, ctx, handle, num_params, num_oracles):
        self.ctx, self._h, self.num_params, self.num_oracles = ctx, handle, num_params, num_oracles
        self.num_out = 0

    def sums(self, oracles, sub_bits, alphas, params=None, out_dev_ptr=None):
        """glp_gate_program_sums: the program on every point of the coset 7 <W_M>, M = n << sub_bits, natural order.  oracles: the
        Batches the program's COL operands name, in order.  alphas [num_challenges] (then params [num_params]) for one proof: returns
        [num_challenges][M]; alphas [num_proofs][num_challenges] (params [num_proofs][num_params]): [num_proofs][num_challenges][M] --
        what perm_quotient_values takes as gate_sums.  out_dev_ptr: the values go to that HBM pointer and None is returned."""
        al = _a(alphas)
        K, nch = (al.shape[0], al.shape[1]) if al.ndim == 2 else (1, al.size)
        pr = None if params is None else _a(params)
        if pr is not None and pr.size != K * self.num_params:
            raise GlpError(-1, "params has %d elements, expected num_proofs * num_params = %d" % (pr.size, K * self.num_params))
        oracles = list(oracles)
        if len(oracles) != self.num_oracles:
            raise GlpError(-1, "%d oracles, the program reads %d" % (len(oracles), self.num_oracles))
        hs = (C.c_void_p * len(oracles))(*[o._h for o in oracles])
        M = 1 << (oracles[0].log_n + int(sub_bits))
        out = None if out_dev_ptr is not None else np.empty((K, nch, M) if al.ndim == 2 else (nch, M), np.uint64)
        _chk(load_library().glp_gate_program_sums(self.ctx._h, self._h, K, hs, int(sub_bits), nch, _p(al), None if pr is None or not pr.size else _p(pr),
                                                  C.c_void_p(out_dev_ptr) if out is None else _p(out), 0 if out is not None else 1))
        return out

    def rows(self, inputs, params=None, in_dev_ptrs=None, out_dev_ptr=None):
        """glp_gate_program_rows: the program on the n rows of H; EMIT number t is column t of the result.  The program is a single
        gate closed by END IMM(1).  inputs: one array per oracle the program names, values on H: [oracle_cols[o]][n] (shared by all
        proofs) or [num_proofs][oracle_cols[o]][n].  params [num_params] for one proof: returns [num_out][n]; [num_proofs][num_params],
        or any input with a leading [num_proofs]: [num_proofs][num_out][n].  in_dev_ptrs: the inputs are in HBM at these pointers and
        `inputs` holds their shapes instead.  out_dev_ptr: the values go to that HBM pointer and None is returned."""
        on_dev = in_dev_ptrs is not None
        ins = [tuple(int(v) for v in i) for i in inputs] if on_dev else [_a(i) for i in inputs]
        shapes = ins if on_dev else [i.shape for i in ins]
        if len(shapes) != self.num_oracles or (on_dev and len(in_dev_ptrs) != len(shapes)):
            raise GlpError(-1, "%d inputs, the program reads %d" % (len(shapes), self.num_oracles))
        if any(len(s) not in (2, 3) or s[-1] & (s[-1] - 1) or s[-1] != shapes[0][-1] or s[-1] == 0 for s in shapes):
            raise GlpError(-1, "an input is [columns][n] or [num_proofs][columns][n], n one power of two")
        pr = None if params is None else _a(params)
        K = pr.shape[0] if pr is not None and pr.ndim == 2 else max([s[0] for s in shapes if len(s) == 3], default=1)
        many = (pr is not None and pr.ndim == 2) or any(len(s) == 3 for s in shapes)
        if pr is not None and pr.size != K * self.num_params:
            raise GlpError(-1, "params has %d elements, expected num_proofs * num_params = %d" % (pr.size, K * self.num_params))
        n = shapes[0][-1]
        ptrs = (C.c_void_p * len(shapes))(*(in_dev_ptrs if on_dev else [i.ctypes.data for i in ins]))
        members = (C.c_uint32 * len(shapes))(*[s[0] if len(s) == 3 else 1 for s in shapes])
        out = None
        if out_dev_ptr is None:
            out = np.empty((K, self.num_out, n) if many else (self.num_out, n), np.uint64)
        _chk(load_library().glp_gate_program_rows(self.ctx._h, self._h, K, n.bit_length() - 1, ptrs, members, 1 if on_dev else 0,
                                                  None if pr is None or not pr.size else _p(pr),
                                                  C.c_void_p(out_dev_ptr) if out is None else _p(out if out.size else np.empty(1, np.uint64)),
                                                  0 if out is not None else 1))
        return out

    def eval_ext(self, points, openings, alphas, params=None, out_dev_ptr=None):
        """glp_gate_program_eval_ext: the program over F_p^2 at points[k], on the openings of num_proofs proofs: the gate_sums at zeta
        that perm_check_zeta takes.  openings: one ExtOpenings per oracle the program names, in order (all over host memory, or all
        over HBM: then points is an HBM pointer too).  points [num_proofs][2]; alphas [num_challenges] (then params [num_params]) for
        one proof: returns [num_challenges][2]; alphas [num_proofs][num_challenges]: [num_proofs][num_challenges][2].  out_dev_ptr:
        the values go to that HBM pointer and None is returned."""
        al = _a(alphas)
        K, nch = (al.shape[0], al.shape[1]) if al.ndim == 2 else (1, al.size)
        pr = None if params is None else _a(params)
        if pr is not None and pr.size != K * self.num_params:
            raise GlpError(-1, "params has %d elements, expected num_proofs * num_params = %d" % (pr.size, K * self.num_params))
        openings = list(openings)
        if len(openings) != self.num_oracles:
            raise GlpError(-1, "%d openings, the program reads %d oracles" % (len(openings), self.num_oracles))
        on_dev = _ext_on_device(openings)
        pts = points if on_dev else _a(points)
        if not on_dev and pts.size != 2 * K:
            raise GlpError(-1, "points has %d words, expected 2 * num_proofs = %d" % (pts.size, 2 * K))
        cs = (_ExtOpenings * len(openings))(*[o._c() for o in openings])
        out = None if out_dev_ptr is not None else np.empty((K, nch, 2) if al.ndim == 2 else (nch, 2), np.uint64)
        _chk(load_library().glp_gate_program_eval_ext(self.ctx._h, self._h, K, nch, C.c_void_p(pts) if on_dev else _p(pts), cs, 1 if on_dev else 0,
                                                      _p(al), None if pr is None or not pr.size else _p(pr),
                                                      C.c_void_p(out_dev_ptr) if out is None else _p(out), 0 if out is not None else 1))
        return out

    def free(self):
        if self._h:
            if getattr(self.ctx, "_h", None):             # never touch a handle whose context is already gone
                load_library().glp_gate_program_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ExtOpenings:
    """glp_ext_openings: the F_p^2 openings of one oracle for num_proofs proofs.  array: the uint64 host array that holds them (the
    whole openings array of fri_verify_many will do; it is kept alive); at: the word offset in it of (proof 0, polynomial 0); at_next:
    the same for the openings at w_n * point, or None; proof_stride: words between proofs (default: the size of array[0]).
    dev_ptr: the words are in HBM from that pointer on, and array is ignored."""

    def __init__(self, array, at=0, at_next=None, proof_stride=None, dev_ptr=None):
        self.dev_ptr = dev_ptr
        self.array = None if dev_ptr is not None else _a(array)
        if proof_stride is None:
            if self.array is None:
                raise GlpError(-1, "proof_stride is needed with dev_ptr")
            proof_stride = self.array.size // self.array.shape[0] if self.array.ndim > 1 else self.array.size
        self.at, self.at_next, self.proof_stride = int(at), None if at_next is None else int(at_next), int(proof_stride)

    @property
    def on_device(self):
        return self.dev_ptr is not None

    def _c(self):
        base = int(self.dev_ptr) if self.on_device else self.array.ctypes.data
        return _ExtOpenings(base + 8 * self.at, None if self.at_next is None else base + 8 * self.at_next, self.proof_stride)


def _ext_on_device(openings):
    dev = [o.on_device for o in openings]
    if any(dev) != all(dev):
        raise GlpError(-1, "the openings are all over host memory or all over HBM")
    return all(dev)


def plonk_ext_openings(desc, openings=None, dev_ptr=None):
    """The openings array of fri_verify_many for the plonk instance of `desc` ([num_proofs][count][2] or [count][2], the order of
    glp_fri_open: constants ++ sigmas, wires, zs ++ partial products, quotient at zeta, then the Z polynomials at g zeta), sliced into
    ExtOpenings: a dict with "program" ([constants ++ sigmas, wires]: what GateProgram.eval_ext takes for a program that names those
    two oracles), "sigmas", "wires", "zs", "zs_next" and "quotient" (what Context.perm_check_zeta takes), and "count"."""
    nc, nr, nw, nch = int(desc.num_constants), int(desc.num_routed_wires), int(desc.num_wires), int(desc.num_challenges)
    nzp, nq = nch * (1 + int(desc.num_partial_products)), nch * int(desc.quotient_degree_factor)
    count = nc + nr + nw + nzp + nq + nch
    if dev_ptr is None:
        openings = _a(openings)
        if openings.size % (2 * count):
            raise GlpError(-1, "openings has %d words, no multiple of 2 * %d" % (openings.size, count))

    def part(at):
        return ExtOpenings(openings, 2 * at, None, 2 * count, dev_ptr)
    return {"program": [part(0), part(nc + nr)], "sigmas": part(nc), "wires": part(nc + nr), "zs": part(nc + nr + nw),
            "zs_next": part(nc + nr + nw + nzp + nq), "quotient": part(nc + nr + nw + nzp), "count": count}


def perm_desc(desc):
    """attribute bag (a synth circuit, or anything with degree_bits, num_wires, num_routed_wires, num_challenges, quotient_degree_factor
    and k_is) -> (glp_perm_desc, the k_is array that must stay alive while it is used)"""
    k = _a(desc.k_is)
    if k.size != int(desc.num_routed_wires):
        raise GlpError(-1, "k_is has %d entries, num_routed_wires is %d" % (k.size, desc.num_routed_wires))
    d = _PermDesc(int(desc.degree_bits), int(desc.num_wires), int(desc.num_routed_wires), int(desc.num_challenges),
                  int(desc.quotient_degree_factor), k.ctypes.data)
    return d, k


def perm_num_polys(desc):
    """glp_perm_num_polys: num_challenges * (1 + num_partial_products), 0 for a description the library refuses"""
    d, _keep = perm_desc(desc)
    return int(load_library().glp_perm_num_polys(C.byref(d)))


def _desc_to_c(desc):
    """synth.Circuit-like attribute bag -> (glp_circuit_desc, objects that must stay alive while it is used)."""
    gates = (_Gate * len(desc.gates))()
    for i, g in enumerate(desc.gates):
        for f, _ in _Gate._fields_:
            setattr(gates[i], f, int(g[f]))
    k, const, sig = _a(desc.k_is), _a(desc.constants), _a(desc.sigmas)
    # the C ABI takes bare pointers: every array's size is checked here so that a wrong shape is a GlpError, not a
    # host over-read
    n = 1 << int(desc.degree_bits)
    if k.size != int(desc.num_routed_wires):
        raise GlpError(-1, "k_is has %d entries, num_routed_wires is %d" % (k.size, desc.num_routed_wires))
    if const.size != int(desc.num_constants) * n:
        raise GlpError(-1, "constants has %d elements, expected num_constants * 2^degree_bits = %d" % (const.size, int(desc.num_constants) * n))
    if sig.size != int(desc.num_routed_wires) * n:
        raise GlpError(-1, "sigmas has %d elements, expected num_routed_wires * 2^degree_bits = %d" % (sig.size, int(desc.num_routed_wires) * n))
    if len(desc.reduction_arity_bits) > 16:
        raise GlpError(-1, "more than 16 FRI reductions")
    d = _CircuitDesc()
    for f in ("degree_bits", "num_wires", "num_routed_wires", "num_constants", "num_selectors", "num_challenges",
              "quotient_degree_factor", "num_partial_products", "num_gate_constraints", "rate_bits", "cap_height",
              "proof_of_work_bits", "num_query_rounds"):
        setattr(d, f, int(getattr(desc, f)))
    d.num_reductions = len(desc.reduction_arity_bits)
    for i, ab in enumerate(desc.reduction_arity_bits):
        d.reduction_arity_bits[i] = int(ab)
    d.num_gates, d.num_public_inputs = len(desc.gates), int(len(desc.public_inputs))
    d.gates = C.cast(gates, C.POINTER(_Gate))
    d.k_is, d.constants, d.sigmas = k.ctypes.data, const.ctypes.data, sig.ctypes.data
    dig = getattr(desc, "circuit_digest", None)
    if dig is not None:
        for i in range(4):
            d.circuit_digest[i] = int(dig[i])
    d.hasher = int(getattr(desc, "hasher", 0))
    return d, (gates, k, const, sig)


def write_circuit_file(path, desc, with_witness=True):
    """glp_circuit_file_write: the hand-off file a machine with the Rust builder produces (include/glp.h)."""
    d, keep = _desc_to_c(desc)
    w = pi = None
    if with_witness:
        w, pi = _a(desc.wires), _a(desc.public_inputs)
        if w.size != int(desc.num_wires) << int(desc.degree_bits):
            raise GlpError(-1, "wires has %d elements, expected num_wires * 2^degree_bits" % w.size)
    _chk(load_library().glp_circuit_file_write(os.fsencode(path), C.byref(d), _p(w) if w is not None else None,
                                               _p(pi) if (pi is not None and pi.size) else None))
    del keep


class _FileDesc:
    pass


class CircuitFile:
    """A mapped circuit hand-off file; `.desc` is an attribute bag `Circuit(ctx, cf.desc)` accepts (numpy views into the
    mapping, valid until close())."""

    def __init__(self, path, verify_checksum=True):
        L = load_library()
        self._h = C.c_void_p()
        _chk(L.glp_circuit_file_open(os.fsencode(path), 1 if verify_checksum else 0, C.byref(self._h)))
        cd = L.glp_circuit_file_desc(self._h).contents
        d = _FileDesc()
        for f in ("degree_bits", "num_wires", "num_routed_wires", "num_constants", "num_selectors", "num_challenges",
                  "quotient_degree_factor", "num_partial_products", "num_gate_constraints", "rate_bits", "cap_height",
                  "proof_of_work_bits", "num_query_rounds"):
            setattr(d, f, int(getattr(cd, f)))
        d.reduction_arity_bits = [int(cd.reduction_arity_bits[i]) for i in range(cd.num_reductions)]
        d.gates = [{f: int(getattr(cd.gates[i], f)) for f, _ in _Gate._fields_} for i in range(cd.num_gates)]
        n = 1 << d.degree_bits

        def view(ptr, shape):
            cnt = int(np.prod(shape))
            if not ptr or cnt == 0:
                return np.zeros(shape, np.uint64)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(cnt,)).reshape(shape)
        d.k_is = view(cd.k_is, (d.num_routed_wires,))
        d.constants = view(cd.constants, (d.num_constants, n))
        d.sigmas = view(cd.sigmas, (d.num_routed_wires, n))
        dig = [int(cd.circuit_digest[i]) for i in range(4)]
        d.circuit_digest = np.array(dig, np.uint64) if any(dig) else None
        d.hasher = int(cd.hasher)
        wp = L.glp_circuit_file_wires(self._h)
        self.has_witness = bool(wp)
        d.wires = view(wp, (d.num_wires, n)) if wp else None
        d.public_inputs = view(L.glp_circuit_file_public_inputs(self._h), (int(cd.num_public_inputs),)) if wp else \
            np.zeros(int(cd.num_public_inputs), np.uint64)
        self.desc = d

    def close(self):
        if getattr(self, "_h", None):
            self.desc = None
            load_library().glp_circuit_file_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Circuit:
    """Device-resident circuit data: what `builder.build::<C>()` hands the prover
    [REF src/ecdsa/gadgets/ecdsa.rs:298].  `desc` is an attribute bag like synth.Circuit."""

    def __init__(self, ctx, desc, programs=None):
        """programs: the gate programs that gates of type GATE_PROGRAM name in p0 (gate_program.Program objects, any bag
        gate_program_desc takes, or (glp_gate_program_desc, keep-alive) pairs as it returns them); given (an empty list too), the
        circuit is made by glp_circuit_create_prog."""
        L = load_library()
        self.ctx, self.desc = ctx, desc
        d, keep = _desc_to_c(desc)
        n = 1 << int(desc.degree_bits)
        self._wire_elems = int(desc.num_wires) * n
        self._num_pis = int(len(desc.public_inputs))
        self._h = C.c_void_p()
        self.zero_knowledge = bool(getattr(desc, "zero_knowledge", False))
        if programs is not None:
            pairs = [p if isinstance(p, tuple) else gate_program_desc(p) for p in programs]
            arr = (_GateProgramDesc * max(len(pairs), 1))(*[p[0] for p in pairs])
            _chk(L.glp_circuit_create_prog(ctx._h, C.byref(d), 1 if self.zero_knowledge else 0, arr if pairs else None, len(pairs), C.byref(self._h)))
            del pairs
        elif self.zero_knowledge:
            _chk(L.glp_circuit_create_ex(ctx._h, C.byref(d), 1, C.byref(self._h)))     # GLP_CIRCUIT_ZERO_KNOWLEDGE
        else:
            _chk(L.glp_circuit_create(ctx._h, C.byref(d), C.byref(self._h)))
        del keep
        self.proof_words = L.glp_proof_words(self._h)

    def free(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):                # never touch a handle whose context is already gone
                load_library().glp_circuit_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def digest(self):
        out = np.empty(4, np.uint64)
        _chk(load_library().glp_circuit_digest(self._h, _p(out)))
        return out

    def constants_sigmas_cap(self):
        out = np.empty((1 << self.desc.cap_height, 4), np.uint64)
        _chk(load_library().glp_circuit_constants_sigmas_cap(self._h, _p(out)))
        return out

    def prove(self, wires=None, public_inputs=None):
        """`data.prove(pw)` after witness generation: full witness in, proof words out (include/glp.h)."""
        w = _a(self.desc.wires if wires is None else wires)
        pi = _a(self.desc.public_inputs if public_inputs is None else public_inputs)
        self._check_witness(w, pi)
        proof = np.zeros(self.proof_words, np.uint64)
        _chk(load_library().glp_prove(self.ctx._h, self._h, _p(w), _p(pi) if pi.size else None, _p(proof)))
        return proof

    def _check_witness(self, w, pi):
        if w is not None and w.size != self._wire_elems:
            raise GlpError(-1, "wires has %d elements, expected num_wires * 2^degree_bits = %d" % (w.size, self._wire_elems))
        if pi.size != self._num_pis:
            raise GlpError(-1, "%d public inputs, the circuit has %d" % (pi.size, self._num_pis))

    def _check_proof(self, proof_words):
        a = _a(proof_words)
        if a.size != self.proof_words:
            raise GlpError(-1, "proof has %d words, a proof of this circuit has %d" % (a.size, self.proof_words))
        return a

    def verify(self, proof_words):
        """`data.verify(proof)`: True if accepted; raises nothing on rejection (reason: `last_error()`)."""
        L = load_library()
        a = _a(proof_words)
        rc = L.glp_verify_n(self._h, _p(a), a.size)
        if rc == 0:
            return True
        if rc == -5:          # GLP_ERR_PROVE: a well-formed call, the proof is rejected
            return False
        _chk(rc)

    def verify_batch(self, proofs, reasons=False):
        """glp_verify_batch: proofs [K][proof_words] -> bool array [K] (and the list of rejection reasons if asked); the query
        rounds of all proofs run in one launch on the GPU."""
        a = _a(proofs)
        if a.ndim != 2 or a.shape[1] != self.proof_words:
            raise GlpError(-1, "proofs must be [K][proof_words]")
        K = a.shape[0]
        status = np.zeros(K, np.int32)
        buf = C.create_string_buffer(K * 160) if reasons else None
        _chk(load_library().glp_verify_batch(self.ctx._h, self._h, K, _p(a), status.ctypes.data_as(C.c_void_p), buf))
        ok = status == 0
        if reasons:
            return ok, [buf.raw[160 * k:160 * (k + 1)].split(b"\0", 1)[0].decode() for k in range(K)]
        return ok

    def proof_to_bytes(self, proof_words):
        """`ProofWithPublicInputs::to_bytes()`."""
        L = load_library()
        n = L.glp_proof_bytes_len(self._h)
        out = np.empty(n, np.uint8)
        _chk(L.glp_proof_to_bytes(self._h, _p(self._check_proof(proof_words)), out.ctypes.data_as(C.c_void_p), n))
        return out.tobytes()

    def proof_from_bytes(self, data):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        words = np.zeros(self.proof_words, np.uint64)
        _chk(load_library().glp_proof_from_bytes(self._h, buf.ctypes.data_as(C.c_void_p), buf.size, _p(words)))
        return words

    def prove_batch(self, wires, public_inputs=None, out=None):
        """glp_prove_batch: wires [K][num_wires][n] (host array) -> proofs [K][proof_words] (into `out` if given: the library
        writes every word, so a caller that proves batch after batch can reuse one buffer)."""
        w = _a(wires)
        if w.ndim != 3 or w[0].size != self._wire_elems:
            raise GlpError(-1, "wires must be [K][num_wires][2^degree_bits]")
        K = w.shape[0]
        pi = _a(np.zeros((K, 0), np.uint64) if public_inputs is None else public_inputs).reshape(K, -1)
        if pi.shape[1] != self._num_pis:
            raise GlpError(-1, "%d public inputs per proof, the circuit has %d" % (pi.shape[1], self._num_pis))
        if out is None:
            out = np.empty((K, self.proof_words), np.uint64)
        elif out.dtype != np.uint64 or out.shape != (K, self.proof_words) or not out.flags.c_contiguous:
            raise GlpError(-1, "out must be a C-contiguous uint64 array [K][proof_words]")
        _chk(load_library().glp_prove_batch(self.ctx._h, self._h, K, _p(w), 0, _p(pi) if pi.size else None, _p(out)))
        return out

    def prove_batch_device(self, dev_wires_ptr, K, public_inputs=None):
        pi = _a(np.zeros((K, 0), np.uint64) if public_inputs is None else public_inputs).reshape(K, -1)
        if pi.shape[1] != self._num_pis:
            raise GlpError(-1, "%d public inputs per proof, the circuit has %d" % (pi.shape[1], self._num_pis))
        out = np.empty((K, self.proof_words), np.uint64)
        _chk(load_library().glp_prove_batch(self.ctx._h, self._h, K, C.c_void_p(dev_wires_ptr), 1, _p(pi) if pi.size else None, _p(out)))
        return out

    def witness_fill(self, dev_wires_ptr, only_advice=False):
        """Row-local witness generation in place on an HBM-resident witness (include/glp.h, glp_witness_fill)."""
        _chk(load_library().glp_witness_fill(self.ctx._h, self._h, C.c_void_p(dev_wires_ptr), 1 if only_advice else 0))

    def check_witness(self, wires=None, public_inputs=None, dev_wires_ptr=None, num_proofs=1, by_gate=False):
        """glp_witness_check: every gate constraint on the rows of H and every copy constraint of num_proofs witnesses
        ([num_proofs][num_wires][n]; host array, default desc.wires, or an HBM pointer).  Returns one WitnessReport (num_proofs == 1
        and a witness without a leading proof axis) or a list of them; with by_gate each report carries rows_failed_by_gate."""
        K = int(num_proofs)
        single = K == 1
        if dev_wires_ptr is None:
            w = _a(self.desc.wires if wires is None else wires)
            if w.ndim == 3:
                K, single = w.shape[0], False
            if w.size != K * self._wire_elems:
                raise GlpError(-1, "wires has %d elements, expected num_proofs * num_wires * 2^degree_bits = %d" % (w.size, K * self._wire_elems))
        pi = _a(self.desc.public_inputs if public_inputs is None and K == 1 else (np.zeros((K, 0), np.uint64) if public_inputs is None else public_inputs))
        if pi.size != K * self._num_pis:
            raise GlpError(-1, "%d public inputs, expected num_proofs * %d" % (pi.size, self._num_pis))
        ng = len(self.desc.gates)
        rep = (_WitnessReport * K)()
        rows = np.zeros((K, ng), np.uint64) if by_gate else None
        _chk(load_library().glp_witness_check(self.ctx._h, self._h, K, C.c_void_p(dev_wires_ptr) if dev_wires_ptr is not None else _p(w),
                                              0 if dev_wires_ptr is None else 1, _p(pi) if pi.size else None, rep, None if rows is None else _p(rows)))
        types = [int(g["type"]) for g in self.desc.gates]
        out = [WitnessReport(rep[k], types, None if rows is None else rows[k]) for k in range(K)]
        return out[0] if single else out

    def witness_columns(self, gate_index):
        """uint8 [num_wires]: 1 = written by witness_fill on rows of that gate, 2 = read as generator input, 0 = untouched."""
        out = np.zeros(int(self.desc.num_wires), np.uint8)
        _chk(load_library().glp_witness_columns(self._h, int(gate_index), out.ctypes.data_as(C.c_void_p)))
        return out

    def witness_units(self, gate_index):
        """The units of a row of that gate (include/glp.h, "witness generation, the dataflow half"): uint8 [num_units][num_wires], one
        row of glp_witness_unit_columns roles per unit (1 = written, 2 = read, 0 = untouched)."""
        L = load_library()
        nu = int(L.glp_witness_num_units(self._h, int(gate_index)))
        out = np.zeros((nu, int(self.desc.num_wires)), np.uint8)
        for u in range(nu):
            _chk(L.glp_witness_unit_columns(self._h, int(gate_index), u, out[u].ctypes.data_as(C.c_void_p)))
        return out

    def witness_plan(self, input_cells, free_units=None, moduli=None, programs=None, random_cells=None):
        """glp_witness_plan_create(_ex, _prog, _rand): input_cells = flat positions col * n + row of the cells the caller sets -> WitnessPlan.
        free_units = (units, cells): the generators that belong to no gate (include/glp.h, FREE UNITS) as a FREE_UNIT_DTYPE array
        (or anything np.asarray makes one of: rows of kind, modulus, cell_begin, len[6]) and the uint64 cells their runs point into;
        moduli = uint32 [num_moduli][8], little-endian limbs.  programs = the unit programs (witness_program.WitnessProgram, or any
        bag of code, pool, num_regs, num_inputs, num_outputs) that units of kind WGEN_PROGRAM name in their modulus field; given
        (an empty list too), the plan is made by glp_witness_plan_create_prog.  random_cells = flat positions of the cells that
        generate() fills from the PRF of include/glp.h (RANDOM CELLS: a built circuit's witness_random_cells); given (an empty list
        too), the plan is made by glp_witness_plan_create_rand."""
        cells = _a(input_cells).reshape(-1)
        h = C.c_void_p()
        if random_cells is not None:
            rnd = _a(random_cells).reshape(-1)
            if cells.size >= 1 << 32 or rnd.size >= 1 << 32:
                raise GlpError(-1, "input_cells or random_cells too long for a uint32 count")
            if free_units is None:
                if moduli is not None:
                    raise GlpError(-1, "moduli without free_units")
                if programs is not None:
                    raise GlpError(-1, "programs without free_units")
                free_units = (np.zeros(0, FREE_UNIT_DTYPE), np.zeros(0, np.uint64))
            if programs is None:
                programs = []
        if free_units is None:
            if moduli is not None:
                raise GlpError(-1, "moduli without free_units")
            if programs is not None:
                raise GlpError(-1, "programs without free_units")
            _chk(load_library().glp_witness_plan_create(self.ctx._h, self._h, _p(cells) if cells.size else None, cells.size, C.byref(h)))
        else:
            units, fcells = free_units
            units = np.ascontiguousarray(units)
            if units.dtype != FREE_UNIT_DTYPE:
                raw = np.ascontiguousarray(units, dtype=np.int64).reshape(-1, 9)
                if raw.size and (raw.min() < 0 or raw[:, :3].max() >= 1 << 32 or raw[:, 3:].max() >= 1 << 16):
                    raise GlpError(-1, "free_units: a field does not fit its C type (uint32 kind, modulus, cell_begin; uint16 len[6])")
                units = np.zeros(raw.shape[0], FREE_UNIT_DTYPE)
                units["kind"], units["modulus"], units["cell_begin"], units["len"] = raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3:]
            assert units.itemsize == C.sizeof(_WitnessFreeUnit) == 24
            fcells = _a(fcells).reshape(-1)
            mod = np.ascontiguousarray(np.zeros((0, 8)) if moduli is None else moduli, dtype=np.uint32)
            if mod.size % 8:
                raise GlpError(-1, "moduli has %d words, expected num_moduli * 8" % mod.size)
            if units.size >= 1 << 32 or mod.size // 8 >= 1 << 32:
                raise GlpError(-1, "free_units or moduli too long for a uint32 count")
            args = (self.ctx._h, self._h, _p(cells) if cells.size else None, cells.size, units.ctypes.data_as(C.c_void_p) if units.size else None,
                    units.size, _p(fcells) if fcells.size else None, fcells.size, mod.ctypes.data_as(C.c_void_p) if mod.size else None, mod.size // 8)
            if random_cells is not None:
                if len(programs) >= 1 << 32:
                    raise GlpError(-1, "programs too long for a uint32 count")
                descs, _keep = witness_program_descs(programs)
                _chk(load_library().glp_witness_plan_create_rand(*args[:4], _p(rnd) if rnd.size else None, rnd.size, *args[4:],
                                                                 descs if len(programs) else None, len(programs), C.byref(h)))
            elif programs is None:
                _chk(load_library().glp_witness_plan_create_ex(*args, C.byref(h)))
            else:
                if len(programs) >= 1 << 32:
                    raise GlpError(-1, "programs too long for a uint32 count")
                descs, _keep = witness_program_descs(programs)
                _chk(load_library().glp_witness_plan_create_prog(*args, descs if len(programs) else None, len(programs), C.byref(h)))
        plan = WitnessPlan(self, h, cells.size)
        self.ctx._plans.add(plan)
        return plan

    def read_cells(self, dev_wires_ptr, cells, K=1):
        """glp_witness_read_cells: the cells (flat positions) of K HBM-resident witnesses -> uint64 [K][len(cells)]."""
        cells = _a(cells).reshape(-1)
        out = np.empty((int(K), cells.size), np.uint64)
        _chk(load_library().glp_witness_read_cells(self.ctx._h, self._h, int(K), C.c_void_p(dev_wires_ptr), _p(cells), cells.size, _p(out)))
        return out

    def stage_witness(self, host_wires, routed_only=False):
        """glp_witness_stage: start uploading a witness on the context's copy stream ([num_wires][n], or with routed_only the routed
        columns [num_routed_wires][n] -- the advice columns are then derived on the GPU); returns a StagedWitness for prove_staged."""
        w = host_wires if (isinstance(host_wires, np.ndarray) and host_wires.dtype == np.uint64 and host_wires.flags.c_contiguous) else _a(host_wires)
        n = 1 << int(self.desc.degree_bits)
        need = (int(self.desc.num_routed_wires) if routed_only else int(self.desc.num_wires)) * n
        if w.size < need or (not routed_only and w.size != need):
            raise GlpError(-1, "staged witness has %d elements, expected %d" % (w.size, need))
        h = C.c_void_p()
        _chk(load_library().glp_witness_stage(self.ctx._h, self._h, _p(w), 1 if routed_only else 0, C.byref(h)))
        return StagedWitness(self, h, w)

    def prove_staged(self, staged, public_inputs=None):
        pi = _a(self.desc.public_inputs if public_inputs is None else public_inputs)
        self._check_witness(None, pi)
        proof = np.zeros(self.proof_words, np.uint64)
        _chk(load_library().glp_prove_staged(self.ctx._h, self._h, staged._h, _p(pi) if pi.size else None, _p(proof)))
        return proof

    def prove_device(self, dev_wires_ptr, public_inputs=None):
        pi = _a(self.desc.public_inputs if public_inputs is None else public_inputs)
        self._check_witness(None, pi)
        proof = np.zeros(self.proof_words, np.uint64)
        _chk(load_library().glp_prove_device(self.ctx._h, self._h, C.c_void_p(dev_wires_ptr), _p(pi) if pi.size else None,
                                             _p(proof)))
        return proof


class WitnessReport:
    """One witness's glp_witness_report (include/glp.h): the three counts, the first failing constraint in (row, constraint) order and the
    first failing copy in (row, column) order (None where the count is 0); rows_failed_by_gate if it was asked for."""
    FIELDS = ("failed_constraints", "failed_rows", "failed_copies", "row", "gate", "constraint", "value", "copy_row", "copy_col", "to_col",
              "to_row", "copy_value", "to_value")

    def __init__(self, c_report, gate_types=None, rows_failed_by_gate=None):
        for f in self.FIELDS:
            setattr(self, f, int(getattr(c_report, f)))
        if not self.failed_constraints:
            self.row = self.gate = self.constraint = self.value = None
        if not self.failed_copies:
            self.copy_row = self.copy_col = self.to_col = self.to_row = self.copy_value = self.to_value = None
        self.gate_type = gate_types[self.gate] if gate_types is not None and self.gate is not None else None
        self.rows_failed_by_gate = None if rows_failed_by_gate is None else [int(x) for x in rows_failed_by_gate]

    @property
    def ok(self):
        return self.failed_constraints == 0 and self.failed_rows == 0 and self.failed_copies == 0

    def as_tuple(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def __str__(self):
        if self.ok:
            return "witness satisfies the circuit"
        parts = []
        if self.failed_constraints:
            name = GATE_TYPE_NAMES.get(self.gate_type, "type %s" % self.gate_type)
            parts.append("row %d: gate %d (%s) constraint %d = 0x%x; %d failing rows" % (self.row, self.gate, name, self.constraint, self.value,
                                                                                     self.failed_rows))
        if self.failed_copies:
            parts.append("first broken copy (col %d, row %d) = 0x%x -> (col %d, row %d) = 0x%x; %d broken copies"
                         % (self.copy_col, self.copy_row, self.copy_value, self.to_col, self.to_row, self.to_value, self.failed_copies))
        return "; ".join(parts)


class WitnessPlan:
    """A glp_witness_plan (include/glp.h, "witness generation, the dataflow half"): which unit runs in which wave and which cell is
    copied from which, for one circuit and one set of input cells.  The circuit must outlive it; closing the context frees the plans
    made on it first (glp_witness_plan_free needs the context alive), so no order of free() and close() leaks the plan's host tables.
    One plan serves one generate() at a time."""
    INFO = ("num_waves", "num_units", "num_stuck_units", "num_copies", "num_cells_known", "widest_wave_units", "stuck_row", "stuck_gate",
            "stuck_unit")

    def __init__(self, circuit, handle, num_inputs):
        self.circuit, self._h, self.num_inputs = circuit, handle, int(num_inputs)

    @property
    def info(self):
        """dict of glp_witness_plan_info; the stuck_* fields are None unless num_stuck_units."""
        raw = _WitnessPlanInfo()
        _chk(load_library().glp_witness_plan_info(self._h, C.byref(raw)))
        out = {f: int(getattr(raw, f)) for f in self.INFO}
        if not out["num_stuck_units"]:
            out["stuck_row"] = out["stuck_gate"] = out["stuck_unit"] = None
        return out

    @property
    def free_info(self):
        """dict of glp_witness_plan_free_info; first_stuck_free_unit is None unless num_stuck_free_units."""
        raw = _WitnessPlanFreeInfo()
        _chk(load_library().glp_witness_plan_free_info(self._h, C.byref(raw)))
        out = {f: int(getattr(raw, f)) for f, _ in _WitnessPlanFreeInfo._fields_}
        if not out["num_stuck_free_units"]:
            out["first_stuck_free_unit"] = None
        return out

    @property
    def num_random(self):
        """glp_witness_plan_num_random: the cells generate() fills from the PRF."""
        return int(load_library().glp_witness_plan_num_random(self._h))

    def cell_waves(self):
        d = self.circuit.desc
        out = np.empty((int(d.num_wires), 1 << int(d.degree_bits)), np.int32)
        _chk(load_library().glp_witness_plan_cell_waves(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def generate(self, dev_ptr, inputs, K=1, zero_first=False):
        """glp_witness_generate: inputs [K][num_inputs] in the order of the plan's input cells -> K witnesses at dev_ptr
        ([K][num_wires][n] in HBM).  Asynchronous on the context's stream."""
        v = _a(inputs).reshape(-1)
        if v.size != int(K) * self.num_inputs:
            raise GlpError(-1, "inputs has %d elements, expected num_proofs * num_inputs = %d" % (v.size, int(K) * self.num_inputs))
        _chk(load_library().glp_witness_generate(self.circuit.ctx._h, self._h, int(K), _p(v) if v.size else None, C.c_void_p(dev_ptr),
                                                 1 if zero_first else 0))

    def free(self):
        if getattr(self, "_h", None):
            if getattr(self.circuit.ctx, "_h", None):
                load_library().glp_witness_plan_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class StagedWitness:
    """A witness on its way to (or in) HBM (glp_witness): keeps the host array alive until the upload has been consumed."""

    def __init__(self, circuit, handle, host_array):
        self.circuit, self._h, self._host = circuit, handle, host_array

    def free(self):
        if getattr(self, "_h", None):
            if getattr(self.circuit.ctx, "_h", None):
                load_library().glp_witness_free(self._h)
            self._h = None
            self._host = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Session:
    """One proof stepped by the caller's transcript (include/glp.h, glp_session_*): every method returns what the
    Rust prover's `Challenger` observes next and takes the challenges it draws next
    [UPSTREAM plonky2 plonk/prover.rs `prove_with_partition_witness`; reached from REF src/ecdsa/gadgets/ecdsa.rs:349]."""

    def __init__(self, circuit, wires=None, public_inputs=None, dev_wires_ptr=None):
        L = load_library()
        self.circuit, d = circuit, circuit.desc
        self._capn = 1 << d.cap_height
        pi = _a(d.public_inputs if public_inputs is None else public_inputs)
        self._h = C.c_void_p()
        self.wires_cap = np.empty((self._capn, 4), np.uint64)
        self.public_inputs_hash = np.empty(4, np.uint64)
        if dev_wires_ptr is not None:
            circuit._check_witness(None, pi)
            wp, on_dev = C.c_void_p(dev_wires_ptr), 1
        else:
            self._w = _a(d.wires if wires is None else wires)     # keep the host array alive
            circuit._check_witness(self._w, pi)
            wp, on_dev = _p(self._w), 0
        _chk(L.glp_session_begin(circuit.ctx._h, circuit._h, wp, on_dev, _p(pi) if pi.size else None, C.byref(self._h),
                                 _p(self.wires_cap), _p(self.public_inputs_hash)))

    def _cap(self, fn, *args):
        out = np.empty((self._capn, 4), np.uint64)
        _chk(fn(self._h, *args, _p(out)))
        return out

    def partial_products(self, betas, gammas):
        self._b, self._g = _a(betas), _a(gammas)
        return self._cap(load_library().glp_session_partial_products, _p(self._b), _p(self._g))

    def quotient(self, alphas):
        self._al = _a(alphas)
        return self._cap(load_library().glp_session_quotient, _p(self._al))

    def open(self, zeta):
        L = load_library()
        out = np.empty((L.glp_num_openings(self.circuit._h), 2), np.uint64)
        _chk(L.glp_session_open(self._h, _p(_a(zeta)), _p(out)))
        return out

    def fri_combine(self, alpha):
        _chk(load_library().glp_session_fri_combine(self._h, _p(_a(alpha))))

    def fri_commit(self):
        return self._cap(load_library().glp_session_fri_commit)

    def fri_fold(self, beta):
        _chk(load_library().glp_session_fri_fold(self._h, _p(_a(beta))))

    def fri_final_poly(self):
        L = load_library()
        out = np.empty((L.glp_final_poly_len(self.circuit._h), 2), np.uint64)
        _chk(L.glp_session_fri_final_poly(self._h, _p(out)))
        return out

    def pow_search(self, sponge_state, pending_inputs, bits):
        st, pend = _a(sponge_state), _a(pending_inputs)
        w = C.c_uint64()
        _chk(load_library().glp_pow_search_h(self.circuit.ctx._h, int(getattr(self.circuit.desc, "hasher", 0)), _p(st),
                                             _p(pend) if pend.size else None, pend.size, int(bits), C.byref(w)))
        return int(w.value)

    def queries(self, pow_witness, indices):
        idx = _a(indices)
        _chk(load_library().glp_session_queries(self._h, C.c_uint64(int(pow_witness)), _p(idx), idx.size))

    def proof(self):
        out = np.zeros(self.circuit.proof_words, np.uint64)
        _chk(load_library().glp_session_proof(self._h, _p(out)))
        return out

    def oracle(self, index):
        """glp_session_oracle: committed oracle 0..3 (constants_sigmas, wires, zs and partial products, quotient) as a Batch borrowed
        from this session: valid until end(), never freed by the Batch."""
        L = load_library()
        h = C.c_void_p()
        _chk(L.glp_session_oracle(self._h, int(index), C.byref(h)))
        nc, lg, rb, ch = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _chk(L.glp_batch_info(h, C.byref(nc), C.byref(lg), C.byref(rb), C.byref(ch)))
        return Batch(self.circuit.ctx, h, nc.value, lg.value, rb.value, ch.value, owner=self)

    def end(self):
        if getattr(self, "_h", None):
            if getattr(self.circuit.ctx, "_h", None):        # a session must not outlive its context: then it is only dropped
                load_library().glp_session_end(self._h)
            self._h = None

    def __del__(self):
        try:
            self.end()
        except Exception:
            pass


def _fri_desc_to_c(oracles, points, reduction_arity_bits, proof_of_work_bits, num_query_rounds):
    """(list of Batch, [(point (a, b), [(oracle, col_begin, num_cols), ...]), ...], FriParams) -> (glp_fri_desc, keep-alive objects)."""
    if len(reduction_arity_bits) > 16:
        raise GlpError(-1, "more than 16 FRI reductions")
    d = _FriDesc()
    handles = (C.c_void_p * max(1, len(oracles)))(*[b._h for b in oracles])
    pts = (_FriPoint * max(1, len(points)))()
    keep = [handles, pts, list(oracles)]
    for i, (z, ranges) in enumerate(points):
        rs = (_FriRange * max(1, len(ranges)))()
        for j, (o, cb, ncol) in enumerate(ranges):
            rs[j].oracle, rs[j].col_begin, rs[j].num_cols = int(o), int(cb), int(ncol)
        pts[i].point[0], pts[i].point[1] = int(z[0]), int(z[1])
        pts[i].num_ranges = len(ranges)
        pts[i].ranges = C.cast(rs, C.POINTER(_FriRange))
        keep.append(rs)
    d.num_oracles, d.oracles = len(oracles), C.cast(handles, C.POINTER(C.c_void_p))
    d.num_points, d.points = len(points), C.cast(pts, C.POINTER(_FriPoint))
    d.num_reductions = len(reduction_arity_bits)
    for i, ab in enumerate(reduction_arity_bits):
        d.reduction_arity_bits[i] = int(ab)
    d.proof_of_work_bits, d.num_query_rounds = int(proof_of_work_bits), int(num_query_rounds)
    return d, keep


class FriOpenings:
    """plonky2 `PolynomialBatch::prove_openings` and the openings themselves for caller-held batches, stepped by the caller's
    transcript (include/glp.h, glp_fri_*).  oracles: Batch objects of one context and shape; points: [((a, b), [(oracle, col_begin,
    num_cols), ...]), ...] = `FriInstanceInfo.batches`.  The batches are borrowed and must outlive this object."""

    def __init__(self, ctx, oracles, points, reduction_arity_bits, proof_of_work_bits, num_query_rounds):
        self.ctx = ctx
        d, self._keep = _fri_desc_to_c(oracles, points, reduction_arity_bits, proof_of_work_bits, num_query_rounds)
        self._capn = 1 << oracles[0].cap_height if oracles else 1
        self._h = C.c_void_p()
        _chk(load_library().glp_fri_begin(ctx._h, C.byref(d), C.byref(self._h)))

    @property
    def num_openings(self):
        return load_library().glp_fri_num_openings(self._h)

    def open(self):
        out = np.empty((self.num_openings, 2), np.uint64)
        _chk(load_library().glp_fri_open(self._h, _p(out)))
        return out

    def combine(self, alpha):
        _chk(load_library().glp_fri_combine(self._h, _p(_a(alpha))))

    def commit(self):
        out = np.empty((self._capn, 4), np.uint64)
        _chk(load_library().glp_fri_commit(self._h, _p(out)))
        return out

    def fold(self, beta):
        _chk(load_library().glp_fri_fold(self._h, _p(_a(beta))))

    def final_poly(self):
        L = load_library()
        out = np.empty((L.glp_fri_final_poly_len(self._h), 2), np.uint64)
        _chk(L.glp_fri_final_poly(self._h, _p(out)))
        return out

    def queries(self, pow_witness, indices):
        idx = _a(indices)
        _chk(load_library().glp_fri_queries(self._h, C.c_uint64(int(pow_witness)), _p(idx), idx.size))

    def proof(self):
        L = load_library()
        out = np.zeros(L.glp_fri_proof_words(self._h), np.uint64)
        _chk(L.glp_fri_proof(self._h, _p(out)))
        return out

    def end(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                load_library().glp_fri_end(self._h)
            self._h = None
            self._keep = None

    def __del__(self):
        try:
            self.end()
        except Exception:
            pass


def fri_proof_words(oracles, reduction_arity_bits, num_query_rounds):
    """words of the FriProof glp_fri_proof / glp_fri_prove write for these oracles (layout: include/glp.h)"""
    b = oracles[0]
    lg_n = b.log_n + b.rate_bits
    q = sum(o.leaf_len + 4 * (lg_n - b.cap_height) for o in oracles)
    lg = lg_n
    for ab in reduction_arity_bits:
        lg -= ab
        q += (2 << ab) + 4 * (lg - b.cap_height)
    return (4 << b.cap_height) * len(reduction_arity_bits) + q * num_query_rounds + (2 << (lg - b.rate_bits)) + 1


def fri_prove(ctx, oracles, points, reduction_arity_bits, proof_of_work_bits, num_query_rounds, sponge_state, pending_inputs=()):
    """glp_fri_prove: the whole of FriOpenings driven by the library's transcript, resumed from the caller's duplex sponge
    (12 state words + fewer than 8 buffered inputs) right after it observed the openings.  Returns (openings [count][2], proof words)."""
    d, keep = _fri_desc_to_c(oracles, points, reduction_arity_bits, proof_of_work_bits, num_query_rounds)
    st, pend = _a(sponge_state), _a(list(pending_inputs))
    if st.size != 12 or pend.size >= 8:
        raise GlpError(-1, "the sponge state is 12 words with fewer than 8 pending inputs")
    nopen = sum(int(nc) for _, ranges in points for _, _, nc in ranges)
    openings = np.zeros((max(nopen, 1), 2), np.uint64)
    proof = np.zeros(fri_proof_words(oracles, reduction_arity_bits, num_query_rounds) if oracles else 1, np.uint64)
    _chk(load_library().glp_fri_prove(ctx._h, C.byref(d), _p(st), _p(pend) if pend.size else None, pend.size, _p(openings), _p(proof)))
    del keep
    return openings[:nopen], proof


class FriOpeningsMany:
    """FriOpenings for num_proofs proofs of one instance in lock step (glp_fri_begin_many).  oracles: Batch objects, each with
    num_proofs members (Context.batch_many_from_*) or with one (shared by all proofs); points: the ranges as for FriOpenings, their
    (a, b) ignored; zs [num_proofs][len(points)][2]: every proof's own points.  Every step takes and returns arrays with a leading
    [num_proofs]."""

    def __init__(self, ctx, oracles, points, zs, reduction_arity_bits, proof_of_work_bits, num_query_rounds):
        self.ctx = ctx
        d, self._keep = _fri_desc_to_c(oracles, points, reduction_arity_bits, proof_of_work_bits, num_query_rounds)
        z = None if zs is None else _a(zs)
        self.num_proofs = 0 if z is None else (z.shape[0] if z.ndim == 3 else -1)
        if z is not None and (z.ndim != 3 or z.shape[1:] != (len(points), 2)):
            raise GlpError(-1, "zs is [num_proofs][%d][2]" % len(points))
        self._capn = 1 << oracles[0].cap_height if oracles else 1
        self._h = C.c_void_p()
        _chk(load_library().glp_fri_begin_many(ctx._h, C.byref(d), self.num_proofs, None if z is None or z.size == 0 else _p(z), C.byref(self._h)))
        self._nq = int(num_query_rounds)

    @property
    def num_openings(self):
        return load_library().glp_fri_num_openings(self._h)

    def open(self):
        out = np.empty((self.num_proofs, self.num_openings, 2), np.uint64)
        _chk(load_library().glp_fri_open(self._h, _p(out)))
        return out

    def _ext(self, x, what):
        a = _a(x)
        if a.shape != (self.num_proofs, 2):
            raise GlpError(-1, "%s is [num_proofs][2]" % what)
        return a

    def combine(self, alphas):
        _chk(load_library().glp_fri_combine(self._h, _p(self._ext(alphas, "alphas"))))

    def commit(self):
        out = np.empty((self.num_proofs, self._capn, 4), np.uint64)
        _chk(load_library().glp_fri_commit(self._h, _p(out)))
        return out

    def fold(self, betas):
        _chk(load_library().glp_fri_fold(self._h, _p(self._ext(betas, "betas"))))

    def final_poly(self):
        L = load_library()
        out = np.empty((self.num_proofs, L.glp_fri_final_poly_len(self._h), 2), np.uint64)
        _chk(L.glp_fri_final_poly(self._h, _p(out)))
        return out

    def queries(self, pow_witnesses, indices):
        w, idx = _a(pow_witnesses), _a(indices)
        if w.shape != (self.num_proofs,) or idx.shape != (self.num_proofs, self._nq):
            raise GlpError(-1, "pow_witnesses is [num_proofs], indices [num_proofs][num_query_rounds]")
        _chk(load_library().glp_fri_queries_many(self._h, _p(w), _p(idx)))

    def proof(self):
        L = load_library()
        out = np.zeros((self.num_proofs, L.glp_fri_proof_words(self._h)), np.uint64)
        _chk(L.glp_fri_proof(self._h, _p(out)))
        return out

    def end(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                load_library().glp_fri_end(self._h)
            self._h = None
            self._keep = None

    def __del__(self):
        try:
            self.end()
        except Exception:
            pass


def fri_prove_many(ctx, oracles, points, zs, reduction_arity_bits, proof_of_work_bits, num_query_rounds, sponge_states, pending_inputs=None):
    """glp_fri_prove_many: num_proofs proofs of one instance in lock step, each resumed from its own duplex sponge (sponge_states
    [num_proofs][12], pending_inputs [num_proofs][num_pending], num_pending < 8).  Returns (openings [num_proofs][count][2], FriProof
    words [num_proofs][words])."""
    d, keep = _fri_desc_to_c(oracles, points, reduction_arity_bits, proof_of_work_bits, num_query_rounds)
    z = _a(zs)
    if z.ndim != 3 or z.shape[1:] != (len(points), 2):
        raise GlpError(-1, "zs is [num_proofs][%d][2]" % len(points))
    K = z.shape[0]
    st = _a(sponge_states)
    pend = np.zeros((K, 0), np.uint64) if pending_inputs is None else _a(pending_inputs)
    pend = pend.reshape(K, pend.size // max(K, 1))
    if st.shape != (K, 12) or pend.shape[1] >= 8:
        raise GlpError(-1, "sponge_states is [num_proofs][12], with fewer than 8 pending inputs per proof")
    nopen = sum(int(nc) for _, ranges in points for _, _, nc in ranges)
    openings = np.zeros((K, max(nopen, 1), 2), np.uint64)
    proofs = np.zeros((K, fri_proof_words(oracles, reduction_arity_bits, num_query_rounds) if oracles else 1), np.uint64)
    _chk(load_library().glp_fri_prove_many(ctx._h, C.byref(d), K, _p(z) if z.size else None, _p(st), _p(pend) if pend.size else None,
                                           pend.shape[1], _p(openings), _p(proofs)))
    del keep
    return openings[:, :nopen], proofs


# ------------------------------------------------------------------ verifying FriProofs of caller-held instances (glp_fri_verify*)
def _fri_verify_desc_to_c(shapes, points, log_n, rate_bits, cap_height, hasher, reduction_arity_bits, proof_of_work_bits, num_query_rounds,
                          num_proofs=1):
    """shapes: per oracle a (num_cols, salted, shared) triple or a live Batch (its shape; shared = it has one member and num_proofs is
    larger); points as for FriOpenings.  A geometry argument left None is taken from the first Batch.  -> (glp_fri_verify_desc, keep)"""
    if len(reduction_arity_bits) > 16:
        raise GlpError(-1, "more than 16 FRI reductions")
    first = next((s for s in shapes if isinstance(s, Batch)), None)
    geo = []
    for name, v in (("log_n", log_n), ("rate_bits", rate_bits), ("cap_height", cap_height)):
        if v is None and first is None:
            raise GlpError(-1, "%s is needed when no oracle is given as a Batch" % name)
        geo.append(int(getattr(first, name) if v is None else v))
    sh = (_FriOracleShape * max(1, len(shapes)))()
    for i, s in enumerate(shapes):
        if isinstance(s, Batch):
            sh[i].num_cols, sh[i].salted, sh[i].shared = s.ncols, int(s.leaf_len != s.ncols), int(s.num_proofs == 1 and num_proofs > 1)
        else:
            sh[i].num_cols, sh[i].salted, sh[i].shared = int(s[0]), int(bool(s[1])), int(bool(s[2]))
    fd, keep = _fri_desc_to_c([], points, reduction_arity_bits, proof_of_work_bits, num_query_rounds)
    d = _FriVerifyDesc()
    d.num_oracles, d.oracles = len(shapes), C.cast(sh, C.POINTER(_FriOracleShape))
    d.log_n, d.rate_bits, d.cap_height = geo
    d.hasher = int(getattr(first, "hasher", 0) if hasher is None else hasher)
    d.num_points, d.points = fd.num_points, fd.points
    d.num_reductions, d.proof_of_work_bits, d.num_query_rounds = fd.num_reductions, fd.proof_of_work_bits, fd.num_query_rounds
    for i in range(16):
        d.reduction_arity_bits[i] = fd.reduction_arity_bits[i]
    return d, keep + [sh, fd]


def fri_verify_sizes(shapes, points, reduction_arity_bits, proof_of_work_bits, num_query_rounds, log_n=None, rate_bits=None, cap_height=None,
                     hasher=None):
    """(glp_fri_verify_proof_words, glp_fri_verify_num_openings) of the description; (0, 0) for one the verifier refuses"""
    d, keep = _fri_verify_desc_to_c(shapes, points, log_n, rate_bits, cap_height, hasher, reduction_arity_bits, proof_of_work_bits, num_query_rounds)
    L = load_library()
    out = int(L.glp_fri_verify_proof_words(C.byref(d))), int(L.glp_fri_verify_num_openings(C.byref(d)))
    del keep
    return out


def _fri_verify_call(ctx, shapes, points, zs, reduction_arity_bits, proof_of_work_bits, num_query_rounds, openings, proofs, caps, geometry, tail):
    """shared marshalling of the two many-proof forms; tail(K, d) -> (C function, arguments between proofs and status_out, keep-alive)"""
    L = load_library()
    z = _a(zs)
    if z.ndim != 3 or z.shape[1:] != (len(points), 2):
        raise GlpError(-1, "zs is [num_proofs][%d][2]" % len(points))
    K = z.shape[0]
    d, keep = _fri_verify_desc_to_c(shapes, points, *geometry, reduction_arity_bits, proof_of_work_bits, num_query_rounds, num_proofs=K)
    words, nopen = int(L.glp_fri_verify_proof_words(C.byref(d))), int(L.glp_fri_verify_num_openings(C.byref(d)))
    capn = 1 << int(d.cap_height)
    if caps is None:
        if not all(isinstance(s, Batch) for s in shapes):
            raise GlpError(-1, "caps is needed unless every oracle is given as a Batch")
        caps = [s.caps() for s in shapes]
    cs = [_a(cp) for cp in caps]
    if len(cs) != len(shapes):
        raise GlpError(-1, "%d caps for %d oracles" % (len(cs), len(shapes)))
    for i, cp in enumerate(cs):
        want = capn * 4 * (1 if d.oracles[i].shared else K)
        if words and cp.size != want:
            raise GlpError(-1, "caps[%d] has %d words, expected %d" % (i, cp.size, want))
    op, pr = _a(openings), _a(proofs)
    if words and (pr.size != K * words or op.size != K * nopen * 2):      # a bad description (words == 0) is the library's to name
        raise GlpError(-1, "proofs is [num_proofs][%d] and openings [num_proofs][%d][2] for this instance" % (words, nopen))
    cap_ptrs = (C.c_void_p * max(1, len(cs)))(*[cp.ctypes.data for cp in cs])
    fn, mid, keep2 = tail(K, d)
    status = np.zeros(max(K, 1), np.int32)
    buf = C.create_string_buffer(max(K, 1) * 160)
    _chk(fn(ctx._h, C.byref(d), K, _p(z) if z.size else None, cap_ptrs, _p(op) if op.size else None, _p(pr) if pr.size else None, *mid,
            status.ctypes.data_as(C.c_void_p), buf))
    del keep, keep2
    return status[:K], [buf.raw[160 * k:160 * (k + 1)].split(b"\0", 1)[0].decode() for k in range(K)]


def fri_verify_many(ctx, shapes, points, zs, reduction_arity_bits, proof_of_work_bits, num_query_rounds, openings, proofs, sponge_states,
                    pending_inputs=None, caps=None, log_n=None, rate_bits=None, cap_height=None, hasher=None):
    """glp_fri_verify_many: num_proofs FriProofs of one instance checked in one launch, each transcript resumed from its own duplex
    sponge as in fri_prove_many.  shapes: (num_cols, salted, shared) triples (then caps and the geometry are needed) or live Batch
    objects (shape and caps() taken from them); zs [num_proofs][len(points)][2]; openings [num_proofs][count][2]; proofs
    [num_proofs][words].  Returns (status [num_proofs] int32: 0 accepted, -5 rejected; reasons [num_proofs] str ending in "[check N]")."""
    def tail(K, d):
        st = _a(sponge_states)
        pend = np.zeros((K, 0), np.uint64) if pending_inputs is None else _a(pending_inputs)
        pend = pend.reshape(K, pend.size // max(K, 1))
        if st.shape != (K, 12):
            raise GlpError(-1, "sponge_states is [num_proofs][12]")
        return load_library().glp_fri_verify_many, (_p(st), _p(pend) if pend.size else None, pend.shape[1]), (st, pend)
    return _fri_verify_call(ctx, shapes, points, zs, reduction_arity_bits, proof_of_work_bits, num_query_rounds, openings, proofs, caps,
                            (log_n, rate_bits, cap_height, hasher), tail)


def fri_verify_queries_many(ctx, shapes, points, zs, reduction_arity_bits, proof_of_work_bits, num_query_rounds, openings, proofs, alphas, betas,
                            indices, caps=None, log_n=None, rate_bits=None, cap_height=None, hasher=None):
    """glp_fri_verify_queries_many: the same checks under the caller's own Fiat-Shamir: alphas [num_proofs][2], betas
    [num_proofs][num_reductions][2], indices [num_proofs][num_query_rounds]; the caller has checked the proof of work."""
    def tail(K, d):
        al, be, ix = _a(alphas), _a(betas), _a(indices)
        if al.size != 2 * K or be.size != 2 * K * len(reduction_arity_bits) or ix.size != K * int(num_query_rounds):
            raise GlpError(-1, "alphas is [num_proofs][2], betas [num_proofs][num_reductions][2], indices [num_proofs][num_query_rounds]")
        return load_library().glp_fri_verify_queries_many, (_p(al), _p(be) if be.size else None, _p(ix) if ix.size else None), (al, be, ix)
    return _fri_verify_call(ctx, shapes, points, zs, reduction_arity_bits, proof_of_work_bits, num_query_rounds, openings, proofs, caps,
                            (log_n, rate_bits, cap_height, hasher), tail)


def fri_verify(ctx, shapes, points, reduction_arity_bits, proof_of_work_bits, num_query_rounds, openings, proof, sponge_state, pending_inputs=(),
               caps=None, log_n=None, rate_bits=None, cap_height=None, hasher=None):
    """glp_fri_verify: one FriProof at the points' own (a, b).  True if accepted, False if rejected (reason: glp_last_error, ending in
    "[check N]"); GlpError for a call the library refuses."""
    L = load_library()
    d, keep = _fri_verify_desc_to_c(shapes, points, log_n, rate_bits, cap_height, hasher, reduction_arity_bits, proof_of_work_bits, num_query_rounds)
    words, nopen = int(L.glp_fri_verify_proof_words(C.byref(d))), int(L.glp_fri_verify_num_openings(C.byref(d)))
    if caps is None:
        if not all(isinstance(s, Batch) for s in shapes):
            raise GlpError(-1, "caps is needed unless every oracle is given as a Batch")
        caps = [s.cap() for s in shapes]
    cs = [_a(cp) for cp in caps]
    if len(cs) != len(shapes) or (words and any(cp.size != 4 << int(d.cap_height) for cp in cs)):
        raise GlpError(-1, "caps is one [2^cap_height][4] array per oracle")
    op, pr, st, pend = _a(openings), _a(proof), _a(sponge_state), _a(list(pending_inputs))
    if st.size != 12 or (words and (pr.size != words or op.size != 2 * nopen)):
        raise GlpError(-1, "proof has %d words and %d openings for this instance; the sponge state is 12 words" % (words, nopen))
    cap_ptrs = (C.c_void_p * max(1, len(cs)))(*[cp.ctypes.data for cp in cs])
    rc = L.glp_fri_verify(ctx._h, C.byref(d), cap_ptrs, _p(op) if op.size else None, _p(pr) if pr.size else None, _p(st),
                          _p(pend) if pend.size else None, pend.size)
    del keep
    if rc == 0:
        return True
    if rc == -5:
        return False
    _chk(rc)
