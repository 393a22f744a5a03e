"""Field words >= p at the library's inputs: the arrays the tests feed (single / pairs / twin) and the inventory of every `uint64_t *`
parameter of include/glp.h.

The rule (glp.h, conventions paragraph): a HOST array of field elements with a word >= p is refused by name (GLP_ERR_ARG, before any
launch); a DEVICE array is reduced mod p once as it is loaded, so every result is word for word the result for `input % p`.

FIELD_INPUTS lists each field-element parameter with where it may live, what happens to a word >= p and the test that pins it;
NOT_FIELD lists every other pointer parameter with the reason.  tests/test_field_input_inventory.py holds both against the prototypes."""
import os
import re

import numpy as np

P = 0xFFFFFFFF00000001
NC = (P, P + 1, P + 0x7FFFFFFF, 2 ** 64 - 2, 2 ** 64 - 1)                 # the words >= p the tests place
SMALL = (0, 1, 2, 0xFFFF, 1 << 31, (1 << 32) - 2)                         # words whose lift by p still fits 64 bits
PAIRS = ((0, 2 ** 64 - 1), (2 ** 64 - 1, 2 ** 64 - 1), (P, 0))            # partners of one butterfly: sub(0, 2^64 - 1) and add(2^64 - 1, 2^64 - 1) go wrong in glf.h


def base(seed, shape):
    """seeded canonical words, uniform on [0, p) up to 2^-32"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 63, shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, shape, dtype=np.uint64)) % np.uint64(P)


def reduced(arr):
    return np.asarray(arr, np.uint64) % np.uint64(P)


def twin(seed, shape):
    """(array, A): A is canonical with exactly ceil(half) of its words from SMALL at seeded places; of the words below 2^32 - 1 exactly
    ceil(half), again seeded, are lifted by p in `array`.  So array % p == A and at least a quarter of the words are >= p, by
    construction."""
    rng = np.random.default_rng(seed)
    A = base(seed + 1, shape).reshape(-1)
    order = rng.permutation(A.size)
    small = order[:(A.size + 1) // 2]
    A[small] = np.asarray(SMALL, np.uint64)[rng.integers(0, len(SMALL), small.size)]
    low = np.flatnonzero(A < np.uint64((1 << 32) - 1))
    lift = rng.permutation(low)[:(low.size + 1) // 2]
    arr = A.copy()
    arr[lift] += np.uint64(P)
    return arr.reshape(shape), A.reshape(shape)


def check_twin(arr, A):
    arr, A = np.asarray(arr, np.uint64), np.asarray(A, np.uint64)
    assert (A < np.uint64(P)).all() and (reduced(arr) == A).all()
    assert 5 * int((arr >= np.uint64(P)).sum()) >= arr.size, "fewer than 1/5 of the words are >= p"


def single_positions(seed, size):
    """flat positions of the single cases: first, last, one seeded in between (fewer for arrays of one or two words)"""
    pos = [0, size - 1]
    if size > 2:
        pos.append(1 + int(np.random.default_rng(seed).integers(0, size - 2)))
    return sorted(set(pos))


def single(seed, shape, word, flat_pos):
    """(array, A): a canonical array with `word` at one flat position; A = array % p"""
    arr = base(seed, shape).reshape(-1)
    arr[flat_pos] = np.uint64(word)
    return arr.reshape(shape), reduced(arr).reshape(shape)


def pairs(seed, shape):
    """(array, A) for [..][n] columns, n >= 2: each kind of PAIRS sits once on the partners of the first butterfly (i, i + n/2) and once
    on an adjacent pair (2j, 2j + 1), kind k in column k mod ncols, at seeded places that do not collide within a column"""
    n = shape[-1]
    assert n >= 2
    rng = np.random.default_rng(seed)
    arr = base(seed + 7, shape).reshape(-1, n)
    used = [set() for _ in range(arr.shape[0])]
    placed = 0
    for k, (a, b) in enumerate(PAIRS):
        col = k % arr.shape[0]
        for spots in ([(i, i + n // 2) for i in rng.permutation(n // 2)], [(2 * j, 2 * j + 1) for j in rng.permutation(n // 2)]):
            for x, y in spots:
                if x not in used[col] and y not in used[col]:
                    arr[col, x], arr[col, y] = np.uint64(a), np.uint64(b)
                    used[col].update((x, y))
                    placed += 1
                    break
    assert placed >= min(3, arr.shape[0])
    return arr.reshape(shape), reduced(arr).reshape(shape)


# ------------------------------------------------------------------------------------------ the inventory
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glp.h")


def pointer_parameters(header=HEADER):
    """[(function, parameter)] for every `uint64_t *`, `uint64_t *const *` and `uint64_t x[k]` parameter of every GLP_API prototype"""
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    out = []
    for m in re.finditer(r"GLP_API\s+[^;{(]*?\b(glp_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        for par in m.group(2).split(","):
            par = " ".join(par.split())
            pm = re.match(r"(?:const )?uint64_t \*(?:const \*)?\s*(\w+)$", par) or re.match(r"(?:const )?uint64_t (\w+)\[\d+\]$", par)
            if pm:
                out.append((m.group(1), pm.group(1)))
    return out


NEW = "test_gpu_noncanonical_inputs.py::"
_T = {      # the tests that pin a row
    "prim": NEW + "test_in_place_primitives_refuse",
    "commit_host": NEW + "test_commitments_refuse_host_words",
    "perm_host": NEW + "test_perm_seam_refuses_host_words",
    "prover_host": NEW + "test_prover_refuses_host_words",
    "commit": NEW + "test_from_values_device",
    "coeffs": NEW + "test_from_coeffs_device",
    "many": NEW + "test_many_from_values_on_device",
    "many_co": NEW + "test_many_from_coeffs_on_device",
    "coset": NEW + "test_from_coset_values_on_device",
    "prove": NEW + "test_prove_device",
    "batch": NEW + "test_prove_batch_on_device",
    "session": NEW + "test_session_on_device",
    "perm": NEW + "test_perm_zs_commit_on_device",
    "fill": NEW + "test_witness_fill",
    "seeds": NEW + "test_seed_words_are_taken_mod_p",
    "pow": NEW + "test_pow_witness_is_refused",
    "session_steps": NEW + "test_session_challenges_are_refused",
}
REFUSE, REDUCE = "refuse", "reduce"
# (function, parameter, where the array may live, a word >= p is ..., the test that pins it)
# An `either` row of the new file names the test of its device side; the host side of the same parameter is swept by the *_refuse_host_words
# test of its group (commitments, permutation seam, prover).
FIELD_INPUTS = [
    ("glp_ctx_set_salt_seed", "seed", "host", REDUCE, _T["seeds"]),
    ("glp_poseidon_permute", "states", "host", REFUSE, _T["prim"]),
    ("glp_fft", "cols", "host", REFUSE, _T["prim"]),
    ("glp_ifft", "cols", "host", REFUSE, _T["prim"]),
    ("glp_coset_ifft", "cols", "host", REFUSE, _T["prim"]),
    ("glp_lde", "coeffs", "host", REFUSE, _T["prim"]),
    ("glp_batch_from_values", "values", "host", REFUSE, _T["commit_host"]),
    ("glp_batch_from_values_h", "values", "host", REFUSE, _T["commit_host"]),
    ("glp_batch_from_values_salted", "values", "host", REFUSE, _T["commit_host"]),
    ("glp_batch_from_values_salted", "seed", "host", REDUCE, _T["seeds"]),
    ("glp_batch_from_coeffs", "coeffs", "host", REFUSE, _T["commit_host"]),
    ("glp_batch_from_coeffs_h", "coeffs", "host", REFUSE, _T["commit_host"]),
    ("glp_batch_from_values_device", "dev_values", "device", REDUCE, _T["commit"]),
    ("glp_batch_from_coeffs_device", "dev_coeffs", "device", REDUCE, _T["coeffs"]),
    ("glp_batch_many_from_values", "values", "either", "refuse / reduce", _T["many"]),
    ("glp_batch_many_from_values", "seed", "host", REDUCE, _T["seeds"]),
    ("glp_batch_many_from_coeffs", "coeffs", "either", "refuse / reduce", _T["many_co"]),
    ("glp_batch_many_from_coeffs", "seed", "host", REDUCE, _T["seeds"]),
    ("glp_batch_from_coset_values", "values", "either", "refuse / reduce", _T["coset"]),
    ("glp_batch_from_coset_values", "seed", "host", REDUCE, _T["seeds"]),
    ("glp_perm_zs_commit", "wires", "either", "refuse / reduce", _T["perm"]),
    ("glp_perm_zs_commit", "sigmas", "either", "refuse / reduce", _T["perm"]),
    ("glp_perm_zs_commit", "betas", "host", REFUSE, "test_gpu_perm_seam.py::test_refusals"),
    ("glp_perm_zs_commit", "gammas", "host", REFUSE, "test_gpu_perm_seam.py::test_refusals"),
    ("glp_perm_zs_commit", "seed", "host", REDUCE, _T["seeds"]),
    ("glp_perm_quotient_values", "betas", "host", REFUSE, "test_gpu_perm_seam.py::test_refusals"),
    ("glp_perm_quotient_values", "gammas", "host", REFUSE, "test_gpu_perm_seam.py::test_refusals"),
    ("glp_perm_quotient_values", "alphas", "host", REFUSE, "test_gpu_perm_seam.py::test_refusals"),
    ("glp_perm_quotient_values", "gate_sums", "either", "refuse / reduce", NEW + "test_perm_quotient_gate_sums"),
    ("glp_gate_program_sums", "alphas", "host", REFUSE, "test_gpu_gate_program.py::test_refusals"),
    ("glp_gate_program_sums", "params", "host", REFUSE, "test_gpu_gate_program.py::test_refusals"),
    ("glp_gate_program_eval_ext", "points", "either", "refuse / reduce", "test_gpu_zeta_check.py::test_eval_ext_refusals"),
    ("glp_gate_program_eval_ext", "alphas", "host", REFUSE, "test_gpu_zeta_check.py::test_eval_ext_refusals"),
    ("glp_gate_program_eval_ext", "params", "host", REFUSE, "test_gpu_zeta_check.py::test_eval_ext_refusals"),
    ("glp_perm_check_zeta", "zetas", "either", "refuse / reduce", "test_gpu_zeta_check.py::test_perm_check_zeta_refusals"),
    ("glp_perm_check_zeta", "betas", "host", REFUSE, "test_gpu_zeta_check.py::test_perm_check_zeta_refusals"),
    ("glp_perm_check_zeta", "gammas", "host", REFUSE, "test_gpu_zeta_check.py::test_perm_check_zeta_refusals"),
    ("glp_perm_check_zeta", "alphas", "host", REFUSE, "test_gpu_zeta_check.py::test_perm_check_zeta_refusals"),
    ("glp_perm_check_zeta", "gate_sums", "either", "refuse / reduce", "test_gpu_zeta_check.py::test_perm_check_zeta_refusals"),
    ("glp_gate_program_rows", "inputs", "either", "refuse / reduce", "test_gpu_trace_program.py::test_refusals"),
    ("glp_gate_program_rows", "params", "host", REFUSE, "test_gpu_trace_program.py::test_refusals"),
    ("glp_running_columns", "nums", "either", "refuse / reduce", "test_gpu_running_columns.py::test_refusals"),
    ("glp_running_columns", "dens", "either", "refuse / reduce", "test_gpu_running_columns.py::test_refusals"),
    ("glp_fri_combine", "alpha", "host", REFUSE, "test_gpu_fri_openings.py::test_steps_out_of_order"),
    ("glp_fri_fold", "beta", "host", REFUSE, "test_gpu_fri_openings.py::test_steps_out_of_order"),
    ("glp_fri_prove", "sponge_state", "host", REFUSE, "test_gpu_pow_search.py::test_refusals"),
    ("glp_fri_prove", "pending_inputs", "host", REFUSE, "test_gpu_pow_search.py::test_refusals"),
    ("glp_fri_begin_many", "points", "host", REFUSE, "test_gpu_fri_many.py::test_refusals"),
    ("glp_fri_queries_many", "pow_witnesses", "host", REFUSE, _T["pow"]),
    ("glp_pow_search_many", "sponge_states", "host", REFUSE, "test_gpu_pow_search.py::test_refusals"),
    ("glp_pow_search_many", "pending_inputs", "host", REFUSE, "test_gpu_pow_search.py::test_refusals"),
    ("glp_fri_prove_many", "points", "host", REFUSE, "test_gpu_fri_many.py::test_refusals"),
    ("glp_fri_prove_many", "sponge_states", "host", REFUSE, "test_gpu_pow_search.py::test_refusals"),
    ("glp_fri_prove_many", "pending_inputs", "host", REFUSE, "test_gpu_pow_search.py::test_refusals"),
    ("glp_fri_verify_queries_many", "alphas", "host", REFUSE, "test_gpu_fri_verify.py::test_refusals"),
    ("glp_fri_verify_queries_many", "betas", "host", REFUSE, "test_gpu_fri_verify.py::test_refusals"),
    ("glp_circuit_file_write", "wires", "host", REFUSE, "test_circuit_file.py::test_the_writer_refuses_a_word_that_is_no_field_element"),
    ("glp_circuit_file_write", "public_inputs", "host", REFUSE, "test_circuit_file.py::test_the_writer_refuses_a_word_that_is_no_field_element"),
    ("glp_prove", "wires", "host", REFUSE, _T["prover_host"]),
    ("glp_prove", "public_inputs", "host", REFUSE, _T["prover_host"]),
    ("glp_prove_device", "dev_wires", "device", REDUCE, _T["prove"]),
    ("glp_prove_device", "public_inputs", "host", REFUSE, _T["prover_host"]),
    ("glp_witness_stage", "host_wires", "host", REFUSE, _T["prover_host"]),
    ("glp_prove_staged", "public_inputs", "host", REFUSE, _T["prover_host"]),
    ("glp_prove_batch", "wires", "either", "refuse / reduce", _T["batch"]),
    ("glp_prove_batch", "public_inputs", "host", REFUSE, _T["prover_host"]),
    ("glp_witness_fill", "dev_wires", "device", REDUCE, _T["fill"]),
    ("glp_witness_generate", "input_values", "host", REFUSE, "test_gpu_witness_generate.py::test_refusals"),
    ("glp_witness_check", "wires", "either", "refuse / reduce", "test_gpu_witness_check.py::test_refusals"),
    ("glp_witness_check", "public_inputs", "host", REFUSE, "test_gpu_witness_check.py::test_refusals"),
    ("glp_session_begin", "wires", "either", "refuse / reduce", _T["session"]),
    ("glp_session_begin", "public_inputs", "host", REFUSE, _T["prover_host"]),
    ("glp_session_partial_products", "betas", "host", REFUSE, "test_gpu_prove.py::test_stepped_session_enforces_order"),
    ("glp_session_partial_products", "gammas", "host", REFUSE, "test_gpu_prove.py::test_stepped_session_enforces_order"),
    ("glp_session_quotient", "alphas", "host", REFUSE, _T["session_steps"]),
    ("glp_session_open", "zeta", "host", REFUSE, _T["session_steps"]),
    ("glp_session_fri_combine", "alpha", "host", REFUSE, _T["session_steps"]),
    ("glp_session_fri_fold", "beta", "host", REFUSE, _T["session_steps"]),
    ("glp_pow_search", "sponge_state", "host", REFUSE, "test_gpu_pow_search.py::test_refusals"),
    ("glp_pow_search", "pending_inputs", "host", REFUSE, "test_gpu_pow_search.py::test_refusals"),
    ("glp_pow_search_h", "sponge_state", "host", REFUSE, "test_gpu_pow_search.py::test_refusals"),
    ("glp_pow_search_h", "pending_inputs", "host", REFUSE, "test_gpu_pow_search.py::test_refusals"),
]
# field elements that are passed by value, not through a pointer: outside the parse, listed so that they are not forgotten
SCALAR_FIELD_INPUTS = [
    ("glp_fri_queries", "pow_witness", "host", REFUSE, _T["pow"]),
    ("glp_session_queries", "pow_witness", "host", REFUSE, _T["pow"]),
    ("glp_lde", "shift", "host", REFUSE, NEW + "test_in_place_primitives_refuse"),
    ("glp_coset_ifft", "shift", "host", REFUSE, "test_gpu_coset_seam.py::test_refusals"),
]

_OUT = "an output: the library writes it"
_PROOF = "proof words (openings, caps, paths): the canonical-form check of a proof is the verifier's own first check, swept by test_gpu_verify_sweep.py and test_gpu_fri_verify_sweep.py"
_IDX = "indices, held to their range by name"
_CELLS = "cell addresses (column * n + row), not field elements"
NOT_FIELD = {
    ("glp_lde", "out"): _OUT, ("glp_fill_random_device", "dev_out"): _OUT, ("glp_batch_cap", "cap_out"): _OUT,
    ("glp_batch_coeffs", "out"): _OUT, ("glp_batch_leaf", "out"): _OUT, ("glp_batch_merkle_proof", "siblings_out"): _OUT,
    ("glp_batch_digests", "out"): _OUT, ("glp_batch_caps", "caps_out"): _OUT, ("glp_batch_lde_values", "out"): _OUT,
    ("glp_perm_quotient_values", "out"): _OUT, ("glp_gate_program_sums", "out"): _OUT, ("glp_gate_program_eval_ext", "out"): _OUT,
    ("glp_gate_program_rows", "out"): _OUT, ("glp_running_columns", "out"): _OUT, ("glp_running_columns", "totals_out"): _OUT,
    ("glp_fri_open", "openings_out"): _OUT, ("glp_fri_commit", "cap_out"): _OUT, ("glp_fri_final_poly", "coeffs_out"): _OUT,
    ("glp_fri_proof", "proof_out"): _OUT, ("glp_fri_prove", "openings_out"): _OUT, ("glp_fri_prove", "proof_out"): _OUT,
    ("glp_pow_search_many", "witnesses_out"): _OUT, ("glp_fri_prove_many", "openings_out"): _OUT, ("glp_fri_prove_many", "proofs_out"): _OUT,
    ("glp_circuit_digest", "digest_out"): _OUT, ("glp_circuit_constants_sigmas_cap", "cap_out"): _OUT, ("glp_prove", "proof_out"): _OUT,
    ("glp_prove_device", "proof_out"): _OUT, ("glp_prove_staged", "proof_out"): _OUT, ("glp_prove_batch", "proofs_out"): _OUT,
    ("glp_witness_generate", "dev_wires"): "an output: every cell of the plan is written, nothing of the caller's is read as a field element before it is",
    ("glp_witness_read_cells", "out"): _OUT, ("glp_witness_check", "rows_failed_by_gate_out"): "an output of counts",
    ("glp_session_begin", "wires_cap_out"): _OUT, ("glp_session_begin", "public_inputs_hash_out"): _OUT,
    ("glp_session_partial_products", "zs_cap_out"): _OUT, ("glp_session_quotient", "quotient_cap_out"): _OUT,
    ("glp_session_open", "openings_out"): _OUT, ("glp_session_fri_commit", "cap_out"): _OUT, ("glp_session_fri_final_poly", "coeffs_out"): _OUT,
    ("glp_pow_search", "witness_out"): _OUT, ("glp_pow_search_h", "witness_out"): _OUT, ("glp_session_proof", "proof_out"): _OUT,
    ("glp_proof_from_bytes", "proof_words_out"): _OUT,
    ("glp_fri_queries", "indices"): _IDX, ("glp_fri_queries_many", "indices"): _IDX, ("glp_session_queries", "indices"): _IDX,
    ("glp_fri_verify_queries_many", "indices"): _IDX,
    ("glp_witness_plan_create", "input_cells"): _CELLS, ("glp_witness_plan_create_ex", "input_cells"): _CELLS,
    ("glp_witness_plan_create_ex", "cells"): _CELLS, ("glp_witness_plan_create_prog", "input_cells"): _CELLS,
    ("glp_witness_plan_create_prog", "cells"): _CELLS, ("glp_witness_plan_create_rand", "input_cells"): _CELLS,
    ("glp_witness_plan_create_rand", "random_cells"): _CELLS, ("glp_witness_plan_create_rand", "cells"): _CELLS,
    ("glp_witness_read_cells", "cells"): _CELLS,
    ("glp_witness_read_cells", "dev_wires"): "copied out word for word, no arithmetic: the caller reads back what is stored",
    ("glp_fri_verify_many", "points"): _PROOF, ("glp_fri_verify_many", "caps"): _PROOF, ("glp_fri_verify_many", "openings"): _PROOF,
    ("glp_fri_verify_many", "proofs"): _PROOF,
    ("glp_fri_verify_many", "sponge_states"): "the transcript state a verifier resumes from: a verifier-side input like the proof words; a wrong state only ever rejects",
    ("glp_fri_verify_many", "pending_inputs"): "the transcript state a verifier resumes from: a verifier-side input like the proof words; a wrong state only ever rejects",
    ("glp_fri_verify_queries_many", "points"): _PROOF, ("glp_fri_verify_queries_many", "caps"): _PROOF,
    ("glp_fri_verify_queries_many", "openings"): _PROOF, ("glp_fri_verify_queries_many", "proofs"): _PROOF,
    ("glp_fri_verify", "caps"): _PROOF, ("glp_fri_verify", "openings"): _PROOF, ("glp_fri_verify", "proof"): _PROOF,
    ("glp_fri_verify", "sponge_state"): "the transcript state a verifier resumes from: a verifier-side input like the proof words; a wrong state only ever rejects",
    ("glp_fri_verify", "pending_inputs"): "the transcript state a verifier resumes from: a verifier-side input like the proof words; a wrong state only ever rejects",
    ("glp_verify", "proof_words"): _PROOF, ("glp_verify_n", "proof_words"): _PROOF, ("glp_verify_batch", "proofs"): _PROOF,
    ("glp_proof_to_bytes", "proof_words"): "proof words on their way to bytes: the byte format's own check (test_verify_host.py::test_proof_bytes)",
}


def test_exists(test_id):
    """`file.py::test_name` names a test function of that file under tests/"""
    fname, name = test_id.split("::")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), fname)
    return os.path.exists(path) and re.search(r"^def %s\(" % re.escape(name), open(path).read(), flags=re.M) is not None
