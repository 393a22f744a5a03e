"""plonky2-lib_amd: MI355X (gfx950) backend for the Goldilocks `CircuitData::prove()` path that
Orbiter-Finance/Plonky2-lib drives.  The product is `libglprover.so` (hand-written HIP kernels
behind the C ABI of include/glp.h); this package is the thin ctypes host layer used by the tests
and bench.py.  There is no CPU fallback anywhere in this package."""
from .binding import (GlpError, Context, Batch, Circuit, Session, StagedWitness, build_library, library_path, load_library,  # noqa: F401
                      exported_symbols, splitmix_field, P, CircuitFile, write_circuit_file, FriOpenings, fri_prove, fri_proof_words,
                      FriOpeningsMany, fri_prove_many, fri_verify, fri_verify_many, fri_verify_queries_many, fri_verify_sizes,
                      LDE_ROW_MAJOR, LDE_COL_MAJOR, perm_desc, perm_num_polys, GateProgram, gate_program_check, gate_program_desc,
                      ExtOpenings, plonk_ext_openings, RUN_SUM, RUN_PRODUCT, WitnessReport, WitnessPlan, GATE_TYPE_NAMES,
                      witness_program_check, witness_program_desc, WGEN_PROGRAM, gate_program_circuit_check, GATE_PROGRAM,
                      GATE_PROGRAM_MAX_CONSTRAINTS)
