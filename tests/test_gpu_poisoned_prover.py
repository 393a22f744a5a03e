"""The provers' oracle comparisons once more, on a context whose device pool is poisoned (tests/poisoned_pool.py): every launch path
of the quotient and the small traces, the stepped session, the many-proofs prover with host and device transcripts, zero knowledge,
program gates, the extension and recursion gate sets and a staged witness.  The test functions are their home modules'; only the `ctx`
they get differs.  The 2^16-row cases stay in the home modules."""
import pytest

from poisoned_pool import only, poisoned_ctx
import test_gpu_ext_gates as ext_gates
import test_gpu_recursion_gates as recursion_gates
import test_gpu_zk as zk
from test_gpu_batch import test_host_and_device_transcripts_agree, test_zkdsa_batch_equals_single_proofs_and_oracle      # noqa: F401
from test_gpu_launch_paths import test_launch_path_parity       # noqa: F401
from test_gpu_program_gates import test_twin_proof_is_the_oracles                                           # noqa: F401
from test_gpu_prove import test_stepped_session_equals_prove, test_stepped_session_with_device_resident_wires             # noqa: F401
from test_gpu_witness import test_staged_witness_routed_columns_only                                        # noqa: F401
from test_gpu_zk import test_zk_proof, test_zk_prove_batch      # noqa: F401

pytestmark = pytest.mark.gpu

ctx = poisoned_ctx(salt_seed=zk.SEED)                           # the zero-knowledge tests' salts; no other test here draws any

test_ext_gates_prove_verify_check = only(ext_gates.test_prove_verify_check, lg=lambda lg: lg < 16)
test_recursion_gates_prove_verify_check = only(recursion_gates.test_prove_verify_check, lg=lambda lg: lg < 16)
