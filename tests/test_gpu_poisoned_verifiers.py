"""The GPU verifiers' comparisons with the restated and the host verifier once more, on a context whose device pool is poisoned
(tests/poisoned_pool.py): status and error words a stale block would have left at "accepted".  The test functions are their home
modules'; only the `ctx` they get differs."""
import pytest

from poisoned_pool import ctx                                    # noqa: F401
from test_gpu_fri_verify import (case_b5, case_c3, test_accepts_the_gpu_provers_proofs, test_accepts_the_restated_provers_proofs,   # noqa: F401
                                 test_accepts_under_keccak_and_without_reductions, test_plonk_instance_from_the_cpu_prover,
                                 test_rejects_with_the_restatements_check_number, test_second_workgroup_partly_idle,
                                 test_stepped_equals_one_call)
from test_gpu_verify_batch import test_a_batch_of_different_proofs, test_verdicts_and_reasons_equal_the_host_verifier   # noqa: F401

pytestmark = pytest.mark.gpu
