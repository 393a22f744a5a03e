"""The seam entry points' comparisons with their Python restatements once more, on a context whose device pool is poisoned
(tests/poisoned_pool.py): the permutation argument, gate and trace programs, running columns and the check at zeta.  The test
functions are their home modules'; only the `ctx` they get differs."""
import pytest

from poisoned_pool import ctx                                    # noqa: F401
from test_gpu_gate_program import (traced, test_three_proofs_in_one_call, test_traced_programs_are_gate_sums,             # noqa: F401
                                   test_traced_seam_program_at_one_three_and_four_challenges)
from test_gpu_gate_program import test_boundary_values as test_gate_program_boundary_values              # noqa: F401
from test_gpu_gate_program import test_random_program_is_the_restated_interpreter as test_gate_program_is_the_restated_interpreter   # noqa: F401
from test_gpu_perm_seam import (test_quotient_values_of_three_proofs_shared_and_per_proof_sigmas, test_quotient_values_on_full_planes,   # noqa: F401
                                test_quotient_values_on_one_and_two_planes, test_quotient_values_over_salted_oracles,
                                test_zs_commit_is_from_values_on_the_restated_values, test_zs_commit_of_three_salted_proofs)
from test_gpu_running_columns import (test_columns_and_totals_are_the_restatement,                           # noqa: F401
                                      test_pass_through_layout_from_hbm_to_hbm_with_a_loose_stride,
                                      test_the_first_zero_denominator_is_named_and_a_repaired_call_succeeds)
from test_gpu_running_columns import test_boundary_values as test_running_columns_boundary_values          # noqa: F401
from test_gpu_trace_program import (test_random_program_is_the_restatement,                                 # noqa: F401
                                    test_three_proofs_shared_and_per_proof_inputs_host_and_device,
                                    test_x_is_the_row_s_root_of_unity_and_col_next_the_next_row)
from test_gpu_zeta_check import (proved, test_device_inputs_and_device_output, test_three_proofs_one_damaged,            # noqa: F401
                                 test_traced_programs_at_zeta, test_whole_check_on_a_proof_and_its_tampered_copies)
from test_gpu_zeta_check import test_boundary_values as test_zeta_check_boundary_values                   # noqa: F401
from test_gpu_zeta_check import test_random_program_is_the_restated_interpreter as test_zeta_program_is_the_restated_interpreter   # noqa: F401

pytestmark = pytest.mark.gpu
