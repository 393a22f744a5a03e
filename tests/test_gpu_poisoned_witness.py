"""The witness checker's and the witness generators' comparisons with their restatements and the oracle once more, on a context whose
device pool is poisoned (tests/poisoned_pool.py): the checker's counters and first-failure keys are atomicAdd and atomicMin targets,
the generators' plans are index tables.  The home modules already vary what the caller's wire buffer holds (FILL, POISON); here the
library's own blocks vary.  The test functions are their home modules'; only the `ctx` they get differs."""
import pytest

from poisoned_pool import poisoned_ctx
import test_gpu_witness_random as witness_random
from test_gpu_witness import test_witness_fill_parity           # noqa: F401
from test_gpu_witness_check import (arith10, test_campaign_against_the_oracle, test_failures_across_workgroups,          # noqa: F401
                                    test_one_changed_cell_of_a_copy_cycle, test_one_wrong_public_input,
                                    test_reports_equal_the_restatement, test_three_witnesses_in_one_call)
from test_gpu_witness_free import test_kind_in_lock_step        # noqa: F401
from test_gpu_witness_generate import test_lock_step_zkdsa, test_values                                    # noqa: F401
from test_gpu_witness_programs import test_both_schedules, test_every_opcode_in_several_chunks             # noqa: F401
from test_gpu_witness_random import test_prf_and_scatter        # noqa: F401

pytestmark = pytest.mark.gpu

ctx = poisoned_ctx(salt_seed=witness_random.SEED)               # the random cells of test_prf_and_scatter; no other test here draws any
