"""The FRI provers' and the proof-of-work search's comparisons with their restatements once more, on a context whose device pool is
poisoned (tests/poisoned_pool.py).  The search's best / next / ticket words are the atomicMin and atomicAdd targets a stale block
flatters most.  The test functions are their home modules'; only the `ctx` they get differs."""
import pytest

from poisoned_pool import poisoned_ctx
import test_gpu_fri_openings as fri_openings
from test_gpu_fri_many import (test_flush_large_form, test_flush_shape_of_the_single_form_test, test_flush_small_form,   # noqa: F401
                               test_members_equal_singles_and_restatement, test_one_proof_through_the_many_call_equals_fri_prove,
                               test_pow_search_many_equals_singles, test_views_and_batches)
from test_gpu_fri_many import test_stepped_equals_one_call as test_fri_many_stepped_equals_one_call      # noqa: F401
from test_gpu_fri_openings import (test_four_points, test_fri_reproduces_the_sessions_fri,                  # noqa: F401
                                   test_more_columns_than_one_accumulator_flush, test_three_oracles_three_points)
from test_gpu_pow_search import (fixtures, pool, test_4096_proofs_bits0, test_chunk_edges, test_deep_witnesses,          # noqa: F401
                                 test_edge_sponges, test_every_candidate_position, test_fixtures_in_a_crowd, test_identical_sponges,
                                 test_many_proofs_bits4, test_more_chunks_wanted_than_leaving_workgroups_grant,
                                 test_reversed_order_gives_reversed_witnesses, test_single_search_second_launch,
                                 test_witness_past_the_workgroups_that_leave)

pytestmark = pytest.mark.gpu

ctx = poisoned_ctx(salt_seed=fri_openings.SEED)                 # as the ctx of test_gpu_fri_openings; the other two modules set none and draw none
