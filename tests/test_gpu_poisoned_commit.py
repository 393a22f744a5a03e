"""The commit path's reference comparisons once more, on a context whose device pool is poisoned (tests/poisoned_pool.py): transforms,
LDE, leaf hashes and trees of every input kind, the Keccak trees and the coset seam.  The test functions are their home modules';
only the `ctx` they get differs.  The 2^16-point and larger cases stay in the home modules."""
import pytest

from poisoned_pool import ctx, only                              # noqa: F401
import test_gpu_commit as commit
from test_gpu_batch_build import test_every_input_kind_against_the_oracle                                  # noqa: F401
from test_gpu_commit import (test_batch_edge_shapes, test_batch_from_coeffs_parity, test_batch_from_values_parity,      # noqa: F401
                             test_mid_size_transforms_ragged_column_counts)
from test_gpu_coset_seam import (test_coset_ifft, test_from_coset_values_is_from_coeffs_on_the_chunks,                    # noqa: F401
                                 test_from_coset_values_keccak_and_device_input, test_from_coset_values_many_proofs_salted,
                                 test_lde_values_against_the_oracle_and_the_leaves, test_lde_values_of_a_many_proof_batch)
from test_gpu_keccak import test_keccak_batch_parity            # noqa: F401

pytestmark = pytest.mark.gpu

test_fft_ifft_parity = only(commit.test_fft_ifft_parity, lg=lambda lg: lg < 16)
test_lde_parity = only(commit.test_lde_parity, lg=lambda lg: lg < 16)
