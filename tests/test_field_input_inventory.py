"""Every `uint64_t *` parameter of include/glp.h is either a field-element input with a stated behaviour for words >= p and a test that
pins it (noncanonical_inputs.FIELD_INPUTS) or listed as something else with the reason (NOT_FIELD).  A new pointer parameter, a row
taken out of either list or a row naming a test that does not exist fails here, without a GPU.  The arrays the GPU tests feed
(single / pairs / twin) are checked here once as well: their properties hold by construction of the draw."""
import numpy as np
import pytest

import noncanonical_inputs as nc


def test_every_pointer_parameter_is_in_exactly_one_list():
    params = nc.pointer_parameters()
    assert len(params) > 150 and len(set(params)) == len(params)
    table = [(f, p) for f, p, _where, _what, _test in nc.FIELD_INPUTS]
    assert len(set(table)) == len(table), "a parameter is listed twice in FIELD_INPUTS"
    both = set(table) & set(nc.NOT_FIELD)
    assert not both, "in both lists: %s" % sorted(both)
    missing = [x for x in params if x not in set(table) and x not in nc.NOT_FIELD]
    assert not missing, "glp.h has pointer parameters in neither list: %s" % missing
    stale = [x for x in table + list(nc.NOT_FIELD) if x not in set(params)]
    assert not stale, "listed, but no such parameter in glp.h: %s" % stale


def test_rows_are_well_formed_and_name_tests_that_exist():
    for f, p, where, what, test in nc.FIELD_INPUTS + nc.SCALAR_FIELD_INPUTS:
        assert where in ("host", "device", "either"), (f, p)
        assert what == {"host": what if what in (nc.REFUSE, nc.REDUCE) else None, "device": nc.REDUCE, "either": "refuse / reduce"}[where], (f, p, what)
        assert nc.test_exists(test), "%s(%s): no test %s" % (f, p, test)
    for key, reason in nc.NOT_FIELD.items():
        assert isinstance(reason, str) and len(reason) > 10, key


def test_entry_points_of_the_older_half_are_field_inputs():
    """the prover's own entry points, the transforms and the commitments -- the half of the API that had neither a scan nor a reduction
    and is the easiest to drop from the table -- each with the side (host, device, either) it is pinned on"""
    rows = {(f, p): (where, what) for f, p, where, what, _t in nc.FIELD_INPUTS + nc.SCALAR_FIELD_INPUTS}
    for f, p, where in (("glp_poseidon_permute", "states", "host"), ("glp_ifft", "cols", "host"), ("glp_lde", "coeffs", "host"),
                        ("glp_batch_from_values_device", "dev_values", "device"), ("glp_batch_from_coeffs_device", "dev_coeffs", "device"),
                        ("glp_batch_many_from_values", "values", "either"), ("glp_batch_from_coset_values", "values", "either"),
                        ("glp_perm_zs_commit", "sigmas", "either"), ("glp_perm_quotient_values", "gate_sums", "either"),
                        ("glp_prove", "wires", "host"), ("glp_prove_device", "dev_wires", "device"), ("glp_prove_staged", "public_inputs", "host"),
                        ("glp_prove_batch", "wires", "either"), ("glp_witness_stage", "host_wires", "host"), ("glp_session_begin", "wires", "either"),
                        ("glp_witness_fill", "dev_wires", "device"), ("glp_fri_queries", "pow_witness", "host"),
                        ("glp_session_queries", "pow_witness", "host")):
        assert rows[(f, p)][0] == where, (f, p)


@pytest.mark.parametrize("shape", [(1, 1), (3, 1), (3, 2), (3, 16), (1, 1 << 10), (3, 135, 8)])
def test_twin_arrays_hold_their_properties_by_construction(shape):
    for seed in range(20):
        arr, A = nc.twin(seed, shape)
        nc.check_twin(arr, A)
        assert arr.shape == tuple(shape) and 2 * int(np.isin(A, np.asarray(nc.SMALL, np.uint64)).sum()) >= A.size


@pytest.mark.parametrize("shape", [(3, 2), (3, 4), (1, 64), (3, 32), (2, 3, 8)])
def test_pairs_arrays_hold_the_three_kinds(shape):
    n = shape[-1]
    arr, A = nc.pairs(5, shape)
    assert (nc.reduced(arr) == A).all() and (A < np.uint64(nc.P)).all()
    cols = arr.reshape(-1, n)
    for a, b in nc.PAIRS:
        if len(cols) >= 3 or n >= 32:          # room for every kind: three columns, or one long one
            assert any(int(c[i]) == a and int(c[i + n // 2]) == b for c in cols for i in range(n // 2)), "no butterfly pair (%x, %x)" % (a, b)
        if n >= 8 and (len(cols) >= 3 or n >= 32):
            assert any(int(c[2 * j]) == a and int(c[2 * j + 1]) == b for c in cols for j in range(n // 2)), "no adjacent pair (%x, %x)" % (a, b)


def test_single_arrays():
    for word in nc.NC:
        for pos in nc.single_positions(3, 48):
            arr, A = nc.single(9, (3, 16), word, pos)
            assert int(arr.reshape(-1)[pos]) == word and int((arr >= np.uint64(nc.P)).sum()) == 1 and (nc.reduced(arr) == A).all()
    assert nc.single_positions(1, 1) == [0] and nc.single_positions(1, 2) == [0, 1] and len(nc.single_positions(1, 48)) == 3
