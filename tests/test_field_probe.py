"""CPU half of the field probe: tests/device/field_probe.hip is built with the library's flags and run in `host` mode (no HIP runtime call),
which drives every GLF_HD function of csrc/glf.h through its host body and the host-only apl_words of csrc/acc.h; every output word is
compared with tests/field_model.py (Python integers, % P).  The device-only functions -- and the device bodies of these -- are
test_gpu_field_probe.py's.  Also here, because they need no GPU: the branch-witness assertions over the committed operand sets of
BOTH halves (each named carry / borrow event fires in some rows and not in others), and the arithmetic behind the accumulators' term
bounds."""
import pytest

import field_model as fm

CANONICAL_OPS = ("add", "sub", "neg", "dbl", "pow", "inv")
EXTENSION_OPS = ("e_add", "e_sub", "e_neg", "e_mul", "e_sqr", "e_scale", "e_inv", "e_pow")
REDUCING_OPS = ("canon", "mul", "sqr", "reduce128", "reduce96", "mul_2exp")
EXACT_OPS = ("root_of_unity", "bitrev32", "apl_words")


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    """the probe, built into a temporary directory, and the directory its one `host` run read and wrote"""
    exe = fm.build_probe(tmp_path_factory.mktemp("field_probe_build"))
    d = tmp_path_factory.mktemp("field_probe_host")
    fm.write_inputs(d, fm.HOST_OPS)
    out = fm.run_probe(exe, "host", d, timeout=300)
    assert "field_probe host: %d operations" % len(fm.HOST_OPS) in out, out
    return d


def test_groups_cover_every_host_operation():
    assert sorted(CANONICAL_OPS + EXTENSION_OPS + REDUCING_OPS + EXACT_OPS) == sorted(fm.HOST_OPS)


@pytest.mark.parametrize("group", ["CANONICAL_OPS", "EXTENSION_OPS", "REDUCING_OPS", "EXACT_OPS"])
def test_host_bodies_match_the_model(host_run, group):
    for name in globals()[group]:
        n = fm.check(name, fm.read_outputs(host_run, name))
        print("%s: %d cases" % (name, n))


def test_host_apl_words_reproduce_the_product(host_run):
    """What AccHL needs from a table row: with m, m' rebuilt from the 22-bit limbs the HOST wrote, vlo m + vhi m' = v m (mod p), every limb
    below 2^22 -- checked on the program's output, not on the model's words."""
    out = fm.read_outputs(host_run, "apl_words")
    rows = fm.cases("apl_words")
    vs = fm.cases("canon")          # another column of the same pools, as the constraint values
    for i, (m,) in enumerate(rows):
        w0, w1, w2, w3 = out[4 * i:4 * i + 4]
        limbs = (w0 & fm.M32, w0 >> 32, w1, w2 & fm.M32, w2 >> 32, w3)
        assert all(l <= fm.L22 for l in limbs), hex(m)
        v = vs[i % len(vs)][0]
        got = (v & fm.M32) * (limbs[0] + (limbs[1] << 22) + (limbs[2] << 44)) + (v >> 32) * (limbs[3] + (limbs[4] << 22) + (limbs[5] << 44))
        assert got % fm.P == v * m % fm.P, (hex(v), hex(m))


def test_model_restates_itself():
    """The reference against properties it was not written from: inverses multiply to one, roots of unity have their order, the model's acc3 sum
    over apl_words equals the plain sum of products, a range product vanishes exactly on the range."""
    for r, (a, b) in zip(fm.cases("e_inv"), fm.reference("e_inv")):
        if r != (0, 0):
            assert fm._emul(r, (a, b)) == (1, 0), r
    for (n,), (w,) in zip(fm.cases("root_of_unity"), fm.reference("root_of_unity")):
        assert pow(w, 1 << n, fm.P) == 1 and (n == 0 or pow(w, 1 << (n - 1), fm.P) == fm.P - 1)
    for r, (s,) in zip(fm.cases("acc3_loop"), fm.reference("acc3_loop")):
        if r[1]:
            assert s == sum(r[2 + 5 * k] * r[3 + 5 * k] for k in range(r[0])) % fm.P
    for bound in range(2, 17):
        assert [v for v in range(20) if fm._range_product(v, bound) == 0] == list(range(bound))
    for r, (x,) in zip(fm.cases("pow")[:2000], fm.reference("pow")):
        assert x == fm._epow((r[0], 0), r[1])[0]


@pytest.mark.parametrize("name", sorted(fm.WITNESS))
def test_branch_witnesses(name):
    """every named event fires in at least 16 rows of the operand set (the events of one operation partition or pair off, so each is also absent
    from some rows); single constructed rows are the exception and are counted as they are"""
    got = fm.witnesses(name)
    print(name, got)
    few = {"b4_value": 1, "mul_small_nc": 16}
    for event, count in got.items():
        assert count >= few.get(name, 16), (name, event, count)
        assert count < len(fm.cases(name)), (name, event, "fires in every row")


def test_which_witnesses_need_constructed_rows():
    """Recorded, so that a change of the pools that loses an event is seen: without CONSTRUCTED only g = 7 of mul_small_nc is never reached
    (7 is in neither the edge list nor the structured halves)."""
    missing = {(name, event) for name in fm.WITNESS for event, count in fm.witnesses(name, constructed=False).items() if count == 0}
    assert missing == {("mul_small_nc", "g = 7")}


def test_parameters_cover_every_code_shape():
    assert {r[1] for r in fm.cases("mul_pow2_c")} == set(range(1, 96))
    assert {r[1] for r in fm.cases("mul_2exp")} == set(range(0, 96))
    assert {r[1] for r in fm.cases("range_product")} == set(range(2, 17))
    assert {r[1] for r in fm.cases("bitrev32")} == set(range(0, 33))
    assert {r[6] for r in fm.cases("acc_add_shifted")} == set(fm.SHIFTS)
    assert {r[0] for r in fm.cases("acc2_loop")} >= {1, 2, 1023, 1024} and max(r[0] for r in fm.cases("acc2_loop")) == fm.ACC_MAX_TERMS
    assert {r[0] for r in fm.cases("acc3_loop")} >= {1, 2, 511, 512} and max(r[0] for r in fm.cases("acc3_loop")) == fm.ACC3_MAX_TERMS
    assert max(r[0] for r in fm.cases("acc_loop")) == 4096
    for name, n in (("acc_flush", 2 * fm.ACC_MAX_TERMS + 3), ("acc2_flush", 2 * fm.ACC_MAX_TERMS + 3), ("acc3_flush", 2 * fm.ACC3_MAX_TERMS + 3)):
        assert max(r[0] for r in fm.cases(name)) == n
    for name in fm.OPS:            # the domains: canonical operands are canonical, 32-bit operands fit
        for j, d in enumerate(fm._DOMAINS.get(name, ())):
            top = fm.P - 1 if d == "canon" else fm.M32 if d == "u32" else fm.M64
            assert all(r[j] <= top for r in fm.cases(name)), (name, j)


def test_accumulator_bounds_hold_and_are_tight():
    """1024 (512) worst-case terms fit a 64-bit register and one more would not; the worst-case rows of the loops are exactly those terms."""
    fm.accumulator_bounds()
    worst2 = [r for r in fm.cases("acc2_loop") if r[0] == fm.ACC_MAX_TERMS and set(r[1:1 + 2 * r[0]]) == {fm.M64}]
    assert len(worst2) == 1
    worst3 = [r for r in fm.cases("acc3_loop") if r[0] == fm.ACC3_MAX_TERMS and r[1] == 0 and r[2] == fm.M64]
    assert len(worst3) == 1
    c = [0, 0, 0]
    for v, w0, w1, w2, w3 in fm.acc3_words(worst3[0]):
        for j, (l, h) in enumerate(((w0 & fm.M32, w2 & fm.M32), (w0 >> 32, w2 >> 32), (w1, w3))):
            c[j] += (v & fm.M32) * l + (v >> 32) * h
    assert c == [fm.accumulator_bounds()["acc3 at 512"]] * 3
    worst = [r for r in fm.cases("acc_loop") if r[0] == 4096 and set(r[1:]) == {fm.M64}]
    assert len(worst) == 1
