"""CPU half of the field probe: tests/device/field_probe.hip is built with the library's flags and run in `host` mode (no HIP runtime call),
which drives every GLF_HD function of csrc/glf.h through its host body and the host-only apl_words of csrc/acc.h; every output word is
compared with tests/field_model.py (Python integers, % P).  The device-only functions -- and the device bodies of these -- are
test_gpu_field_probe.py's.  Also here, because they need no GPU: the branch-witness assertions over the committed operand sets of
BOTH halves (each named carry / borrow event fires in some rows and not in others), and the arithmetic behind the accumulators' term
bounds.  The host schedule of csrc/poseidon.h runs here too (POSEIDON_HOST_OPS): pos::host::fold over constructed (al, ah, k) on both sides
of its wrap branch and at the bound a block can hand it, the six pos::host::partial_block over any u64 (the all-ones state among them),
pos::host::mds_add and the whole pos::permute, against a round loop that does not use the tables of namespace pblk."""
import pytest

import field_model as fm

CANONICAL_OPS = ("add", "sub", "neg", "dbl", "pow", "inv")
EXTENSION_OPS = ("e_add", "e_sub", "e_neg", "e_mul", "e_sqr", "e_scale", "e_inv", "e_pow")
REDUCING_OPS = ("canon", "mul", "sqr", "reduce128", "reduce96", "mul_2exp")
EXACT_OPS = ("root_of_unity", "bitrev32", "apl_words")
# the host schedule of csrc/poseidon.h: its fold over constructed (al, ah, k), its six blocks over any u64, its linear layer, the whole
POSEIDON_HOST_OPS = ("host_fold",) + tuple("host_pblock_" + t for t in fm.BLOCKS) + ("host_mds_add", "permute")


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
    assert sorted(CANONICAL_OPS + EXTENSION_OPS + REDUCING_OPS + EXACT_OPS + POSEIDON_HOST_OPS) == sorted(fm.HOST_OPS)


@pytest.mark.parametrize("group", ["CANONICAL_OPS", "EXTENSION_OPS", "REDUCING_OPS", "EXACT_OPS", "POSEIDON_HOST_OPS"])
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
    over apl_words equals the plain sum of products, a range product vanishes exactly on the range; the block model, chained as permute_body
    chains it, is the package's plain Python permutation, and the proof-of-work form (round-0 constants, then the row-7 tail) gives element 7
    of it; the blocks propagated symbolically (what the witnesses and bounds use) fold to the same values as the round loop."""
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
    from plonky2_lib_amd import poseidon_py
    perm_rows = fm.cases("permute")
    for r, want in list(zip(perm_rows, fm.reference("permute")))[::7]:
        assert list(want) == poseidon_py.permute(r), r
    rc0 = fm.round_constants()[0]
    for i, r in enumerate(fm.cases("pow_round0_consts")[::11]):
        pos, cand = r[12], (1 << 40) + 255 - i if i % 2 else i
        k = fm.pow_round0(r)
        sp = pow(cand + rc0[pos], 7, fm.P)
        entering = [(k[j] + fm.MDS_M[j][pos] * sp) % fm.P for j in range(12)]
        full = list(r[:12])
        full[pos] = cand
        assert fm.rounds_from(entering, 1)[7] == poseidon_py.permute(full)[7], r
    for tag in fm.BLOCKS:
        name = "pblock_%s_hook" % tag
        for r, want in list(zip(fm.cases(name), fm.reference(name)))[::5]:
            folded = [(al + (ah << 32) + k) % fm.P for al, ah, k in fm.block_folds(tag, r[:12], r[12:])]
            assert tuple(folded[-12:]) == want[:12], (tag, r)
            nz = len(folded) - 12          # a plain block's z_0 is its entering word, not a fold
            assert tuple(folded[:nz]) == want[12 + fm.BLOCKS[tag][1] - nz:], (tag, r)


@pytest.mark.parametrize("name", sorted(fm.WITNESS))
def test_branch_witnesses(name):
    """every named event fires in at least 16 rows of the operand set (the events of one operation partition or pair off, so each is also absent
    from some rows); single constructed rows are the exception and are counted as they are.  The Poseidon layers count units (one fold, one
    byte dot product, one half of an output row) in place of rows."""
    got = fm.witnesses(name)
    print(name, got)
    few = {"b4_value": 1, "mul_small_nc": 16}
    for event, count in got.items():
        count, total = count if isinstance(count, tuple) else (count, len(fm.cases(name)))
        assert count >= few.get(name, 16), (name, event, count)
        assert count < total, (name, event, "fires in every row")


def test_which_witnesses_need_constructed_rows():
    """Recorded, so that a change of the pools that loses an event is seen: without CONSTRUCTED only g = 7 of mul_small_nc is never reached
    (7 is in neither the edge list nor the structured halves)."""
    missing = {(name, event) for name in fm.WITNESS if not callable(fm.WITNESS[name])
               for event, count in fm.witnesses(name, constructed=False).items() if count == 0}
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
    assert {r[12] for r in fm.cases("pow_round0_consts")} == set(range(8))
    # the shared set of the two linear layers: every edge row in every lane of a wave, opposite extremes in lanes l and l + 32, a partial wave
    rows, start, edge_at, pair_at = fm.mds_layout()
    assert fm.cases("mds_add_wave") == fm.cases("mds_add_nc") == rows and len(rows) % 64 == 33
    assert fm.mds_edge_lanes() == set(range(64)) and {at % 64 for at in edge_at} == set(fm.WAVE_SHIFTS) and start <= edge_at[0]
    pairs = [(rows[pair_at + l][:12], rows[pair_at + l + 32][:12]) for l in range(32)]
    assert pair_at % 64 == 0 and {((0,) * 12, (fm.M64,) * 12), ((fm.M64,) * 12, (0,) * 12)} <= set(pairs)
    assert all(((0,) * 12 in p or (fm.M64,) * 12 in p) and p[0] != p[1] for p in pairs)
    for name in ("full_round_wave", "permute_wave"):
        assert len(fm.cases(name)) % 64 != 0
    for name in fm.POSEIDON_LAYER_OPS:      # canonical where the contract says so
        if name in ("permute", "permute_wave", "pow_round0_consts", "host_mds_add"):
            assert all(v < fm.P for r in fm.cases(name) for v in r[:12]), name
    assert any(v >= fm.P for r in fm.cases("tail7") for v in r)
    twins = {}
    for r, (w,) in zip(fm.cases("tail7"), fm.reference("tail7")):
        assert twins.setdefault(tuple(v % fm.P for v in r), w) == w
    assert len(twins) < len(fm.cases("tail7"))
    for name in fm.OPS:            # the domains: canonical operands are canonical, 32-bit operands fit
        for j, d in enumerate(fm._DOMAINS.get(name, ())):
            top = fm.P - 1 if d == "canon" else fm.M32 if d == "u32" else fm.M64
            assert all(r[j] <= top for r in fm.cases(name)), (name, j)


def test_block_bounds_hold_and_the_all_ones_state_meets_them():
    """per table shape the largest row weight of the model's own matrices stays below 2^32 - 2 (the static_assert of partial_block_nc), the
    all-ones state of the operand sets reaches (2^32 - 1) x (row sum of G) in the y-part of al, and host_fold is driven at that bound"""
    got = fm.block_bounds()
    print(got)
    assert got["m3"][0] == got["4a"][0] == got["4d"][0] > got["3"][0]       # (M E)^3 M over twelve variables either way
    b = fm.fold_bound()
    assert b == fm.M32 * got["m3"][0] + (1 << 32) and any(r[0] == b and r[1] == b for r in fm.cases("host_fold"))


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
