"""Unit programs on the GPU (include/glp.h, "witness generation, the dataflow half", UNIT PROGRAMS): k_witness_programs and the plans of
glp_witness_plan_create_prog against tests/witness_program_restate.py -- a Python interpreter of the instruction word glued to the
restated planner -- and, for the reference's sparse-Merkle and Keccak circuits, against the witnesses the gadget builders hold and the
reference's golden digests.  The GPU is never compared with itself.

Inputs of a builder circuit's plan are `witness_inputs` -- what a caller sets -- followed by `witness_zero_inputs`, cells of value 0
that the unused operations of partly filled rows read (gadgets.py, `_attach_free_units`)."""
import functools

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding, gadgets, synth
from plonky2_lib_amd import witness_program as wprog
import witness_plan_restate as wp
import witness_program_restate as wpr
from test_witness_programs import ADD, BITS, COL, EMIT, GOOD, IMM, REG, Bag, ins, opd

pytestmark = pytest.mark.gpu

P = binding.P
ENV = "GLP_WITNESS_NARROW_MAX"
FORMS = ("0", str(1 << 31))                 # every wave wide; every wave walked that may be
FILL = 0x0BADC0DE0BADC0DE                   # what the buffer holds before a generation
EDGE = wpr.EDGE_VALUES
NO_CELL = wpr.NO_CELL


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _generate(ctx, plan, shape, inputs, K, zero_first=False):
    W = np.full((K,) + tuple(shape), FILL, np.uint64)
    ptr = ctx.dev_alloc(W.nbytes)
    ctx.dev_upload(ptr, W)
    plan.generate(ptr, inputs, K, zero_first=zero_first)
    ctx.dev_download(ptr, W)
    return ptr, W


def _clean(reps):
    return all((r.failed_constraints, r.failed_rows, r.failed_copies) == (0, 0, 0) for r in (reps if isinstance(reps, list) else [reps]))


def _values(rng, count):
    """`count` field elements: the edge values first, then random ones"""
    out = [EDGE[i] if i < len(EDGE) else int(rng.integers(0, 1 << 63)) * 2 % P for i in range(count)]
    return [out[i] for i in rng.permutation(count)]


def _units(rows):
    """[(kind, program index, input cells, output cells)] -> (int64 [num][9], uint64 cells); kind 1 is GLP_WGEN_EQUALITY (x, y -> equal, inv)"""
    recs, cells = [], []
    for kind, prog, cin, cout in rows:
        recs.append([kind, prog, len(cells)] + ([len(cin), len(cout), 0, 0] if kind == wpr.PROGRAM else [1, 1, 1, 1]) + [0, 0])
        cells += list(cin) + list(cout)
    return np.array(recs, np.int64).reshape(-1, 9), np.array(cells, np.uint64)


# ------------------------------------------------------------------------------------------------ 1. every opcode, several chunks
def program_a():
    """3 inputs, 6 outputs: ADD, SUB, MUL, MOV, INV0, BITS, LT, EMIT of a register, a pool word and an input cell"""
    asm = wprog.Assembler(3)
    s = asm.add(asm.reg(), asm.input(0), asm.input(1))
    d = asm.sub(asm.reg(), s, asm.imm(7))
    m = asm.mul(asm.reg(), d, asm.input(2))
    asm.emit(asm.mov(asm.reg(), m))
    asm.emit(asm.inv0(asm.reg(), d))
    asm.emit(asm.bits(asm.reg(), asm.input(0), 31, 2))
    asm.emit(asm.lt(asm.reg(), asm.input(1), asm.input(2)))
    asm.emit(asm.imm(9))
    asm.emit(asm.input(2))
    return asm.assemble()


def program_b():
    """2 inputs, 3 outputs: operands of every kind on either side, BITS at both ends of the word, INV0 of an input cell"""
    asm = wprog.Assembler(2)
    asm.emit(asm.lt(asm.reg(), asm.imm(1 << 32), asm.input(0)))
    whole = asm.bits(asm.reg(), asm.input(1), 0, 64)
    top = asm.bits(asm.reg(), whole, 63, 1)
    inv = asm.inv0(asm.reg(), asm.input(0))
    asm.emit(asm.add(asm.reg(), asm.mul(asm.reg(), inv, whole), top))
    asm.emit(asm.sub(asm.reg(), asm.imm(0), asm.input(1)))
    return asm.assemble()


@functools.lru_cache(maxsize=None)
def noop_circuit():
    cfg = synth.Config(80, 80)
    cfg.proof_of_work_bits = 0
    return synth.Builder(cfg, 6, seed=0, random_from_row=64).build()


@functools.lru_cache(maxsize=None)
def every_opcode():
    """-> (circuit, programs, units, cells, input cells, restated plan).  65 units of each program, interleaved; the B units of odd
    number read an output of their A neighbour, so that wave 1 holds both programs and wave 2 the rest."""
    c = noop_circuit()
    n = 64
    progs = [program_a(), program_b()]
    nxt = iter(range(80 * n))
    take = lambda k: [next(nxt) * 7 % (80 * n) for _ in range(k)]          # 7 is coprime to 5120: distinct cells all over the trace
    rows, inputs = [], []
    for i in range(65):
        a_in, a_out = take(3), take(6)
        if i == 64:
            a_out[1] = NO_CELL                                              # a target that was placed nowhere
        b_own, b_out = take(2), take(3)
        b_in = [a_out[0], b_own[1]] if i % 2 else b_own
        rows += [(wpr.PROGRAM, 0, a_in, a_out), (wpr.PROGRAM, 1, b_in, b_out)]
        inputs += a_in + (b_own[1:] if i % 2 else b_own)
    units, cells = _units(rows)
    free = wpr.from_arrays(units, cells, None, progs)
    return c, progs, units, cells, inputs, wpr.plan(c, inputs, free, np.arange(80 * n, dtype=np.int64))


def test_every_opcode_in_several_chunks(ctx):
    c, progs, units, cells, inputs, pl = every_opcode()
    assert progs[0].num_outputs == 6 and progs[1].num_outputs == 3 and pl.num_waves == 2
    assert pl.free_info == dict(num_free_units=130, num_stuck_free_units=0, first_stuck_free_unit=None, widest_wave_free_units=65 + 33)
    K = 3
    rng = np.random.default_rng(5)
    values = np.array([_values(rng, len(inputs)) for _ in range(K)], np.uint64)
    start = np.full(c.wires.shape, FILL, np.uint64)
    want = [wpr.generate(pl, values[k], start) for k in range(K)]
    assert all((w == FILL).sum() > 80 * 64 // 2 for w in want)                  # most cells are no unit's
    gc = glp.Circuit(ctx, c)
    plan = gc.witness_plan(inputs, free_units=(units, cells), programs=progs)
    assert plan.info == pl.info and plan.free_info == pl.free_info
    assert (plan.cell_waves() == pl.cell_waves).all()
    ptr, W = _generate(ctx, plan, c.wires.shape, values, K)
    for k in range(K):
        assert (W[k] == want[k]).all(), "proof %d: %d cells differ" % (k, (W[k] != want[k]).sum())
    ctx.dev_free(ptr)
    plan.free()
    gc.free()


# ------------------------------------------------------------------------------------------------ 2, 4, 5. one dataflow, both schedules
def program_c():
    """2 inputs, 2 outputs: a b + 7 and bits 3..11 of a"""
    asm = wprog.Assembler(2)
    asm.emit(asm.add(asm.reg(), asm.mul(asm.reg(), asm.input(0), asm.input(1)), asm.imm(7)))
    asm.emit(asm.bits(asm.reg(), asm.input(0), 3, 9))
    return asm.assemble()


@functools.lru_cache(maxsize=None)
def chain():
    """2^4 rows, row 0 an ArithmeticGate of two operations (3 x y + 5 z), six waves:
      1 program C (A, B) -> X, Y                  copies X -> op 0's x, Y -> op 0's y (A -> op 0's z is a wave-0 copy)
      2 ArithmeticGate op 0                       copy   its output -> Z
      3 program low_high (Z) -> U, V              copy   U -> U'
      4 EQUALITY kind (U', C) -> E, I             copies I -> op 1's x, E -> op 1's y (B -> op 1's z is a wave-0 copy)
      5 program equality (E, I) -> S, T; ArithmeticGate op 1          copies S -> S', op 1's output -> R
      6 program C (S', R) -> two cells
    -> (circuit, programs, units, cells, input cells A B C, restated plan of all three inputs)"""
    cfg = synth.Config(135, 80)
    cfg.proof_of_work_bits = 0
    b = synth.Builder(cfg, 4, seed=0, random_from_row=16)
    n = 16
    b.set_rows(np.array([0]), synth.GATE_ARITHMETIC, 2)
    b.gate_consts[0, 0], b.gate_consts[1, 0] = 3, 5
    cell = lambda col, row: col * n + row
    pairs = [((2, 8), (0, 0)), ((3, 8), (1, 0)), ((0, 8), (2, 0)), ((3, 0), (10, 9)), ((11, 9), (20, 10)), ((22, 10), (4, 0)), ((21, 10), (5, 0)),
             ((1, 8), (6, 0)), ((30, 11), (40, 12)), ((7, 0), (41, 12))]
    for (c0, r0), (c1, r1) in pairs:
        b.connect_cycle([r0, r1], [c0, c1])
    c = b.build()
    progs = [program_c(), wprog.low_high(5, 64), wprog.equality()]
    A, B, C = cell(0, 8), cell(1, 8), cell(5, 8)
    rows = [(wpr.PROGRAM, 0, [cell(40, 12), cell(41, 12)], [cell(42, 12), cell(43, 12)]),        # the caller's order is not the waves'
            (1, 0, [cell(20, 10), C], [cell(21, 10), cell(22, 10)]),
            (wpr.PROGRAM, 2, [cell(21, 10), cell(22, 10)], [cell(30, 11), cell(31, 11)]),
            (wpr.PROGRAM, 1, [cell(10, 9)], [cell(11, 9), cell(12, 9)]),
            (wpr.PROGRAM, 0, [A, B], [cell(2, 8), cell(3, 8)])]
    units, cells = _units(rows)
    free = wpr.from_arrays(units, cells, np.zeros((0, 8), np.uint32), progs)
    cls = wp.classes(c)
    return c, progs, units, cells, [A, B, C], free, cls, wpr.plan(c, [A, B, C], free, cls)


def _chain_values(K, seed):
    rng = np.random.default_rng(seed)
    vals = np.array([[int(rng.integers(0, 1 << 63)) * 2 % P for _ in range(3)] for _ in range(K)], np.uint64)
    for i, (a, b) in enumerate([(x, y) for x in EDGE for y in EDGE][:K]):
        vals[i, 0], vals[i, 1] = a, b
    return vals


def test_the_chain_is_what_it_says():
    c, progs, units, cells, inputs, free, cls, pl = chain()
    ng = len(pl.units)
    assert ng == 2 and pl.num_waves == 6 and pl.info["num_stuck_units"] == 0 and pl.free_info["num_stuck_free_units"] == 0
    assert [pl.unit_wave[ng + i] for i in range(5)] == [6, 4, 5, 3, 1] and pl.unit_wave[:ng] == [2, 5]
    assert wpr.program_waves(pl) == [1, 3, 5, 6] and sorted(pl.copies) == [0, 1, 2, 3, 4, 5]


def test_both_schedules(ctx, monkeypatch):
    c, progs, units, cells, inputs, free, cls, pl = chain()
    K = 4
    values = _chain_values(K, 11)
    start = np.full(c.wires.shape, FILL, np.uint64)
    want = [wpr.generate(pl, values[k], start) for k in range(K)]
    gc = glp.Circuit(ctx, c)
    for form in FORMS:
        monkeypatch.setenv(ENV, form)
        plan = gc.witness_plan(inputs, free_units=(units, cells), programs=progs)
        assert plan.info == pl.info and plan.free_info == pl.free_info
        assert (plan.cell_waves() == pl.cell_waves).all()
        ptr, W = _generate(ctx, plan, c.wires.shape, values, K)
        for k in range(K):
            assert (W[k] == want[k]).all(), "form %s, proof %d: %d cells differ" % (form, k, (W[k] != want[k]).sum())
        ctx.dev_free(ptr)
        plan.free()
    gc.free()


def test_lock_step_above_the_cu_count(ctx, monkeypatch):
    """300 proofs are more than the chip has CUs: no wave is wide by its size, and those with program units still get their launches"""
    monkeypatch.delenv(ENV, raising=False)
    c, progs, units, cells, inputs, free, cls, pl = chain()
    K = 300
    values = _chain_values(K, 12)
    start = np.full(c.wires.shape, FILL, np.uint64)
    gc = glp.Circuit(ctx, c)
    plan = gc.witness_plan(inputs, free_units=(units, cells), programs=progs)
    ptr, W = _generate(ctx, plan, c.wires.shape, values, K)
    for k in range(K):
        want = wpr.generate(pl, values[k], start)
        assert (W[k] == want).all(), "proof %d: %d cells differ" % (k, (W[k] != want).sum())
    ctx.dev_free(ptr)
    plan.free()
    gc.free()


def test_a_stuck_program_unit(ctx):
    """without A the first program unit is stuck, and with it everything but the EQUALITY unit's wait for U' -- which never comes"""
    c, progs, units, cells, inputs, free, cls, full = chain()
    pl = wpr.plan(c, inputs[1:], free, cls)
    assert pl.free_info == dict(num_free_units=5, num_stuck_free_units=5, first_stuck_free_unit=0, widest_wave_free_units=0)
    assert pl.info["num_stuck_units"] == 2 and pl.num_waves == 0
    gc = glp.Circuit(ctx, c)
    plan = gc.witness_plan(inputs[1:], free_units=(units, cells), programs=progs)
    assert plan.info == pl.info and plan.free_info == pl.free_info
    assert (plan.cell_waves() == pl.cell_waves).all()
    # the named unit reads a cell nothing provides; the unit that reads A itself is units[4]
    assert any(pl.cell_waves.reshape(-1)[p] == -1 for p in free[plan.free_info["first_stuck_free_unit"]].ins)
    values = _chain_values(2, 13)[:, 1:]
    ptr, W = _generate(ctx, plan, c.wires.shape, values, 2)
    start = np.full(c.wires.shape, FILL, np.uint64)
    for k in range(2):
        want = wpr.generate(pl, values[k], start)
        assert (W[k] == want).all()
        assert all(W[k].reshape(-1)[p] == FILL for f in free for p in f.outs)          # nothing that is stuck has run
        assert (W[k] != FILL).sum() == 3                                                # B and its copy, C
    ctx.dev_free(ptr)
    plan.free()
    gc.free()


# ------------------------------------------------------------------------------------------------ 3. equality() against the built-in kind
def test_the_equality_program_is_the_equality_kind(ctx):
    c = noop_circuit()
    n = 64
    pairs = [(5, 5), (0, 0), (P - 1, P - 1), (0, 1), (1, 0), (P - 1, 0), (0, P - 1), (1 << 32, (1 << 32) - 1), (1 << 63, 1)] + [(x, y) for x in EDGE for y in EDGE]
    assert (0 - 1) % P == P - 1 and len(pairs) <= 64
    rows, inputs, values = [], [], []
    for i, (x, y) in enumerate(pairs):
        cx, cy = 0 * n + i, 1 * n + i
        rows += [(1, 0, [cx, cy], [2 * n + i, 3 * n + i]), (wpr.PROGRAM, 0, [cx, cy], [4 * n + i, 5 * n + i])]
        inputs += [cx, cy]
        values += [x, y]
    units, cells = _units(rows)
    progs = [wprog.equality()]
    free = wpr.from_arrays(units, cells, np.zeros((0, 8), np.uint32), progs)
    pl = wpr.plan(c, inputs, free, np.arange(80 * n, dtype=np.int64))
    want = wpr.generate(pl, values, np.full(c.wires.shape, FILL, np.uint64))
    m = len(pairs)
    assert (want[2, :m] == want[4, :m]).all() and (want[3, :m] == want[5, :m]).all()
    assert [int(v) for v in want[2, :m]] == [1 if x == y else 0 for x, y in pairs]
    gc = glp.Circuit(ctx, c)
    plan = gc.witness_plan(inputs, free_units=(units, cells), programs=progs)
    assert plan.free_info == pl.free_info
    ptr, W = _generate(ctx, plan, c.wires.shape, np.array([values], np.uint64), 1)
    assert (W[0] == want).all(), "%d cells differ" % (W[0] != want).sum()
    ctx.dev_free(ptr)
    plan.free()
    gc.free()


# ------------------------------------------------------------------------------------------------ 6. refusals of the plan
def test_plan_refusals(ctx):
    c = noop_circuit()
    gc = glp.Circuit(ctx, c)
    good = wprog.wire_split([63, 63])
    cells = np.arange(10, dtype=np.uint64)
    fn = r"glp_witness_plan_create_prog: "

    def refused(message, rows, programs=(good,), cells=cells):
        with pytest.raises(glp.GlpError, match=message) as e:
            gc.witness_plan([0], free_units=(np.array(rows, np.int64), cells), programs=None if programs is None else list(programs))
        assert e.value.code == -1
    unit = [9, 0, 0, 1, 2, 0, 0, 0, 0]
    gc.witness_plan([0], free_units=(np.array([unit]), cells), programs=[good]).free()
    refused(fn + r"units\[0\]\.modulus = 1, a program unit names its program there and num_programs = 1", [[9, 1, 0, 1, 2, 0, 0, 0, 0]])
    refused(fn + r"units\[1\]\.modulus = 0, a program unit names its program there and num_programs = 0", [[1, 0, 0, 1, 1, 1, 1, 0, 0], unit], programs=())
    refused(fn + r"units\[0\]\.len\[0\] = 2, programs\[0\] has num_inputs = 1", [[9, 0, 0, 2, 2, 0, 0, 0, 0]])
    refused(fn + r"units\[0\]\.len\[1\] = 3, programs\[0\] has num_outputs = 2", [[9, 0, 0, 1, 3, 0, 0, 0, 0]])
    refused(fn + r"units\[0\]\.len\[2\] = 1, a program unit has two operands: unused entries are 0", [[9, 0, 0, 1, 2, 1, 0, 0, 0]])
    refused(fn + r"units\[0\]\.len\[5\] = 7, a program unit has two operands", [[9, 0, 0, 1, 2, 0, 0, 0, 7]])
    refused(fn + r"programs\[1\]: instruction 1, field b: register 1 is read before it is written", [unit],
            programs=(good, Bag([GOOD[0], ins(ADD, 0, opd(REG, 0), opd(REG, 1)), GOOD[1], GOOD[2]])))
    refused(fn + r"programs\[0\]: desc\.num_outputs = 2, the program has 1 EMITs", [unit], programs=(Bag(GOOD, num_outputs=2),))
    refused(fn + r"programs\[0\]: instruction 0, field b: the bit range of BITS has lo \+ width = 33 \+ 32, more than 64", [unit],
            programs=(Bag([ins(BITS, 0, opd(COL, 0), opd(IMM, 1)), ins(EMIT, a=opd(REG, 0)), ins(EMIT, a=opd(REG, 0)), GOOD[2]], pool=(1, 33 + 256 * 32), num_outputs=2),))
    # a program unit is a free unit: its run, its cells and its outputs are held to the same rules
    refused(fn + r"units\[0\]\.cell_begin = 8: its run of 3 cells leaves cells\[\] \(num_cells = 10\)", [[9, 0, 8, 1, 2, 0, 0, 0, 0]])
    refused(fn + r"units\[1\]: output cell 2 is also written by units\[0\]", [unit, [9, 0, 1, 1, 2, 0, 0, 0, 0]])
    refused(fn + r"units\[0\]: cells\[0\] = 18446744073709551615 is out of range", [unit], cells=np.array([NO_CELL, 1, 2], np.uint64))
    # glp_witness_plan_create_ex knows no programs: kind 9 stays an unknown kind
    with pytest.raises(glp.GlpError, match=r"glp_witness_plan_create_ex: units\[0\]\.kind = 9 is not a GLP_WGEN_\* kind"):
        gc.witness_plan([0], free_units=(np.array([unit]), cells))
    gc.free()
    # an output cell that a gate unit of the row also writes: the ArithmeticGate row of the chain
    ch = chain()
    gc = glp.Circuit(ctx, ch[0])
    with pytest.raises(glp.GlpError, match=fn + r"units\[0\]: output cell 48 \(column 3, row 0\) is also written by unit 0 of gate \d+ of that row"):
        gc.witness_plan(ch[4], free_units=(np.array([[9, 1, 0, 1, 2, 0, 0, 0, 0]]), np.array([ch[4][0], 3 * 16 + 0, 50 * 16 + 3], np.uint64)), programs=ch[1])
    gc.free()


# ------------------------------------------------------------------------------------------------ 7, 8. the reference's SMT circuits
def _from_its_inputs(ctx, c, prove=True):
    """plan from witness_inputs + witness_zero_inputs and the attached units and programs; generate from the values the builder's
    witness holds there; no stuck unit, the builder's witness in every cell the plan reaches, a clean check, a proof that verifies"""
    flat = c.wires.reshape(-1)
    inputs = [int(p) for p in c.witness_inputs] + [int(p) for p in c.witness_zero_inputs]
    assert not flat[c.witness_zero_inputs.astype(np.int64)].any()
    assert len(c.witness_programs) >= 1 and (c.free_units[:, 0] == wpr.PROGRAM).any()
    gc = glp.Circuit(ctx, c)
    plan = gc.witness_plan(inputs, free_units=(c.free_units, c.free_cells), moduli=c.moduli, programs=c.witness_programs)
    assert plan.info["num_stuck_units"] == 0 and plan.free_info["num_stuck_free_units"] == 0
    assert plan.free_info["num_free_units"] == c.free_units.shape[0]
    ptr, W = _generate(ctx, plan, c.wires.shape, np.array([[int(flat[p]) for p in inputs]], np.uint64), 1, zero_first=True)
    known = plan.cell_waves() >= 0
    assert (W[0][known] == c.wires[known]).all(), "%d cells differ" % (W[0][known] != c.wires[known]).sum()
    rep = gc.check_witness(dev_wires_ptr=ptr, public_inputs=c.public_inputs)
    assert (rep.failed_constraints, rep.failed_rows, rep.failed_copies) == (0, 0, 0), str(rep)
    if prove:
        assert gc.verify(gc.prove_device(ptr)), binding.load_library().glp_last_error()
    ctx.dev_free(ptr)
    plan.free()
    gc.free()


def _tree(pairs):
    tree = gadgets.SparseMerkleTree()
    for k, v in pairs:
        tree.insert(gadgets.hash_out_from_u128(k), gadgets.hash_out_from_u128(v))
    return tree


@pytest.mark.parametrize("levels,key", [(16, 5), (16, 9), (3, 1)], ids=["16 levels, inclusion", "16 levels, non-inclusion", "3 levels"])
def test_smt_inclusion_from_its_inputs(ctx, levels, key):
    tree = _tree(((1, 2), (12, 1), (5, 51)) if levels == 16 else ((1, 2), (2, 7)))
    c = gadgets.smt_inclusion_circuit(tree, gadgets.hash_out_from_u128(key), n_levels=levels)
    assert c.smt_witness["found"] == (key != 9) and c.computed_root == tree.root
    assert (c.free_units[:, 0] == wpr.PROGRAM).sum() == 4                      # split_le of the key's four elements
    _from_its_inputs(ctx, c)


@pytest.mark.parametrize("op", ["insert", "update"])
def test_smt_process_from_its_inputs(ctx, op):
    tree = _tree(((1, 2), (12, 1), (5, 51)))
    proof = gadgets.smt_set(tree, gadgets.hash_out_from_u128(9 if op == "insert" else 12), gadgets.hash_out_from_u128(77))
    assert proof["fnc"] == ((1, 0) if op == "insert" else (0, 1))
    c = gadgets.smt_process_circuit(proof)
    assert c.computed_roots == (proof["old_root"], proof["new_root"])
    assert (c.free_units[:, 0] == wpr.PROGRAM).sum() == 8                      # split_le of both keys
    _from_its_inputs(ctx, c)


# ------------------------------------------------------------------------------------------------ 9. Keccak-256 from the message limbs
def test_keccak256_from_the_message_limbs(ctx):
    from test_oracle_keccak import SHORT
    msgs = SHORT[:2]
    cs = [gadgets.keccak256_circuit(bytes.fromhex(m)) for m, _ in msgs]
    c = cs[0]
    n = 1 << int(c.degree_bits)
    assert c.witness_inputs.size == 34 and c.free_units.shape[0] == 0          # one block: 34 limbs, no flag; no generator outside the gates
    for d in cs:
        assert (d.sigmas == c.sigmas).all() and (d.witness_inputs == c.witness_inputs).all() and (d.witness_zero_inputs == c.witness_zero_inputs).all()
    for d, (m, _) in zip(cs, msgs):                                             # the inputs are the padded message and nothing else
        padded = bytearray(136)
        padded[:len(m) // 2] = bytes.fromhex(m)
        padded[len(m) // 2] |= 1
        padded[135] |= 0x80
        assert [int(v) for v in d.wires.reshape(-1)[d.witness_inputs.astype(np.int64)]] == [int.from_bytes(padded[4 * i:4 * i + 4], "little") for i in range(34)]
    inputs = [int(p) for p in c.witness_inputs] + [int(p) for p in c.witness_zero_inputs]
    values = np.array([[int(v) for v in d.wires.reshape(-1)[d.witness_inputs.astype(np.int64)]] + [0] * c.witness_zero_inputs.size for d in cs], np.uint64)
    # the public inputs sit on wires 0..7 of the PoseidonGate row that hashes them, the row before the PublicInputGate's
    pi_cells = [k * n + c.gadget_rows - 2 for k in range(8)]
    assert (c.wires.reshape(-1)[pi_cells] == c.public_inputs).all()
    gc = glp.Circuit(ctx, c)
    plan = gc.witness_plan(inputs)
    assert plan.info["num_stuck_units"] == 0
    ptr = ctx.dev_alloc(2 * c.wires.nbytes)
    plan.generate(ptr, values, 2, zero_first=True)
    got = gc.read_cells(ptr, pi_cells, K=2)
    for k, (_, digest) in enumerate(msgs):
        assert b"".join(int(v).to_bytes(4, "little") for v in got[k]).hex() == digest
    assert _clean(gc.check_witness(dev_wires_ptr=ptr, num_proofs=2, public_inputs=got))
    ctx.dev_free(ptr)
    plan.free()
    gc.free()
