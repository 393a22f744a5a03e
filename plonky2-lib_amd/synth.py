"""Synthetic plonky2 circuits + satisfying witnesses (host side, numpy).

The reference's circuits are built by Rust code (`CircuitBuilder` + the gadget traits of
src/{ecdsa,hash,smt,zkdsa}) that cannot run here, so tests and bench.py use stand-ins with the same
*shape*: `standard_ecc_config` (136 wires / 80 routed, [REF src/ecdsa/gadgets/ecdsa.rs:476-483]) or
`standard_recursion_config` (135 / 80), rows of ArithmeticGate / ConstantGate / PublicInputGate /
NoopGate and the reference's own three u32 gates [REF src/u32/gates/*.rs], copy constraints, and a
witness that satisfies every gate.  What `builder.build::<C>()` would produce for the prover is
restated: gates sorted by (degree, id), `selector_polynomials` grouping, k_is = 7^i, sigma values
k_is[col'] * w^row'.

Nothing here touches the GPU or the oracle.
"""
import os

import numpy as np

from . import gl_numpy as gl

P = gl.P

GATE_NOOP, GATE_CONSTANT, GATE_PUBLIC_INPUT, GATE_ARITHMETIC, GATE_POSEIDON = 0, 1, 2, 3, 4
GATE_U32_INTERLEAVE, GATE_UNINTERLEAVE_U32, GATE_UNINTERLEAVE_B32 = 5, 6, 7
GATE_U32_ARITHMETIC, GATE_U32_ADD_MANY, GATE_U32_SUBTRACTION, GATE_U32_RANGE_CHECK = 8, 9, 10, 11
GATE_COMPARISON, GATE_BASE_SUM, GATE_RANDOM_ACCESS = 12, 13, 14
# plonky2's extension-field arithmetic (D = 2: an F_p^2 value a + b X, X^2 = 7, on two consecutive wires)
GATE_ARITHMETIC_EXTENSION, GATE_MUL_EXTENSION, GATE_REDUCING, GATE_REDUCING_EXTENSION = 15, 16, 17, 18
EXT_GATES = (GATE_ARITHMETIC_EXTENSION, GATE_MUL_EXTENSION, GATE_REDUCING, GATE_REDUCING_EXTENSION)
# the rest of the recursive verifier's gate set (19 is unassigned): exp_from_bits, the FRI fold step, Poseidon's MDS on ext targets
GATE_EXPONENTIATION, GATE_COSET_INTERPOLATION, GATE_POSEIDON_MDS = 20, 21, 22
RECURSION_GATES = (GATE_EXPONENTIATION, GATE_COSET_INTERPOLATION, GATE_POSEIDON_MDS)

# (degree, id string as plonky2's `Gate::id` prints it) -- the build() sort key
_GATE_META = {
    GATE_NOOP: (0, "NoopGate"),
    GATE_CONSTANT: (1, "ConstantGate {{ num_consts: {p0} }}"),
    GATE_PUBLIC_INPUT: (1, "PublicInputGate"),
    GATE_ARITHMETIC: (3, "ArithmeticGate {{ num_ops: {p0} }}"),
    GATE_POSEIDON: (7, "PoseidonGate(PhantomData<plonky2_field::goldilocks_field::GoldilocksField>)<WIDTH=12>"),
    GATE_U32_INTERLEAVE: (2, "U32InterleaveGate {{ num_ops: {p0} }}"),
    GATE_UNINTERLEAVE_U32: (2, "UninterleaveToU32Gate {{ num_ops: {p0} }}"),
    GATE_UNINTERLEAVE_B32: (2, "UninterleaveToB32Gate {{ num_ops: {p0} }}"),
    GATE_U32_ARITHMETIC: (4, "U32ArithmeticGate {{ num_ops: {p0} }}"),
    GATE_U32_ADD_MANY: (4, "U32AddManyGate {{ num_addends: {p0}, num_ops: {p1} }}"),
    GATE_U32_SUBTRACTION: (4, "U32SubtractionGate {{ num_ops: {p0} }}"),
    GATE_U32_RANGE_CHECK: (4, "U32RangeCheckGate {{ num_input_limbs: {p0} }}"),
    GATE_COMPARISON: (4, "ComparisonGate {{ num_bits: {p0}, num_chunks: {p1} }}"),
    GATE_BASE_SUM: (4, "BaseSumGate {{ num_limbs: {p0} }} + Base: {p1}"),
    GATE_RANDOM_ACCESS: (5, "RandomAccessGate {{ bits: {p0} }}"),
    GATE_ARITHMETIC_EXTENSION: (3, "ArithmeticExtensionGate {{ num_ops: {p0} }}"),
    GATE_MUL_EXTENSION: (3, "MulExtensionGate {{ num_ops: {p0} }}"),
    GATE_REDUCING: (2, "ReducingGate {{ num_coeffs: {p0} }}"),
    GATE_REDUCING_EXTENSION: (2, "ReducingExtensionGate {{ num_coeffs: {p0} }}"),
    # id strings recalled; CosetInterpolationGate's degree is its p1 (gate_degree)
    GATE_EXPONENTIATION: (4, "ExponentiationGate {{ num_power_bits: {p0} }}"),
    GATE_COSET_INTERPOLATION: (None, "CosetInterpolationGate {{ subgroup_bits: {p0}, degree: {p1} }}"),
    GATE_POSEIDON_MDS: (1, "PoseidonMdsGate"),
}


def gate_degree(t, p0=0, p1=0):
    """`Gate::degree`: fixed per type except BaseSumGate<B> (the range product has B factors) and ComparisonGate (the
    range product of a chunk has 2^chunk_bits factors)."""
    if t == GATE_COMPARISON:
        return 1 << -(-p0 // p1)
    return p1 if t in (GATE_BASE_SUM, GATE_COSET_INTERPOLATION) else _GATE_META[t][0]


def gate_num_constraints(t, p0, p1=0):
    if t == GATE_U32_ADD_MANY:
        return p1 * 21
    if t == GATE_COMPARISON:
        cb = -(-p0 // p1)
        return 2 + 5 * p1 + 1 + (cb + 1) + 2
    if t == GATE_BASE_SUM:
        return 1 + p0
    if t == GATE_RANDOM_ACCESS:
        return (p1 & 0xFFFF) * (p0 + 2) + (p1 >> 16)
    if t in EXT_GATES:
        return 2 * p0
    if t == GATE_EXPONENTIATION:
        return p0 + 1
    if t == GATE_COSET_INTERPOLATION:
        return 2 * (2 + 2 * coset_num_intermediates(p0, p1))
    if t == GATE_POSEIDON_MDS:
        return 24
    return {GATE_NOOP: 0, GATE_CONSTANT: p0, GATE_PUBLIC_INPUT: 4, GATE_ARITHMETIC: p0, GATE_POSEIDON: 123,
            GATE_U32_INTERLEAVE: p0 * 34, GATE_UNINTERLEAVE_U32: p0 * 67, GATE_UNINTERLEAVE_B32: p0 * 67,
            GATE_U32_ARITHMETIC: p0 * 36, GATE_U32_SUBTRACTION: p0 * 19, GATE_U32_RANGE_CHECK: p0 * 17}[t]


class Config:
    """plonk/circuit_data.rs `CircuitConfig` presets the reference selects in code."""

    def __init__(self, num_wires, num_routed_wires, num_constants=2, num_challenges=2, max_quotient_degree_factor=8,
                 rate_bits=3, cap_height=4, proof_of_work_bits=16, num_query_rounds=28, arity_bits=4, final_poly_bits=5,
                 zero_knowledge=False):
        self.num_wires, self.num_routed_wires, self.num_constants = num_wires, num_routed_wires, num_constants
        self.num_challenges, self.max_quotient_degree_factor = num_challenges, max_quotient_degree_factor
        self.rate_bits, self.cap_height, self.proof_of_work_bits = rate_bits, cap_height, proof_of_work_bits
        self.num_query_rounds, self.arity_bits, self.final_poly_bits = num_query_rounds, arity_bits, final_poly_bits
        self.zero_knowledge = zero_knowledge

    @classmethod
    def standard_recursion_config(cls, **kw):
        return cls(135, 80, **kw)

    @classmethod
    def standard_recursion_zk_config(cls, **kw):
        return cls(135, 80, zero_knowledge=True, **kw)

    @classmethod
    def standard_ecc_config(cls, **kw):
        return cls(136, 80, **kw)

    def reduction_arity_bits(self, degree_bits):
        """fri/reduction_strategies.rs ConstantArityBits(arity_bits, final_poly_bits)."""
        out, d = [], degree_bits
        while d > self.final_poly_bits and d + self.rate_bits - self.arity_bits >= self.cap_height:
            out.append(self.arity_bits)
            d -= self.arity_bits
        return out


D = 2   # extension degree of every config here


def blinding_counts(cfg, num_gates):
    """plonk/circuit_builder.rs `blinding_counts` (recalled from plonky2 0.1.x, unpinned): the rows `blind()` adds to a zero-knowledge
    circuit of num_gates gate rows.  Searches degrees from 2^ceil(log2 num_gates) upwards until num_gates + r + 2 z fits, with
    fri_openings = num_query_rounds (1 + D sum(arity - 1) + D final_poly_coeffs) at that degree, r = D + fri_openings (rows of
    random wires) and z = 2 D + fri_openings (pairs of rows whose routed wires are random and copy-constrained to each other).
    Returns (r, z, degree_bits)."""
    lg = max(0, (int(num_gates) - 1).bit_length())
    while True:
        ab = cfg.reduction_arity_bits(lg)
        folding = sum((1 << a) - 1 for a in ab)
        final_poly_coeffs = 1 << (lg - sum(ab))
        fri_openings = cfg.num_query_rounds * (1 + D * folding + D * final_poly_coeffs)
        r, z = D + fri_openings, 2 * D + fri_openings
        if num_gates + r + 2 * z <= 1 << lg:
            return r, z, lg
        lg += 1


def blinding_values(shape, seed=None):
    """Values of the blinding rows and of the unused PublicInputGate wires: plonky2 draws them per proof (RandomValueGenerator),
    so they must be unpredictable to the verifier.  seed None (the default): OS entropy (os.urandom), reduced mod p.  A seed gives
    reproducible values, for tests only: a known seed voids the hiding."""
    count = int(np.prod(shape))
    if seed is not None:
        return gl.rand(np.random.default_rng(seed), shape)
    raw = np.frombuffer(os.urandom(8 * count), dtype=np.uint64) if count else np.zeros(0, np.uint64)
    return np.where(raw >= np.uint64(gl.P), raw - np.uint64(gl.P), raw).reshape(shape)


def zk_degree_bits(cfg, num_gates, min_log_n=0):
    """degree_bits of a circuit of num_gates gate rows under cfg: with zero_knowledge, large enough for the blinding rows"""
    lg = max(min_log_n, (int(num_gates) - 1).bit_length())
    if getattr(cfg, "zero_knowledge", False):
        lg = max(lg, blinding_counts(cfg, num_gates)[2])
    return lg


class Circuit:
    """Flat CommonCircuitData + ProverOnlyCircuitData (what prove() reads) and a witness."""
    pass


def _selector_groups(gates, max_degree):
    """gates/selectors.rs `selector_polynomials`: returns (selector_indices, groups)."""
    num_gates = len(gates)
    max_gate_degree = gates[-1][0]
    if max_gate_degree + num_gates - 1 <= max_degree:
        return [0] * num_gates, [(0, num_gates)]
    groups, start = [], 0
    while start < num_gates:
        size = 0
        while start + size < num_gates and size + gates[start + size][0] < max_degree:
            size += 1
        if size == 0:
            raise ValueError("gate of degree %d does not fit max_quotient_degree_factor %d (plonky2 panics here too)"
                             % (gates[start][0], max_degree - 1))
        groups.append((start, start + size))
        start += size
    sel = []
    for i in range(num_gates):
        sel.append(next(k for k, (a, b) in enumerate(groups) if a <= i < b))
    return sel, groups


class Builder:
    def __init__(self, config, log_n, seed=0, random_from_row=0):
        """random_from_row: rows below it start as zeros (a caller that fills them all saves the random draw)"""
        self.cfg, self.log_n, self.n = config, log_n, 1 << log_n
        self.rng = np.random.default_rng(seed)
        n, nw, nr = self.n, config.num_wires, config.num_routed_wires
        self.row_gate = np.zeros(n, dtype=np.int64)            # per row: key into self.gate_kinds
        self.gate_kinds = {}                                   # (type, p0) -> key
        self.gate_consts = np.zeros((config.num_constants, n), dtype=np.uint64)
        if random_from_row:                                    # unconstrained cells stay random
            self.wires = np.zeros((nw, n), dtype=np.uint64)
            if random_from_row < n:
                self.wires[:, random_from_row:] = gl.rand(self.rng, (nw, n - random_from_row))
        else:
            self.wires = gl.rand(self.rng, (nw, n))
        self.sig_row = np.tile(np.arange(n, dtype=np.int64), (nr, 1))
        self.sig_col = np.tile(np.arange(nr, dtype=np.int64)[:, None], (1, n))
        self.public_inputs = np.zeros(0, dtype=np.uint64)
        self._kind(GATE_NOOP, 0)

    def _kind(self, t, p0, p1=0):
        return self.gate_kinds.setdefault((t, p0, p1), len(self.gate_kinds))

    def set_rows(self, rows, t, p0, p1=0):
        self.row_gate[rows] = self._kind(t, p0, p1)

    def connect_pairs(self, rows_a, col_a, rows_b, col_b):
        """2-cycles between fresh cells (rows_a[i], col_a) <-> (rows_b[i], col_b)."""
        self.sig_row[col_a, rows_a], self.sig_col[col_a, rows_a] = rows_b, col_b
        self.sig_row[col_b, rows_b], self.sig_col[col_b, rows_b] = rows_a, col_a

    def blind(self, first_row, pi_row=None, seed=None):
        """circuit_builder.rs `randomize_unused_pi_wires` (wires 4.. of the PublicInputGate row pi_row, if given) and `blind()`
        (zero_knowledge): after the num_gates = first_row gate rows, r NoopGate rows of random wires, then z pairs of NoopGate rows
        whose routed wires are random, each copy-constrained to the same wire of the other row.  The random values come from
        blinding_values(.., seed): OS entropy unless a test passes a seed.  Returns the first row after the blinding rows."""
        cfg, nr = self.cfg, self.cfg.num_routed_wires
        r, z, _ = blinding_counts(cfg, first_row)
        end = first_row + r + 2 * z
        if end > self.n:
            raise ValueError("%d gate rows and %d blinding rows do not fit 2^%d rows" % (first_row, r + 2 * z, self.log_n))
        vals = blinding_values((cfg.num_wires * r + nr * z + (cfg.num_wires - 4 if pi_row is not None else 0),), seed)
        if pi_row is not None:
            self.wires[4:, pi_row] = vals[nr * z + cfg.num_wires * r:]
        self.row_gate[first_row:end] = self._kind(GATE_NOOP, 0)
        self.wires[:, first_row:first_row + r] = vals[:cfg.num_wires * r].reshape(cfg.num_wires, r)
        r1 = first_row + r + 2 * np.arange(z, dtype=np.int64)
        r2 = r1 + 1
        self.wires[:nr, r1] = vals[cfg.num_wires * r:cfg.num_wires * r + nr * z].reshape(nr, z)
        self.wires[:nr, r2] = self.wires[:nr, r1]
        for col in range(nr):
            self.connect_pairs(r1, col, r2, col)
        self.blinded = True
        # the cells randomised above, as a witness plan's random_cells (flat positions col * n + row, column by column so that
        # consecutive entries are consecutive rows): the r rows, row r1 of every pair (r2 is its copy), the unused PublicInputGate wires
        wires, routed = np.arange(cfg.num_wires, dtype=np.int64)[:, None] * self.n, np.arange(nr, dtype=np.int64)[:, None] * self.n
        cells = [(wires + np.arange(first_row, first_row + r, dtype=np.int64)).reshape(-1), (routed + r1).reshape(-1)]
        if pi_row is not None:
            cells.append(wires[4:, 0] + pi_row)
        self.random_cells = np.concatenate(cells).astype(np.uint64)
        return end

    def connect_cycle(self, rows, cols):
        """One cycle through fresh cells (rows[i], cols[i]) in the given order."""
        rows, cols = np.asarray(rows), np.asarray(cols)
        self.sig_row[cols, rows] = np.roll(rows, -1)
        self.sig_col[cols, rows] = np.roll(cols, -1)

    def build(self):
        cfg, n, lg = self.cfg, self.n, self.log_n
        c = Circuit()
        kinds = sorted(self.gate_kinds.items(),
                       key=lambda kv: (gate_degree(*kv[0]), _GATE_META[kv[0][0]][1].format(p0=kv[0][1], p1=kv[0][2])))
        gates = [(gate_degree(t, p0, p1), t, p0, p1) for (t, p0, p1), _ in kinds]
        key_to_index = {key: i for i, (_, key) in enumerate(kinds)}
        sel_idx, groups = _selector_groups(gates, cfg.max_quotient_degree_factor + 1)
        num_selectors = len(groups)
        gate_index = np.array([key_to_index[k] for k in self.row_gate], dtype=np.int64)
        consts = np.zeros((num_selectors + cfg.num_constants, n), dtype=np.uint64)
        for g in range(num_selectors):
            a, b = groups[g]
            in_group = (gate_index >= a) & (gate_index < b)
            consts[g] = np.where(in_group, gate_index.astype(np.uint64), np.uint64(0xFFFFFFFF)) if num_selectors > 1 \
                else gate_index.astype(np.uint64)
        consts[num_selectors:] = self.gate_consts
        c.gates = [dict(type=t, p0=p0, p1=p1, selector_index=sel_idx[i], group_start=groups[sel_idx[i]][0],
                        group_end=groups[sel_idx[i]][1], row=i, num_constraints=gate_num_constraints(t, p0, p1))
                   for i, (_, t, p0, p1) in enumerate(gates)]
        c.degree_bits = lg
        c.num_wires, c.num_routed_wires = cfg.num_wires, cfg.num_routed_wires
        c.num_constants, c.num_selectors = consts.shape[0], num_selectors
        c.num_challenges, c.quotient_degree_factor = cfg.num_challenges, cfg.max_quotient_degree_factor
        c.num_partial_products = -(-cfg.num_routed_wires // c.quotient_degree_factor) - 1
        c.num_gate_constraints = max(g["num_constraints"] for g in c.gates)
        c.rate_bits, c.cap_height = cfg.rate_bits, cfg.cap_height
        c.proof_of_work_bits, c.num_query_rounds = cfg.proof_of_work_bits, cfg.num_query_rounds
        c.reduction_arity_bits = cfg.reduction_arity_bits(lg)
        c.k_is = gl.powers(7, cfg.num_routed_wires)          # get_unique_coset_shifts: powers of the generator
        if getattr(cfg, "scramble_k_is", False):               # test hook: any distinct coset shifts are valid
            c.k_is = np.ascontiguousarray(c.k_is[::-1])
        subgroup = gl.powers(gl.root_of_unity(lg), n)
        c.constants = consts
        c.sigmas = gl.mul(c.k_is[self.sig_col], subgroup[self.sig_row])
        c.wires = self.wires
        c.public_inputs = self.public_inputs
        c.circuit_digest = None     # filled by the prover library / the oracle (needs the constants+sigmas cap)
        c.zero_knowledge = bool(getattr(cfg, "zero_knowledge", False))
        if c.zero_knowledge and not getattr(self, "blinded", False):
            raise ValueError("a zero_knowledge config needs the blinding rows: call blind() before build()")
        # what blind() randomised, for Circuit.witness_plan(random_cells=...); empty for a circuit without blinding
        c.witness_random_cells = np.array(getattr(self, "random_cells", ()), dtype=np.uint64)
        return c


def _digits(v, base_bits, count):
    return [(v >> (base_bits * j)) & ((1 << base_bits) - 1) for j in range(count)]


def fill_gate_row(b, row, t, p0, p1=0, equal_inputs=False):
    """One row of gate (t, p0, p1) with a satisfying witness built from the gate's definition, for the gates whose
    parameters vary: U32Arithmetic(num_ops), U32AddMany(num_addends, num_ops), U32Subtraction(num_ops),
    U32RangeCheck(num_input_limbs), Comparison(num_bits, num_chunks; equal_inputs: both inputs the same value),
    BaseSum(num_limbs, base) and RandomAccess(bits, copies | num_extra_constants << 16)."""
    w, rng = b.wires, b.rng
    M32 = (1 << 32) - 1
    ri = lambda hi: int(rng.integers(0, hi))
    b.set_rows(np.array([row]), t, p0, p1)
    if t == GATE_U32_ARITHMETIC:                # m0*m1 + addend = out_hi 2^32 + out_lo
        for i in range(p0):
            m0, m1, ad = ri(1 << 32), ri(1 << 32), ri(1 << 32)
            prod = m0 * m1 + ad
            lo, hi = prod & M32, prod >> 32
            w[6 * i:6 * i + 6, row] = [m0, m1, ad, lo, hi, pow((M32 - hi) % P, P - 2, P)]
            w[6 * p0 + 32 * i:6 * p0 + 32 * i + 32, row] = _digits(prod, 2, 32)
    elif t == GATE_U32_ADD_MANY:                # sum of the addends and the carry in = carry out 2^32 + result
        na, n_ops = p0, p1
        top = 1 << 32 if na < 16 else 1 << 31   # the carry out has two base-4 limbs: the sum stays below 2^36
        for i in range(n_ops):
            vals = [ri(top) for _ in range(na + 1)]
            tot = sum(vals)
            o = (na + 3) * i
            w[o:o + na + 1, row] = vals
            w[o + na + 1, row], w[o + na + 2, row] = tot & M32, tot >> 32
            lo = (na + 3) * n_ops + 18 * i
            w[lo:lo + 16, row] = _digits(tot & M32, 2, 16)
            w[lo + 16:lo + 18, row] = _digits(tot >> 32, 2, 2)
    elif t == GATE_U32_SUBTRACTION:
        for i in range(p0):
            x, y, bi = ri(1 << 32), ri(1 << 32), ri(2)
            d = x - y - bi
            bo = 1 if d < 0 else 0
            res = d + (bo << 32)
            w[5 * i:5 * i + 5, row] = [x, y, bi, res, bo]
            w[5 * p0 + 16 * i:5 * p0 + 16 * i + 16, row] = _digits(res, 2, 16)
    elif t == GATE_U32_RANGE_CHECK:
        for i in range(p0):
            v = ri(1 << 32)
            w[i, row] = v
            w[p0 + 16 * i:p0 + 16 * i + 16, row] = _digits(v, 2, 16)
    elif t == GATE_COMPARISON:
        nbits, nch = p0, p1
        cb = -(-nbits // nch)
        first, second = ri(1 << nbits), ri(1 << nbits)
        if equal_inputs:
            second = first                      # all chunks equal
        a, bb = _digits(first, cb, nch), _digits(second, cb, nch)
        ed, ce, iv, msd = [], [], [], 0
        for i in range(nch):
            diff = (bb[i] - a[i]) % P
            eq = 1 if diff == 0 else 0
            ed.append(1 if eq else pow(diff, P - 2, P))
            ce.append(eq)
            inter = eq * msd % P
            iv.append(inter)
            msd = (inter + (1 - eq) * diff) % P
        top = ((1 << cb) + msd) % P
        bits = _digits(top, 1, cb + 1)
        w[0, row], w[1, row], w[2, row], w[3, row] = first, second, bits[cb], msd
        o = 4
        for arr in (a, bb, ed, ce, iv, bits):
            w[o:o + len(arr), row] = arr
            o += len(arr)
        assert bits[cb] == (1 if first <= second else 0)
    elif t == GATE_BASE_SUM:
        nl, base = p0, p1
        v = ri(base ** nl)
        w[0, row] = v
        w[1:1 + nl, row] = [(v // base ** j) % base for j in range(nl)]
    elif t == GATE_RANDOM_ACCESS:
        bits_ra, copies, nextra = p0, p1 & 0xFFFF, p1 >> 16
        vs = 1 << bits_ra
        for c in range(copies):
            idx = ri(vs)
            lst = [int(x) for x in gl.rand(rng, vs)]
            o = (2 + vs) * c
            w[o, row], w[o + 1, row] = idx, lst[idx]
            w[o + 2:o + 2 + vs, row] = lst
            w[(2 + vs) * copies + nextra + bits_ra * c:(2 + vs) * copies + nextra + bits_ra * (c + 1), row] = _digits(idx, 1, bits_ra)
        ex = [int(x) for x in gl.rand(rng, nextra)]
        b.gate_consts[:nextra, row] = ex
        w[(2 + vs) * copies:(2 + vs) * copies + nextra, row] = ex
    elif t in EXT_GATES:
        _fill_ext_rows(b, np.array([row]), t, p0)
    else:
        raise ValueError("fill_gate_row: gate type %d has no parametrised witness here" % t)
    return row + 1


def ext_gate_params(cfg):
    """The widest instance of each extension-field gate a config fits (plonky2's `new_from_config` /
    `max_coeffs_len`): ArithmeticExtension routed/8 ops, MulExtension routed/6 ops, Reducing
    min(routed - 6, (wires - 4)/3) base coefficients, ReducingExtension min((routed - 6)/2, (wires - 4)/4) ext
    coefficients."""
    nw, nr = cfg.num_wires, cfg.num_routed_wires
    return {GATE_ARITHMETIC_EXTENSION: nr // 8, GATE_MUL_EXTENSION: nr // 6,
            GATE_REDUCING: min(nr - 6, (nw - 4) // 3), GATE_REDUCING_EXTENSION: min((nr - 6) // 2, (nw - 4) // 4)}


def ext_gate_wires(t, p0):
    """Wire columns a row of extension-field gate (t, p0) uses."""
    return {GATE_ARITHMETIC_EXTENSION: 8 * p0, GATE_MUL_EXTENSION: 6 * p0, GATE_REDUCING: 3 * p0 + 4,
            GATE_REDUCING_EXTENSION: 4 * p0 + 4}[t]


def ext_mul(a0, a1, b0, b1):
    """(a0 + a1 X)(b0 + b1 X) in F_p[X]/(X^2 - 7), elementwise over arrays."""
    return (gl.add(gl.mul(a0, b0), gl.mul(np.uint64(7), gl.mul(a1, b1))), gl.add(gl.mul(a0, b1), gl.mul(a1, b0)))


def _reducing_acc_col(p0, cw, i):
    """Wire of accumulator i of a Reducing(Extension)Gate: acc_{N-1} is the output (wires 0, 1)."""
    return 6 + cw * p0 + 2 * i if i + 1 < p0 else 0


def _fill_ext_rows(b, rows, t, p0, chain=True):
    """Rows `rows` of extension-field gate (t, p0): the outputs / accumulators follow from the inputs already in the
    wires (the row-local generators).  ArithmeticExtension / MulExtension draw their gate constants here, and with
    `chain` op i's output is copy-constrained into op i + 1 (its addend, resp. its second multiplicand)."""
    w = b.wires
    rows = np.asarray(rows)
    b.set_rows(rows, t, p0)
    if len(rows) == 0:
        return
    if t in (GATE_ARITHMETIC_EXTENSION, GATE_MUL_EXTENSION):
        ae = t == GATE_ARITHMETIC_EXTENSION
        st = 8 if ae else 6
        cst = gl.rand(b.rng, (2 if ae else 1, len(rows)))
        b.gate_consts[:cst.shape[0], rows] = cst
        for i in range(p0):
            o = st * i
            if chain and i:
                dst = o + (4 if ae else 2)
                w[dst:dst + 2, rows] = w[o - 2:o, rows]
                for k in range(2):
                    b.connect_pairs(rows, o - 2 + k, rows, dst + k)
            p0_, p1_ = ext_mul(w[o, rows], w[o + 1, rows], w[o + 2, rows], w[o + 3, rows])
            r0, r1 = gl.mul(p0_, cst[0]), gl.mul(p1_, cst[0])
            if ae:
                r0, r1 = gl.add(r0, gl.mul(w[o + 4, rows], cst[1])), gl.add(r1, gl.mul(w[o + 5, rows], cst[1]))
            w[o + st - 2, rows], w[o + st - 1, rows] = r0, r1
    else:
        cw = 1 if t == GATE_REDUCING else 2
        al0, al1 = w[2, rows], w[3, rows]
        a0, a1 = w[4, rows], w[5, rows]
        for i in range(p0):
            c = 6 + cw * i
            a0, a1 = ext_mul(a0, a1, al0, al1)
            a0 = gl.add(a0, w[c, rows])
            if cw == 2:
                a1 = gl.add(a1, w[c + 1, rows])
            dst = _reducing_acc_col(p0, cw, i)
            w[dst, rows], w[dst + 1, rows] = a0, a1


def ext_gates_circuit(log_n, config=None, seed=11, num_challenges=2, public_inputs=(), pi_hash=None, gates=EXT_GATES,
                      witness_seed=None, blinding_seed=None):
    """A recursion-shaped circuit of plonky2's extension-field gates, each at the widest instance the config fits
    (ext_gate_params), with satisfying witnesses and copy constraints between them:
    [PublicInput][Constant x2][unit ...][Noop x3 from 16 rows on], a unit being ArithmeticExtension, MulExtension,
    Reducing, Reducing, ReducingExtension, ReducingExtension (restricted to `gates`; a single Reducing type keeps its pair).
    The last ArithmeticExtension op of a unit feeds the first MulExtension op's first multiplicand; within a row op i's
    output feeds op i + 1; the second Reducing(Extension) row of a unit continues the first one's reduction (its old_acc is
    the first one's output and both share alpha), as plonky2's chunked `reduce` does.  2^3 .. 2^20 rows, both presets.
    witness_seed: draw the free wire values from their own seed -- the same circuit (gate constants, sigmas) with another
    satisfying witness, as a batch of proofs of one circuit needs.
    With config.zero_knowledge the 2^log_n gate rows above are followed by the blinding rows (Builder.blind, values from OS entropy
    unless blinding_seed is given) and the circuit grows to the degree blinding_counts asks for."""
    import copy
    cfg = copy.copy(config or Config.standard_recursion_config())
    cfg.num_challenges = num_challenges
    zk = bool(getattr(cfg, "zero_knowledge", False))
    b = Builder(cfg, zk_degree_bits(cfg, 1 << log_n, log_n) if zk else log_n, seed)
    n = 1 << log_n                                             # gate rows (all of them without zero_knowledge)
    if witness_seed is not None:
        b.wires = gl.rand(np.random.default_rng(witness_seed), b.wires.shape)
    gates = tuple(gates)
    if not gates or any(t not in EXT_GATES for t in gates):
        raise ValueError("gates must be a non-empty subset of EXT_GATES")
    par = ext_gate_params(cfg)
    pi = np.asarray(public_inputs, dtype=np.uint64)
    b.public_inputs = pi
    if pi_hash is None:
        if len(pi):
            raise ValueError("pass pi_hash = hash_no_pad(public_inputs) when public inputs are non-empty")
        pi_hash = np.zeros(4, np.uint64)
    num_noop = 3 if n >= 16 else 0
    rows_c = np.array([1, 2])
    body = np.arange(3, n - num_noop)
    if len(body) < 2:
        raise ValueError("log_n too small")
    # PublicInputGate wires = hash, copy-constrained to the constant cells that hold it
    b.set_rows(np.array([0]), GATE_PUBLIC_INPUT, 0)
    b.set_rows(rows_c, GATE_CONSTANT, cfg.num_constants)
    cvals = gl.rand(b.rng, (cfg.num_constants, 2))
    cvals[0, 0], cvals[1, 0], cvals[0, 1], cvals[1, 1] = pi_hash[0], pi_hash[1], pi_hash[2], pi_hash[3]
    b.gate_consts[:, rows_c] = cvals
    b.wires[:cfg.num_constants, rows_c] = cvals
    b.wires[:4, 0] = pi_hash
    for k in range(4):
        b.connect_pairs(np.array([0]), k, np.array([rows_c[k // 2]]), k % 2)
    unit = [t for t in (GATE_ARITHMETIC_EXTENSION, GATE_MUL_EXTENSION, GATE_REDUCING, GATE_REDUCING, GATE_REDUCING_EXTENSION,
                        GATE_REDUCING_EXTENSION) if t in gates]
    slot = np.arange(len(body)) % len(unit)                    # position of each body row in its unit

    def rows_at(pos):
        return body[slot == pos]
    w = b.wires
    pos = {t: [i for i, u in enumerate(unit) if u == t] for t in gates}
    if GATE_ARITHMETIC_EXTENSION in gates:
        _fill_ext_rows(b, rows_at(pos[GATE_ARITHMETIC_EXTENSION][0]), GATE_ARITHMETIC_EXTENSION, par[GATE_ARITHMETIC_EXTENSION])
    if GATE_MUL_EXTENSION in gates:
        rm = rows_at(pos[GATE_MUL_EXTENSION][0])
        if GATE_ARITHMETIC_EXTENSION in gates:
            ra = rows_at(pos[GATE_ARITHMETIC_EXTENSION][0])[:len(rm)]
            rm2 = rm[:len(ra)]
            o = 8 * par[GATE_ARITHMETIC_EXTENSION] - 2
            w[0:2, rm2] = w[o:o + 2, ra]
            for k in range(2):
                b.connect_pairs(ra, o + k, rm2, k)
        _fill_ext_rows(b, rm, GATE_MUL_EXTENSION, par[GATE_MUL_EXTENSION])
    for t in (GATE_REDUCING, GATE_REDUCING_EXTENSION):
        if t not in gates:
            continue
        r1, r2 = rows_at(pos[t][0]), rows_at(pos[t][1])
        _fill_ext_rows(b, r1, t, par[t])
        r1 = r1[:len(r2)]
        w[2:6, r2] = w[np.ix_([2, 3, 0, 1], r1)]                 # same alpha; old_acc = the first row's output
        for src, dst in ((2, 2), (3, 3), (0, 4), (1, 5)):
            b.connect_pairs(r1, src, r2, dst)
        _fill_ext_rows(b, r2, t, par[t])
    if zk:
        b.blind(n, pi_row=0, seed=blinding_seed)
    return b.build()


def coset_num_intermediates(subgroup_bits, degree):
    """Checkpoints of CosetInterpolationGate's barycentric chain: the first chunk takes `degree` points, each later one degree - 1."""
    return ((1 << subgroup_bits) - 2) // (degree - 1)


def coset_degree(subgroup_bits, max_degree):
    """CosetInterpolationGate::with_max_degree (recalled): the smallest degree that needs no more intermediates than max_degree does."""
    n_points = 1 << subgroup_bits
    return (n_points - 2) // ((n_points - 2) // (max_degree - 1) + 1) + 2


def recursion_gate_params(cfg, subgroup_bits=4):
    """(p0, p1) of each recursion gate as plonky2 picks them under a config (recalled): ExponentiationGate::new_from_config takes
    min(routed - 3, (wires - 2) / 2) power bits; the FRI fold interpolates 2^arity_bits = 16 points at the degree
    max_quotient_degree_factor admits."""
    return {GATE_EXPONENTIATION: (min(cfg.num_routed_wires - 3, (cfg.num_wires - 2) // 2), 0),
            GATE_COSET_INTERPOLATION: (subgroup_bits, coset_degree(subgroup_bits, cfg.max_quotient_degree_factor)),
            GATE_POSEIDON_MDS: (0, 0)}


def recursion_gate_wires(t, p0=0, p1=0):
    """(wire columns, routed wire columns) of a row of recursion gate (t, p0, p1)."""
    if t == GATE_EXPONENTIATION:
        return 2 * p0 + 2, p0 + 2
    if t == GATE_COSET_INTERPOLATION:
        return 7 + (2 << p0) + 4 * coset_num_intermediates(p0, p1), 5 + (2 << p0)
    return 48, 48


def _fill_exponentiation_rows(b, rows, nb):
    """intermediate_i = intermediate_{i-1}^2 (base if bit n-1-i else 1) from 1; output = the last one.  Base (wire 0) and bits
    (wires 1..n, little-endian) are already in the wires."""
    w = b.wires
    b.set_rows(rows, GATE_EXPONENTIATION, nb)
    base, cur = w[0, rows], np.ones(len(rows), np.uint64)
    for i in range(nb):
        cur = gl.mul(gl.mul(cur, cur), np.where(w[nb - i, rows] != 0, base, np.uint64(1)))
        w[nb + 2 + i, rows] = cur
    w[nb + 1, rows] = cur


def _fill_coset_rows(b, rows, bits, d):
    """shifted point = evaluation point / shift, then the barycentric chain over the subgroup x_i = g^i with weights x_i / N:
    (eval, prod) <- (eval (x - x_i) + w_i value_i prod, prod (x - x_i)), stored into the intermediates after the first d points and
    then after every d - 1; the final eval is the evaluation value.  Shift, values and evaluation point are already in the wires."""
    w = b.wires
    b.set_rows(rows, GATE_COSET_INTERPOLATION, bits, d)
    if len(rows) == 0:
        return
    n_pts, ni = 1 << bits, coset_num_intermediates(bits, d)
    o_pt = 1 + 2 * n_pts
    o_ie, o_ip, o_sp = o_pt + 4, o_pt + 4 + 2 * ni, o_pt + 4 + 4 * ni
    sh_inv = np.array([gl.inv_scalar(int(v)) for v in w[0, rows]], dtype=np.uint64)
    x0, x1 = gl.mul(w[o_pt, rows], sh_inv), gl.mul(w[o_pt + 1, rows], sh_inv)
    w[o_sp, rows], w[o_sp + 1, rows] = x0, x1
    xs = gl.powers(gl.root_of_unity(bits), n_pts)
    n_inv = np.uint64(gl.inv_scalar(n_pts))
    e0 = e1 = q1 = np.zeros(len(rows), np.uint64)
    q0 = np.ones(len(rows), np.uint64)
    j = 0
    for c in range(ni + 1):
        end = min(n_pts, d + c * (d - 1))
        while j < end:
            d0 = gl.sub(x0, xs[j])
            wi = gl.mul(xs[j], n_inv)
            a0, a1 = ext_mul(e0, e1, d0, x1)
            v0, v1 = ext_mul(w[1 + 2 * j, rows], w[2 + 2 * j, rows], q0, q1)
            e0, e1 = gl.add(a0, gl.mul(v0, wi)), gl.add(a1, gl.mul(v1, wi))
            q0, q1 = ext_mul(q0, q1, d0, x1)
            j += 1
        if c < ni:
            w[o_ie + 2 * c, rows], w[o_ie + 2 * c + 1, rows] = e0, e1
            w[o_ip + 2 * c, rows], w[o_ip + 2 * c + 1, rows] = q0, q1
    w[o_pt + 2, rows], w[o_pt + 3, rows] = e0, e1


def _fill_poseidon_mds_rows(b, rows):
    """output_r = sum_i CIRC[i] input[(i + r) mod 12] + DIAG[r] input[r] on each F_p^2 component (DIAG = 8 at r = 0)."""
    from .poseidon_py import CIRC
    w = b.wires
    b.set_rows(rows, GATE_POSEIDON_MDS, 0)
    for cmp in range(2):
        for r in range(12):
            acc = gl.mul(w[cmp, rows], np.uint64(8)) if r == 0 else np.zeros(len(rows), np.uint64)
            for i in range(12):
                acc = gl.add(acc, gl.mul(w[2 * ((i + r) % 12) + cmp, rows], np.uint64(CIRC[i])))
            w[24 + 2 * r + cmp, rows] = acc


def recursion_gates_circuit(log_n, config=None, seed=13, num_challenges=2, public_inputs=(), pi_hash=None, gates=RECURSION_GATES,
                            params=None, mix_ext=False, witness_seed=None, blinding_seed=None):
    """A circuit of the recursive verifier's remaining gates -- Exponentiation, CosetInterpolation, PoseidonMds (restricted to
    `gates`) -- with satisfying witnesses, wired the way the verifier circuit uses them:
    [PublicInput][Constant x2][unit ...][Noop ...], a unit being
      BaseSum<2>, Exponentiation      the power bits are the limbs of the BaseSum row (its 63 limbs; further bits are free 0 / 1 wires),
      ArithmeticExtension, CosetInterpolation
                                      the evaluation point and the first values are ArithmeticExtension outputs (one row of them:
                                      the remaining values are free wires); the shift is the Exponentiation output,
      PoseidonMds                     input 0 is the CosetInterpolation result,
    and with mix_ext one row each of MulExtension, Reducing, ReducingExtension.  The two helper rows come with their gate.
    params: {gate: (p0, p1)} overrides recursion_gate_params (what plonky2 picks under the config: 66 power bits, 16 points at degree 6
    for standard_recursion_config).  2^3 .. 2^20 rows; 2^4 at least with mix_ext.  witness_seed, blinding_seed and
    config.zero_knowledge as in ext_gates_circuit."""
    import copy
    cfg = copy.copy(config or Config.standard_recursion_config())
    cfg.num_challenges = num_challenges
    zk = bool(getattr(cfg, "zero_knowledge", False))
    b = Builder(cfg, zk_degree_bits(cfg, 1 << log_n, log_n) if zk else log_n, seed)
    n = 1 << log_n
    if witness_seed is not None:
        b.wires = gl.rand(np.random.default_rng(witness_seed), b.wires.shape)
    gates = tuple(gates)
    if not gates or any(t not in RECURSION_GATES for t in gates):
        raise ValueError("gates must be a non-empty subset of RECURSION_GATES")
    par = recursion_gate_params(cfg)
    par.update(params or {})
    nw, nr = cfg.num_wires, cfg.num_routed_wires
    for t in gates:
        need = recursion_gate_wires(t, *par[t])
        if need[0] > nw or need[1] > nr:
            raise ValueError("gate %d with parameters %r needs %d wires / %d routed" % (t, par[t], need[0], need[1]))
    pi = np.asarray(public_inputs, dtype=np.uint64)
    b.public_inputs = pi
    if pi_hash is None:
        if len(pi):
            raise ValueError("pass pi_hash = hash_no_pad(public_inputs) when public inputs are non-empty")
        pi_hash = np.zeros(4, np.uint64)
    ext_par = ext_gate_params(cfg)
    unit = []
    if GATE_EXPONENTIATION in gates:
        unit += [GATE_BASE_SUM, GATE_EXPONENTIATION]
    if GATE_COSET_INTERPOLATION in gates:
        unit += [GATE_ARITHMETIC_EXTENSION, GATE_COSET_INTERPOLATION]
    if GATE_POSEIDON_MDS in gates:
        unit += [GATE_POSEIDON_MDS]
    if mix_ext:
        unit += [GATE_MUL_EXTENSION, GATE_REDUCING, GATE_REDUCING_EXTENSION]
    num_noop = 3 if n >= 16 else 0
    rows_c = np.array([1, 2])
    units = (n - num_noop - 3) // len(unit)
    if units < 1:
        raise ValueError("log_n too small")
    b.set_rows(np.array([0]), GATE_PUBLIC_INPUT, 0)
    b.set_rows(rows_c, GATE_CONSTANT, cfg.num_constants)
    cvals = gl.rand(b.rng, (cfg.num_constants, 2))
    cvals[0, 0], cvals[1, 0], cvals[0, 1], cvals[1, 1] = pi_hash[0], pi_hash[1], pi_hash[2], pi_hash[3]
    b.gate_consts[:, rows_c] = cvals
    b.wires[:cfg.num_constants, rows_c] = cvals
    b.wires[:4, 0] = pi_hash
    for k in range(4):
        b.connect_pairs(np.array([0]), k, np.array([rows_c[k // 2]]), k % 2)
    b.set_rows(np.arange(3 + units * len(unit), n), GATE_NOOP, 0)

    def rows_of(t):
        return 3 + unit.index(t) + len(unit) * np.arange(units, dtype=np.int64)
    w = b.wires
    if GATE_EXPONENTIATION in gates:
        nb = par[GATE_EXPONENTIATION][0]
        r_bs, r_ex = rows_of(GATE_BASE_SUM), rows_of(GATE_EXPONENTIATION)
        nl = min(nr - 1, 63, nb)
        b.set_rows(r_bs, GATE_BASE_SUM, nl, 2)
        v = b.rng.integers(0, 1 << nl, size=units, dtype=np.uint64)
        w[0, r_bs] = v
        for j in range(nl):
            w[1 + j, r_bs] = (v >> np.uint64(j)) & np.uint64(1)
            w[1 + j, r_ex] = w[1 + j, r_bs]
            b.connect_pairs(r_bs, 1 + j, r_ex, 1 + j)
        if nb > nl:
            w[1 + nl:1 + nb, r_ex] = b.rng.integers(0, 2, size=(nb - nl, units), dtype=np.uint64)
        _fill_exponentiation_rows(b, r_ex, nb)
    if GATE_COSET_INTERPOLATION in gates:
        bits, d = par[GATE_COSET_INTERPOLATION]
        r_ae, r_co = rows_of(GATE_ARITHMETIC_EXTENSION), rows_of(GATE_COSET_INTERPOLATION)
        ops = ext_par[GATE_ARITHMETIC_EXTENSION]
        _fill_ext_rows(b, r_ae, GATE_ARITHMETIC_EXTENSION, ops, chain=False)
        n_pts = 1 << bits
        # ArithmeticExtension output 0 -> the evaluation point, outputs 1.. -> values 0..
        dst = [1 + 2 * n_pts] + [1 + 2 * i for i in range(min(n_pts, ops - 1))]
        for i, col in enumerate(dst):
            for k in range(2):
                w[col + k, r_co] = w[8 * i + 6 + k, r_ae]
                b.connect_pairs(r_ae, 8 * i + 6 + k, r_co, col + k)
        if GATE_EXPONENTIATION in gates:
            w[0, r_co] = w[par[GATE_EXPONENTIATION][0] + 1, r_ex]
            b.connect_pairs(r_ex, par[GATE_EXPONENTIATION][0] + 1, r_co, 0)
        w[0, r_co] = np.where(w[0, r_co] == 0, np.uint64(1), w[0, r_co])     # a coset needs a non-zero shift (never hit by random wires)
        _fill_coset_rows(b, r_co, bits, d)
    if GATE_POSEIDON_MDS in gates:
        r_md = rows_of(GATE_POSEIDON_MDS)
        if GATE_COSET_INTERPOLATION in gates:
            o_val = 3 + 2 * n_pts
            for k in range(2):
                w[k, r_md] = w[o_val + k, r_co]
                b.connect_pairs(r_co, o_val + k, r_md, k)
        _fill_poseidon_mds_rows(b, r_md)
    if mix_ext:
        for t in (GATE_MUL_EXTENSION, GATE_REDUCING, GATE_REDUCING_EXTENSION):
            _fill_ext_rows(b, rows_of(t), t, ext_par[t])
    if zk:
        b.blind(n, pi_row=0, seed=blinding_seed)
    return b.build()


def fill_ecdsa_gate_rows(b, first_row, rows_per_gate=2, only=None):
    """Rows of the seven remaining gate types of the secp256k1 circuit [REF src/ecdsa/gadgets/ecdsa.rs:72-96]
    with the parameters `standard_ecc_config` gives them (136 wires / 80 routed / 2 constants), each with a
    satisfying witness built from the gate's definition.  Returns the next free row."""
    cfg = b.cfg
    nw, nr = cfg.num_wires, cfg.num_routed_wires
    na = 3                                      # U32AddManyGate, 3 addends
    bits_ra = 4                                 # RandomAccessGate(bits = 4)
    copies = min(nr // (2 + (1 << bits_ra)), nw // (2 + (1 << bits_ra) + bits_ra))
    nextra = min(nr - copies * (2 + (1 << bits_ra)), cfg.num_constants)
    kinds = [(GATE_U32_ARITHMETIC, min(nr // 6, nw // 38), 0),
             (GATE_U32_ADD_MANY, na, min(nr // (na + 3), nw // (na + 3 + 18))),
             (GATE_U32_SUBTRACTION, min(nr // 5, nw // 21), 0),
             (GATE_U32_RANGE_CHECK, min(8, nw // 17), 0),           # 8 limbs: exactly 136 wires
             (GATE_COMPARISON, 32, 16),
             (GATE_BASE_SUM, 16, 4),
             (GATE_RANDOM_ACCESS, bits_ra, copies | (nextra << 16))]
    row = first_row
    for t, p0, p1 in kinds:
        if only is None or t in only:
            for k in range(rows_per_gate):
                row = fill_gate_row(b, row, t, p0, p1, equal_inputs=(t == GATE_COMPARISON and k == 1))
    return row


def arith_circuit(log_n, config=None, seed=1, public_inputs=(), pi_hash=None, num_const_rows=4, num_noop_rows=3,
                  ecdsa_gate_rows=0, ecdsa_gate_subset=None, extra_rows=None):
    """ECDSA-shaped stand-in: one PublicInputGate row, a few ConstantGate rows, ArithmeticGate rows
    (20 ops wide for 80 routed wires) chained through copy constraints, NoopGate padding."""
    cfg = config or Config.standard_ecc_config()
    b = Builder(cfg, log_n, seed)
    n = b.n
    num_ops = cfg.num_routed_wires // 4
    pi = np.asarray(public_inputs, dtype=np.uint64)
    b.public_inputs = pi
    if pi_hash is None:
        if len(pi):
            raise ValueError("pass pi_hash = hash_no_pad(public_inputs) when public inputs are non-empty")
        pi_hash = np.zeros(4, np.uint64)
    need_const_rows = max(num_const_rows, 2)
    if n < 1 + need_const_rows + num_noop_rows + 2 + 10 * ecdsa_gate_rows:
        raise ValueError("log_n too small")
    row_pi = 0
    rows_c = np.arange(1, 1 + need_const_rows)
    first_arith = 1 + need_const_rows
    if ecdsa_gate_rows:
        first_arith = fill_ecdsa_gate_rows(b, first_arith, ecdsa_gate_rows, ecdsa_gate_subset)
    if extra_rows is not None:
        first_arith = extra_rows(b, first_arith)
    rows_a = np.arange(first_arith, n - num_noop_rows)
    b.set_rows(np.array([row_pi]), GATE_PUBLIC_INPUT, 0)
    b.set_rows(rows_c, GATE_CONSTANT, cfg.num_constants)
    b.set_rows(rows_a, GATE_ARITHMETIC, num_ops)
    na = len(rows_a)
    # ConstantGate rows: wire i = constant i.  Rows 0,1 carry the public-input hash.
    cvals = gl.rand(b.rng, (cfg.num_constants, need_const_rows))
    cvals[0, 0], cvals[1, 0], cvals[0, 1], cvals[1, 1] = pi_hash[0], pi_hash[1], pi_hash[2], pi_hash[3]
    b.gate_consts[:, rows_c] = cvals
    b.wires[:cfg.num_constants, rows_c] = cvals
    # PublicInputGate wires 0..3 = hash, copy-constrained to the constant cells
    b.wires[:4, row_pi] = pi_hash
    for k in range(4):
        b.connect_pairs(np.array([row_pi]), k, np.array([rows_c[k // 2]]), k % 2)
    # ArithmeticGate rows: per-row constants c0, c1; out_j = c0*m0*m1 + c1*addend; out_j -> addend_{j+1}
    c01 = gl.rand(b.rng, (2, na))
    b.gate_consts[0, rows_a], b.gate_consts[1, rows_a] = c01[0], c01[1]
    shared = gl.rand(b.rng, 1)[0]
    b.wires[1, rows_a] = shared                               # m1 of op 0: one big cycle over all rows
    b.connect_cycle(rows_a, np.full(na, 1))
    # remaining ConstantGate cells feed m0 of op 0 of the first arithmetic rows
    extra = [(r, k) for r in range(2, need_const_rows) for k in range(cfg.num_constants)]
    for t, (r, k) in enumerate(extra[:na]):
        b.wires[0, rows_a[t]] = cvals[k, r]
        b.connect_pairs(np.array([rows_c[r]]), k, np.array([rows_a[t]]), 0)
    for j in range(num_ops):
        m0, m1, ad = b.wires[4 * j, rows_a], b.wires[4 * j + 1, rows_a], b.wires[4 * j + 2, rows_a]
        out = gl.add(gl.mul(gl.mul(m0, m1), c01[0]), gl.mul(ad, c01[1]))
        b.wires[4 * j + 3, rows_a] = out
        if j + 1 < num_ops:
            b.wires[4 * (j + 1) + 2, rows_a] = out
            b.connect_pairs(rows_a, 4 * j + 3, rows_a, 4 * (j + 1) + 2)
    return b.build()


def ecdsa_shape_circuit(log_n, seed=3, rows_per_gate=2):
    """The headline stand-in: `standard_ecc_config`, every one of the 11 gate types the reference registers for
    its secp256k1 circuit [REF src/ecdsa/gadgets/ecdsa.rs:72-96] present (so the quotient kernel evaluates the
    same constraint set at every point, in three selector groups), ArithmeticGate rows filling the trace."""
    return arith_circuit(log_n, Config.standard_ecc_config(), seed=seed, ecdsa_gate_rows=rows_per_gate)


def _fill_interleave_rows(b, row, rows_per_gate=2):
    """Rows of the reference's three gates [REF src/u32/gates/*.rs] with satisfying witnesses."""
    cfg = b.cfg
    n_il = min(cfg.num_wires // 34, cfg.num_routed_wires // 2)
    n_ul = min(cfg.num_wires // 67, cfg.num_routed_wires // 3)

    def interleave(x):
        r = 0
        for i in range(32):
            r |= ((x >> i) & 1) << (2 * i)
        return r
    for _ in range(rows_per_gate):
        b.set_rows(np.array([row]), GATE_U32_INTERLEAVE, n_il)
        for op in range(n_il):
            x = int(b.rng.integers(0, 1 << 32))
            b.wires[2 * op, row], b.wires[2 * op + 1, row] = x, interleave(x)
            b.wires[2 * n_il + 32 * op:2 * n_il + 32 * op + 32, row] = [(x >> (31 - k)) & 1 for k in range(32)]
        row += 1
    for t in (GATE_UNINTERLEAVE_U32, GATE_UNINTERLEAVE_B32):
        for _ in range(rows_per_gate):
            b.set_rows(np.array([row]), t, n_ul)
            for op in range(n_ul):
                x, y = int(b.rng.integers(0, 1 << 31)), int(b.rng.integers(0, 1 << 31))
                v = interleave(x) + interleave(y)
                bits = [(v >> (63 - k)) & 1 for k in range(64)]
                ev = sum(bits[2 * j] << (31 - j) for j in range(32))
                od = sum(bits[2 * j + 1] << (31 - j) for j in range(32))
                if t == GATE_UNINTERLEAVE_B32:
                    ev, od = interleave(ev), interleave(od)
                b.wires[3 * op:3 * op + 3, row] = [v, ev, od]
                b.wires[3 * n_ul + 64 * op:3 * n_ul + 64 * op + 64, row] = bits
            row += 1
    return row


def keccak_shape_circuit(log_n, seed=4, rows_per_gate=2):
    """BASELINE configs 1 and 2 shape: `standard_recursion_config` (135 wires), the gate set SURVEY section 8 row Q
    lists for the u32 / Keccak circuits -- U32Arithmetic, U32AddMany, U32Subtraction, the reference's own
    U32Interleave / UninterleaveToU32 / UninterleaveToB32 [REF src/u32/interleaved_u32.rs:93-130], Constant,
    Arithmetic, PublicInput, Noop -- with ArithmeticGate rows filling the trace.  (The Keccak-f1600 wiring itself
    [REF src/hash/keccak256.rs:79-128] needs the Rust builder; the known-answer digests of that file pin the
    witness generator, not the prover.)"""
    return arith_circuit(log_n, Config.standard_recursion_config(), seed=seed, ecdsa_gate_rows=rows_per_gate,
                         ecdsa_gate_subset=(GATE_U32_ARITHMETIC, GATE_U32_ADD_MANY, GATE_U32_SUBTRACTION),
                         extra_rows=lambda b, row: _fill_interleave_rows(b, row, rows_per_gate))


def u32_circuit(log_n=6, config=None, seed=2):
    """Exercises the reference's own gates [REF src/u32/gates/interleave_u32.rs, uninterleave_to_u32.rs,
    uninterleave_to_b32.rs] next to arithmetic rows: x -> interleave(x), y -> interleave(y), then
    uninterleave(interleave(x) + interleave(y)) gives the AND (odds) and XOR (evens) bits -- the
    one-add XOR/AND trick of [REF src/u32/interleaved_u32.rs:145-179]."""
    cfg = config or Config.standard_recursion_config()
    b = Builder(cfg, log_n, seed)
    n = b.n
    n_il = min(cfg.num_wires // 34, cfg.num_routed_wires // 2)     # U32InterleaveGate::num_ops
    n_ul = min(cfg.num_wires // 67, cfg.num_routed_wires // 3)     # UninterleaveTo*Gate::num_ops
    num_ops = cfg.num_routed_wires // 4
    rows_il = np.arange(1, 1 + 4)
    rows_u32 = np.arange(5, 5 + 2)
    rows_b32 = np.arange(7, 7 + 2)
    rows_c = np.arange(9, 11)
    rows_a = np.arange(11, n - 2)
    b.set_rows(np.array([0]), GATE_PUBLIC_INPUT, 0)
    b.set_rows(rows_il, GATE_U32_INTERLEAVE, n_il)
    b.set_rows(rows_u32, GATE_UNINTERLEAVE_U32, n_ul)
    b.set_rows(rows_b32, GATE_UNINTERLEAVE_B32, n_ul)
    b.set_rows(rows_c, GATE_CONSTANT, cfg.num_constants)
    b.set_rows(rows_a, GATE_ARITHMETIC, num_ops)
    b.wires[:4, 0] = 0
    b.gate_consts[:, rows_c] = 0
    b.wires[:cfg.num_constants, rows_c] = 0
    for k in range(4):
        b.connect_pairs(np.array([0]), k, np.array([rows_c[k // 2]]), k % 2)

    def interleave(x):
        r = 0
        for i in range(32):
            r |= ((x >> i) & 1) << (2 * i)
        return r

    # interleave rows
    for r in rows_il:
        for op in range(n_il):
            x = int(b.rng.integers(0, 1 << 32))
            b.wires[2 * op, r] = x
            b.wires[2 * op + 1, r] = interleave(x)
            for k in range(32):     # big-endian bits
                b.wires[2 * n_il + 32 * op + k, r] = (x >> (31 - k)) & 1
    # uninterleave rows: input = interleave(x) + interleave(y) (< 2^64, in the field by construction of the test values)
    for rows, b32 in ((rows_u32, False), (rows_b32, True)):
        for r in rows:
            for op in range(n_ul):
                x, y = int(b.rng.integers(0, 1 << 31)), int(b.rng.integers(0, 1 << 31))
                v = interleave(x) + interleave(y)
                b.wires[3 * op, r] = v
                bits = [(v >> (63 - k)) & 1 for k in range(64)]
                ev = sum(bits[2 * j] << (31 - j) for j in range(32))
                od = sum(bits[2 * j + 1] << (31 - j) for j in range(32))
                if b32:
                    ev, od = interleave(ev), interleave(od)
                else:
                    assert od == (x ^ y) and ev == (x & y)
                b.wires[3 * op + 1, r], b.wires[3 * op + 2, r] = ev, od
                for k in range(64):
                    b.wires[3 * n_ul + 64 * op + k, r] = bits[k]
    # arithmetic rows as in arith_circuit (no cross-row wiring except the shared m1 cycle)
    na = len(rows_a)
    c01 = gl.rand(b.rng, (2, na))
    b.gate_consts[0, rows_a], b.gate_consts[1, rows_a] = c01[0], c01[1]
    b.wires[1, rows_a] = gl.rand(b.rng, 1)[0]
    b.connect_cycle(rows_a, np.full(na, 1))
    for j in range(num_ops):
        m0, m1, ad = b.wires[4 * j, rows_a], b.wires[4 * j + 1, rows_a], b.wires[4 * j + 2, rows_a]
        out = gl.add(gl.mul(gl.mul(m0, m1), c01[0]), gl.mul(ad, c01[1]))
        b.wires[4 * j + 3, rows_a] = out
        if j + 1 < num_ops:
            b.wires[4 * (j + 1) + 2, rows_a] = out
            b.connect_pairs(rows_a, 4 * j + 3, rows_a, 4 * (j + 1) + 2)
    return b.build()


def _fill_poseidon_row(b, row, inputs):
    """Sets the 135 wires of a PoseidonGate row (gates/poseidon.rs layout) for `inputs` with swap = 0."""
    from . import poseidon_py as pp
    out, f0, part, f1 = pp.permute_trace(inputs)
    w = b.wires
    for i in range(12):
        w[i, row] = inputs[i]
        w[12 + i, row] = out[i]
    w[24, row] = 0
    for i in range(4):
        w[25 + i, row] = 0
    for r in range(3):
        for i in range(12):
            w[29 + 12 * r + i, row] = f0[r][i]
    for r in range(22):
        w[65 + r, row] = part[r]
    for r in range(4):
        for i in range(12):
            w[87 + 12 * r + i, row] = f1[r][i]
    return out


def zkdsa_circuit(log_n=3, config=None, seed=5, private_key=None, message=None, blinding_seed=None):
    """The reference's simple-signature circuit [REF src/zkdsa/circuits/mod.rs:24-43,
    src/zkdsa/gadgets/signature/mod.rs:49-62]: public_key = H(sk || sk), signature = H(sk || msg) with
    `poseidon_two_to_one` [REF src/poseidon/gadgets/mod.rs:7-22]; public inputs = message, public_key,
    signature (12 elements), whose in-circuit hash (two more permutations) feeds the PublicInputGate.
    Rows: PublicInputGate, 4 x PoseidonGate, ConstantGate (zero), NoopGate padding -- 2^3 rows like
    the real circuit; gate placement and wiring are this builder's, not plonky2's.  With config.zero_knowledge
    (Config.standard_recursion_zk_config, what [REF src/zkdsa/circuits/mod.rs:412] leaves as a TODO) the blinding rows follow
    the 6 gate rows and the circuit grows to 2^14 rows (blinding_counts), and wires 4.. of the PublicInputGate row are redrawn
    (`randomize_unused_pi_wires`); both from OS entropy unless blinding_seed is given (tests only)."""
    cfg = config or Config.standard_recursion_config()
    b = Builder(cfg, zk_degree_bits(cfg, 6, log_n), seed)
    rng = b.rng
    sk = [int(x) for x in (gl.rand(rng, 4) if private_key is None else private_key)]
    msg = [int(x) for x in (gl.rand(rng, 4) if message is None else message)]
    rows_p = [1, 2, 3, 4]
    row_c = 5
    b.set_rows(np.array([0]), GATE_PUBLIC_INPUT, 0)
    b.set_rows(np.array(rows_p), GATE_POSEIDON, 0)
    b.set_rows(np.array([row_c]), GATE_CONSTANT, cfg.num_constants)
    b.gate_consts[:, row_c] = 0
    b.wires[:cfg.num_constants, row_c] = 0
    pk = _fill_poseidon_row(b, 1, sk + sk + [0] * 4)[:4]
    sig = _fill_poseidon_row(b, 2, sk + msg + [0] * 4)[:4]
    pis = msg + pk + sig
    o3 = _fill_poseidon_row(b, 3, pis[:8] + [0] * 4)
    o4 = _fill_poseidon_row(b, 4, pis[8:12] + o3[4:12])
    b.public_inputs = np.array(pis, dtype=np.uint64)
    b.wires[:4, 0] = o4[:4]
    cyc = lambda cells: b.connect_cycle([r for r, _ in cells], [c for _, c in cells])
    for i in range(4):
        cyc([(1, i), (1, 4 + i), (2, i)])                 # private key
        cyc([(2, 4 + i), (3, i)])                          # message
        cyc([(1, 12 + i), (3, 4 + i)])                     # public key
        cyc([(2, 12 + i), (4, i)])                         # signature
        cyc([(4, 12 + i), (0, i)])                         # public-input hash -> PublicInputGate
    for i in range(4, 12):
        cyc([(3, 12 + i), (4, i)])                         # sponge state carried into the second absorb
    zeros = [(row_c, 0)] + [(r, 24) for r in rows_p] + [(r, 8 + i) for r in (1, 2, 3) for i in range(4)]
    cyc(zeros)                                             # constant zero: swap flags and capacity lanes
    if cfg.zero_knowledge:
        b.blind(6, pi_row=0, seed=blinding_seed)
    return b.build()


def poseidon_chain_circuit(log_n, config=None, seed=6):
    """SMT-shaped stand-in [REF src/smt/gadgets/verify/verify_smt.rs:214-307: a chain of Poseidon hashes
    walking up a Merkle path]: rows 1..n-3 are PoseidonGate rows, each absorbing the previous digest."""
    cfg = config or Config.standard_recursion_config()
    b = Builder(cfg, log_n, seed)
    n = b.n
    rows_p = list(range(1, n - 2))
    row_c = n - 2
    b.set_rows(np.array([0]), GATE_PUBLIC_INPUT, 0)
    b.set_rows(np.array(rows_p), GATE_POSEIDON, 0)
    b.set_rows(np.array([row_c]), GATE_CONSTANT, cfg.num_constants)
    b.gate_consts[:, row_c] = 0
    b.wires[:cfg.num_constants, row_c] = 0
    b.wires[:4, 0] = 0
    cur = [int(x) for x in gl.rand(b.rng, 4)]
    zeros = [(row_c, 0), (0, 0), (0, 1), (0, 2), (0, 3)]
    prev = None
    for r in rows_p:
        sib = [int(x) for x in gl.rand(b.rng, 4)]
        out = _fill_poseidon_row(b, r, cur + sib + [0] * 4)
        if prev is not None:
            for i in range(4):
                b.connect_cycle([prev, r], [12 + i, i])
        zeros += [(r, 24)] + [(r, 8 + i) for i in range(4)]
        cur, prev = out[:4], r
    b.connect_cycle([r for r, _ in zeros], [c for _, c in zeros])
    return b.build()


def _fill_arith_rows(b, rows_a, num_ops=None):
    """ArithmeticGate rows (by default 20 ops wide at 80 routed wires): per-row constants c0, c1; out_j = c0 m0 m1 + c1 addend, each
    output copy-constrained into the next op's addend; m1 of op 0 is one cycle through all rows."""
    cfg = b.cfg
    num_ops = num_ops or cfg.num_routed_wires // 4
    na = len(rows_a)
    if na == 0:
        return
    b.set_rows(rows_a, GATE_ARITHMETIC, num_ops)
    c01 = gl.rand(b.rng, (2, na))
    b.gate_consts[0, rows_a], b.gate_consts[1, rows_a] = c01[0], c01[1]
    b.wires[1, rows_a] = gl.rand(b.rng, 1)[0]
    b.connect_cycle(rows_a, np.full(na, 1))
    for j in range(num_ops):
        m0, m1, ad = b.wires[4 * j, rows_a], b.wires[4 * j + 1, rows_a], b.wires[4 * j + 2, rows_a]
        out = gl.add(gl.mul(gl.mul(m0, m1), c01[0]), gl.mul(ad, c01[1]))
        b.wires[4 * j + 3, rows_a] = out
        if j + 1 < num_ops:
            b.wires[4 * (j + 1) + 2, rows_a] = out
            b.connect_pairs(rows_a, 4 * j + 3, rows_a, 4 * (j + 1) + 2)


def smt_shape_circuit(log_n, config=None, seed=7, levels=16):
    """BASELINE config 4 stand-in: the gate mix of the sparse-Merkle-tree inclusion circuit
    [REF src/smt/gadgets/verify/verify_smt.rs:214-307, src/smt/gadgets/common.rs:87-112], `standard_recursion_config`.
    One inclusion proof of `levels` levels instantiates: 2 leaf hashes of 12 inputs (2 permutations each) + one
    two-to-one hash per level = levels + 4 PoseidonGate rows [common.rs:87-101,16-25]; `split_le(key[i], 64)` for the four
    key elements [verify_smt.rs:240-242] = 8 BaseSumGate<2> rows (63 limbs per gate at 80 routed wires: a 63-bit gate and a
    1-bit gate per element); the level state machine, conditional selects and equality checks = ArithmeticGate ops
    (about 30 per level, 20 ops per row).  The trace is filled with that proportion (levels + 4 : 8 : 1.5 levels),
    repeated as in a batch of inclusion proofs; ConstantGate / PublicInputGate / NoopGate as in every circuit.
    Rows: [PublicInput][Constant x2][Poseidon chain ...][BaseSum<2> ...][Arithmetic ...][Noop x2]."""
    cfg = config or Config.standard_recursion_config()
    b = Builder(cfg, log_n, seed)
    n = b.n
    if n < 16:
        raise ValueError("log_n too small")
    body = n - 5
    wp, wb, wa = levels + 4, 8, (3 * levels + 1) // 2
    n_p = max(1, body * wp // (wp + wb + wa))
    n_b = max(2, body * wb // (wp + wb + wa))
    rows_p = list(range(3, 3 + n_p))
    rows_b = list(range(3 + n_p, 3 + n_p + n_b))
    rows_a = np.arange(3 + n_p + n_b, n - 2)
    rows_c = np.array([1, 2])
    b.set_rows(np.array([0]), GATE_PUBLIC_INPUT, 0)
    b.set_rows(rows_c, GATE_CONSTANT, cfg.num_constants)
    b.set_rows(np.array(rows_p), GATE_POSEIDON, 0)
    b.gate_consts[:, rows_c] = 0
    b.wires[:cfg.num_constants, rows_c] = 0
    b.wires[:4, 0] = 0
    # Poseidon rows: chains of `levels` two-to-one hashes, each absorbing the previous digest and a sibling
    zeros = [(1, 0), (0, 0), (0, 1), (0, 2), (0, 3)]
    cur, prev = None, None
    for t, r in enumerate(rows_p):
        if t % (levels + 4) == 0:
            cur, prev = [int(x) for x in gl.rand(b.rng, 4)], None
        sib = [int(x) for x in gl.rand(b.rng, 4)]
        out = _fill_poseidon_row(b, r, cur + sib + [0] * 4)
        if prev is not None:
            for i in range(4):
                b.connect_cycle([prev, r], [12 + i, i])
        zeros += [(r, 24)] + [(r, 8 + i) for i in range(4)]
        cur, prev = out[:4], r
    b.connect_cycle([r for r, _ in zeros], [c for _, c in zeros])
    # BaseSumGate<2>, 63 limbs: alternately a 63-bit value and a single bit (the two gates of one split_le(x, 64))
    nl = min(cfg.num_routed_wires - 1, 63)
    for t, r in enumerate(rows_b):
        b.set_rows(np.array([r]), GATE_BASE_SUM, nl, 2)
        v = int(b.rng.integers(0, 1 << 62)) * 2 + int(b.rng.integers(0, 2)) if t % 2 == 0 else int(b.rng.integers(0, 2))
        b.wires[0, r] = v
        b.wires[1:1 + nl, r] = _digits(v, 1, nl)
    # the bit wires of a pair of split gates feed arithmetic rows in the real circuit; here: limb 0 of consecutive gates
    # with equal values are tied (a copy constraint between BaseSum rows)
    lim0 = {}
    for r in rows_b:
        lim0.setdefault(int(b.wires[1, r]), []).append(r)
    for rows in lim0.values():
        if len(rows) > 1:
            b.connect_cycle(rows, [1] * len(rows))
    _fill_arith_rows(b, rows_a)
    return b.build()
