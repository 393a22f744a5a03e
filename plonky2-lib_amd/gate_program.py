"""Gate programs (include/glp.h, glp_gate_program_*): the host side, no GPU and no library needed.

  Assembler    operand constructors and the six operations over VIRTUAL registers (as many as the caller likes); assemble() maps them
               onto the machine's 24 by linear scan over the straight-line code and encodes the instruction words
  TraceField   the field protocol of a gate body written over an abstract field (zero, one, lift, add, sub, mul): run the body once
               over it and the assembler holds its program
  Program      what assemble() returns: .instructions (physical registers, for readers that want no decoder), .code, .pool, ...

    asm = Assembler(oracle_cols=[nc, nw], num_params=4)
    F = TraceField(asm)
    for constraint in gate_body(F, [asm.col(0, j) for j in ...], [asm.col(1, j) for j in ...]):
        asm.emit(constraint)
    asm.end(filter_value)                      # an AIR: asm.end(asm.imm(1))
    prog = asm.assemble(hoist_emits=True)
"""
from collections import namedtuple

import numpy as np

P = 0xFFFFFFFF00000001
MAX_REGS = 24                  # GLP_GP_MAX_REGS
MAX_INSTRUCTIONS = 65536       # GLP_GP_MAX_INSTRUCTIONS
MAX_CONSTRAINTS = 4096         # GLP_GP_MAX_CONSTRAINTS
MAX_ORACLES = 4                # GLP_GP_MAX_ORACLES

OP_ADD, OP_SUB, OP_MUL, OP_MOV, OP_EMIT, OP_END = 1, 2, 3, 4, 5, 6
OP_NAMES = {OP_ADD: "ADD", OP_SUB: "SUB", OP_MUL: "MUL", OP_MOV: "MOV", OP_EMIT: "EMIT", OP_END: "END"}
REG, COL, COL_NEXT, IMM, PARAM, X = 0, 1, 2, 3, 4, 5
_DST_SHIFT, _A_SHIFT, _B_SHIFT, _COL_ORACLE_SHIFT = 4, 9, 36, 22

# kind: one of REG .. X; index: register (virtual in the Assembler, physical in a Program), polynomial, pool word or param; oracle: COL / COL_NEXT only
Operand = namedtuple("Operand", "kind index oracle")
# op: OP_*; dst: a REG operand or None; a, b: operands or None
Instruction = namedtuple("Instruction", "op dst a b")


class AssemblerError(ValueError):
    pass


def encode_operand(o):
    """the 27 bits of one operand (GLP_GP_OPERAND)"""
    if o is None:
        return 0
    payload = (o.oracle << _COL_ORACLE_SHIFT | o.index) if o.kind in (COL, COL_NEXT) else o.index
    return o.kind | payload << 3


def encode(ins):
    """one instruction word (GLP_GP_INSTR)"""
    return ins.op | (ins.dst.index if ins.dst is not None else 0) << _DST_SHIFT | encode_operand(ins.a) << _A_SHIFT | encode_operand(ins.b) << _B_SHIFT


class Program:
    """An assembled program.  instructions: Instruction tuples over physical registers; code: their words, np.uint64; pool: np.uint64;
    num_regs: physical registers used (at least 1); max_live: the most virtual registers alive at once; max_constraints: the most EMITs
    in one gate."""

    def __init__(self, instructions, pool, num_regs, num_params, oracle_cols, max_live):
        self.instructions = list(instructions)
        self.pool = np.array(pool, np.uint64)
        self.num_regs, self.num_params, self.oracle_cols, self.max_live = num_regs, num_params, list(oracle_cols), max_live
        self.code = np.array([encode(i) for i in self.instructions], np.uint64)
        emits, self.max_constraints = 0, 0
        for i in self.instructions:
            if i.op == OP_EMIT:
                emits += 1
            elif i.op == OP_END:
                self.max_constraints, emits = max(self.max_constraints, emits), 0

    def __len__(self):
        return len(self.instructions)


class Assembler:
    def __init__(self, oracle_cols, num_params=0):
        self.oracle_cols = [int(c) for c in oracle_cols]
        if not 1 <= len(self.oracle_cols) <= MAX_ORACLES:
            raise AssemblerError("1..%d oracles, not %d" % (MAX_ORACLES, len(self.oracle_cols)))
        self.num_params = int(num_params)
        self.x = Operand(X, 0, 0)
        self._pool, self._pool_index = [], {}
        self._ins = []
        self._nvirt = 0

    # ---- operands
    def reg(self):
        """a fresh virtual register"""
        self._nvirt += 1
        return Operand(REG, self._nvirt - 1, 0)

    def _col(self, kind, oracle, col):
        if not 0 <= oracle < len(self.oracle_cols) or not 0 <= col < self.oracle_cols[oracle]:
            raise AssemblerError("no polynomial %d in oracle %d (oracle_cols = %s)" % (col, oracle, self.oracle_cols))
        return Operand(kind, int(col), int(oracle))

    def col(self, oracle, col):
        return self._col(COL, oracle, col)

    def col_next(self, oracle, col):
        return self._col(COL_NEXT, oracle, col)

    def imm(self, value):
        """the pool word holding value mod p, added to the pool if it is not there yet"""
        v = int(value) % P
        if v not in self._pool_index:
            self._pool_index[v] = len(self._pool)
            self._pool.append(v)
        return Operand(IMM, self._pool_index[v], 0)

    def imm_value(self, operand):
        return self._pool[operand.index]

    def param(self, j):
        if not 0 <= j < self.num_params:
            raise AssemblerError("no param %d (num_params = %d)" % (j, self.num_params))
        return Operand(PARAM, int(j), 0)

    # ---- operations
    def _push(self, op, dst, a, b):
        for o in (a, b):
            if o is not None and not isinstance(o, Operand):
                raise AssemblerError("%r is not an operand" % (o,))
        if dst is not None and (not isinstance(dst, Operand) or dst.kind != REG):
            raise AssemblerError("the destination must be a register")
        self._ins.append(Instruction(op, dst, a, b))
        return dst

    def add(self, dst, a, b):
        return self._push(OP_ADD, dst, a, b)

    def sub(self, dst, a, b):
        return self._push(OP_SUB, dst, a, b)

    def mul(self, dst, a, b):
        return self._push(OP_MUL, dst, a, b)

    def mov(self, dst, a):
        return self._push(OP_MOV, dst, a, None)

    def emit(self, a):
        self._push(OP_EMIT, None, a, None)

    def end(self, a):
        self._push(OP_END, None, a, None)

    # ---- assembly
    @staticmethod
    def _hoist(ins):
        """Every EMIT moved up to just behind the instruction that computes its operand, never past another EMIT or an END: the
        order of the EMITs, which is what numbers the constraints, stays.  A body that returns all its constraints at once (as
        zeta_identity.gate_constraints does) would otherwise keep every one of them in a register until the first is emitted."""
        out, barrier, last_write = [], 0, {}                   # barrier: index in `out` behind the latest EMIT / END
        for i in ins:
            if i.op == OP_EMIT:
                at = barrier
                if i.a.kind == REG:
                    at = max(at, last_write.get(i.a.index, -1) + 1)
                out.insert(at, i)
                for r, w in last_write.items():                # instructions behind the insertion point moved down by one
                    if w >= at:
                        last_write[r] = w + 1
                barrier = at + 1
            else:
                out.append(i)
                if i.dst is not None:
                    last_write[i.dst.index] = len(out) - 1
                if i.op == OP_END:
                    barrier = len(out)
        return out

    @staticmethod
    def _sink(ins):
        """Every instruction whose result is read exactly once, by an instruction other than EMIT or END, moved down to just before its reader (and what it alone reads with
        it); results read several times stay where they are, in their order.  A body that builds a list of products and then sums
        it (an MDS layer) keeps one product alive at a time instead of all of them.  Only for code in which no register is written
        twice (what a TraceField produces); other code is returned as it is."""
        uses, defs = {}, {}
        for idx, i in enumerate(ins):
            for o in (i.a, i.b):
                if o is not None and o.kind == REG:
                    uses[o.index] = uses.get(o.index, 0) + (1 if i.dst is not None else 2)      # an EMIT's or END's operand stays in place
            if i.dst is not None:
                if i.dst.index in defs:
                    return list(ins)
                defs[i.dst.index] = idx
        out, placed = [], set()
        for idx, i in enumerate(ins):
            if i.dst is not None and uses.get(i.dst.index, 0) == 1:
                continue                                       # placed with its one reader
            stack = [idx]
            while stack:
                top = stack[-1]
                if top in placed:
                    stack.pop()
                    continue
                need = [defs[o.index] for o in (ins[top].a, ins[top].b)
                        if o is not None and o.kind == REG and o.index in defs and defs[o.index] not in placed]
                if need:
                    stack.extend(reversed(need))               # operand a's instructions first
                else:
                    placed.add(top)
                    out.append(ins[top])
                    stack.pop()
        return out

    def assemble(self, hoist_emits=False, sink_single_use=False):
        """-> Program.  sink_single_use: see _sink (applied first); hoist_emits: see _hoist.  Linear scan: a virtual register lives from its first write to its last read (or last write); the registers
        an instruction reads for the last time are released before its destination is placed, so a result may overwrite one of its
        own operands.  Raises AssemblerError if more than MAX_REGS are alive at once, if a register is read before it is written, or
        if the program breaks a rule glp_gate_program_check would refuse it for."""
        ins = self._sink(self._ins) if sink_single_use else list(self._ins)
        if hoist_emits:
            ins = self._hoist(ins)
        if not ins or ins[-1].op != OP_END:
            raise AssemblerError("the last instruction must be END")
        if len(ins) > MAX_INSTRUCTIONS:
            raise AssemblerError("%d instructions, more than %d" % (len(ins), MAX_INSTRUCTIONS))
        first, last = {}, {}
        for i, it in enumerate(ins):
            for o in (it.a, it.b):
                if o is not None and o.kind == REG:
                    if o.index not in first:
                        raise AssemblerError("instruction %d reads virtual register %d before it is written" % (i, o.index))
                    last[o.index] = i
            if it.dst is not None:
                first.setdefault(it.dst.index, i)
                last[it.dst.index] = max(last.get(it.dst.index, i), i)
        free, phys, out, max_live, num_regs, emits = list(range(MAX_REGS)), {}, [], 0, 1, 0

        def place(o):
            return o if o is None or o.kind != REG else Operand(REG, phys[o.index], 0)
        for i, it in enumerate(ins):
            a, b = place(it.a), place(it.b)
            for o in {o.index for o in (it.a, it.b) if o is not None and o.kind == REG}:
                if last[o] == i and not (it.dst is not None and it.dst.index == o):
                    free.append(phys.pop(o))
            dst = None
            if it.dst is not None:
                v = it.dst.index
                if v not in phys:
                    if not free:
                        raise AssemblerError("instruction %d: more than %d registers are live at once" % (i, MAX_REGS))
                    free.sort()
                    phys[v] = free.pop(0)
                max_live = max(max_live, len(phys))
                num_regs = max(num_regs, phys[v] + 1)
                dst = Operand(REG, phys[v], 0)
                if last[v] == i:                               # never read: dead at once
                    free.append(phys.pop(v))
            if it.op == OP_EMIT:
                emits += 1
                if emits > MAX_CONSTRAINTS:
                    raise AssemblerError("instruction %d: more than %d EMITs in one gate" % (i, MAX_CONSTRAINTS))
            elif it.op == OP_END:
                emits = 0
            out.append(Instruction(it.op, dst, a, b))
        return Program(out, self._pool, num_regs, self.num_params, self.oracle_cols, max_live)


class TraceField:
    """The field protocol of tests' `_Fp` (zero, one, lift, add, sub, mul) over an Assembler: every operation appends one instruction
    and returns the register holding its result.  lift takes an int, which becomes an immediate, or an operand, which stays itself.
    Operations on two immediates are folded into a new immediate."""

    def __init__(self, asm):
        self.asm = asm
        self.zero, self.one = asm.imm(0), asm.imm(1)

    def lift(self, x):
        return x if isinstance(x, Operand) else self.asm.imm(int(x))

    def _op(self, emit, fold, a, b):
        a, b = self.lift(a), self.lift(b)
        if a.kind == IMM and b.kind == IMM:
            return self.asm.imm(fold(self.asm.imm_value(a), self.asm.imm_value(b)))
        return emit(self.asm.reg(), a, b)

    def add(self, a, b):
        return self._op(self.asm.add, lambda x, y: x + y, a, b)

    def sub(self, a, b):
        return self._op(self.asm.sub, lambda x, y: x - y, a, b)

    def mul(self, a, b):
        return self._op(self.asm.mul, lambda x, y: x * y, a, b)
