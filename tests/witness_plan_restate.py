"""The dataflow half of witness generation restated on the CPU (include/glp.h, "witness generation, the dataflow half"): the unit
table of glp_witness_num_units / glp_witness_unit_columns, the copy classes, the wave rule, the stuck rule and glp_witness_generate.

A unit is one independent generator of a row.  Its value is never restated here: a unit is run through witness_fill_restate.fill_row
on the row as it stands at the unit's wave, and only the unit's own output columns are kept.  The permutation comes from
witness_check_restate.decode_sigmas.  Nothing here shares code with csrc/.

The rule (cells are flat positions col * n + row):
  class wave   minimum over the members of a copy class of 0 for an input cell and the wave of the unit that writes the member; a class
               with neither is never known
  source       the member attaining that minimum, ties to the smallest flat position
  unit wave    1 + the maximum wave of the classes of the cells it reads; 1 for a unit with no inputs
  stuck        a unit reading a never-known class, and everything downstream of it (dependency cycles included); never run
  wave w       wave 0 scatters the inputs; every other wave runs its units first; then every class of wave w is copied from its
               source to all its other members
"""
import numpy as np

import limb_gates_restate as lg
import witness_check_restate as wcr
import witness_fill_restate as wfr
import zeta_identity_recursion as zr


def units(g, num_wires):
    """[(ins, outs)] per unit of a row of gate g: the columns the unit reads and writes (below num_wires)."""
    t, p0, p1 = int(g["type"]), int(g["p0"]), int(g["p1"])
    span = lambda a, cnt: list(range(a, a + cnt))
    us = []
    if t == 1:
        us = [([], span(0, p0))]
    elif t == 3:
        us = [(span(4 * i, 3), [4 * i + 3]) for i in range(p0)]
    elif t == lg.U32_INTERLEAVE:
        us = [([2 * i], [2 * i + 1] + span(2 * p0 + 32 * i, 32)) for i in range(p0)]
    elif t in (lg.UNINTERLEAVE_U32, lg.UNINTERLEAVE_B32):
        us = [([3 * i], [3 * i + 1, 3 * i + 2] + span(3 * p0 + 64 * i, 64)) for i in range(p0)]
    elif t == lg.U32_ARITHMETIC:
        us = [(span(6 * i, 3), span(6 * i + 3, 3) + span(6 * p0 + 32 * i, 32)) for i in range(p0)]
    elif t == lg.U32_ADD_MANY:
        wd = p0 + 3
        us = [(span(wd * i, p0 + 1), span(wd * i + p0 + 1, 2) + span(wd * p1 + 18 * i, 18)) for i in range(p1)]
    elif t == lg.U32_SUBTRACTION:
        us = [(span(5 * i, 3), span(5 * i + 3, 2) + span(5 * p0 + 16 * i, 16)) for i in range(p0)]
    elif t == lg.U32_RANGE_CHECK:
        us = [([i], span(p0 + 16 * i, 16)) for i in range(p0)]
    elif t == lg.RANDOM_ACCESS:
        lay = lg.random_access_layout(p0, p1)
        for c in range(lay["copies"]):
            o = lay["per_copy"] * c
            us.append(([o] + span(o + 2, lay["size"]), [o + 1] + span(lay["bits"] + p0 * c, p0)))
        us.append(([], span(lay["extras"], lay["extra"])))
    elif t in (15, 16):
        st = 8 if t == 15 else 6
        us = [(span(st * i, st - 2), span(st * i + st - 2, 2)) for i in range(p0)]
    elif t in wfr.GENERATOR_TYPES:                       # one generator per row: Poseidon, Comparison, BaseSum, Reducing*, the recursion gates
        role = wfr.roles(g, num_wires)
        us = [([c for c in range(num_wires) if role[c] == 2], [c for c in range(num_wires) if role[c] == 1])]
    return [([c for c in i if c < num_wires], [c for c in o if c < num_wires]) for i, o in us]


def unit_roles(g, num_wires, unit):
    """glp_witness_unit_columns: the roles of glp_witness_columns restricted to one unit."""
    ins, outs = units(g, num_wires)[unit]
    role = [0] * num_wires
    for c in ins:
        role[c] = 2
    for c in outs:
        role[c] = 1
    return role


def row_gates(desc):
    n = 1 << int(desc.degree_bits)
    out = np.full(n, -1, np.int64)
    for gi in range(len(desc.gates)):
        out[zr.gate_rows(desc, gi)] = gi
    return out


def classes(desc, sigma_map=None):
    """int64 [num_wires * n]: the smallest flat position of each cell's copy class (the cycles of the decoded permutation; a
    non-routed cell is a class of its own)."""
    n, nw = 1 << int(desc.degree_bits), int(desc.num_wires)
    sm = wcr.decode_sigmas(desc) if sigma_map is None else sigma_map
    cls = np.arange(nw * n, dtype=np.int64)
    seen = set()
    for (j, i) in sm:
        p = j * n + i
        if p in seen:
            continue
        cyc = []
        while p not in seen:
            seen.add(p)
            cyc.append(p)
            j2, i2 = sm[(p // n, p % n)]
            p = j2 * n + i2
        cls[cyc] = min(cyc)
    return cls


class Plan:
    pass


def all_units(desc):
    """[(row, gate, unit, in positions, out positions)] in (row, unit) order."""
    n, nw = 1 << int(desc.degree_bits), int(desc.num_wires)
    tables = [units(g, nw) for g in desc.gates]
    out = []
    for r, gi in enumerate(row_gates(desc)):
        if gi < 0:
            continue
        for u, (ins, outs) in enumerate(tables[gi]):
            out.append((r, int(gi), u, [c * n + r for c in ins], [c * n + r for c in outs]))
    return out


def default_inputs(desc, cls=None):
    """One cell per class, the smallest position, for classes that some unit reads and no unit writes."""
    cls = classes(desc) if cls is None else cls
    us = all_units(desc)
    written = {int(cls[p]) for u in us for p in u[4]}
    read = {int(cls[p]) for u in us for p in u[3]}
    return sorted(read - written)


def plan(desc, input_cells, cls=None):
    n, nw = 1 << int(desc.degree_bits), int(desc.num_wires)
    cls = classes(desc) if cls is None else cls
    us = all_units(desc)
    inputs = [int(p) for p in input_cells]
    assert len(set(inputs)) == len(inputs) and len({int(cls[p]) for p in inputs}) == len(inputs)
    class_wave = {int(cls[p]): 0 for p in inputs}
    readers = {}
    pending = []
    for k, u in enumerate(us):
        need = {int(cls[p]) for p in u[3] if int(cls[p]) not in class_wave}
        pending.append(len(need))
        for c in need:
            readers.setdefault(c, []).append(k)
    unit_wave = [-1] * len(us)
    ready = [k for k in range(len(us)) if pending[k] == 0]
    w = 0
    while ready:
        w += 1
        nxt = []
        for k in ready:
            unit_wave[k] = w
        for k in ready:
            for p in us[k][4]:
                c = int(cls[p])
                if c not in class_wave:
                    class_wave[c] = w
                    for r in readers.get(c, ()):
                        pending[r] -= 1
                        if pending[r] == 0:
                            nxt.append(r)
        ready = nxt
    pl = Plan()
    pl.desc, pl.cls, pl.units, pl.unit_wave, pl.inputs, pl.class_wave = desc, cls, us, unit_wave, inputs, class_wave
    pl.num_waves = w
    cw = np.full(nw * n, -1, np.int64)
    for p in range(nw * n):
        cw[p] = class_wave.get(int(cls[p]), -1)
    writer = {}
    for k, u in enumerate(us):
        for p in u[4]:
            assert p not in writer, "two units write one cell"
            writer[p] = k
            if unit_wave[k] >= 0:
                cw[p] = unit_wave[k]
    pl.cell_waves = cw.reshape(nw, n)
    # the source of every known class and its copies
    members = {}
    for p in range(nw * n):
        c = int(cls[p])
        if c in class_wave:
            members.setdefault(c, []).append(p)
    inset = set(inputs)
    pl.copies = {}                      # wave -> [(source, destination)]
    for c, ms in members.items():
        cwv = class_wave[c]
        src = min(p for p in ms if (cwv == 0 and p in inset) or (p in writer and unit_wave[writer[p]] == cwv))
        for p in ms:
            if p != src:
                pl.copies.setdefault(cwv, []).append((src, p))
    stuck = [k for k in range(len(us)) if unit_wave[k] < 0]
    per_wave = np.bincount([x for x in unit_wave if x > 0], minlength=w + 1) if us else np.zeros(1, np.int64)
    pl.info = dict(num_waves=w, num_units=len(us), num_stuck_units=len(stuck), num_copies=sum(len(v) for v in pl.copies.values()),
                   num_cells_known=int((cw >= 0).sum()), widest_wave_units=int(per_wave.max()) if len(per_wave) else 0,
                   stuck_row=us[stuck[0]][0] if stuck else 0, stuck_gate=us[stuck[0]][1] if stuck else 0,
                   stuck_unit=us[stuck[0]][2] if stuck else 0)
    pl.stuck = [(us[k][0], us[k][1], us[k][2]) for k in stuck]
    return pl


def generate(pl, input_values, start):
    """glp_witness_generate on a copy of `start` [num_wires][n]: input_values in the order of the plan's inputs."""
    desc = pl.desc
    n, nsel = 1 << int(desc.degree_bits), int(desc.num_selectors)
    W = np.array(start, np.uint64).copy()
    flat = W.reshape(-1)
    for p, v in zip(pl.inputs, input_values):
        flat[p] = int(v)
    by_wave = {}
    for k, wv in enumerate(pl.unit_wave):
        if wv > 0:
            by_wave.setdefault(wv, []).append(k)
    for w in range(0, pl.num_waves + 1):
        puts = []
        for k in by_wave.get(w, ()):
            r, gi, u, _, outs = pl.units[k]
            keep = {p // n for p in outs}
            row = [int(v) for v in W[:, r]]
            gc = [int(v) for v in desc.constants[nsel:, r]]
            wfr.fill_row(desc.gates[gi], gc, row, lambda col, val, r=r, keep=keep: puts.append((col, r, val)) if col in keep else None)
        for col, r, val in puts:                  # every unit of a wave reads the witness as the wave found it
            W[col, r] = val
        for src, dst in pl.copies.get(w, ()):
            flat[dst] = flat[src]
    return W
