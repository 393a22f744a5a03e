"""The verifier's reading of a gate program (include/glp.h, glp_gate_program_eval_ext) and the permutation half of the vanishing
identity at zeta (glp_perm_check_zeta), restated in plain Python integers over zeta_identity._Fp2.

`run_ext` reads the Assembler's instruction list (Instruction tuples over physical registers), as gate_program_restate.run does,
never the encoded words: it shares no decoder with the library.  `perm_check` is written from the formula in the header.
tests/test_zeta_check.py pins the two together against zeta_identity.check on oracle proofs before the GPU tests rely on them."""
import numpy as np

from plonky2_lib_amd import gate_program as gp
from zeta_identity import P, _Fp2 as F, UNUSED_SELECTOR
import zeta_identity as zi

ZETA_IS_ONE = "zeta = 1"
MISMATCH = "Mismatch between evaluation and opening of quotient polynomial (challenge %d)"


def pairs(words):
    """[count][2] (or flat) words -> a list of F_p^2 elements"""
    return [(int(a), int(b)) for a, b in np.asarray(words, np.uint64).reshape(-1, 2)]


def run_ext(prog, openings, openings_next, point, alphas, params=()):
    """prog: a gate_program.Program; openings[o][c]: the opening of polynomial c of oracle o at the point, an (a, b) pair;
    openings_next[o]: the same at w_n * point, or None; point: (a, b); alphas [num_challenges]; params [num_params]
    -> [num_challenges] pairs: sum_gates filter_g sum_t alpha_c^t v_{g,t}"""
    alphas = [int(a) for a in alphas]
    regs = {}

    def value(o):
        if o.kind == gp.REG:
            return regs[o.index]
        if o.kind == gp.COL:
            return openings[o.oracle][o.index]
        if o.kind == gp.COL_NEXT:
            return openings_next[o.oracle][o.index]
        if o.kind == gp.IMM:
            return F.lift(prog.pool[o.index])
        if o.kind == gp.PARAM:
            return F.lift(params[o.index])
        assert o.kind == gp.X
        return (int(point[0]), int(point[1]))
    acc, total, t = [F.zero] * len(alphas), [F.zero] * len(alphas), 0
    for ins in prog.instructions:
        a = value(ins.a)
        if ins.op == gp.OP_ADD:
            regs[ins.dst.index] = F.add(a, value(ins.b))
        elif ins.op == gp.OP_SUB:
            regs[ins.dst.index] = F.sub(a, value(ins.b))
        elif ins.op == gp.OP_MUL:
            regs[ins.dst.index] = F.mul(a, value(ins.b))
        elif ins.op == gp.OP_MOV:
            regs[ins.dst.index] = a
        elif ins.op == gp.OP_EMIT:
            acc = [F.add(acc[c], F.mul(a, F.lift(pow(alphas[c], t, P)))) for c in range(len(alphas))]
            t += 1
        else:
            assert ins.op == gp.OP_END
            total = [F.add(total[c], F.mul(acc[c], a)) for c in range(len(alphas))]
            acc, t = [F.zero] * len(alphas), 0
    return total


def perm_sides(desc, num_chunks, zeta, sigmas, wires, zs, zs_next, quotient, betas, gammas, alphas, gate_sums=None):
    """Both sides of the identity of glp_perm_check_zeta for one proof.  desc: degree_bits, num_routed_wires, num_challenges,
    quotient_degree_factor (routed wires per partial-product chunk) and k_is; the openings are lists of pairs: sigmas and wires of the
    routed wires at least, zs the Z of every challenge then each challenge's partial products, zs_next the Z at g zeta, quotient
    [num_challenges * num_chunks]; gate_sums: None or [num_challenges] pairs.
    -> (Z_H(zeta), [(left side, right side) per challenge]); zeta must not be 1"""
    lg, nr, nch, qdf = int(desc.degree_bits), int(desc.num_routed_wires), int(desc.num_challenges), int(desc.quotient_degree_factor)
    npp = -(-nr // qdf) - 1
    k_is = [int(x) for x in desc.k_is]
    zeta = (int(zeta[0]), int(zeta[1]))
    assert zeta != F.one
    zn = zeta
    for _ in range(lg):
        zn = F.mul(zn, zn)
    zh = F.sub(zn, F.one)
    l0 = F.mul(zh, F.inv(F.mul(F.lift(1 << lg), F.sub(zeta, F.one))))
    terms = [F.mul(l0, F.sub(zs[j], F.one)) for j in range(nch)]
    for j in range(nch):
        beta, gamma = int(betas[j]), F.lift(gammas[j])
        for c in range(npp + 1):
            num, den = F.one, F.one
            for w in range(c * qdf, min((c + 1) * qdf, nr)):
                num = F.mul(num, F.add(F.add(wires[w], F.mul(zeta, F.lift(k_is[w] * beta))), gamma))
                den = F.mul(den, F.add(F.add(wires[w], F.mul(sigmas[w], F.lift(beta))), gamma))
            prev = zs[j] if c == 0 else zs[nch + j * npp + c - 1]
            nxt = zs_next[j] if c == npp else zs[nch + j * npp + c]
            terms.append(F.sub(F.mul(prev, num), F.mul(nxt, den)))
    assert len(terms) == nch * (npp + 2)
    sides = []
    for c in range(nch):
        alpha = int(alphas[c])
        van = F.zero
        for t, v in enumerate(terms):
            van = F.add(van, F.mul(v, F.lift(pow(alpha, t, P))))
        if gate_sums is not None:
            van = F.add(van, F.mul(gate_sums[c], F.lift(pow(alpha, len(terms), P))))
        q = F.zero
        for j in reversed(range(num_chunks)):
            q = F.add(F.mul(q, zn), quotient[c * num_chunks + j])
        sides.append((van, F.mul(zh, q)))
    return zh, sides


def perm_check(desc, num_chunks, zeta, *args, **kw):
    """perm_sides' arguments -> "" if the identity holds for every challenge, else the reason in glp_verify's words"""
    if (int(zeta[0]), int(zeta[1])) == F.one:
        return ZETA_IS_ONE
    for c, (left, right) in enumerate(perm_sides(desc, num_chunks, zeta, *args, **kw)[1]):
        if left != right:
            return MISMATCH % c
    return ""


def trace_circuit(desc, gate_constraints):
    """gate_program_restate.trace_circuit over another set of gate bodies (zeta_identity_recursion.gate_constraints): oracle 0 is
    constants ++ sigmas, oracle 1 the wires, the params are the public-input hash"""
    nsel, nc = int(desc.num_selectors), int(desc.num_constants)
    asm = gp.Assembler([nc, int(desc.num_wires)], num_params=4)
    T = gp.TraceField(asm)
    cs = [asm.col(0, j) for j in range(nc)]
    lw = [asm.col(1, j) for j in range(int(desc.num_wires))]
    pih = [asm.param(j) for j in range(4)]
    for g in desc.gates:
        s = cs[int(g["selector_index"])]
        filt = T.one
        for v in range(int(g["group_start"]), int(g["group_end"])):
            if v != int(g["row"]):
                filt = T.mul(filt, T.sub(T.lift(v), s))
        if nsel > 1:
            filt = T.mul(filt, T.sub(T.lift(UNUSED_SELECTOR), s))
        for v in gate_constraints(T, g, cs[nsel:], lw, pih):
            asm.emit(v)
        asm.end(filt)
    return asm.assemble(hoist_emits=True)


def proof_openings(desc, proof):
    """the opening section of a proof (include/glp.h layout) -> {name: list of pairs} for constants, sigmas, wires, zs, zs_next, pp, q"""
    lay = zi.proof_layout(desc)
    return {name: pairs(np.asarray(proof, np.uint64)[lay[name][0]:lay[name][0] + 2 * lay[name][1]])
            for name in ("constants", "sigmas", "wires", "zs", "zs_next", "pp", "q")}


def _proof_args(desc, prog, proof, digest, hasher):
    betas, gammas, alphas, zeta, pih = zi.challenges(desc, proof, digest, hasher)
    op = proof_openings(desc, proof)
    sums = run_ext(prog, [op["constants"] + op["sigmas"], op["wires"]], None, zeta, alphas, pih)
    return (desc, int(desc.quotient_degree_factor), zeta, op["sigmas"], op["wires"], op["zs"] + op["pp"], op["zs_next"], op["q"],
            betas, gammas, alphas, sums)


def check_proof(desc, prog, proof, digest, hasher=0):
    """The whole identity for one proof by the two restatements above, challenges from zeta_identity.challenges -> the reason, "" = accepted"""
    return perm_check(*_proof_args(desc, prog, proof, digest, hasher))


def with_solved_quotient(desc, prog, proof, digest, hasher=0):
    """A copy of the proof whose opening of each challenge's first quotient chunk is moved by (left - right) / Z_H(zeta), so that these
    restatements accept it: for circuits no host prover can prove.  A checker that shares nothing with them accepts the copy only if
    their left side is the vanishing polynomial's value."""
    zh, sides = perm_sides(*_proof_args(desc, prog, proof, digest, hasher))
    out = np.array(proof, np.uint64)
    o, qdf = zi.proof_layout(desc)["q"][0], int(desc.quotient_degree_factor)
    for c, (left, right) in enumerate(sides):
        at = o + 2 * c * qdf
        q0 = F.add((int(out[at]), int(out[at + 1])), F.mul(F.sub(left, right), F.inv(zh)))
        out[at], out[at + 1] = q0
    return out
