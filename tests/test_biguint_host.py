"""csrc/biguint_dev.h -- the limb arithmetic of the free units of witness generation -- compiled into a plain host program
(csrc/examples/biguint_host.cpp, built with -fsanitize=address,undefined and run directly) and compared with Python integers
(witness_free_restate.run_free) on structured and random limbs, every length from 0 to 18, both secp256k1 moduli and two short odd
ones, and the named edges of every kind.  The division estimates quotient digits and corrects them: the program counts how often each
correction branch ran, and both counts must be non-zero, or the vectors would not have reached that code.

EQUALITY is field arithmetic and lives in witness.hip, not in the header: it has no host instance."""
import os
import subprocess

import numpy as np
import pytest

import witness_free_restate as fr

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(HERE, "plonky2-lib_amd", "csrc", "examples", "biguint_host.cpp")
FP = 2 ** 256 - 2 ** 32 - 977
FN = fr.FN
SPECIAL = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF]
MODULI = [FP, FN, 0xFFFFFFFB, (0x80000000 << 64) | (0xFFFFFFFF << 32) | 0x7FFFFFFF]      # 8, 8, 1 and 3 limbs, all odd


def _limbs(v, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def _mod_limbs(m):
    return _limbs(m, (m.bit_length() + 31) // 32)


def _draw(rng, n, mode):
    """n limbs: mode 0 structured, 1 random, 2 mixed"""
    out = []
    for _ in range(n):
        if mode == 0 or (mode == 2 and rng.integers(2)):
            out.append(SPECIAL[int(rng.integers(len(SPECIAL)))])
        else:
            out.append(int(rng.integers(0, 1 << 32)))
    return out


def vectors():
    """[(kind, modulus, len[6], input cells)]"""
    rng = np.random.default_rng(24)
    out = []
    nonnative = lambda kind, m, a, b, lo=None: out.append(
        (kind, m, [len(a), len(b), 8 if lo is None else lo[0], (8 if kind == fr.MUL else 1) if lo is None else lo[1], 0, 0], a + b))
    for m in MODULI:
        ml = len(_mod_limbs(m))
        L = lambda v: _limbs(v, ml)
        edges = [(m - 1, m - 1), (1, m - 1), (2, m - 1), (m - 1, 0), (0, 0), (3, 5), (5, 3), (7, 7), (m // 2, m // 2 + 1), (m // 2 + 1, m // 2 + 1)]
        for kind in (fr.ADD, fr.SUB, fr.MUL):
            for a, b in edges:                       # a = b = m - 1, a + b = m, a + b = m + 1, a < b, a = b, ...
                nonnative(kind, m, L(a), L(b), (ml, ml if kind == fr.MUL else 1))
            for mode in (0, 1, 2):
                for _ in range(12):
                    nonnative(kind, m, _draw(rng, 8, mode), _draw(rng, 8, mode))             # unreduced 8-limb operands
                for la in range(0, 19):
                    for lb in (0, 1, ml, 18) if mode else range(0, 19):
                        nonnative(kind, m, _draw(rng, la, mode), _draw(rng, lb, mode), (int(rng.integers(0, 19)), int(rng.integers(0, 19)) if kind == fr.MUL else 1))
        for x in [1, m - 1, 0, 2, m // 2, m // 2 + 1, 3, m - 2] + [int.from_bytes(rng.bytes(40), "little") for _ in range(12)]:
            out.append((fr.INV, m, [ml if x < m else 10, ml, ml, 0, 0, 0], _limbs(x, ml if x < m else 10)))
        for mode in (0, 2):
            for lx in range(0, 19):
                out.append((fr.INV, m, [lx, int(rng.integers(0, 19)), int(rng.integers(0, 19)), 0, 0, 0], _draw(rng, lx, mode)))
        for cnt in (0, 1, 2, 3, 17):
            for ll in (0, 1, 8, 18):
                out.append((fr.MULTI_ADD, m, [cnt, ll, ml, 1, 0, 0], [v for _ in range(cnt) for v in _draw(rng, ll, 2)]))
        out.append((fr.MULTI_ADD, m, [3, ml, ml, 1, 0, 0], L(m - 1) * 3))
    out.append((fr.INV, 15, [1, 1, 1, 0, 0, 0], [5]))                    # gcd(x, m) != 1: inv = div = 0
    out.append((fr.INV, 15, [1, 1, 1, 0, 0, 0], [4]))
    # BIGUINT_DIV_REM: every pair of lengths, the divisor's top limbs zero or not, divisor 0, a shorter dividend, a quotient with zero
    # top limbs, and the classic digit-correction cases
    for la in range(0, 19):
        for lb in range(0, 9):
            for mode in (0, 1, 2):
                a, b = _draw(rng, la, mode), _draw(rng, lb, mode)
                out.append((fr.DIV_REM, 0, [la, lb, max(la - lb + 1, 0) if lb <= la + 1 else 0, lb, 0, 0], a + b))
    out.append((fr.DIV_REM, 0, [8, 4, 5, 4, 0, 0], _draw(rng, 8, 1) + [0, 0, 0, 0]))                       # divisor 0
    out.append((fr.DIV_REM, 0, [2, 6, 0, 6, 0, 0], _draw(rng, 2, 1) + _draw(rng, 6, 1)))                   # dividend shorter than divisor
    out.append((fr.DIV_REM, 0, [8, 2, 7, 2, 0, 0], [5, 6, 7, 0, 0, 0, 0, 0] + [9, 1]))                      # quotient with zero top limbs
    out.append((fr.DIV_REM, 0, [3, 3, 1, 3, 0, 0], [3, 0, 0x80000000] + [1, 0, 0x20000000]))               # the add-back case
    out.append((fr.DIV_REM, 0, [4, 3, 2, 3, 0, 0], [0, 0xFFFE0000, 0x80000000 - 1, 0x7FFF8000][:4] + [1, 0, 0x80000000]))
    out.append((fr.DIV_REM, 0, [18, 8, 11, 8, 0, 0], [0xFFFFFFFF] * 18 + [0xFFFFFFFF] * 8))
    out.append((fr.DIV_REM, 0, [4, 1, 2, 1, 0, 0], [1 << 40, 7, 1 << 63, 9] + [3]))                         # cells >= 2^32: the low 32 bits; quotient truncated
    # GLV: 0, 1, n - 1, values either side of the sign flips of k1 and k2 (found by bisection on the restated decomposition)
    ks = [0, 1, 2, FN - 1, FN - 2, FN // 2, FN // 2 + 1, FN, FN + 5, 2 ** 256 - 1] + [int.from_bytes(rng.bytes(32), "little") for _ in range(24)]
    for which in (2, 3):
        for _ in range(6):
            lo, hi = sorted(int.from_bytes(rng.bytes(32), "little") % FN for _ in range(2))
            if fr.glv_decompose(lo)[which] == fr.glv_decompose(hi)[which]:
                continue
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if fr.glv_decompose(mid)[which] == fr.glv_decompose(lo)[which]:
                    lo = mid
                else:
                    hi = mid
            ks += [lo, hi]
    for k in ks:
        out.append((fr.GLV, 0, [8, 4, 4, 1, 1, 0], _limbs(k, 8)))
    out.append((fr.GLV, 0, [8, 4, 4, 1, 1, 0], [v | (5 << 32) for v in _limbs(FN - 3, 8)]))
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("biguint") / "biguint_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    return exe


def test_sign_flips_are_among_the_vectors():
    ks = [fr._big(v[3]) for v in vectors() if v[0] == fr.GLV]
    flips = [(a, b) for a, b in zip(ks, ks[1:]) if b == a + 1 and fr.glv_decompose(a)[2:] != fr.glv_decompose(b)[2:]]
    assert len(flips) >= 4
    assert {fr.glv_decompose(k)[2:] for k in ks} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_restated_glv_is_the_builders():
    import plonky2_lib_amd.gadgets_ecdsa as ge
    rng = np.random.default_rng(3)
    for k in [0, 1, FN - 1] + [int.from_bytes(rng.bytes(32), "little") % FN for _ in range(50)]:
        assert fr.glv_decompose(k) == tuple(int(x) for x in ge.decompose_secp256k1_scalar(k))


def test_every_kind_against_python_integers(program):
    vs = vectors()
    lines = []
    for kind, m, ln, ins in vs:
        ml = _mod_limbs(m) if kind in (fr.ADD, fr.MULTI_ADD, fr.SUB, fr.MUL, fr.INV) else []
        lines.append(" ".join("%x" % v for v in [kind, len(ml)] + ml + ln + ins))
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(vs) + 1
    kinds = set()
    for i, (kind, m, ln, ins) in enumerate(vs):
        want = fr.run_free(kind, ln, m, ins)
        assert [int(x, 16) for x in got[i].split()] == want, (i, kind, hex(m), ln, [hex(v) for v in ins])
        kinds.add(kind)
    assert kinds == {fr.ADD, fr.MULTI_ADD, fr.SUB, fr.MUL, fr.INV, fr.DIV_REM, fr.GLV}
    tag, digit, add_back = got[-1].split()
    print("digit corrections %s, add-backs %s over %d units" % (digit, add_back, len(vs)))
    assert tag == "stats" and int(digit) > 0 and int(add_back) > 0
