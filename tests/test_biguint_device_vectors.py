"""The vectors of tests/biguint_device_vectors.py -- what tests/test_gpu_biguint_device.py sends to the GPU -- through the host program
(csrc/examples/biguint_host.cpp, the sanitizer build of tests/test_biguint_host.py) with --per-unit: every output against Python
integers (witness_free_restate.run_free), and proof that the set reaches what it is there for.  The program reports per unit which
instance of csrc/biguint_dev.h ran it, how many quotient digits it corrected, how many of them twice, and how many add-backs it took;
the conditions below are asserted on those reports, per instance, and the counts are printed."""
import collections
import os
import subprocess

import pytest

import biguint_device_vectors as V
import witness_free_restate as fr

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(HERE, "plonky2-lib_amd", "csrc", "examples", "biguint_host.cpp")
Unit = collections.namedtuple("Unit", "index shape k all8 corrections twice add_backs")


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    """every unit of the set: its shape, its value set, and what the host program says it did"""
    exe = str(tmp_path_factory.mktemp("biguint") / "biguint_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    shs, want = V.shapes(), V.expected()
    r = subprocess.run([exe, "--per-unit"], input="\n".join(V.host_lines(shs)) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(shs) * V.K + 1
    units = []
    for i, sh in enumerate(shs):
        for k in range(V.K):
            f = got[i * V.K + k].split()
            assert [int(x, 16) for x in f[4:]] == want[i][k], "%r, value set %d: inputs %s" % (sh, k, [hex(v) for v in sh.sets[k]])
            assert f[0] == ("all8" if sh.all8 else "any"), repr(sh)
            units.append(Unit(i, sh, k, sh.all8, int(f[1]), int(f[2]), int(f[3])))
    tag, corrections, add_backs, twice = got[-1].split()
    assert tag == "stats" and (int(corrections), int(add_backs), int(twice)) == tuple(sum(getattr(u, name) for u in units) for name in ("corrections", "add_backs", "twice"))
    return units


def _operands(u):
    sh = u.shape
    return fr._big(sh.sets[u.k][:sh.len[0]]), fr._big(sh.sets[u.k][sh.len[0]:])


def test_every_output_is_what_python_integers_say(reports):
    shs = V.shapes()
    for inst in (True, False):
        mine = [sh for sh in shs if sh.all8 == inst]
        print("%s instance: %d shapes, %d units" % ("all8" if inst else "any", len(mine), len(mine) * V.K))
    assert 16 <= V.K <= 32 and len(reports) == len(shs) * V.K


def test_both_instances_reach_every_correction_branch(reports):
    for inst in (True, False):
        mine = [u for u in reports if u.all8 == inst]
        add_back, none, twice = [u for u in mine if u.add_backs], [u for u in mine if not u.corrections and not u.add_backs], [u for u in mine if u.twice]
        print("%s instance: %d units; %d with an add-back, %d with no correction at all, %d with a digit corrected twice, %d with a digit correction"
              % ("all8" if inst else "any", len(mine), len(add_back), len(none), len(twice), sum(1 for u in mine if u.corrections)))
        assert add_back and none and twice


def test_all8_corrects_at_every_kind_of_shift(reports):
    """s = 0: nothing is shifted; s = 31: all but one bit of every limb moves to its neighbour; 0 < s < 31"""
    groups = {"s = 0": lambda s: s == 0, "s = 31": lambda s: s == 31, "0 < s < 31": lambda s: 0 < s < 31}
    mine = [u for u in reports if u.all8]
    for name, inside in groups.items():
        here = [u for u in mine if inside(V.shift_of(u.shape.modulus))]
        add_back, corrected = [u for u in here if u.add_backs], [u for u in here if u.corrections]
        print("all8 instance, %s: %d units over %d moduli; %d with an add-back, %d with a digit correction"
              % (name, len(here), len({u.shape.modulus for u in here}), len(add_back), len(corrected)))
        assert add_back and corrected
    per_top = collections.Counter(u.shape.modulus >> 224 for u in mine if u.add_backs)
    print("all8 instance, units with an add-back by the modulus's top limb: %s" % {hex(t): c for t, c in sorted(per_top.items())})
    assert {V.shift_of(u.shape.modulus) for u in mine} >= {31, 30, 15, 1, 0}


def test_all8_reduces_operands_that_exceed_the_modulus(reports):
    """the 8-by-8 division in front of ADD, SUB and MUL gives a non-zero quotient"""
    for kind in (fr.ADD, fr.SUB, fr.MUL):
        over = [u for u in reports if u.all8 and u.shape.kind == kind and max(_operands(u)) >= u.shape.modulus]
        under = [u for u in reports if u.all8 and u.shape.kind == kind and max(_operands(u)) < u.shape.modulus]
        print("all8 instance, kind %d: %d units with an operand >= m, %d with both below" % (kind, len(over), len(under)))
        assert over and under
    named = {(a - u.shape.modulus, b - u.shape.modulus) for u in reports if u.all8 and u.shape.kind == fr.ADD for a, b in [_operands(u)]}
    assert {(0, 1), (-1, -1)} <= named and any(a == V.ONES for u in reports if u.all8 for a, _ in [_operands(u)])


def test_every_kind_and_every_modulus_length(reports):
    shs = V.shapes()
    assert {sh.kind for sh in shs} == set(range(2, 9))
    assert {sh.kind for sh in shs if sh.all8} == {fr.ADD, fr.SUB, fr.MUL, fr.INV}
    assert {V.num_limbs(sh.modulus) for sh in shs if sh.kind in V.HAS_MODULUS and not sh.all8} == set(range(1, 9))
    assert {sh.len[0] for sh in shs if sh.kind == fr.MULTI_ADD} == {0, 1, 3, 17}
    for sh in shs:
        if sh.kind in (fr.ADD, fr.SUB, fr.MUL) and not sh.all8 and V.num_limbs(sh.modulus) < 8:
            nm = V.num_limbs(sh.modulus)
            assert sh.len[0] in {0, 1, nm - 1, nm, nm + 1, 17, 18}
    lens = {(V.num_limbs(sh.modulus), sh.len[0]) for sh in shs if sh.kind in (fr.ADD, fr.SUB, fr.MUL) and not sh.all8}
    assert all((nm, la) in lens for nm in range(1, 8) for la in (0, 1, nm - 1, nm, nm + 1, 17, 18))
    # results truncated and zero-padded
    assert any(sh.len[2] < V.num_limbs(sh.modulus) for sh in shs if sh.kind == fr.MUL) and any(sh.len[2] > V.num_limbs(sh.modulus) for sh in shs if sh.kind == fr.MUL)
    # per kind and instance: an output cell that is not placed, and a cell with bits above bit 31
    for kind in range(2, 9):
        for inst in ((True, False) if kind in (fr.ADD, fr.SUB, fr.MUL, fr.INV) else (False,)):
            mine = [sh for sh in shs if sh.kind == kind and sh.all8 == inst]
            assert any(sh.unplaced for sh in mine), (kind, inst)
            assert any(v >> 32 for sh in mine for s in sh.sets for v in s), (kind, inst)
    assert all(v < fr.P for sh in shs for s in sh.sets for v in s)


def test_the_inverse_at_its_edges(reports):
    from math import gcd
    for inst in (True, False):
        seen = collections.Counter()
        for u in reports:
            sh = u.shape
            if sh.kind != fr.INV or u.all8 != inst or sh.len[1] < V.num_limbs(sh.modulus):
                continue
            m = sh.modulus
            x = fr._big(sh.sets[u.k]) % m
            inv = fr._big(V.expected()[u.index][u.k][:sh.len[1]])
            if x == 0:
                seen["x = 0"] += 1
                assert inv == 0
            elif gcd(x, m) != 1:
                seen["gcd(x, m) != 1"] += 1
                assert inv == 0
            else:
                assert x * inv % m == 1
                for name, at in (("x = 1", 1), ("x = m - 1", m - 1), ("x = (m + 1) / 2", (m + 1) // 2)):
                    if x == at:
                        seen[name] += 1
        print("%s instance, the inverse: %s" % ("all8" if inst else "any", dict(seen)))
        assert all(seen[name] for name in ("x = 0", "gcd(x, m) != 1", "x = 1", "x = m - 1", "x = (m + 1) / 2"))


def test_div_rem_and_glv_edges():
    shs = V.shapes()
    div = [(sh, s) for sh in shs if sh.kind == fr.DIV_REM for s in sh.sets]
    b_of = lambda sh, s: s[sh.len[0]:]
    assert any(sh.len[1] and not any(v & fr.M32 for v in b_of(sh, s)) for sh, s in div)                        # a zero divisor
    assert any(fr._big(b_of(sh, s)) and not b_of(sh, s)[-1] & fr.M32 for sh, s in div if sh.len[1])            # top declared limbs zero
    assert any(sh.len[0] < sh.len[1] for sh, s in div) and any(sh.len[:2] == [18, 8] for sh, s in div)
    assert ([3, 0, 0x80000000, 1, 0, 0x20000000] in [s for _, s in div]) and ([0, 0xFFFE0000, 0x7FFFFFFF, 0x7FFF8000, 1, 0, 0x80000000] in [s for _, s in div])
    ks = [fr._big(s) for sh in shs if sh.kind == fr.GLV for s in sh.sets]
    flips = [(a, b) for a, b in zip(ks, ks[1:]) if b == a + 1 and fr.glv_decompose(a)[2:] != fr.glv_decompose(b)[2:]]
    assert len(flips) >= 8 and any(k >= fr.FN for k in ks)
    assert {fr.glv_decompose(k % fr.FN)[2:] for k in ks} == {(0, 0), (0, 1), (1, 0), (1, 1)}
