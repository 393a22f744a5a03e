"""Reference model and operands for tests/device/field_probe.hip (shared by test_field_probe.py and test_gpu_field_probe.py).

Every expected value here is a Python integer expression `% P` of the operation's mathematical definition; nothing is imported
from the package under test and no numpy arithmetic touches a field value.

Operands per operation (`cases(name)`), rows of `OPS[name].nin` words:
  (a) the cross product of EDGES over the operands, filtered to the operation's domain (the domain its comment in glf.h / acc.h /
      poseidon.h states: canonical, any u64, or a small parameter range);
  (b) 2^16 structured-random rows, fixed seed: each 32-bit half is 0, 1, 0xFFFFFFFE or 0xFFFFFFFF with probability 3/16 each, else
      uniform -- the values at which a carry or borrow fix-up fires with probability ~1 instead of 2^-32;
  (c) 2^16 uniform rows;
  (d) constructed rows (CONSTRUCTED), named, for events (a)-(c) cannot be relied on to reach.
A canonical operand is made from a pool value v >= P by reflecting it to P - 1 - (v - P), just below p.  Extension-field operations
take pairs of canonical EDGES as elements, capped to a cross product of at most 2^16 rows, plus 2^12 uniform rows.  mds_add_nc has
12 independent folds per row, so it takes 2^13 + 2^13 rows (2 * 10^5 folds); pow runs ~96 products per row and takes 2^13 + 2^13.  The accumulator loops take a few dozen rows of up to
4096 terms each: the worst case at the term bound, and the same N with uniform and structured operands.

The layers of csrc/poseidon.h (POSEIDON_LAYER_OPS) are modelled from the round definition alone -- M = circulant(MDS_C) + 8 at [0][0], x^7,
the constants of tests/golden/poseidon_round_constants.npy -- never from the tables of namespace pblk, so make_tab / make_blk are checked
too.  `block` is the contract of a partial-round block as a plain round loop; `block_linear` propagates the same rounds symbolically and
gives the model's own row weights (`block_weight`, `fold_bound`, `block_bounds`).  mds_add_nc and mds_add_wave share ONE operand set
(`mds_layout`): the rows mds_add_nc always had, then byte states (0x00 / 0x7f / 0x80 / 0xff, 2^64 - 1, one-hot / one-cold) four times over,
shifted so that each sits in four lanes and both halves of a wave, 64 rows with opposite extremes in lanes l and l + 32, and a partial
wave at the end.  Blocks take 2^10 + 2^10 random states on top of their edges (a block is 36 to 60 S-boxes and products per row in Python).

`witnesses(name)` counts, per carry / borrow event named in WITNESS, the rows where the event fires, computing the intermediate from
the operands with Python integers.  `accumulator_bounds()` is the arithmetic behind ACC_MAX_TERMS and ACC3_MAX_TERMS.

Pass rule (`check`): canonical -> out < P and out == ref;  congruent -> out % P == ref;  exact -> out == ref.  Every case is
compared; a mismatch names the operation and the first failing operands in hex."""
import functools
import itertools
import os
import random
import re
import subprocess
import sys
from array import array
from collections import namedtuple

P = 0xFFFFFFFF00000001
EPS = 0xFFFFFFFF
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
W = 7
ACC_MAX_TERMS = 1024
ACC3_MAX_TERMS = 512
ACC_TERMS, ACC2_TERMS, ACC3_TERMS = 4096, 2 * ACC_MAX_TERMS + 3, 2 * ACC3_MAX_TERMS + 3      # row capacities of the probe
MDS_C = (17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20)
SHIFTS = (0, 22, 32, 44, 54, 76)          # acc2_reduce uses all six, acc3_reduce 0, 22, 44: nine calls
L22 = 0x3FFFFF

EDGES = tuple(dict.fromkeys((0, 1, 2, 3, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**63 - 1, 2**63, 0xFFFFFFFE00000001, 0xFFFFFFFEFFFFFFFF,
         0xFFFFFFFF00000000, P - 2, P - 3, P, P + 1, 2**64 - 2**32, 2**64 - 2, 2**64 - 1, 0x8000000080000000, 0x00000001FFFFFFFF,
         EPS, EPS - 1)))
assert len(EDGES) == 20          # four of the 24 are named twice: EPS, EPS - 1, p - 1 = 2^64 - 2^32, p - 2 = 0xFFFFFFFEFFFFFFFF
EDGES_C = tuple(v for v in EDGES if v < P)
EDGES_32 = tuple(v for v in EDGES if v <= M32)
NRANDOM = 1 << 16

Op = namedtuple("Op", "name nin nout kind host device")
CANONICAL, CONGRUENT, EXACT = "canonical", "congruent", "exact"


# ---- operand pools ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _pool(kind):
    rng = random.Random(0x676C66 + (kind == "uniform"))
    n = 4 * NRANDOM
    if kind == "uniform":
        return [rng.getrandbits(64) for _ in range(n)]
    consts = (0, 1, 0xFFFFFFFE, 0xFFFFFFFF)

    def half():
        r = rng.randrange(16)
        return consts[r // 3] if r < 12 else rng.getrandbits(32)
    return [(half() << 32) | half() for _ in range(n)]


def _canon_operand(v):
    return v if v < P else P - 1 - (v - P)


def _column(kind, name, j, n, canonical=False, mask=M64):
    pool = _pool(kind)
    off = (sum(name.encode()) * 257 + j * 10007) % len(pool)
    col = [pool[(off + i) % len(pool)] & mask for i in range(n)]
    return [_canon_operand(v) for v in col] if canonical else col


def _rows(name, domains, n=NRANDOM, edges=True):
    """domains: per operand 'any' | 'canon' | 'u32' | ('range', lo, hi) (a parameter: every value, cycled in the random rows)"""
    rows = []
    if edges:
        edge_cols = []
        for d in domains:
            edge_cols.append(EDGES if d == "any" else EDGES_C if d == "canon" else EDGES_32 if d == "u32" else tuple(range(d[1], d[2] + 1)))
        rows = list(itertools.product(*edge_cols))
    for kind in ("structured", "uniform"):
        cols = []
        for j, d in enumerate(domains):
            if isinstance(d, tuple):
                cols.append([d[1] + i % (d[2] - d[1] + 1) for i in range(n)])
            else:
                cols.append(_column(kind, name, j, n, canonical=d == "canon", mask=M32 if d == "u32" else M64))
        rows.extend(zip(*cols))
    return rows


EXT_ELEMS = tuple(itertools.product(EDGES_C, EDGES_C))


def _ext_rows(name, second):
    """second: None | 'ext' | 'canon' | 'exp' -- the second operand of an extension-field operation"""
    if second is None:
        rows = [e for e in EXT_ELEMS]
    elif second == "ext":
        step = -(-len(EXT_ELEMS) ** 2 // (1 << 16))
        rows = [x + y for x in EXT_ELEMS for y in EXT_ELEMS[::step]]
    elif second == "canon":
        rows = [x + (s,) for x in EXT_ELEMS for s in EDGES_C]
    else:       # exponent: any u64; the Python reference costs 128 extension products per row
        rows = [x + (e,) for x in EXT_ELEMS[::8] for e in EDGES]
    assert len(rows) <= 1 << 16
    n = 64 if second == "exp" else 1 << 12
    width = 2 + {None: 0, "ext": 2, "canon": 1, "exp": 1}[second]
    cols = [_column("uniform", name, j, n, canonical=not (second == "exp" and j == 2)) for j in range(width)]
    rows.extend(zip(*cols))
    return rows


def _pad(row, width):
    return tuple(row) + (0,) * (width - len(row))


def _term_rows(name, width, counts, worst, repeats=3):
    """accumulator rows over (v, m) terms: for each N the worst case, `repeats` uniform and `repeats` structured fillings"""
    rows = []
    j = 0
    for n in counts:
        rows.append(_pad((n,) + worst * n, width))
        for kind in ("uniform", "structured"):
            for _ in range(repeats):
                col = _column(kind, name, j, 2 * n)
                j += 1
                rows.append(_pad((n,) + tuple(col), width))
    return rows


def apl_words(m):
    """the four table words of one multiplier: the 22-bit limbs of m and of m' = m 2^32 mod p"""
    mp = (m << 32) % P
    return ((m & L22) | (((m >> 22) & L22) << 32), m >> 44, (mp & L22) | (((mp >> 22) & L22) << 32), mp >> 44)


def _acc3_rows(name, counts, repeats=3):
    width = 2 + 5 * ACC3_TERMS
    worst_words = (L22 | (L22 << 32), L22, L22 | (L22 << 32), L22)
    rows = []
    j = 0
    for n in counts:
        rows.append(_pad((n, 0) + ((M64,) + worst_words) * n, width))             # every table limb 2^22 - 1, v = 2^64 - 1
        rows.append(_pad((n, 1) + (M64, M64, 0, 0, 0) * n, width))               # the largest multiplier a table can be made from
        for kind in ("uniform", "structured"):
            for _ in range(repeats):
                col = _column(kind, name, j, 2 * n)
                j += 1
                terms = tuple(itertools.chain.from_iterable((col[2 * k], col[2 * k + 1], 0, 0, 0) for k in range(n)))
                rows.append(_pad((n, 1) + terms, width))
        col = _column("uniform", name, j, 5 * n)                                  # raw table words with 22-bit limbs
        j += 1
        lm = L22 | (L22 << 32)
        terms = tuple(itertools.chain.from_iterable((col[5 * k], col[5 * k + 1] & lm, col[5 * k + 2] & L22, col[5 * k + 3] & lm,
                                                     col[5 * k + 4] & L22) for k in range(n)))
        rows.append(_pad((n, 0) + terms, width))
    return rows


# ---- the Poseidon layers: round definition, blocks, operand sets ------------------------------------------------------------------
# M = circulant(MDS_C) with 8 added at [0][0];  a round is  s <- M sbox(s + rc)  (full: every element, partial: element 0 only).
MDS_M = tuple(tuple(MDS_C[(c - r) % 12] + (8 if r == c == 0 else 0) for c in range(12)) for r in range(12))
ZERO12 = (0,) * 12
# block tag -> (first partial round, K, merged with the linear layer of full round 3): the six blocks of permute_body, in order
BLOCKS = {"m3": (4, 3, True), "4a": (7, 4, False), "4b": (11, 4, False), "4c": (15, 4, False), "4d": (19, 4, False), "3": (23, 3, False)}
BYTE_WORDS = (0, 0x7F7F7F7F7F7F7F7F, 0x8080808080808080, M64, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF)
WAVE_RC = (0, P - 1, EPS)
WAVE_SHIFTS = (0, 17, 32, 45)


@functools.lru_cache(None)
def round_constants():
    """RC[r] = the twelve constants of round r, from tests/golden/poseidon_round_constants.npy (data; pinned to the reference elsewhere)"""
    import numpy as np
    rc = [int(v) for v in np.load(os.path.join(ROOT, "tests", "golden", "poseidon_round_constants.npy"))]
    assert len(rc) == 360 and all(v < P for v in rc)
    return tuple(tuple(rc[12 * r:12 * r + 12]) for r in range(30))


def _lin(s, rc):
    return [(sum(m * v for m, v in zip(MDS_M[r], s)) + rc[r]) % P for r in range(12)]


def _sbox_all(s):
    return [pow(v, 7, P) for v in s]


def block(tag, s, w=None):
    """The contract of a block, as a plain round loop: if merged s <- M s + RC[first]; then for j < K: z_j = s[0],
    s[0] <- sbox(w_j if hooked else z_j), s <- M s + RC[first + j + 1].  Returns (state, (z_0 .. z_{K-1})), all mod p."""
    first, k, merged = BLOCKS[tag]
    rc = round_constants()
    s = list(s)
    if merged:
        s = _lin(s, rc[first])
    z = []
    for j in range(k):
        z.append(s[0] % P)
        s[0] = pow(s[0] if w is None else w[j], 7, P)
        s = _lin(s, rc[first + j + 1])
    return tuple(s), tuple(z)


def rounds_from(s, start):
    """s = the state entering the S-boxes of full round `start` (0 or 1, that round's constants added) -> the permutation's output,
    chained the way permute_body chains its layers and blocks"""
    rc = round_constants()
    for r in range(start, 3):
        s = _lin(_sbox_all(s), rc[r + 1])
    s = _sbox_all(s)                              # round 3; its linear layer is the merged block's
    for tag in BLOCKS:
        s = block(tag, s)[0]
    for r in range(26, 30):
        s = _lin(_sbox_all(s), rc[r + 1] if r < 29 else ZERO12)
    return tuple(s)


def permute(s):
    return rounds_from([v + c for v, c in zip(s, round_constants()[0])], 0)


def pow_round0(r):
    """(st, pos) -> K: the state entering round 1's S-boxes is K_r + M[r][pos] sbox(candidate + RC[0][pos])"""
    rc = round_constants()
    c = [0 if i == r[12] else pow(r[i] + rc[0][i], 7, P) for i in range(12)]
    return tuple(_lin(c, rc[1]))


@functools.lru_cache(None)
def block_linear(tag):
    """The same rounds propagated symbolically: every folded row of the block as (coefficients over y_0..y_11, sigma_1..sigma_K; constant),
    first the rows z_j[0] that feed an S-box (j = 0 only if merged), then the twelve outputs.  Integer matrices, constants mod p: what
    make_tab / make_blk must have tabulated, reached without their recursion."""
    first, k, merged = BLOCKS[tag]
    rc = round_constants()
    n = 12 + k

    def mul(rows, const, add):
        return ([[sum(MDS_M[r][i] * rows[i][c] for i in range(12)) for c in range(n)] for r in range(12)],
                [(sum(MDS_M[r][i] * const[i] for i in range(12)) + add[r]) % P for r in range(12)])
    rows, const = [[int(c == i) for c in range(n)] for i in range(12)], [0] * 12
    if merged:
        rows, const = mul(rows, const, rc[first])
    zrows = []
    for j in range(k):
        if merged or j:
            zrows.append((tuple(rows[0]), const[0]))
        rows[0], const[0] = [int(c == 12 + j) for c in range(n)], 0
        rows, const = mul(rows, const, rc[first + j + 1])
    return tuple(zrows), tuple((tuple(r), c) for r, c in zip(rows, const))


def block_weight(tag):
    """the largest total coefficient weight of one folded row: the W of  al <= (2^32 - 1) W + 2^32"""
    zrows, out = block_linear(tag)
    return max(sum(coef) for coef, _ in zrows + out)


def fold_bound():
    """the largest al / ah a block can hand its fold: (2^32 - 1) W + 2^32, W the largest weight of the three table shapes"""
    return M32 * max(block_weight(t) for t in ("m3", "4a", "3")) + (1 << 32)


def block_folds(tag, s, w=None):
    """(al, ah, k) of every folded row for the entering state s, with canonical S-box outputs (the host's integers; the device's sigma
    is some u64 congruent to them): al = sum of low halves times coefficients, ah the same of the high halves, k the row's constant"""
    zrows, out = block_linear(tag)
    _, z = block(tag, s, w)
    sig = [pow(z[j] if w is None else w[j], 7, P) for j in range(BLOCKS[tag][1])]
    var = list(s) + sig
    return [(sum(c * (v & M32) for c, v in zip(coef, var)), sum(c * (v >> 32) for c, v in zip(coef, var)), k) for coef, k in zrows + out]


def host_fold_steps(al, ah, k):
    """pos::host::fold in integers: (h, t1, unwrapped t2); the u64 sums must not overflow"""
    al += k & M32
    h = ah + (al >> 32) + (k >> 32)
    assert al <= M64 and h <= M64
    return h, (h >> 32) * EPS, (((h << 32) | (al & M32)) & M64) + (h >> 32) * EPS


def _one_hot_cold(v=M64):
    return [tuple(v if k == j else 0 for k in range(12)) for j in range(12)] + [tuple(0 if k == j else v for k in range(12)) for j in range(12)]


def _state_rows(name, n=1 << 10):
    """any-u64 states: twelve equal words of every edge (2^64 - 1, p, p + 1 among them), one-hot and one-cold 2^64 - 1, n structured + n uniform"""
    return [(e,) * 12 for e in EDGES] + _one_hot_cold() + _rows(name, ("any",) * 12, n=n, edges=False)


def _canon_state_rows(name, n=1 << 10):
    one = [tuple(e if k == j else 0 for k in range(12)) for e in EDGES_C for j in range(12)]
    return [(e,) * 12 for e in EDGES_C] + one + _rows(name, ("canon",) * 12, n=n, edges=False)[n:]


def _mds_edge_block():
    """66 rows: byte states x the three constants, one-hot / one-cold 2^64 - 1, and per output row r and half the state whose half-words
    are 0xffffffff at the six largest coefficients of row r and 0 elsewhere (all other bytes 0x00)"""
    rows = [(v,) * 12 + (c,) * 12 for v in BYTE_WORDS for c in WAVE_RC]
    rows += [s + (WAVE_RC[i % 3],) * 12 for i, s in enumerate(_one_hot_cold())]
    for r in range(12):
        top = sorted(range(12), key=lambda c: -MDS_M[r][c])[:6]
        for half in (0, 1):
            rows.append(tuple((M32 << (32 * half)) if c in top else 0 for c in range(12)) + (WAVE_RC[(r + half) % 3],) * 12)
    assert len(rows) == 66
    return rows


@functools.lru_cache(None)
def mds_layout():
    """The one operand set of mds_add_nc and mds_add_wave, and where its parts lie: (rows, first row of the wave part, first rows of the
    four copies of the edge block, first row of the lane-pair stretch).  Row i runs in lane i % 64 (256 threads per block)."""
    name, n = "mds_add_nc", 1 << 13
    rows = [(e,) * 12 + (c,) * 12 for e in EDGES for c in EDGES_C]
    for kind in ("structured", "uniform"):
        rows.extend(zip(*[_column(kind, name, j, n, canonical=j >= 12) for j in range(24)]))
    wave_start = len(rows)
    filler = iter(list(zip(*[_column("uniform", "mds_add_wave", j, 512, canonical=j >= 12) for j in range(24)])))

    def fill(k):
        rows.extend(next(filler) for _ in range(k))
    edge, edge_at = _mds_edge_block(), []
    fill(-len(rows) % 64)
    for shift in WAVE_SHIFTS:                     # every edge row in four lanes, in both halves of a wave
        fill(shift)
        edge_at.append(len(rows))
        rows.extend(edge)
        fill(-len(rows) % 64)
    pair_at = len(rows)                           # lanes l and l + 32 share a column of the matrix instruction: opposite extremes in them
    lo, hi = [], []
    for l in range(32):
        c = (WAVE_RC[l % 3],) * 12
        if l < 16:
            a, b = ((0,) * 12, (M64,) * 12)[::1 if l % 2 == 0 else -1]
        else:
            a, b = ((0,) * 12 if l % 4 < 2 else (M64,) * 12, next(filler)[:12])[::1 if l % 2 == 0 else -1]
        lo.append(a + c)
        hi.append(b + c)
    rows.extend(lo + hi)
    rows.extend(edge[:33])                        # the set ends in a partial wave
    assert len(rows) % 64 == 33 and pair_at % 64 == 0
    return rows, wave_start, tuple(edge_at), pair_at


def mds_edge_lanes():
    _, _, edge_at, _ = mds_layout()
    return {(at + i) % 64 for at in edge_at for i in range(66)}


def _hook_rows(tag):
    """the block's states, each followed by the K words the hook returns: 0, 1, p - 1 (sigma = p - 1, the largest canonical S-box
    output), 2^32 - 1, 2^32 or a uniform word, one chance in six each"""
    first, k, _ = BLOCKS[tag]
    rng = random.Random(0x686F6F6B + first)
    pick = (0, 1, P - 1, M32, 1 << 32, None)
    rows = []
    for s in _state_rows("pblock_%s_hook" % tag):
        w = [pick[rng.randrange(6)] for _ in range(k)]
        rows.append(s + tuple(rng.getrandbits(64) if v is None else v for v in w))
    return rows


def _twin(row):
    return tuple(v + P if v + P <= M64 else v for v in row)


def _host_fold_rows():
    bound = fold_bound()
    rows = []
    # the two sides of t2 < t1: with a = h >> 32 >= 1, l + a (2^32 - 1) reaches 2^64 exactly at l = (2^32 - a) 2^32 + a.  h and the low
    # word are then spread over ah, al >> 32, k >> 32 and the carry of al + (u32)k in five ways.
    for a in (1, 2, 0x7FFFFFFF, (bound >> 32) - 2):
        h = (a << 32) | ((1 << 32) - a)
        for low in (a, a - 1):
            rows += [(low, h, 0), ((1 << 32) + low, h - 1, 0), (low, h - 1, 1 << 32), (low - 1 if low else 0, h, 1 if low else 0),
                     (M32, h - 1, low + 1)]
    rows += [(low, h, k) for h in (0, 1, M32) for low in (0, M32) for k in (0, M32)]          # h >> 32 = 0: t1 = 0
    rows += [(bound, bound, k) for k in (0, 1, EPS, P - 1, M64)] + [(bound, 0, 0), (0, bound, 0)]
    n = 1 << 14
    for kind in ("structured", "uniform"):
        cols = [[v % (bound + 1) for v in _column(kind, "host_fold", j, n)] for j in range(2)] + [_column(kind, "host_fold", 2, n)]
        rows.extend(zip(*cols))
    assert all(r[0] <= bound and r[1] <= bound for r in rows)
    return rows


@functools.lru_cache(None)
def _poseidon_cases(name):
    if name in ("mds_add_nc", "mds_add_wave"):
        return mds_layout()[0]
    if name == "sbox_layer_nc":                   # every edge in every one of the twelve chains
        return [tuple(EDGES[(i + j) % len(EDGES)] for j in range(12)) for i in range(len(EDGES))] + _state_rows(name)
    if name in ("full_round_nc", "full_round_wave"):
        name = "full_round_nc"
        edge = [(e,) * 12 + (c,) * 12 for e in EDGES for c in WAVE_RC]
        rnd = []
        for kind in ("structured", "uniform"):
            rnd.extend(zip(*[_column(kind, name, j, 1 << 10, canonical=j >= 12) for j in range(24)]))
        return edge + rnd
    if name == "host_mds_add":
        edge = [(e,) * 12 + (c,) * 12 for e in EDGES_C for c in EDGES_C] + [s + (P - 1,) * 12 for s in _one_hot_cold(P - 1)]
        rnd = []
        for kind in ("structured", "uniform"):
            rnd.extend(zip(*[_column(kind, name, j, 1 << 10, canonical=True) for j in range(24)]))
        return edge + rnd
    if name == "host_fold":
        return _host_fold_rows()
    if name.endswith("_hook"):
        return _hook_rows(name[len("pblock_"):-len("_hook")])
    if name.startswith("pblock_") or name.startswith("host_pblock_"):
        return _state_rows(name)
    if name in ("permute", "permute_wave"):
        return _canon_state_rows("permute")
    if name == "tail7":                           # canonical rows, their twins v + p (where that fits a u64), and non-canonical edges
        rows = _canon_state_rows(name)
        return rows + [t for r, t in zip(rows, map(_twin, rows)) if t != r] + [(e,) * 12 for e in EDGES if e >= P]
    if name == "pow_round0_consts":
        rows = _canon_state_rows(name)
        nuni = len(EDGES_C)
        return [r + (p,) for r in rows[:nuni] for p in range(8)] + [r + (i % 8,) for i, r in enumerate(rows[nuni:])]
    raise KeyError(name)


# ---- constructed rows: (operation, label, row) ----------------------------------------------------------------------------------
CONSTRUCTED = (
    ("b4_value", "all 16 limbs p - 1", (P - 1,) * 16),
    ("b4_value", "all 16 limbs 2^64 - 1", (M64,) * 16),
    ("fold128_mad_nc", "largest h: lo = hi = 2^64 - 1", (M64, M64)),
    ("fold128_nc", "borrow and carry, h0 = 0xFFFFFFFF", (0, (1 << 32) | 0xFFFFFFFF)),
    ("reduce128", "borrow and carry", (0, 0x00000001FFFFFFFF)),
    ("acc_reduce", "all words 2^32 - 1", (M32,) * 5),
    ("acc2_reduce", "all registers 2^64 - 1", (M64,) * 6),
    ("acc3_reduce", "all registers 2^64 - 1", (M64,) * 3),
) + tuple(("mul_small_nc", "g = 7", (x, 7)) for x in EDGES) + tuple(
    ("acc_add_shifted", "all words 2^32 - 1, x = 2^64 - 1, E = %d" % e, (M32,) * 5 + (M64, e)) for e in SHIFTS)


def _specs():
    ops = []

    def add(name, nin, nout, kind, host=False, device=True):
        ops.append(Op(name, nin, nout, kind, host, device))
    for name, nin in (("add", 2), ("sub", 2), ("neg", 1), ("dbl", 1), ("pow", 2), ("inv", 1)):
        add(name, nin, 1, CANONICAL, host=True)
    for name, nin in (("e_add", 4), ("e_sub", 4), ("e_neg", 2), ("e_mul", 4), ("e_sqr", 2), ("e_scale", 3), ("e_inv", 2), ("e_pow", 3)):
        add(name, nin, 2, CANONICAL, host=True)
    for name, nin in (("canon", 1), ("mul", 2), ("sqr", 1), ("reduce128", 2), ("reduce96", 2), ("mul_2exp", 2)):
        add(name, nin, 1, CANONICAL, host=True)
    for name, nin in (("mul_c", 2), ("mul_pow2_c", 2), ("b4_value", 16), ("acc_reduce", 5), ("acc2_reduce", 6), ("acc3_reduce", 3)):
        add(name, nin, 1, CANONICAL)
    for name in ("mul_nc", "mul_nc_cc", "mul_nc_chain", "fold96_nc", "fold96_c", "fold128_nc", "fold128_mad_nc", "mul_small_nc", "add_cnc",
                 "range_product"):
        add(name, 2, 1, CONGRUENT)
    add("sbox7_nc", 1, 1, CONGRUENT)
    add("mds_add_nc", 24, 12, CONGRUENT)
    add("acc_add_shifted", 7, 5, EXACT)
    add("root_of_unity", 1, 1, EXACT, host=True)
    add("bitrev32", 2, 1, EXACT, host=True)
    add("acc_loop", 1 + 2 * ACC_TERMS, 1, CANONICAL)
    add("acc_flush", 1 + 2 * ACC_TERMS, 1, CANONICAL)
    add("acc2_loop", 1 + 2 * ACC2_TERMS, 1, CANONICAL)
    add("acc2_flush", 1 + 2 * ACC2_TERMS, 1, CANONICAL)
    add("acc3_loop", 2 + 5 * ACC3_TERMS, 1, CANONICAL)
    add("acc3_flush", 2 + 5 * ACC3_TERMS, 1, CANONICAL)
    add("apl_words", 1, 4, EXACT, host=True, device=False)
    # the layers of csrc/poseidon.h
    add("mds_add_wave", 24, 12, CONGRUENT)
    add("sbox_layer_nc", 12, 12, CONGRUENT)
    add("full_round_nc", 24, 12, CONGRUENT)
    add("full_round_wave", 24, 12, CONGRUENT)
    for tag, (_, k, _) in BLOCKS.items():
        add("pblock_" + tag, 12, 12, CONGRUENT)
        add("pblock_%s_hook" % tag, 12 + k, 12 + k, CONGRUENT)
    add("tail7", 12, 1, CANONICAL)
    add("pow_round0_consts", 13, 12, CANONICAL)
    add("permute_wave", 12, 12, CANONICAL)
    add("permute", 12, 12, CANONICAL, host=True)
    add("host_fold", 3, 1, CONGRUENT, host=True, device=False)
    for tag in BLOCKS:
        add("host_pblock_" + tag, 12, 12, CONGRUENT, host=True, device=False)
    add("host_mds_add", 24, 12, CANONICAL, host=True, device=False)
    return {o.name: o for o in ops}


OPS = _specs()
HOST_OPS = tuple(n for n, o in OPS.items() if o.host)
DEVICE_OPS = tuple(n for n, o in OPS.items() if o.device)
# operations whose operand sets _poseidon_cases builds (mds_add_nc shares its set with mds_add_wave, row for row)
POSEIDON_LAYER_OPS = ("mds_add_nc",) + tuple(n for n in OPS if n in ("mds_add_wave", "sbox_layer_nc", "full_round_nc", "full_round_wave", "tail7",
                                                                   "pow_round0_consts", "permute_wave", "permute", "host_fold", "host_mds_add")
                                             or n.startswith("pblock_") or n.startswith("host_pblock_"))
# pairs that must agree word for word on their shared operand set (the header of mds_add_wave: "the outputs are bit-identical")
SAME_WORDS = (("mds_add_wave", "mds_add_nc"), ("full_round_wave", "full_round_nc"), ("permute_wave", "permute"))
# the range_product bounds the gate bodies pass: 4 (limb gates), 2^cb for 1 <= cb <= 4 (ComparisonGate), the base 2..16 of a BaseSumGate
RANGE_BOUNDS = ("range", 2, 16)

_DOMAINS = {
    "add": ("canon", "canon"), "sub": ("canon", "canon"), "neg": ("canon",), "dbl": ("canon",), "pow": ("canon", "any"), "inv": ("canon",),
    "canon": ("any",), "mul": ("any", "any"), "sqr": ("any",), "reduce128": ("any", "any"), "reduce96": ("any", "u32"),
    "mul_2exp": ("any", ("range", 0, 95)), "mul_c": ("any", "any"), "mul_pow2_c": ("any", ("range", 1, 95)),
    "acc3_reduce": ("any",) * 3, "mul_nc": ("any", "any"), "mul_nc_cc": ("any", "any"), "mul_nc_chain": ("any", "any"),
    "fold96_nc": ("any", "u32"), "fold96_c": ("any", "u32"), "fold128_nc": ("any", "any"), "fold128_mad_nc": ("any", "any"),
    "mul_small_nc": ("any", "u32"), "add_cnc": ("canon", "any"), "range_product": ("canon", RANGE_BOUNDS), "sbox7_nc": ("any",),
    "bitrev32": ("u32", ("range", 0, 32)), "apl_words": ("any",),
}


@functools.lru_cache(None)
def _base_cases(name):
    if name == "pow":               # ~96 multiplications per row on both sides: 2^13 + 2^13 rows are 10^6 products
        return _rows(name, _DOMAINS[name], n=1 << 13)
    if name in _DOMAINS:
        return _rows(name, _DOMAINS[name])
    if name in ("e_add", "e_sub", "e_mul"):
        return _ext_rows(name, "ext")
    if name in ("e_neg", "e_sqr", "e_inv"):
        return _ext_rows(name, None)
    if name == "e_scale":
        return _ext_rows(name, "canon")
    if name == "e_pow":
        return _ext_rows(name, "exp")
    if name == "b4_value":          # the full cross product is 23^16 rows: every edge on the diagonal and in every single position
        rows = [(e,) * 16 for e in EDGES] + [tuple(e if k == j else 0 for k in range(16)) for e in EDGES for j in range(16)]
        return rows + _rows(name, ("any",) * 16, edges=False)
    if name == "acc_reduce":
        return _rows(name, ("u32",) * 5)
    if name == "acc2_reduce":
        rows = [(e,) * 6 for e in EDGES] + [tuple(e if k == j else 0 for k in range(6)) for e in EDGES for j in range(6)]
        return rows + _rows(name, ("any",) * 6, edges=False)
    if name == "acc_add_shifted":
        edge = [w + (x, e) for w in ((0,) * 5, (M32,) * 5, (M32, M32, M32, M32, 0), (0, 0, 0, 0, M32)) for x in EDGES for e in SHIFTS]
        rnd = []
        for kind in ("structured", "uniform"):
            cols = [_column(kind, name, j, NRANDOM, mask=M32) for j in range(5)] + [_column(kind, name, 5, NRANDOM)]
            cols.append([SHIFTS[i % 6] for i in range(NRANDOM)])
            rnd.extend(zip(*cols))
        return edge + rnd
    if name in POSEIDON_LAYER_OPS:
        return _poseidon_cases(name)
    if name == "root_of_unity":
        return [(n,) for n in range(33)]
    worst = (M64, M64)
    if name == "acc_loop":
        return _term_rows(name, 1 + 2 * ACC_TERMS, (0, 1, 2, 1023, 1024, 1025, 4096), worst)
    if name == "acc_flush":
        return _term_rows(name, 1 + 2 * ACC_TERMS, (1024, 1025, 2048, 2 * ACC_MAX_TERMS + 3), worst)
    if name == "acc2_loop":
        return _term_rows(name, 1 + 2 * ACC2_TERMS, (0, 1, 2, 1023, 1024), worst)
    if name == "acc2_flush":
        return _term_rows(name, 1 + 2 * ACC2_TERMS, (1024, 1025, 2048, 2 * ACC_MAX_TERMS + 3), worst)
    if name == "acc3_loop":
        return _acc3_rows(name, (0, 1, 2, 511, 512))
    if name == "acc3_flush":
        return _acc3_rows(name, (512, 513, 1024, 2 * ACC3_MAX_TERMS + 3))
    raise KeyError(name)


@functools.lru_cache(None)
def cases(name, constructed=True):
    rows = _base_cases(name)
    if constructed:
        rows = [r for op, _, r in CONSTRUCTED if op == name] + rows
    assert all(len(r) == OPS[name].nin for r in rows[:4] + rows[-4:]), name
    return rows


# ---- reference ----------------------------------------------------------------------------------------------------------------
def _emul(x, y):
    return ((x[0] * y[0] + W * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def _epow(b, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = _emul(r, b)
        b = _emul(b, b)
        e >>= 1
    return r


def _einv(x):
    ni = pow((x[0] * x[0] - W * x[1] * x[1]) % P, P - 2, P)
    return (x[0] * ni % P, -x[1] * ni % P)


def _range_product(v, bound):
    r = 1
    for x in range(bound):
        r = r * (v - x) % P
    return r


def _mds_add(r):
    s, rc = r[:12], r[12:]
    return tuple((sum(s[(i + row) % 12] * MDS_C[i] for i in range(12)) + (8 * s[0] if row == 0 else 0) + rc[row]) % P for row in range(12))


def _add_shifted(r):
    t = (r[0] | (r[1] << 32) | (r[2] << 64) | (r[3] << 96) | (r[4] << 128)) + (r[5] << r[6])       # mod 2^160: w4's carry-out is dropped
    return (t & M32, (t >> 32) & M32, (t >> 64) & M32, (t >> 96) & M32, (t >> 128) & M32)


def _bitrev(x, bits):
    return int(format(x & ((1 << bits) - 1), "0%db" % bits)[::-1], 2) if bits else 0


def acc3_words(r):
    """the table words the kernel sees for row r of an acc3 loop: (v, w0..w3) per term"""
    n = min(r[0], ACC3_TERMS)
    out = []
    for k in range(n):
        v, w = r[2 + 5 * k], r[3 + 5 * k:7 + 5 * k]
        out.append((v,) + (apl_words(w[0]) if r[1] else tuple(w)))
    return out


def _acc3_sum(r):
    t = 0
    for v, w0, w1, w2, w3 in acc3_words(r):
        m = (w0 & M32) + ((w0 >> 32) << 22) + ((w1 & M32) << 44)
        mp = (w2 & M32) + ((w2 >> 32) << 22) + ((w3 & M32) << 44)
        t += (v & M32) * m + (v >> 32) * mp           # v m = vlo m + vhi m',  m' = m 2^32
    return t % P


def _terms_sum(r, cap):
    n = min(r[0], cap)
    return sum(r[1 + 2 * k] * r[2 + 2 * k] for k in range(n)) % P


POW2_GEN = pow(7, (P - 1) >> 32, P)          # plonky2's POWER_OF_TWO_GENERATOR: the generator 7 raised to the odd part of p - 1
assert pow(POW2_GEN, 1 << 31, P) == P - 1

_REF = {
    "add": lambda r: ((r[0] + r[1]) % P,), "sub": lambda r: ((r[0] - r[1]) % P,), "neg": lambda r: (-r[0] % P,),
    "dbl": lambda r: (2 * r[0] % P,), "pow": lambda r: (pow(r[0], r[1], P),), "inv": lambda r: (pow(r[0], -1, P) if r[0] else 0,),
    "e_add": lambda r: ((r[0] + r[2]) % P, (r[1] + r[3]) % P), "e_sub": lambda r: ((r[0] - r[2]) % P, (r[1] - r[3]) % P),
    "e_neg": lambda r: (-r[0] % P, -r[1] % P), "e_mul": lambda r: _emul(r[:2], r[2:]), "e_sqr": lambda r: _emul(r, r),
    "e_scale": lambda r: (r[0] * r[2] % P, r[1] * r[2] % P), "e_inv": _einv, "e_pow": lambda r: _epow(r[:2], r[2]),
    "canon": lambda r: (r[0] % P,), "mul": lambda r: (r[0] * r[1] % P,), "sqr": lambda r: (r[0] * r[0] % P,),
    "reduce128": lambda r: ((r[0] + (r[1] << 64)) % P,), "reduce96": lambda r: ((r[0] + (r[1] << 64)) % P,),
    "mul_2exp": lambda r: ((r[0] << r[1]) % P,), "mul_c": lambda r: (r[0] * r[1] % P,), "mul_pow2_c": lambda r: ((r[0] << r[1]) % P,),
    "b4_value": lambda r: (sum(v << (2 * j) for j, v in enumerate(r)) % P,),
    "acc_reduce": lambda r: (sum(v << (32 * j) for j, v in enumerate(r)) % P,),
    # a[i][j] = limb i of v (weight 2^(22 i)) times half j of m (weight 2^(32 j)); row order a00 a01 a10 a11 a20 a21
    "acc2_reduce": lambda r: (sum(r[2 * i + j] << (22 * i + 32 * j) for i in range(3) for j in range(2)) % P,),
    "acc3_reduce": lambda r: ((r[0] + (r[1] << 22) + (r[2] << 44)) % P,),
    "mul_nc": lambda r: (r[0] * r[1] % P,), "mul_nc_cc": lambda r: (r[0] * r[1] % P,), "mul_nc_chain": lambda r: (r[0] * r[1] * r[1] % P,),
    "fold96_nc": lambda r: ((r[0] + (r[1] << 64)) % P,), "fold96_c": lambda r: ((r[0] + (r[1] << 64)) % P,),
    "fold128_nc": lambda r: ((r[0] + (r[1] << 64)) % P,), "fold128_mad_nc": lambda r: ((r[0] + (r[1] << 64)) % P,),
    "mul_small_nc": lambda r: (r[0] * r[1] % P,), "add_cnc": lambda r: ((r[0] + r[1]) % P,),
    "range_product": lambda r: (_range_product(r[0], r[1]),), "sbox7_nc": lambda r: (pow(r[0], 7, P),), "mds_add_nc": _mds_add,
    "acc_add_shifted": _add_shifted,
    "root_of_unity": lambda r: (pow(POW2_GEN, 1 << (32 - r[0]), P),), "bitrev32": lambda r: (_bitrev(r[0], r[1]),),
    "acc_loop": lambda r: (_terms_sum(r, ACC_TERMS),), "acc_flush": lambda r: (_terms_sum(r, ACC_TERMS),),
    "acc2_loop": lambda r: (_terms_sum(r, ACC2_TERMS),), "acc2_flush": lambda r: (_terms_sum(r, ACC2_TERMS),),
    "acc3_loop": lambda r: (_acc3_sum(r),), "acc3_flush": lambda r: (_acc3_sum(r),),
    "apl_words": lambda r: apl_words(r[0]),
    "mds_add_wave": _mds_add, "host_mds_add": _mds_add, "sbox_layer_nc": lambda r: tuple(_sbox_all(r)),
    "full_round_nc": lambda r: _mds_add(tuple(_sbox_all(r[:12])) + r[12:]), "full_round_wave": lambda r: _mds_add(tuple(_sbox_all(r[:12])) + r[12:]),
    "tail7": lambda r: (rounds_from(r, 1)[7],), "pow_round0_consts": pow_round0, "permute": permute, "permute_wave": permute,
    "host_fold": lambda r: ((r[0] + (r[1] << 32) + r[2]) % P,),
}
for _tag in BLOCKS:
    _REF["pblock_" + _tag] = _REF["host_pblock_" + _tag] = functools.partial(lambda r, t: block(t, r)[0], t=_tag)
    _REF["pblock_%s_hook" % _tag] = functools.partial(lambda r, t: sum(block(t, r[:12], r[12:]), ()), t=_tag)
assert set(_REF) == set(OPS)


@functools.lru_cache(None)
def reference(name):
    for a, b in SAME_WORDS:         # one operand set, one definition: computed once
        if name == a:
            assert cases(a) is cases(b) or cases(a) == cases(b)
            return reference(b)
    f = _REF[name]
    return [f(r) for r in cases(name)]


# ---- branch witnesses: event -> predicate over a row, intermediates recomputed with Python integers ---------------------------
def _r128(lo, hi):
    hh, hl = hi >> 32, hi & M32
    borrow = lo < hh
    t0 = (lo - hh - (EPS if borrow else 0)) & M64
    return borrow, t0 + hl * EPS > M64


def _f128(lo, hi):             # fold128_nc(l0, l1, h0, h1): hi = h0 + 2^32 h1
    h0, h1 = hi & M32, hi >> 32
    borrow = lo < h1
    t0 = (lo - h1 - (EPS if borrow else 0)) & M64
    return borrow, t0 + h0 * EPS > M64


def _mad_h(lo, hi):            # the 97-bit y = lo + hi (2^32 - 1) and its top word h
    return (lo + hi * EPS) >> 64


def _chi(a, b):
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    mm = a0 * b1 + ((a0 * b0) >> 32)
    assert mm <= M64
    return a1 * b0 + mm > M64


_F96 = {"wraps": lambda r: r[1] * EPS + r[0] > M64, "does not wrap": lambda r: r[1] * EPS + r[0] <= M64}
WITNESS = {
    "add": {"sum wraps 2^64": lambda r: r[0] + r[1] > M64, "sum in [p, 2^64)": lambda r: P <= r[0] + r[1] <= M64,
            "sum below p": lambda r: r[0] + r[1] < P},
    "sub": {"a < b": lambda r: r[0] < r[1], "a >= b": lambda r: r[0] >= r[1]},
    "reduce128": {"borrow only": lambda r: _r128(*r) == (True, False), "carry only": lambda r: _r128(*r) == (False, True),
                  "borrow and carry": lambda r: _r128(*r) == (True, True), "neither": lambda r: _r128(*r) == (False, False)},
    "reduce96": _F96, "fold96_nc": _F96, "fold96_c": _F96,
    "fold128_nc": {"borrow only": lambda r: _f128(*r) == (True, False), "carry only": lambda r: _f128(*r) == (False, True),
                   "borrow and carry": lambda r: _f128(*r) == (True, True), "neither": lambda r: _f128(*r) == (False, False),
                   "h0 = 0": lambda r: r[1] & M32 == 0, "h0 != 0": lambda r: r[1] & M32 != 0},
    "fold128_mad_nc": {"first carry 0": lambda r: (r[1] & M32) * EPS + r[0] <= M64, "first carry 1": lambda r: (r[1] & M32) * EPS + r[0] > M64,
                       "h = 0": lambda r: _mad_h(*r) == 0, "h = 2^32 - 1 (largest)": lambda r: _mad_h(*r) == M32},
    "mul_nc_cc": {"chi = 0": lambda r: not _chi(*r), "chi = 1": lambda r: _chi(*r)},
    "add_cnc": {"wraps": lambda r: r[0] + r[1] > M64, "does not wrap": lambda r: r[0] + r[1] <= M64},
    "mul_small_nc": {"g = 0": lambda r: r[1] == 0, "g = 1": lambda r: r[1] == 1, "g = 7": lambda r: r[1] == 7, "g = 2^32 - 1": lambda r: r[1] == M32},
    "b4_value": {"all 16 limbs p - 1": lambda r: all(v == P - 1 for v in r)},
}
assert (M64 + M64 * EPS) >> 64 == M32          # h cannot exceed 2^32 - 1: y <= 2^96 - 2^32


def _fold_events(units):
    """units: (64-bit word, top word) handed to a 96-bit fold"""
    n = sum(1 for u in units if _F96["wraps"](u))
    return {"final fold wraps": (n, len(units)), "final fold does not wrap": (len(units) - n, len(units))}


def wave_row(row):
    """mds_add_wave in integers, for one row: per output row r and half the four byte dot products D_b (circulant part, bytes as u - 128),
    the partial sum x = D_0 + 2^8 D_1 (+ the low half's overflow), and the pair (al, ah); asserts that (al, ah) are the integers
    mds_add_nc forms, which is the claim of the header."""
    s, rc = row[:12], row[12:]
    bias = 128 * 256 * 0x01010101
    out = []
    for r in range(12):
        al = ah = 0
        for half in (0, 1):
            w = [(v >> (32 * half)) & M32 for v in s]
            d = [sum(MDS_C[(c - r) % 12] * (((w[c] >> (8 * b)) & 0xFF) - 128) for c in range(12)) for b in range(4)]
            carry = al >> 32 if half else 0
            assert carry < 1 << 31
            x = d[0] + (d[1] << 8) + carry
            v = x + bias + ((rc[r] >> (32 * half)) & M32) + (8 * w[0] if r == 0 else 0) + ((d[2] + (d[3] << 8)) << 16)
            assert v == sum(m * u for m, u in zip(MDS_M[r], w)) + ((rc[r] >> (32 * half)) & M32) + carry and 0 <= v <= M64
            out.append((r, half, d, x))
            if half:
                ah = v
            else:
                al = v
        out[-1] += (((ah << 32) | (al & M32)) & M64, ah >> 32)
    return out


def _wave_witnesses():
    rows, start, _, _ = mds_layout()
    rows = rows[start:]              # the wave part: edge blocks, lane pairs and their uniform filler (~1200 dot products per row in Python)
    dmin = dmax = xneg = nd = nx = 0
    folds = []
    for row in rows:
        for t in wave_row(row):
            nd += 4
            dmin += sum(1 for v in t[2] if v == -32768)
            dmax += sum(1 for v in t[2] if v == 127 * 256)
            nx += 1
            xneg += t[3] < 0
            if len(t) > 4:
                folds.append(t[4:])
    out = {"D = -32768": (dmin, nd), "D = 127 * 256": (dmax, nd), "x negative": (xneg, nx), "x non-negative": (nx - xneg, nx),
           "8 lo0 >= 2^32": (sum(1 for r in rows if 8 * (r[0] & M32) > M32), len(rows)),
           "8 hi0 >= 2^32": (sum(1 for r in rows if 8 * (r[0] >> 32) > M32), len(rows))}
    out.update(_fold_events(folds))
    return out


def _block_witnesses(tag, hooked):
    name = "pblock_%s%s" % (tag, "_hook" if hooked else "")
    folds = []
    for r in cases(name):
        for al, ah, k in block_folds(tag, r[:12], r[12:] if hooked else None):
            al += k & M32
            ah += (al >> 32) + (k >> 32)
            assert ah <= M64
            folds.append((((ah << 32) | (al & M32)) & M64, ah >> 32))
    return _fold_events(folds)


def _host_fold_witnesses():
    steps = [host_fold_steps(*r) for r in cases("host_fold")]
    n = len(steps)
    wraps, hzero = sum(1 for h, t1, t2 in steps if t2 > M64), sum(1 for h, t1, t2 in steps if h >> 32 == 0)
    return {"t2 < t1": (wraps, n), "t2 >= t1": (n - wraps, n), "h >> 32 = 0": (hzero, n), "h >> 32 != 0": (n - hzero, n)}


WITNESS["mds_add_wave"] = _wave_witnesses
WITNESS["host_fold"] = _host_fold_witnesses
for _tag in BLOCKS:
    WITNESS["pblock_" + _tag] = functools.partial(_block_witnesses, _tag, False)
    WITNESS["pblock_%s_hook" % _tag] = functools.partial(_block_witnesses, _tag, True)


def witnesses(name, constructed=True):
    """event -> rows in which it fires; for the Poseidon layers event -> (units in which it fires, units), a unit being one fold, one byte dot
    product or one half of one output row"""
    if callable(WITNESS[name]):
        return WITNESS[name]()
    rows = cases(name, constructed)
    return {event: sum(1 for r in rows if f(r)) for event, f in WITNESS[name].items()}


def block_bounds():
    """The overflow bound of the blocks from the model's own matrices: per table shape the largest row weight W (below 2^32 - 2, so that
    al <= (2^32 - 1) W + 2^32 and ah fit 64 bits), reached exactly by the all-ones state of the operand sets."""
    out = {}
    for tag in BLOCKS:
        w = block_weight(tag)
        assert w + 2 < 1 << 32, (tag, w)
        ones = (M64,) * 12
        assert ones in cases("pblock_" + tag) and ones in cases("host_pblock_" + tag)
        zrows, rows = block_linear(tag)
        top = 0
        for (coef, k), (al, ah, k2) in zip(zrows + rows, block_folds(tag, ones)):
            sig = [pow(z, 7, P) for z in block(tag, ones)[1]]
            ypart = al - sum(c * (v & M32) for c, v in zip(coef[12:], sig))
            assert k == k2 and ypart == M32 * sum(coef[:12]), tag          # every half 2^32 - 1: the y-part is (2^32 - 1) x (row sum of G)
            assert al + (k & M32) <= M32 * w + (1 << 32) and ah + (k >> 32) + (1 << 32) <= M32 * w + (1 << 33)
            top = max(top, sum(coef[:12]))
        out[tag] = (w, top)
    return out


def accumulator_bounds():
    """The arithmetic behind the term bounds, as a dict of the largest register values; asserts that each bound holds and is tight."""
    prod = (2**22 - 1) * (2**32 - 1)                       # the largest product one v_mad_u64_u32 adds to an AccLimb / AccHL register
    out = {"acc2 at 1024": prod * ACC_MAX_TERMS, "acc2 at 1025": prod * (ACC_MAX_TERMS + 1),
           "acc3 at 512": 2 * prod * ACC3_MAX_TERMS, "acc3 at 513": 2 * prod * (ACC3_MAX_TERMS + 1),
           "acc160 at 4096": 4096 * M64 * M64}
    assert out["acc2 at 1024"] < 2**64 <= out["acc2 at 1025"]
    assert out["acc3 at 512"] < 2**64 <= out["acc3 at 513"]
    assert out["acc160 at 4096"] < 2**160
    # the worst-case rows reach exactly these: limbs (0x3FFFFF, 0x3FFFFF, 0xFFFFF) of v = 2^64 - 1 against both halves of m = 2^64 - 1
    v = M64
    assert (v & L22, (v >> 22) & L22, v >> 44) == (0x3FFFFF, 0x3FFFFF, 0xFFFFF)
    return out


# ---- files and the probe --------------------------------------------------------------------------------------------------------
def _to_bytes(words):
    a = array("Q", words)
    assert a.itemsize == 8
    if sys.byteorder != "little":
        a.byteswap()
    return a.tobytes()


def write_inputs(directory, names):
    for name in names:
        with open(os.path.join(directory, name + ".in"), "wb") as f:
            f.write(_to_bytes(itertools.chain.from_iterable(cases(name))))


def read_outputs(directory, name):
    a = array("Q")
    with open(os.path.join(directory, name + ".out"), "rb") as f:
        a.frombytes(f.read())
    if sys.byteorder != "little":
        a.byteswap()
    return a


def check(name, out):
    """out: the flat words of <name>.out.  Compares every case by the operation's pass rule."""
    op, rows, ref = OPS[name], cases(name), reference(name)
    assert len(out) == len(rows) * op.nout, "%s: %d words out for %d cases of %d" % (name, len(out), len(rows), op.nout)
    k = op.nout
    if out == array("Q", itertools.chain.from_iterable(ref)):      # word for word the canonical value: passes every rule
        return len(rows)
    for i, want in enumerate(ref):
        got = tuple(out[i * k:i * k + k])
        if got == want:
            continue
        if op.kind == CONGRUENT and all(g % P == w for g, w in zip(got, want)):
            continue
        shown = rows[i] if op.nin <= 24 else rows[i][:2] + ("... %d words" % op.nin,)
        raise AssertionError("%s (%s), case %d of %d: operands %s -> %s, expected %s" % (
            name, op.kind, i, len(rows), _hex(shown), _hex(got), _hex(want)))
    return len(rows)


def _hex(t):
    return "(" + ", ".join(v if isinstance(v, str) else hex(v) for v in t) + ")"


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky2-lib_amd", "csrc")


def build_probe(directory, extra_flags=()):
    """Compiles tests/device/field_probe.hip into `directory` with the CXXFLAGS of csrc/Makefile minus -fPIC; returns the program."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(\w+) \?= (.*)$", mk, re.M)}
    flags = [f for f in var["CXXFLAGS"].replace("$(ARCH)", var["ARCH"]).split() if f != "-fPIC"]
    exe = os.path.join(str(directory), "field_probe")
    cmd = [os.environ.get("HIPCC", var["HIPCC"])] + flags + list(extra_flags) + ["-I", CSRC, os.path.join(ROOT, "tests", "device", "field_probe.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "building field_probe failed:\n%s\n%s" % (" ".join(cmd), r.stderr[-4000:])
    return exe


def run_probe(exe, mode, directory, timeout):
    """One fresh child process; a signal, a non-zero status or the time limit is an AssertionError (nothing is run again)."""
    try:
        r = subprocess.run([exe, mode, str(directory)], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        raise AssertionError("field_probe %s did not end within %d s" % (mode, timeout))
    assert r.returncode == 0, "field_probe %s ended with status %d:\n%s%s" % (mode, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout
