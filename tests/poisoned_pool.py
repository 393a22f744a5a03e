"""A `ctx` fixture whose device pool is poisoned (GLP_POOL_POISON, include/glp.h): every block the library's allocator hands out,
its own scratch, outputs and tables as well as the caller's glp_dev_alloc, holds one known byte instead of whatever a fresh hipMalloc
block or the block's last user left there, and is filled again when it comes back.

The test_gpu_poisoned_*.py modules import this fixture under the name `ctx` beside test functions (and the module-level fixtures those
use) of the existing GPU modules; pytest collects the functions again there, and they run, unchanged, on the poisoned context.  Two bytes:

    0xFF  words are non-canonical and maximal: breaks sums and counters that were never cleared, "non-zero means failed" flags and
          outputs left partly unwritten
    0x00  wins every atomicMin and defeats every "all ones means none" sentinel

The variable stays set for the fixture's lifetime, so a context a test makes for itself is poisoned too; it is restored on teardown."""
import functools
import os

import numpy as np
import pytest

import plonky2_lib_amd as glp

VAR = "GLP_POOL_POISON"
BYTES = (0xFF, 0x00)


class poisoned:
    """GLP_POOL_POISON = byte inside the with block, the earlier state of the variable after it"""

    def __init__(self, byte):
        self.byte = byte

    def __enter__(self):
        self.old = os.environ.get(VAR)
        if self.byte is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = str(self.byte)
        return self

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = self.old


def only(fn, **keep):
    """The test function `fn` once more, with fewer cases: keep[argument] is a predicate on that argument's value, applied to the rows
    of fn's parametrize marks (a row stays if every predicate that names one of its arguments holds).  For the tests whose larger
    shapes stay in their home module only."""
    @functools.wraps(fn)
    def test(*args, **kwargs):
        return fn(*args, **kwargs)

    marks, used = [], set()
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize":
            names = [s.strip() for s in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
            rows = list(m.args[1])
            if set(names) & set(keep):
                used |= set(names) & set(keep)
                ids = m.kwargs.get("ids")
                stay = [i for i, r in enumerate(rows)
                        if all(keep[a](v) for a, v in zip(names, r if len(names) > 1 else (r,)) if a in keep)]
                assert 0 < len(stay) < len(rows), (fn.__name__, names)
                kw = dict(m.kwargs)
                if isinstance(ids, (list, tuple)):
                    kw["ids"] = [ids[i] for i in stay]
                m = pytest.mark.parametrize(m.args[0], [rows[i] for i in stay], **kw).mark
        marks.append(m)
    assert used == set(keep), (fn.__name__, sorted(set(keep) - used))
    test.pytestmark = marks
    return test


def block_bytes(ctx, ptr, nbytes):
    back = np.empty(nbytes, np.uint8)
    ctx.dev_download(ptr, back)
    return back


def poisoned_ctx(salt_seed=None):
    """the module-scoped `ctx` fixture, one context per poison byte.  salt_seed: what the home module's own `ctx` fixture sets with
    set_salt_seed (test_gpu_zk, test_gpu_fri_openings, test_gpu_witness_random: their expected values are drawn from that seed)"""
    @pytest.fixture(scope="module", params=BYTES, ids=["poison-%02x" % b for b in BYTES])
    def ctx(request):
        byte = request.param
        with poisoned(byte):
            c = glp.Context(0)
            try:
                # the switch took: without this a module of re-collected tests would pass on an ordinary context
                p = c.dev_alloc(1000)
                got = block_bytes(c, p, 1000)
                c.dev_free(p)
                assert (got == byte).all(), "GLP_POOL_POISON=%d: a fresh block holds %s" % (byte, np.unique(got))
                if salt_seed is not None:
                    c.set_salt_seed(salt_seed)
                yield c
            finally:
                c.close()
    return ctx


ctx = poisoned_ctx()
