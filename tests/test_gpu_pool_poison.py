"""GLP_POOL_POISON (include/glp.h): the device pool's poison switch itself.  Hand-out and return are both filled, the fill reaches a
kernel's input (the canary: a commit over a block nobody wrote is the oracle's commit of constant columns), and a context made without
the variable recycles blocks as it always did.  tests/poisoned_pool.py and the test_gpu_poisoned_*.py modules rest on this."""
import ctypes as C
import os

import numpy as np
import pytest

import plonky2_lib_amd as glp
from poisoned_pool import block_bytes, poisoned

pytestmark = pytest.mark.gpu

BYTE = 0x01
NBYTES = 4096


def _hip():
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64.so not found")


def _other(nbytes, seed=5):
    """bytes that are nowhere the poison byte"""
    a = np.random.default_rng(seed).integers(2, 256, nbytes, dtype=np.uint8)
    assert not (a == BYTE).any()
    return a


def test_hand_out_is_poisoned_fresh_and_recycled():
    with poisoned(BYTE), glp.Context(0) as ctx:
        p = ctx.dev_alloc(NBYTES)
        assert (block_bytes(ctx, p, NBYTES) == BYTE).all()              # a fresh hipMalloc block
        data = _other(NBYTES)
        ctx.dev_upload(p, data)
        assert (block_bytes(ctx, p, NBYTES) == data).all()
        ctx.dev_free(p)
        q = ctx.dev_alloc(NBYTES)
        assert q == p                                                   # the size-keyed free list hands the same block out again
        assert (block_bytes(ctx, q, NBYTES) == BYTE).all()
        ctx.dev_free(q)


def test_a_size_that_is_rounded_up_is_poisoned_to_its_end():
    """the pool rounds a request up to 256 bytes: the pad a kernel may read past the request is poison too"""
    with poisoned(BYTE), glp.Context(0) as ctx:
        p = ctx.dev_alloc(1000)
        assert (block_bytes(ctx, p, 1024) == BYTE).all()
        ctx.dev_free(p)


def test_release_is_poisoned_seen_without_another_hand_out():
    """the block is read where it lies in the free list, by the HIP runtime and not through the pool: what a kernel that outlives the
    release would read.  (The pool keeps the block allocated; glp_dev_download refuses a pointer that is not handed out.)"""
    hip = _hip()
    with poisoned(BYTE), glp.Context(0) as ctx:
        p = ctx.dev_alloc(NBYTES)
        data = _other(NBYTES)
        ctx.dev_upload(p, data)
        back = np.empty(NBYTES, np.uint8)
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(NBYTES), 2) == 0      # hipMemcpyDeviceToHost
        assert (back == data).all()                                     # this reader sees the block's content
        ctx.dev_free(p)
        with pytest.raises(glp.GlpError):
            ctx.dev_download(p, back)
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(NBYTES), 2) == 0
        assert (back == BYTE).all()


def test_canary_a_never_written_block_commits_as_constant_columns(oracle):
    """poison reaches kernel inputs: 3 columns x 2^3 of a block that was allocated and never written"""
    ncols, lg, rb, ch = 3, 3, 3, 2
    word = int.from_bytes(bytes([BYTE]) * 8, "little")
    assert word == 0x0101010101010101 and word < oracle.P              # a canonical word
    ref = oracle.batch_from_values(np.full((ncols, 1 << lg), word, np.uint64), rb, ch)
    # hipMalloc may hand a new context memory that a closed one gave back, and a poisoned context gives its blocks back full of the
    # poison byte (the fill at release): without the hand-out fill the block below could hold the right words by inheritance.  An
    # unpoisoned context writes other bytes over what the driver is likely to hand out next, at this test's sizes and the earlier ones'.
    with poisoned(None), glp.Context(0) as plain:
        dirt = [(plain.dev_alloc(size), size) for size in [256] * 512 + [1024] * 16 + [NBYTES] * 16]
        for p, size in dirt:
            plain.dev_upload(p, np.full(size, 0xEE, np.uint8))
        for p, size in dirt:
            plain.dev_free(p)
    with poisoned(BYTE), glp.Context(0) as ctx:
        p = ctx.dev_alloc(ncols * 8 << lg)
        b = ctx.batch_from_values_device(p, ncols, lg, rb, ch)
        assert (b.cap() == ref.cap).all()
        assert (b.coeffs() == ref.coeffs).all()
        assert (b.digests() == ref.digests).all()
        for j in (0, 5, (1 << (lg + rb)) - 1):
            assert (b.leaf(j) == ref.leaves[j]).all() and (b.prove(j) == ref.prove(j)).all()
        b.free()
        ctx.dev_free(p)


@pytest.mark.parametrize("value", [None, "", "256", "-1", "0x10", "7 ", "ff"])
def test_unset_or_out_of_range_recycles_blocks_unchanged(value):
    """a context made without the variable (or with a value outside 0..255, which is ignored as the other switches' are) behaves as
    before: release puts the block back as it is, and the next request of that size gets it with its content"""
    with poisoned(value), glp.Context(0) as ctx:
        p = ctx.dev_alloc(NBYTES)
        data = _other(NBYTES, seed=6)
        ctx.dev_upload(p, data)
        ctx.dev_free(p)
        q = ctx.dev_alloc(NBYTES)
        assert q == p and (block_bytes(ctx, q, NBYTES) == data).all()
        ctx.dev_free(q)


def test_the_switch_is_read_when_the_context_is_made():
    """set after the context exists: not poisoned; unset after a poisoned context exists: still poisoned"""
    with poisoned(None), glp.Context(0) as plain:
        with poisoned(BYTE):
            late = glp.Context(0)
            p = plain.dev_alloc(NBYTES)
            data = _other(NBYTES, seed=7)
            plain.dev_upload(p, data)
            plain.dev_free(p)
            q = plain.dev_alloc(NBYTES)
            assert q == p and (block_bytes(plain, q, NBYTES) == data).all()
            plain.dev_free(q)
        with late:
            r = late.dev_alloc(NBYTES)
            assert (block_bytes(late, r, NBYTES) == BYTE).all()
            late.dev_free(r)
