"""GPU half of the field probe: tests/device/field_probe.hip runs every primitive of csrc/glf.h, csrc/acc.h and the non-canonical Poseidon
layers of csrc/poseidon.h in a kernel of its own, one case per thread, over the operand sets of tests/field_model.py, and every output
word is compared with the model (Python integers, % P): canonical operations word for word, the _nc forms modulo p.  The operand sets
hold the non-canonical range of the _nc functions, every shift of mul_pow2_c and the worst-case operands at the term bounds of the
accumulators -- what no whole-proof test controls (test_field_probe.py asserts, on the CPU, that each named carry / borrow fires in them).

Group poseidon_layers runs the permutation of csrc/poseidon.h layer by layer over ANY u64 a layer may be handed -- the matrix-pipe layer
mds_add_wave on states of 0x00 / 0x7f / 0x80 / 0xff bytes and 2^64 - 1 in every lane of a wave, the twelve S-box chains of sbox_layer_nc, a
full round with nothing between its two layers, the six partial-round blocks plain and hooked at the all-ones state, the row-7 tail and the
round-0 constants of the proof-of-work form -- which a whole-permutation test cannot: its state passes round 0's S-boxes first.  The
matrix-pipe forms must also equal the VALU forms word for word, and the host schedule's permutation the device's.

One child process per session runs all operations; a fault, a non-zero status or its time limit fails the fixture once, every test here then
reports that failure and nothing is run again."""
import time

import pytest

import field_model as fm

pytestmark = pytest.mark.gpu

GROUPS = {
    "canonical": ("add", "sub", "neg", "dbl", "pow", "inv"),
    "extension": ("e_add", "e_sub", "e_neg", "e_mul", "e_sqr", "e_scale", "e_inv", "e_pow"),
    "reducing": ("canon", "mul", "sqr", "mul_c", "reduce128", "reduce96", "mul_2exp", "mul_pow2_c"),
    "products_nc": ("mul_nc", "mul_nc_cc", "mul_nc_chain", "mul_small_nc", "add_cnc", "range_product"),
    "folds_nc": ("fold96_nc", "fold96_c", "fold128_nc", "fold128_mad_nc"),
    "poseidon_nc": ("sbox7_nc", "mds_add_nc"),
    "accumulator_words": ("b4_value", "acc_reduce", "acc2_reduce", "acc3_reduce", "acc_add_shifted"),
    "accumulator_loops": ("acc_loop", "acc_flush", "acc2_loop", "acc2_flush", "acc3_loop", "acc3_flush"),
    "exact": ("root_of_unity", "bitrev32"),
    "poseidon_layers": ("mds_add_wave", "sbox_layer_nc", "full_round_nc", "full_round_wave") + tuple(
        "pblock_%s%s" % (t, h) for t in fm.BLOCKS for h in ("", "_hook")) + ("tail7", "pow_round0_consts", "permute_wave", "permute"),
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(directory of the one `device` run, directory of a `host` run over the same operands)"""
    exe = fm.build_probe(tmp_path_factory.mktemp("field_probe_build"))
    dev, host = tmp_path_factory.mktemp("field_probe_device"), tmp_path_factory.mktemp("field_probe_host")
    fm.write_inputs(dev, fm.DEVICE_OPS)
    t = time.time()
    out = fm.run_probe(exe, "device", dev, timeout=120)
    print("field_probe device: %.2f s wall for %d operations, %d cases" % (time.time() - t, len(fm.DEVICE_OPS), sum(len(fm.cases(n)) for n in fm.DEVICE_OPS)))
    assert "field_probe device: %d operations" % len(fm.DEVICE_OPS) in out, out
    both = [n for n in fm.HOST_OPS if n in fm.DEVICE_OPS]
    fm.write_inputs(host, both)
    fm.run_probe(exe, "host", host, timeout=300)
    return dev, host


def test_groups_cover_every_device_operation():
    assert sorted(n for g in GROUPS.values() for n in g) == sorted(fm.DEVICE_OPS)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_device_matches_the_model(runs, group):
    for name in GROUPS[group]:
        n = fm.check(name, fm.read_outputs(runs[0], name))
        print("%s: %d cases" % (name, n))


def test_host_and_device_bodies_agree_word_for_word(runs):
    """every operation that exists in both modes is canonical or exact: the two bodies (mul is reduce128 on the host and the limb form on the
    device, bitrev32 a loop and a v_bfrev) must write the same words"""
    both = [n for n in fm.HOST_OPS if n in fm.DEVICE_OPS]
    assert len(both) == 23 and all(fm.OPS[n].kind != fm.CONGRUENT for n in both)
    for name in both:
        assert fm.read_outputs(runs[0], name) == fm.read_outputs(runs[1], name), name


def test_matrix_pipe_layers_equal_the_valu_layers_word_for_word(runs):
    """poseidon.h: "(al, ah) are the integers mds_add_nc forms, so the outputs are bit-identical" -- on the whole shared operand set, not
    only modulo p; the same for a full round and for the whole permutation"""
    assert len(fm.DEVICE_OPS) == 67 and len(GROUPS["poseidon_layers"]) == 20
    for wave, valu in fm.SAME_WORDS:
        assert fm.cases(wave) == fm.cases(valu)
        a, b = fm.read_outputs(runs[0], wave), fm.read_outputs(runs[0], valu)
        if a != b:
            k = fm.OPS[wave].nout
            i = next(i for i in range(len(a)) if a[i] != b[i]) // k
            raise AssertionError("%s != %s, case %d (lane %d): operands %s -> %s against %s" % (
                wave, valu, i, i % 64, fm._hex(fm.cases(wave)[i]), fm._hex(a[i * k:i * k + k]), fm._hex(b[i * k:i * k + k])))
        print("%s == %s: %d cases" % (wave, valu, len(fm.cases(wave))))
