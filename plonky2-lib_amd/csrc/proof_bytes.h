// proof_bytes.h -- the proof as bytes (util/serialization.rs): words little-endian, u8 sibling count before each Merkle path.  Reads
// the verifier's view of the circuit alone (circuit_common.h): host only, no context.  proof_from_bytes parses bytes from outside;
// examples/verify_host.cpp runs it under the host sanitizers.  The entry points glp_proof_* are in circuit_create.inc.
#pragma once
#include "circuit_common.h"

namespace {
// calls f(offset_words, count_words, kind) for the pieces of a proof in order.  PW_FIELD: field elements; PW_DIGESTS: digests of
// the proof's hasher, 4 words each (caps); PW_PATH: a Merkle path (digests, preceded by a one-byte sibling count on the wire)
enum { PW_FIELD = 0, PW_DIGESTS = 1, PW_PATH = 2 };
template <class F> void walk_proof(const CircuitCommon &cc, F f) {
    const Layout &L = cc.L;
    const glp_circuit_desc &d = cc.d;
    f((size_t)0, L.openings, PW_DIGESTS);                                   // wires, Z / partial products, quotient caps
    f(L.openings, L.fri_caps - L.openings, PW_FIELD);                       // openings
    f(L.fri_caps, L.queries - L.fri_caps, PW_DIGESTS);                      // commit-phase caps
    for (u32 q = 0; q < d.num_query_rounds; q++) {
        size_t o = L.queries + (size_t)q * L.query_stride;
        for (int k = 0; k < 4; k++) {
            f(o, (size_t)L.leaf_len[k], PW_FIELD); o += L.leaf_len[k];
            f(o, 4 * (size_t)L.depth0, PW_PATH); o += 4 * (size_t)L.depth0;
        }
        for (u32 r = 0; r < d.num_reductions; r++) {
            const size_t ev = (size_t)2 << d.reduction_arity_bits[r];
            f(o, ev, PW_FIELD); o += ev;
            f(o, 4 * (size_t)L.step_depth[r], PW_PATH); o += 4 * (size_t)L.step_depth[r];
        }
    }
    f(L.final_poly, L.total - L.final_poly, PW_FIELD);     // final poly, pow witness, public inputs
}

// bytes of one digest on the wire: a Poseidon HashOut is 4 field elements, a KeccakHash<25> digest 25 bytes
size_t digest_wire_bytes(const CircuitCommon &cc) { return cc.d.hasher == GLP_HASH_KECCAK25 ? 25 : 32; }

size_t proof_bytes_len(const CircuitCommon &cc) {
    size_t bytes = 0;
    const size_t db = digest_wire_bytes(cc);
    walk_proof(cc, [&](size_t, size_t cnt, int kind) { bytes += kind == PW_FIELD ? cnt * 8 : (cnt / 4) * db + (kind == PW_PATH ? 1 : 0); });
    return bytes;
}

int proof_to_bytes(const CircuitCommon &cc, const uint64_t *words, uint8_t *out, size_t len) {
    GLP_REQUIRE(len == proof_bytes_len(cc), "bytes_len must equal glp_proof_bytes_len()");
    size_t o = 0;
    const bool kec25 = cc.d.hasher == GLP_HASH_KECCAK25;
    walk_proof(cc, [&](size_t off, size_t cnt, int kind) {
        if (kind == PW_PATH) out[o++] = (uint8_t)(cnt / 4);
        for (size_t i = 0; i < cnt; i++) {
            const u64 w = words[off + i];
            const int nb = (kind != PW_FIELD && kec25 && (i & 3) == 3) ? 1 : 8;        // last word of a 25-byte digest: one byte
            for (int b = 0; b < nb; b++) out[o++] = (uint8_t)(w >> (8 * b));
        }
    });
    return GLP_OK;
}

int proof_from_bytes(const CircuitCommon &cc, const uint8_t *in, size_t len, uint64_t *words) {
    GLP_REQUIRE(len == proof_bytes_len(cc), "byte length does not match this circuit");
    size_t o = 0;
    int bad = 0;
    const bool kec25 = cc.d.hasher == GLP_HASH_KECCAK25;
    walk_proof(cc, [&](size_t off, size_t cnt, int kind) {
        if (kind == PW_PATH && in[o++] != (uint8_t)(cnt / 4)) bad = 1;
        for (size_t i = 0; i < cnt; i++) {
            const bool dig = kind != PW_FIELD && kec25;
            const int nb = (dig && (i & 3) == 3) ? 1 : 8;
            u64 w = 0;
            for (int b = 0; b < nb; b++) w |= (u64)in[o++] << (8 * b);
            if (!dig && w >= glf::P) bad = 2;                // field elements and Poseidon digests are canonical; Keccak digests are bytes
            words[off + i] = w;
        }
    });
    if (bad == 1) return set_error(GLP_ERR_ARG, "Merkle path length byte does not match the circuit's FRI parameters");
    if (bad == 2) return set_error(GLP_ERR_ARG, "non-canonical field element in proof bytes");
    return GLP_OK;
}
}  // namespace
