// PRODUCT PATH — the host half of the five PlonK rounds, written once.
//
// The prover (plonk_prove_impl: k >= 1 proofs in lockstep, behind rng_prove
// with k = 1 and rng_prove_cohort) and rng_verify go through this file for
// everything that is not device choreography: the per-proof state, the
// blinder order, rounds 4 and 5, the
// linearization scalars, proof and link-hint serialization and the 9-word
// affine record.  Host-only: no HIP runtime call, no device pointer.
#pragma once
#include <vector>
#include <cstring>
#include "plonk_host.hpp"
#include "gpu_curve.hpp"

// internal to the library: nothing here joins its exported symbols
#pragma GCC visibility push(hidden)
namespace rng {

// ---- 9-u64 affine record (x, y Montgomery limbs, infinity flag) ----

inline void g1_record_store(const G1Aff& a, bool inf, uint64_t* rec) {
    if (inf) {  // canonical infinity record: zeroed coords + flag
        memset(rec, 0, 8 * 8);
        rec[8] = 1;
        return;
    }
    memcpy(rec, a.x.l, 32);
    memcpy(rec + 4, a.y.l, 32);
    rec[8] = 0;
}

// returns the infinity flag; the coordinates are copied as they stand
inline bool g1_record_load(const uint64_t* rec, G1Aff* a) {
    memcpy(a->x.l, rec, 32);
    memcpy(a->y.l, rec + 4, 32);
    return rec[8] != 0;
}

inline G1Jac g1_record_load_jac(const uint64_t* rec) {
    G1Aff a;
    return g1_record_load(rec, &a) ? G1Jac::identity() : G1Jac::from_affine(a);
}

// Jacobian -> affine with host field ops; zero coordinates at infinity
inline void jac_to_affine(const G1Jac& j, G1Aff* a, bool* inf) {
    *inf = j.Z.is_zero();
    if (*inf) {
        a->x = Fq::zero();
        a->y = Fq::zero();
        return;
    }
    Fq zinv = j.Z.inverse();
    Fq zinv2 = zinv.sqr();
    a->x = j.X.mul(zinv2);
    a->y = j.Y.mul(zinv2.mul(zinv));
}

inline void jac_to_affine_record(const G1Jac& j, uint64_t* out9) {
    G1Aff a;
    bool inf;
    jac_to_affine(j, &a, &inf);
    g1_record_store(a, inf, out9);
}

// ---- host half of a proving key ----

struct PlonkPkHost {
    uint64_t n = 0, npub = 0;
    Fr k[5];
    std::vector<Fr> selq[13], sigp[5];  // host coeffs
    std::vector<Fr> sig_evals[5];       // host evals (z build)
    G1Aff sel_comms[13], sig_comms[5];
    bool sel_inf[13] = {false}, sig_inf[5] = {false};
};

// transcript init shared with the verifier side (spec: oracle/transcript.hpp)
inline void h_transcript_init(HostTranscript& tr, const PlonkPkHost& pk, const Fr* pubs) {
    tr.append_u64(pk.n);
    tr.append_u64(pk.npub);
    for (int s = 0; s < 13; ++s) tr.append_g1(pk.sel_comms[s], pk.sel_inf[s]);
    for (int j = 0; j < 5; ++j) tr.append_g1(pk.sig_comms[j], pk.sig_inf[j]);
    for (uint64_t i = 0; i < pk.npub; ++i) tr.append_fr(pubs[i]);
}

// ---- per-proof host state ----

// Blinders in DRBG counter order.  HostDrbg::next() depends on (seed,
// counter) only, so all 17 are drawn when the state is created.
enum : int {
    BLIND_WIRES = 0,    // 0..9: wire j takes (2j, 2j + 1)
    BLIND_Z = 10,       // 10..12: (b2, b3, b4)
    BLIND_CHUNKS = 13,  // 13..16: quotient chunks 0..3
    BLIND_COUNT = 17,
};

// commitment slots of the proof (layout: include/rng_prover.h)
enum : int { COMM_WIRES = 0, COMM_Z = 5, COMM_CHUNKS = 6, COMM_WZ = 11, COMM_COUNT = 13 };

struct ProofState {
    HostTranscript tr;
    Fr blind[BLIND_COUNT];
    std::vector<Fr> wpoly[5], zpoly, quot_chunks[5];
    G1Aff comms[COMM_COUNT];
    bool inf[COMM_COUNT] = {false};
    Fr beta, gamma, alpha, zeta, v;
    Fr wire_evals[5], sigma_evals[4], z_shift_eval;

    ProofState(const PlonkPkHost& pk, const Fr* pubs, uint64_t seed) {
        h_transcript_init(tr, pk, pubs);
        HostDrbg drbg(seed);
        for (Fr& b : blind) b = drbg.next();
    }

    // copy one round's commitments into the state and absorb them
    void take_comms(int first, int count, const G1Aff* c, const bool* c_inf) {
        for (int i = 0; i < count; ++i) {
            comms[first + i] = c[i];
            inf[first + i] = c_inf[i];
            tr.append_g1(c[i], c_inf[i]);
        }
    }

    // hint = wire-0 polynomial (n+2 coeffs, Montgomery) + its commitment
    void write_link_hint(uint64_t* out) const {
        memcpy(out, wpoly[0].data(), wpoly[0].size() * sizeof(Fr));
        g1_record_store(comms[0], inf[0], out + 4 * wpoly[0].size());
    }

    // 13 records + 10 evaluations (layout: include/rng_prover.h)
    void serialize(uint64_t* out_proof) const {
        for (int i = 0; i < COMM_COUNT; ++i)
            g1_record_store(comms[i], inf[i], out_proof + 9 * i);
        uint64_t* e = out_proof + 9 * COMM_COUNT;
        for (int i = 0; i < 5; ++i) memcpy(e + 4 * i, wire_evals[i].l, 32);
        for (int i = 0; i < 4; ++i) memcpy(e + 20 + 4 * i, sigma_evals[i].l, 32);
        memcpy(e + 36, z_shift_eval.l, 32);
    }
};

// ---- linearization ----

// The scalars of the linearization D, applied to polynomials by the provers
// and to commitments by the verifier.
struct LinScalars {
    Fr sel[13];    // per selector, indexed like selq / sel_comms
    Fr z;          // z
    Fr sigma4;     // sigma_4
    Fr chunk[5];   // quotient chunks
    Fr fbar, Bbar, l1_zeta, zh_zeta;
};

inline LinScalars lin_scalars(const Fr k[5], uint64_t n, const Fr wb[5], const Fr se[4],
                              const Fr& z_shift, const Fr& beta, const Fr& gamma,
                              const Fr& alpha, const Fr& zeta) {
    LinScalars s;
    s.zh_zeta = zeta.pow_u64(n).sub(Fr::one());
    s.l1_zeta = s.zh_zeta.mul(Fr::from_u64(n).mul(zeta.sub(Fr::one())).inverse());
    auto p5 = [](const Fr& x) {
        Fr x2 = x.sqr();
        return x2.sqr().mul(x);
    };
    for (int j = 0; j < 4; ++j) s.sel[j] = wb[j];
    s.sel[4] = wb[0].mul(wb[1]);
    s.sel[5] = wb[2].mul(wb[3]);
    for (int j = 0; j < 4; ++j) s.sel[6 + j] = p5(wb[j]);
    s.sel[10] = wb[4].neg();
    s.sel[11] = Fr::one();
    s.sel[12] = wb[0].mul(wb[1]).mul(wb[2]).mul(wb[3]).mul(wb[4]);
    s.fbar = Fr::one();
    s.Bbar = Fr::one();
    for (int j = 0; j < 5; ++j)
        s.fbar = s.fbar.mul(wb[j].add(beta.mul(k[j]).mul(zeta)).add(gamma));
    for (int j = 0; j < 4; ++j) s.Bbar = s.Bbar.mul(wb[j].add(beta.mul(se[j])).add(gamma));
    s.z = alpha.mul(s.fbar).add(alpha.sqr().mul(s.l1_zeta));
    s.sigma4 = alpha.mul(beta).mul(z_shift).mul(s.Bbar).neg();
    Fr zpow = s.zh_zeta.neg();
    Fr step = zeta.pow_u64(n + 2);
    for (int i = 0; i < 5; ++i) {
        s.chunk[i] = zpow;
        zpow = zpow.mul(step);
    }
    return s;
}

// ---- R4 + R5 in three pieces, shared by the host path (rounds_4_5) and the
// device stage (open_dev in prover_api.hip) ----

// Piece 1: the ten evaluations already in the state go into the transcript
// (wires, sigma_0..3, z at zeta*w) and v is drawn.
inline void absorb_evals(ProofState& st) {
    for (int j = 0; j < 5; ++j) st.tr.append_fr(st.wire_evals[j]);
    for (int j = 0; j < 4; ++j) st.tr.append_fr(st.sigma_evals[j]);
    st.tr.append_fr(st.z_shift_eval);
    st.v = st.tr.challenge();
}

// Piece 2: the scalars of the batched opening C = D + sum v^i (opened
// polynomial i).  This is the one place that fixes the order of the 29
// polynomials, for the host loops below and for k_open_lincomb:
//   0..12  selectors            17      sigma_4        23      z
//   13..16 sigma_0..3 (v^6..9)  18..22  wires (v^1..5) 24..28  quotient chunks
enum : int {
    OPEN_SEL = 0,
    OPEN_SIGMA = 13,
    OPEN_WIRES = 18,
    OPEN_Z = 23,
    OPEN_CHUNKS = 24,
    OPEN_COUNT = 29,
    OPEN_PROOF_POLYS = 11,  // per proof: wires 0..4, z, chunks 0..4
};

inline void open_scalars(const LinScalars& ls, const Fr& v, Fr out[OPEN_COUNT]) {
    for (int i = 0; i < 13; ++i) out[OPEN_SEL + i] = ls.sel[i];
    Fr vp = Fr::one();
    for (int j = 0; j < 5; ++j) {
        vp = vp.mul(v);
        out[OPEN_WIRES + j] = vp;
    }
    for (int j = 0; j < 4; ++j) {
        vp = vp.mul(v);
        out[OPEN_SIGMA + j] = vp;
    }
    out[OPEN_SIGMA + 4] = ls.sigma4;
    out[OPEN_Z] = ls.z;
    for (int i = 0; i < 5; ++i) out[OPEN_CHUNKS + i] = ls.chunk[i];
}

// Piece 3, host form: C from the 29 scalars, then the two opening
// quotients.  polys = the proof's own 11 polynomials (wires 0..4, z, chunks
// 0..4); the other 18 are the key's.
inline void open_host(const PlonkPkHost& pk, const std::vector<Fr>* const polys[OPEN_PROOF_POLYS],
                      const Fr s[OPEN_COUNT], const Fr& zeta, const Fr& zeta_w,
                      std::vector<Fr>& Wz, std::vector<Fr>& Wzw) {
    std::vector<Fr> C;
    for (int i = 0; i < 13; ++i) hpoly_add_scaled(C, pk.selq[i], s[OPEN_SEL + i]);
    for (int j = 0; j < 5; ++j) hpoly_add_scaled(C, pk.sigp[j], s[OPEN_SIGMA + j]);
    for (int j = 0; j < OPEN_PROOF_POLYS; ++j) hpoly_add_scaled(C, *polys[j], s[OPEN_WIRES + j]);
    Wz = hpoly_div_linear(C, zeta);
    Wzw = hpoly_div_linear(*polys[5], zeta_w);
}

// R4 + R5 of one proof on the host: evaluations at zeta into the state and
// the transcript, v, the linearization D, the batched opening C, and the two
// opening quotients.  w = the n-th root of unity of the proof domain.
inline void rounds_4_5(const PlonkPkHost& pk, const Fr& w, ProofState& st,
                       std::vector<Fr>& Wz, std::vector<Fr>& Wzw) {
    const Fr zeta_w = st.zeta.mul(w);
    for (int j = 0; j < 5; ++j) st.wire_evals[j] = hpoly_eval(st.wpoly[j], st.zeta);
    for (int j = 0; j < 4; ++j) st.sigma_evals[j] = hpoly_eval(pk.sigp[j], st.zeta);
    st.z_shift_eval = hpoly_eval(st.zpoly, zeta_w);
    absorb_evals(st);

    const LinScalars ls = lin_scalars(pk.k, pk.n, st.wire_evals, st.sigma_evals,
                                      st.z_shift_eval, st.beta, st.gamma, st.alpha, st.zeta);
    Fr s[OPEN_COUNT];
    open_scalars(ls, st.v, s);
    const std::vector<Fr>* polys[OPEN_PROOF_POLYS] = {
        &st.wpoly[0], &st.wpoly[1], &st.wpoly[2], &st.wpoly[3], &st.wpoly[4], &st.zpoly,
        &st.quot_chunks[0], &st.quot_chunks[1], &st.quot_chunks[2], &st.quot_chunks[3],
        &st.quot_chunks[4]};
    open_host(pk, polys, s, st.zeta, zeta_w, Wz, Wzw);
}

}  // namespace rng
#pragma GCC visibility pop
