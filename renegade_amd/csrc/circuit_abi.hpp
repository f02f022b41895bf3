// PRODUCT PATH — circuit-construction C ABI (include/rng_prover.h): the
// rng_circ_build_* / rng_witness_statement* / rng_circ_from_scalars family,
// the Rd/Wt cursors, LinkLayouts, the jubjub, Schnorr and ElGamal test hooks
// and the table getters.  Host-only: no HIP call, no context, no
// thread-local scratch.  Included by prover_api.hip inside its
// `extern "C"` block, after `using namespace rng`; not a stand-alone header.
#pragma once

// ---- circuit construction (arithmetization front-end) ----
// The tables handle wraps rng::CircuitTables; getters copy flat arrays out
// so tests (and the oracle prover) consume identical inputs.

void* rng_testcirc_build(uint64_t seed, uint64_t scale) {
    try {
        PlonkCircuit cs;
        build_mixed_circuit(cs, seed, scale);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_testcirc_build: %s\n", why.c_str());
            return nullptr;
        }
        auto* t = new CircuitTables(cs.finalize());
        return t;
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_testcirc_build: %s\n", e.what());
        return nullptr;
    }
}

// `Valid Balance Create` circuit builder (zk_circuits/valid_balance_create.rs)
// with fixed-seed witness/statement; returns finalized tables.
void* rng_circ_build_vbc(uint64_t seed) {
    try {
        VbcWitness w;
        VbcStatement st;
        vbc_build_witness_statement(seed, w, st);
        PlonkCircuit cs;
        vbc_apply_constraints(cs, w, st);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_vbc: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_vbc: %s\n", e.what());
        return nullptr;
    }
}

// `Intent And Balance Private Settlement` circuit builder (the VALID MATCH
// MPC successor; zk_circuits/settlement/intent_and_balance_private_settlement.rs)
void* rng_circ_build_settlement(uint64_t seed) {
    try {
        SettlementWitness w;
        SettlementStatement st;
        settlement_build_witness_statement(seed, w, st);
        PlonkCircuit cs;
        settlement_apply_constraints(cs, w, st);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_settlement: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_settlement: %s\n", e.what());
        return nullptr;
    }
}

// --- validity <-> settlement proof bundle builders ---
// (zk_circuits/validity_proofs/intent_and_balance.rs; the validity circuit's
//  two link groups are placed at the SETTLEMENT circuit's layout, :316-341.)

// settlement circuit whose pre-update shares come from the two validity
// witnesses of the same seed (the consistent production bundle)
void* rng_circ_build_settlement_bundle(uint64_t seed) {
    try {
        ValidityBundle b;
        validity_bundle_build(seed, b);
        PlonkCircuit cs;
        settlement_apply_constraints(cs, b.sw, b.sst);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_settlement_bundle: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_settlement_bundle: %s\n", e.what());
        return nullptr;
    }
}

// INTENT AND BALANCE VALIDITY circuit for party 0 or 1 of the seed's bundle
void* rng_circ_build_validity(uint64_t seed, uint64_t party) {
    try {
        ValidityBundle b;
        validity_bundle_build(seed, b);
        // read the settlement circuit's link-group placement (inherited layout)
        uint64_t align = 0;
        int64_t off[2] = {0, 0};
        {
            PlonkCircuit scs;
            settlement_apply_constraints(scs, b.sw, b.sst);
            CircuitTables stt = scs.finalize();
            const char* names[2] = {"intent_and_balance_settlement_party0",
                                    "intent_and_balance_settlement_party1"};
            for (auto& g : stt.link_groups)
                for (int i = 0; i < 2; ++i)
                    if (g.id == names[i]) {
                        align = g.alignment;
                        off[i] = (int64_t)g.offset;
                    }
        }
        int p = (int)(party & 1);
        PlonkCircuit cs;
        validity_apply_constraints(cs, b.vw[p], b.vst[p], (int)align, off[0], off[1]);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_validity: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_validity: %s\n", e.what());
        return nullptr;
    }
}

// OUTPUT BALANCE VALIDITY circuit for party 0 or 1 of the seed's bundle
// (validity_proofs/output_balance.rs; links at the settlement's
//  output_balance_settlement_party{0,1} layout)
void* rng_circ_build_ob_validity(uint64_t seed, uint64_t party) {
    try {
        ValidityBundle b;
        validity_bundle_build(seed, b);
        uint64_t align = 0;
        int64_t off[2] = {0, 0};
        {
            PlonkCircuit scs;
            settlement_apply_constraints(scs, b.sw, b.sst);
            CircuitTables stt = scs.finalize();
            const char* names[2] = {"output_balance_settlement_party0",
                                    "output_balance_settlement_party1"};
            for (auto& g : stt.link_groups)
                for (int i = 0; i < 2; ++i)
                    if (g.id == names[i]) {
                        align = g.alignment;
                        off[i] = (int64_t)g.offset;
                    }
        }
        int p = (int)(party & 1);
        PlonkCircuit cs;
        ob_validity_apply_constraints(cs, b.ow[p], b.ost[p], (int)align, off[0], off[1]);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_ob_validity: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_ob_validity: %s\n", e.what());
        return nullptr;
    }
}

// INTENT AND BALANCE PUBLIC SETTLEMENT circuit for party 0 of the seed's
// bundle (settlement/intent_and_balance_public_settlement.rs); its two link
// groups are placed at the private settlement's party-0 layout.
void* rng_circ_build_public_settlement(uint64_t seed) {
    try {
        ValidityBundle b;
        validity_bundle_build(seed, b);
        uint64_t align = 0;
        int64_t pg_off = 0, og_off = 0;
        {
            PlonkCircuit scs;
            settlement_apply_constraints(scs, b.sw, b.sst);
            CircuitTables stt = scs.finalize();
            for (auto& g : stt.link_groups) {
                if (g.id == "intent_and_balance_settlement_party0") {
                    align = g.alignment;
                    pg_off = (int64_t)g.offset;
                }
                if (g.id == "output_balance_settlement_party0") og_off = (int64_t)g.offset;
            }
        }
        PubSettlementStatement st;
        pub_settlement_statement_from_bundle(b, st);
        PlonkCircuit cs;
        pub_settlement_apply_constraints(cs, b.sw.p[0], st, (int)align, pg_off, og_off);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_public_settlement: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_public_settlement: %s\n", e.what());
        return nullptr;
    }
}

// INTENT ONLY PUBLIC SETTLEMENT circuit (intent_only_public_settlement.rs)
void* rng_circ_build_io_settlement(uint64_t seed) {
    try {
        IoValidityWitness vw;
        IoValidityStatement vs;
        IoSettlementStatement ss;
        io_bundle_build(seed, vw, vs, ss);
        PlonkCircuit cs;
        io_settlement_apply_constraints(cs, vw.intent, ss);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_io_settlement: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_io_settlement: %s\n", e.what());
        return nullptr;
    }
}

// INTENT ONLY VALIDITY circuit (validity_proofs/intent_only.rs); its link
// group inherits the INTENT ONLY PUBLIC SETTLEMENT placement
void* rng_circ_build_io_validity(uint64_t seed) {
    try {
        IoValidityWitness vw;
        IoValidityStatement vs;
        IoSettlementStatement ss;
        io_bundle_build(seed, vw, vs, ss);
        uint64_t align = 0;
        int64_t off = 0;
        {
            PlonkCircuit scs;
            io_settlement_apply_constraints(scs, vw.intent, ss);
            CircuitTables stt = scs.finalize();
            for (auto& g : stt.link_groups)
                if (g.id == "intent_only_settlement") {
                    align = g.alignment;
                    off = (int64_t)g.offset;
                }
        }
        PlonkCircuit cs;
        io_validity_apply_constraints(cs, vw, vs, (int)align, off);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_io_validity: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_io_validity: %s\n", e.what());
        return nullptr;
    }
}

// INTENT ONLY BOUNDED SETTLEMENT circuit (intent_only_bounded_settlement.rs)
void* rng_circ_build_io_bounded_settlement(uint64_t seed) {
    try {
        IoValidityWitness vw;
        IoValidityStatement vs;
        IoSettlementStatement ss;
        io_bundle_build(seed, vw, vs, ss);
        uint64_t align = 0;
        int64_t off = 0;
        {
            PlonkCircuit scs;
            io_settlement_apply_constraints(scs, vw.intent, ss);
            CircuitTables stt = scs.finalize();
            for (auto& g : stt.link_groups)
                if (g.id == "intent_only_settlement") {
                    align = g.alignment;
                    off = (int64_t)g.offset;
                }
        }
        IoBoundedStatement st;
        io_bounded_statement_build(seed, vw, ss, st);
        PlonkCircuit cs;
        io_bounded_apply_constraints(cs, vw.intent, st, (int)align, off);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_io_bounded_settlement: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_io_bounded_settlement: %s\n", e.what());
        return nullptr;
    }
}

// INTENT AND BALANCE BOUNDED SETTLEMENT circuit
// (intent_and_balance_bounded_settlement.rs; party-0 groups at the private
//  settlement layout)
void* rng_circ_build_ib_bounded_settlement(uint64_t seed) {
    try {
        ValidityBundle b;
        validity_bundle_build(seed, b);
        uint64_t align = 0;
        int64_t pg_off = 0, og_off = 0;
        {
            PlonkCircuit scs;
            settlement_apply_constraints(scs, b.sw, b.sst);
            CircuitTables stt = scs.finalize();
            for (auto& g : stt.link_groups) {
                if (g.id == "intent_and_balance_settlement_party0") {
                    align = g.alignment;
                    pg_off = (int64_t)g.offset;
                }
                if (g.id == "output_balance_settlement_party0") og_off = (int64_t)g.offset;
            }
        }
        IbBoundedStatement st;
        ib_bounded_statement_from_bundle(b, st);
        PlonkCircuit cs;
        ib_bounded_apply_constraints(cs, b.sw.p[0], st, (int)align, pg_off, og_off);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_ib_bounded_settlement: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_ib_bounded_settlement: %s\n", e.what());
        return nullptr;
    }
}

// INTENT ONLY FIRST FILL VALIDITY (validity_proofs/intent_only_first_fill.rs);
// shares the seed's intent with rng_circ_build_io_settlement so the proofs link
void* rng_circ_build_ioff(uint64_t seed) {
    try {
        IoffWitness w;
        IoffStatement st;
        ioff_build(seed, w, st);
        uint64_t align = 0;
        int64_t off = 0;
        {
            IoValidityWitness vw;
            IoValidityStatement vs;
            IoSettlementStatement ss;
            io_bundle_build(seed, vw, vs, ss);
            PlonkCircuit scs;
            io_settlement_apply_constraints(scs, vw.intent, ss);
            CircuitTables stt = scs.finalize();
            for (auto& g : stt.link_groups)
                if (g.id == "intent_only_settlement") {
                    align = g.alignment;
                    off = (int64_t)g.offset;
                }
        }
        PlonkCircuit cs;
        ioff_apply_constraints(cs, w, st, (int)align, off);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_ioff: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_ioff: %s\n", e.what());
        return nullptr;
    }
}

// Baby Jubjub native test shims (tests/test_jubjub.py pins the C++ curve
// arithmetic + Schnorr/ElGamal against an independent pure-Python bignum
// implementation).  Scalars: 4 u64 plain LE; points: x,y Montgomery Fr.
int rng_jj_mul(const uint64_t* scalar4, const uint64_t* px4, const uint64_t* py4,
               uint64_t* out_xy8) {
    JjPoint p;
    memcpy(p.x.l, px4, 32);
    memcpy(p.y.l, py4, 32);
    if (!jj_on_curve(p) && !(p.x.is_zero())) return RNG_ERR_BAD_ARG;
    JjPoint r = jj_mul(scalar4, p);
    memcpy(out_xy8, r.x.l, 32);
    memcpy(out_xy8 + 4, r.y.l, 32);
    return RNG_OK;
}

void rng_jj_base(uint64_t* out_xy8) {
    JjPoint b = jj_base();
    memcpy(out_xy8, b.x.l, 32);
    memcpy(out_xy8 + 4, b.y.l, 32);
}

// sign/verify round trip: sk, nonce k as plain scalars; msg = n Fr
// (Montgomery); out = s (4 u64 plain), R (8 u64 Montgomery xy)
int rng_jj_sign(const uint64_t* sk4, const uint64_t* k4, const uint64_t* msg,
                uint64_t n, uint64_t* out_s4, uint64_t* out_r8) {
    JjScalar sk, k;
    memcpy(sk.v, sk4, 32);
    memcpy(k.v, k4, 32);
    JjSignature sig = jj_sign(sk, k, (const Fr*)msg, n);
    memcpy(out_s4, sig.s.v, 32);
    memcpy(out_r8, sig.R.x.l, 32);
    memcpy(out_r8 + 4, sig.R.y.l, 32);
    return RNG_OK;
}

int rng_jj_verify(const uint64_t* vk8, const uint64_t* s4, const uint64_t* r8,
                  const uint64_t* msg, uint64_t n) {
    JjPoint vk;
    memcpy(vk.x.l, vk8, 32);
    memcpy(vk.y.l, vk8 + 4, 32);
    JjSignature sig;
    memcpy(sig.s.v, s4, 32);
    memcpy(sig.R.x.l, r8, 32);
    memcpy(sig.R.y.l, r8 + 4, 32);
    return jj_verify(vk, sig, (const Fr*)msg, n) ? 1 : 0;
}

int rng_jj_elgamal(const uint64_t* pk8, const uint64_t* k4, const uint64_t* msg12,
                   uint64_t* out_eph8, uint64_t* out_c12) {
    JjPoint pk;
    memcpy(pk.x.l, pk8, 32);
    memcpy(pk.y.l, pk8 + 4, 32);
    JjScalar k;
    memcpy(k.v, k4, 32);
    JjCiphertext<3> ct = jj_elgamal_encrypt<3>(pk, k, (const Fr*)msg12);
    memcpy(out_eph8, ct.ephemeral_key.x.l, 32);
    memcpy(out_eph8 + 4, ct.ephemeral_key.y.l, 32);
    memcpy(out_c12, ct.ciphertext, 96);
    return RNG_OK;
}

// embedded-curve gadget self-tests (Schnorr / ElGamal over Baby Jubjub):
// native-sign -> in-circuit verify; returns the finalized tables or null if
// the circuit is unsatisfied (tamper != 0 flips a signature/ciphertext bit
// and MUST yield null)
void* rng_testcirc_schnorr(uint64_t seed, int tamper) {
    try {
        Lcg rng(seed);
        auto sc = [&]() {
            JjScalar s{{rng.next() | (rng.next() << 52),
                        rng.next() | (rng.next() << 52),
                        rng.next() | (rng.next() << 52), rng.next() & 0x3FFFFFFFFFFull}};
            return s;  // < 2^250 < l
        };
        JjScalar sk = sc(), k = sc();
        Fr msg[3] = {rng.fr(), rng.fr(), rng.fr()};
        JjPoint vk = jj_pubkey(sk);
        JjSignature sig = jj_sign(sk, k, msg, 3);
        if (!jj_verify(vk, sig, msg, 3)) {
            fprintf(stderr, "rng_testcirc_schnorr: native verify failed\n");
            return nullptr;
        }
        if (tamper) sig.s.v[0] ^= 1;
        PlonkCircuit cs;
        JjPointVars vkv{cs.create_variable(vk.x), cs.create_variable(vk.y)};
        JjPointVars Rv{cs.create_variable(sig.R.x), cs.create_variable(sig.R.y)};
        Fr s_fr = Fr::from_canonical(sig.s.v);
        Var sv = cs.create_variable(s_fr);
        std::vector<Var> mv;
        for (int i = 0; i < 3; ++i) mv.push_back(cs.create_variable(msg[i]));
        schnorr_verify_gadget(cs, vkv, Rv, sv, mv);
        std::string why;
        if (!cs.check_satisfied(&why)) return nullptr;
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_testcirc_schnorr: %s\n", e.what());
        return nullptr;
    }
}

void* rng_testcirc_elgamal(uint64_t seed, int tamper) {
    try {
        Lcg rng(seed);
        JjScalar dk{{rng.next() | (rng.next() << 52), rng.next() | (rng.next() << 52),
                     rng.next() | (rng.next() << 52), rng.next() & 0x3FFFFFFFFFFull}};
        JjScalar k{{rng.next() | (rng.next() << 52), rng.next() | (rng.next() << 52),
                    rng.next() | (rng.next() << 52), rng.next() & 0x3FFFFFFFFFFull}};
        JjPoint pk = jj_pubkey(dk);
        Fr msg[3] = {rng.fr(), rng.fr(), rng.fr()};
        JjCiphertext<3> ct = jj_elgamal_encrypt<3>(pk, k, msg);
        if (tamper) ct.ciphertext[1] = ct.ciphertext[1].add(Fr::one());
        PlonkCircuit cs;
        JjPointVars pkv{cs.create_variable(pk.x), cs.create_variable(pk.y)};
        Var kv = cs.create_variable(Fr::from_canonical(k.v));
        std::vector<Var> mv;
        for (int i = 0; i < 3; ++i) mv.push_back(cs.create_variable(msg[i]));
        JjPointVars eph;
        std::vector<Var> cipher;
        elgamal_encrypt_gadget(cs, pkv, kv, mv, eph, cipher);
        // constrain against the native ciphertext (the statement shape)
        Var ex = cs.create_public_variable(ct.ephemeral_key.x);
        Var ey = cs.create_public_variable(ct.ephemeral_key.y);
        cs.enforce_equal(eph.x, ex);
        cs.enforce_equal(eph.y, ey);
        for (int i = 0; i < 3; ++i) {
            Var ci = cs.create_public_variable(ct.ciphertext[i]);
            cs.enforce_equal(cipher[i], ci);
        }
        std::string why;
        if (!cs.check_satisfied(&why)) return nullptr;
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_testcirc_elgamal: %s\n", e.what());
        return nullptr;
    }
}

// ---- fee circuits (zk_circuits/fees/) ----

// VALID NOTE REDEMPTION (fees/valid_note_redemption.rs)
void* rng_circ_build_note_redemption(uint64_t seed) {
    try {
        NoteRedemptionWitness w;
        NoteRedemptionStatement st;
        note_redemption_build(seed, w, st);
        PlonkCircuit cs;
        note_redemption_apply_constraints(cs, w, st);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_note_redemption: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_note_redemption: %s\n", e.what());
        return nullptr;
    }
}

// shared fee-payment builder; variant: 0 = public relayer, 1 = public
// protocol, 2 = private relayer (fees/valid_{public,private}_{relayer,
// protocol}_fee_payment.rs; private protocol needs in-circuit ElGamal and
// lands with the embedded-curve gadget)
static void* build_fee_payment(uint64_t seed, int variant, const char* name) {
    try {
        VdWitness w;
        FeePaymentStatement st;
        Note note;
        int field = (variant == 1) ? 6 : 5;
        fee_payment_build(seed, field, w, st, note);
        std::vector<Fr> ss = {st.merkle_root, st.old_balance_nullifier,
                              st.new_balance_commitment, st.recovery_id,
                              st.new_fee_balance_share};
        int note_mode = (variant == 2) ? 1 : 0;
        if (note_mode == 0) {
            auto nv = note.to_scalars();
            ss.insert(ss.end(), nv.begin(), nv.end());
        } else {
            ss.push_back(note.receiver);
            ss.push_back(native_note_commitment(note));
        }
        PlonkCircuit cs;
        fee_payment_apply_constraints(cs, w, note.blinder, field, note_mode,
                                      /*check_receiver=*/variant != 1, ss);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "%s: %s\n", name, why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s: %s\n", name, e.what());
        return nullptr;
    }
}

void* rng_circ_build_fee_public_relayer(uint64_t seed) {
    return build_fee_payment(seed, 0, "rng_circ_build_fee_public_relayer");
}
void* rng_circ_build_fee_public_protocol(uint64_t seed) {
    return build_fee_payment(seed, 1, "rng_circ_build_fee_public_protocol");
}
void* rng_circ_build_fee_private_relayer(uint64_t seed) {
    return build_fee_payment(seed, 2, "rng_circ_build_fee_private_relayer");
}

// VALID PRIVATE PROTOCOL FEE PAYMENT (in-circuit ElGamal note encryption)
void* rng_circ_build_fee_private_protocol(uint64_t seed) {
    try {
        VdWitness w;
        FeePaymentStatement st;
        Note note;
        fee_payment_build(seed, 6, w, st, note);
        Lcg rng(seed ^ 0xE161A3A1E161A3A1ull);
        // protocol receiver comes from the statement, not the balance
        u64 al[4] = {rng.next() | (rng.next() << 53), rng.next() | (rng.next() << 53),
                     rng.next() & 0xFFFFFFFF, 0};
        note.receiver = Fr::from_canonical(al);
        JjScalar dk = jj_random_scalar(rng);
        JjScalar k = jj_random_scalar(rng);
        JjPoint pk = jj_pubkey(dk);
        Fr plain[3] = {note.mint, note.amount, note.blinder};
        JjCiphertext<3> ct = jj_elgamal_encrypt<3>(pk, k, plain);
        std::vector<Fr> ss = {st.merkle_root, st.old_balance_nullifier,
                              st.new_balance_commitment, st.recovery_id,
                              st.new_fee_balance_share, note.receiver,
                              native_note_commitment(note), ct.ephemeral_key.x,
                              ct.ephemeral_key.y, ct.ciphertext[0], ct.ciphertext[1],
                              ct.ciphertext[2], pk.x, pk.y};
        PlonkCircuit cs;
        fee_private_protocol_apply_constraints(cs, w, note.blinder,
                                               Fr::from_canonical(k.v), ss);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_fee_private_protocol: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_fee_private_protocol: %s\n", e.what());
        return nullptr;
    }
}

// INTENT AND BALANCE FIRST FILL VALIDITY for bundle party 0/1
// (validity_proofs/intent_and_balance_first_fill.rs; links at the private
//  settlement's party layouts)
void* rng_circ_build_ff_validity(uint64_t seed, uint64_t party) {
    try {
        ValidityBundle b;
        validity_bundle_build(seed, b);
        uint64_t align = 0;
        int64_t off[2] = {0, 0};
        {
            PlonkCircuit scs;
            settlement_apply_constraints(scs, b.sw, b.sst);
            CircuitTables stt = scs.finalize();
            const char* names[2] = {"intent_and_balance_settlement_party0",
                                    "intent_and_balance_settlement_party1"};
            for (auto& g : stt.link_groups)
                for (int i = 0; i < 2; ++i)
                    if (g.id == names[i]) {
                        align = g.alignment;
                        off[i] = (int64_t)g.offset;
                    }
        }
        int p = (int)(party & 1);
        FfWitness w;
        FfStatement st;
        ff_build(b, p, seed, w, st);
        PlonkCircuit cs;
        ff_apply_constraints(cs, w, st, (int)align, off[0], off[1]);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_ff_validity: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_ff_validity: %s\n", e.what());
        return nullptr;
    }
}

// NEW OUTPUT BALANCE VALIDITY (validity_proofs/new_output_balance.rs; links
// at the settlement's output-balance layouts)
void* rng_circ_build_nob_validity(uint64_t seed) {
    try {
        NobWitness w;
        NobStatement st;
        nob_build(seed, w, st);
        uint64_t align = 0;
        int64_t off[2] = {0, 0};
        {
            ValidityBundle b;
            validity_bundle_build(seed, b);
            PlonkCircuit scs;
            settlement_apply_constraints(scs, b.sw, b.sst);
            CircuitTables stt = scs.finalize();
            const char* names[2] = {"output_balance_settlement_party0",
                                    "output_balance_settlement_party1"};
            for (auto& g : stt.link_groups)
                for (int i = 0; i < 2; ++i)
                    if (g.id == names[i]) {
                        align = g.alignment;
                        off[i] = (int64_t)g.offset;
                    }
        }
        PlonkCircuit cs;
        nob_apply_constraints(cs, w, st, (int)align, off[0], off[1]);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_nob_validity: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_nob_validity: %s\n", e.what());
        return nullptr;
    }
}

// ---- link-group layouts of the placing circuits (computed once) ----
// The settlement circuits PLACE the groups; validity circuits inherit them.
// Layout depends only on circuit structure, so compute from a fixed seed.
struct LinkLayouts {
    uint64_t ib_align = 0;
    int64_t pg0 = 0, og0 = 0, pg1 = 0, og1 = 0;  // private-settlement groups
    uint64_t io_align = 0;
    int64_t io_off = 0;  // intent-only settlement group
};
static const LinkLayouts& link_layouts() {
    static LinkLayouts L;
    static std::once_flag once;
    std::call_once(once, [] {
        ValidityBundle b;
        validity_bundle_build(42, b);
        PlonkCircuit scs;
        settlement_apply_constraints(scs, b.sw, b.sst);
        CircuitTables t = scs.finalize();
        for (auto& g : t.link_groups) {
            if (g.id == "intent_and_balance_settlement_party0") {
                L.ib_align = g.alignment;
                L.pg0 = (int64_t)g.offset;
            } else if (g.id == "intent_and_balance_settlement_party1") {
                L.pg1 = (int64_t)g.offset;
            } else if (g.id == "output_balance_settlement_party0") {
                L.og0 = (int64_t)g.offset;
            } else if (g.id == "output_balance_settlement_party1") {
                L.og1 = (int64_t)g.offset;
            }
        }
        IoValidityWitness vw;
        IoValidityStatement vs;
        IoSettlementStatement ss;
        io_bundle_build(42, vw, vs, ss);
        PlonkCircuit c2;
        io_settlement_apply_constraints(c2, vw.intent, ss);
        CircuitTables t2 = c2.finalize();
        for (auto& g : t2.link_groups)
            if (g.id == "intent_only_settlement") {
                L.io_align = g.alignment;
                L.io_off = (int64_t)g.offset;
            }
    });
    return L;
}

// ---- witness/statement parsers (scalar cursor over the field orders the
//      route bodies use; see rng_prover.h kind table) ----
namespace {
struct Rd {
    const Fr* p;
    Fr f() { return *p++; }
    uint64_t u() {
        u64 l[4];
        (*p).to_canonical(l);
        ++p;
        return l[0];
    }
    void frs(Fr* dst, int n) {
        for (int i = 0; i < n; ++i) dst[i] = f();
    }
    Csprng cs() {
        Csprng c;
        c.seed = f();
        c.index = u();
        return c;
    }
    Balance bal() {
        Balance b;
        Fr s[8];
        frs(s, 8);
        b.from_scalars(s);
        return b;
    }
    Intent in() {
        Intent i;
        i.in_token = f();
        i.out_token = f();
        i.owner = f();
        i.min_price_repr = f();
        i.amount_in = f();
        return i;
    }
    PostMatchShare pms() {
        PostMatchShare s;
        s.relayer_fee_balance = f();
        s.protocol_fee_balance = f();
        s.amount = f();
        return s;
    }
    Obligation ob() {
        Obligation o;
        o.input_token = f();
        o.output_token = f();
        o.amount_in = f();
        o.amount_out = f();
        return o;
    }
    StateBalance sbal() {
        StateBalance s;
        s.recovery = cs();
        s.share = cs();
        s.inner = bal();
        frs(s.public_share, 8);
        return s;
    }
    StateIntent sint() {
        StateIntent s;
        s.recovery = cs();
        s.share = cs();
        s.inner = in();
        frs(s.public_share, 5);
        return s;
    }
    void opening(Fr* elems, bool* idx) {
        frs(elems, MERKLE_HEIGHT);
        for (int i = 0; i < MERKLE_HEIGHT; ++i) idx[i] = u() != 0;
    }
    JjSignature sig() {
        JjSignature s;
        Fr sf = f();
        sf.to_canonical(s.s.v);
        s.R.x = f();
        s.R.y = f();
        return s;
    }
    Note note() {
        Note n;
        n.mint = f();
        n.amount = f();
        n.receiver = f();
        n.blinder = f();
        return n;
    }
    SettlementParty party_no_ob() {  // public/bounded settlement witness (28)
        SettlementParty p;
        p.intent = in();
        p.pre_amount_share = f();
        p.input_balance = bal();
        p.pre_in_shares = pms();
        p.output_balance = bal();
        p.pre_out_shares = pms();
        return p;
    }
};
}  // namespace

namespace {
struct Wt {  // writer mirroring Rd
    Fr* p;
    void f(const Fr& v) { *p++ = v; }
    void u(uint64_t x) { *p++ = Fr::from_u64(x); }
    void frs(const Fr* src, int n) {
        for (int i = 0; i < n; ++i) f(src[i]);
    }
    void cs(const Csprng& c) {
        f(c.seed);
        u(c.index);
    }
    void bal(const Balance& b) {
        for (auto& s : b.to_scalars()) f(s);
    }
    void in(const Intent& i) {
        for (auto& s : i.to_scalars()) f(s);
    }
    void pms(const PostMatchShare& s_) {
        for (auto& s : s_.to_scalars()) f(s);
    }
    void sbal(const StateBalance& s_) {
        for (auto& s : s_.to_scalars()) f(s);
    }
    void sint(const StateIntent& s_) {
        for (auto& s : s_.to_scalars()) f(s);
    }
    void opening(const Fr* elems, const bool* idx) {
        frs(elems, MERKLE_HEIGHT);
        for (int i = 0; i < MERKLE_HEIGHT; ++i) u(idx[i] ? 1 : 0);
    }
    void sig(const JjSignature& s_) {
        f(Fr::from_canonical(s_.s.v));
        f(s_.R.x);
        f(s_.R.y);
    }
    void st(const std::vector<Fr>& v) {
        for (auto& s : v) f(s);
    }
};
}  // namespace

// per-kind witness/statement scalar counts (the route body sizes)
int rng_ws_sizes(int kind, uint64_t* out_nw, uint64_t* out_ns) {
    struct {
        int k, nw, ns;
    } T[] = {{1, 40, 8},  {2, 40, 8},  {3, 34, 3},  {4, 91, 10}, {5, 69, 11},
             {6, 39, 7},  {7, 14, 8},  {8, 74, 10}, {9, 51, 5},  {11, 28, 14},
             {12, 28, 16}, {13, 5, 6},  {14, 5, 9},  {15, 20, 6}, {16, 40, 9},
             {17, 40, 9}, {18, 41, 7}, {19, 42, 14}};
    for (auto& t : T)
        if (t.k == kind) {
            *out_nw = t.nw;
            *out_ns = t.ns;
            return 0;
        }
    return RNG_ERR_BAD_ARG;
}

// fixed-seed witness/statement generator for any kind (test vectors for the
// prover-service routes; same serialization rng_circ_from_scalars parses)
int rng_witness_statement(int kind, uint64_t seed, uint64_t* out_w, uint64_t* out_s) {
    try {
        Wt w{(Fr*)out_w};
        Wt s{(Fr*)out_s};
        switch (kind) {
            case 1: {
                VdWitness vw;
                VdStatement st;
                vd_build_witness_statement(seed, vw, st);
                w.sbal(vw.old_balance);
                w.opening(vw.opening_elems, vw.opening_indices);
                s.st(st.to_scalars());
                break;
            }
            case 2: {
                VdWitness vw;
                VwStatement st;
                vw_build_witness_statement(seed, vw, st);
                w.sbal(vw.old_balance);
                w.opening(vw.opening_elems, vw.opening_indices);
                s.st(st.to_scalars());
                break;
            }
            case 3: {
                VocWitness vw;
                VocStatement st;
                voc_build_witness_statement(seed, vw, st);
                w.sint(vw.old_intent);
                w.opening(vw.opening_elems, vw.opening_idx);
                s.st(st.to_scalars());
                break;
            }
            case 4: {
                ValidityBundle b;
                validity_bundle_build(seed, b);
                const ValidityWitness& vw = b.vw[0];
                w.sint(vw.old_intent);
                w.opening(vw.intent_opening_elems, vw.intent_opening_idx);
                w.in(vw.intent);
                w.f(vw.new_amount_public_share);
                w.sbal(vw.old_balance);
                w.opening(vw.balance_opening_elems, vw.balance_opening_idx);
                w.bal(vw.balance);
                w.pms(vw.post_match_balance_shares);
                s.st(b.vst[0].to_scalars());
                break;
            }
            case 5: {
                ValidityBundle b;
                validity_bundle_build(seed, b);
                FfWitness vw;
                FfStatement st;
                ff_build(b, 0, seed, vw, st);
                w.in(vw.intent);
                w.cs(vw.share_stream);
                w.cs(vw.recovery_stream);
                w.frs(vw.private_intent_shares, 5);
                w.f(vw.new_amount_public_share);
                w.sig(vw.sig);
                w.sbal(vw.old_balance);
                w.bal(vw.balance);
                w.pms(vw.post_match_balance_shares);
                w.opening(vw.opening_elems, vw.opening_idx);
                s.st(st.to_scalars());
                break;
            }
            case 6: {
                IoValidityWitness vw;
                IoValidityStatement vs;
                IoSettlementStatement ss;
                io_bundle_build(seed, vw, vs, ss);
                w.sint(vw.old_intent);
                w.opening(vw.opening_elems, vw.opening_idx);
                w.in(vw.intent);
                s.st(vs.to_scalars());
                break;
            }
            case 7: {
                IoffWitness vw;
                IoffStatement st;
                ioff_build(seed, vw, st);
                w.in(vw.intent);
                w.cs(vw.share_stream);
                w.cs(vw.recovery_stream);
                w.frs(vw.private_shares, 5);
                s.st(st.to_scalars());
                break;
            }
            case 8: {
                NobWitness vw;
                NobStatement st;
                nob_build(seed, vw, st);
                w.sbal(vw.new_balance);
                w.bal(vw.balance);
                w.pms(vw.post_match_balance_shares);
                w.sbal(vw.existing_balance);
                w.opening(vw.opening_elems, vw.opening_idx);
                w.sig(vw.sig);
                s.st(st.to_scalars());
                break;
            }
            case 9: {
                ValidityBundle b;
                validity_bundle_build(seed, b);
                const ObValidityWitness& vw = b.ow[0];
                w.sbal(vw.old_balance);
                w.opening(vw.opening_elems, vw.opening_idx);
                w.bal(vw.balance);
                w.pms(vw.post_match_balance_shares);
                s.st(b.ost[0].to_scalars());
                break;
            }
            case 11: {
                ValidityBundle b;
                validity_bundle_build(seed, b);
                const SettlementParty& p = b.sw.p[0];
                w.in(p.intent);
                w.f(p.pre_amount_share);
                w.bal(p.input_balance);
                w.pms(p.pre_in_shares);
                w.bal(p.output_balance);
                w.pms(p.pre_out_shares);
                PubSettlementStatement st;
                pub_settlement_statement_from_bundle(b, st);
                s.st(st.to_scalars());
                break;
            }
            case 12: {
                ValidityBundle b;
                validity_bundle_build(seed, b);
                const SettlementParty& p = b.sw.p[0];
                w.in(p.intent);
                w.f(p.pre_amount_share);
                w.bal(p.input_balance);
                w.pms(p.pre_in_shares);
                w.bal(p.output_balance);
                w.pms(p.pre_out_shares);
                IbBoundedStatement st;
                ib_bounded_statement_from_bundle(b, st);
                s.st(st.to_scalars());
                break;
            }
            case 13: {
                IoValidityWitness vw;
                IoValidityStatement vs;
                IoSettlementStatement ss;
                io_bundle_build(seed, vw, vs, ss);
                w.in(vw.intent);
                s.st(ss.to_scalars());
                break;
            }
            case 14: {
                IoValidityWitness vw;
                IoValidityStatement vs;
                IoSettlementStatement ss;
                io_bundle_build(seed, vw, vs, ss);
                IoBoundedStatement st;
                io_bounded_statement_build(seed, vw, ss, st);
                w.in(vw.intent);
                s.st(st.to_scalars());
                break;
            }
            case 15: {
                NoteRedemptionWitness vw;
                NoteRedemptionStatement st;
                note_redemption_build(seed, vw, st);
                w.opening(vw.opening_elems, vw.opening_idx);
                s.st(st.to_scalars());
                break;
            }
            case 16:
            case 17:
            case 18: {
                VdWitness vw;
                FeePaymentStatement st;
                Note note;
                int field = (kind == 17) ? 6 : 5;
                fee_payment_build(seed, field, vw, st, note);
                w.sbal(vw.old_balance);
                w.opening(vw.opening_elems, vw.opening_indices);
                std::vector<Fr> ss = {st.merkle_root, st.old_balance_nullifier,
                                      st.new_balance_commitment, st.recovery_id,
                                      st.new_fee_balance_share};
                if (kind == 18) {
                    w.f(note.blinder);
                    ss.push_back(note.receiver);
                    ss.push_back(native_note_commitment(note));
                } else {
                    auto nv = note.to_scalars();
                    ss.insert(ss.end(), nv.begin(), nv.end());
                }
                s.st(ss);
                break;
            }
            case 19: {
                VdWitness vw;
                FeePaymentStatement st;
                Note note;
                fee_payment_build(seed, 6, vw, st, note);
                Lcg rng(seed ^ 0xE161A3A1E161A3A1ull);
                u64 al[4] = {rng.next() | (rng.next() << 53),
                             rng.next() | (rng.next() << 53), rng.next() & 0xFFFFFFFF, 0};
                note.receiver = Fr::from_canonical(al);
                JjScalar dk = jj_random_scalar(rng);
                JjScalar k = jj_random_scalar(rng);
                JjPoint pk = jj_pubkey(dk);
                Fr plain[3] = {note.mint, note.amount, note.blinder};
                JjCiphertext<3> ct = jj_elgamal_encrypt<3>(pk, k, plain);
                w.sbal(vw.old_balance);
                w.opening(vw.opening_elems, vw.opening_indices);
                w.f(note.blinder);
                w.f(Fr::from_canonical(k.v));
                s.st({st.merkle_root, st.old_balance_nullifier, st.new_balance_commitment,
                      st.recovery_id, st.new_fee_balance_share, note.receiver,
                      native_note_commitment(note), ct.ephemeral_key.x,
                      ct.ephemeral_key.y, ct.ciphertext[0], ct.ciphertext[1],
                      ct.ciphertext[2], pk.x, pk.y});
                break;
            }
            default:
                return RNG_ERR_BAD_ARG;
        }
        return RNG_OK;
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_witness_statement: %s\n", e.what());
        return RNG_ERR_BAD_ARG;
    }
}

// Party-aware test vectors for the two per-party validity kinds (4 = intent-
// and-balance validity, 9 = output-balance validity): the private-settlement
// route takes FOUR external hints (party 0/1 of each), all from one seed's
// consistent bundle (native_proof_manager.rs:554-590).
int rng_witness_statement_party(int kind, uint64_t seed, uint64_t party,
                                uint64_t* out_w, uint64_t* out_s) {
    try {
        Wt w{(Fr*)out_w};
        Wt s{(Fr*)out_s};
        int p = (int)(party & 1);
        ValidityBundle b;
        validity_bundle_build(seed, b);
        if (kind == 4) {
            const ValidityWitness& vw = b.vw[p];
            w.sint(vw.old_intent);
            w.opening(vw.intent_opening_elems, vw.intent_opening_idx);
            w.in(vw.intent);
            w.f(vw.new_amount_public_share);
            w.sbal(vw.old_balance);
            w.opening(vw.balance_opening_elems, vw.balance_opening_idx);
            w.bal(vw.balance);
            w.pms(vw.post_match_balance_shares);
            s.st(b.vst[p].to_scalars());
        } else if (kind == 9) {
            const ObValidityWitness& vw = b.ow[p];
            w.sbal(vw.old_balance);
            w.opening(vw.opening_elems, vw.opening_idx);
            w.bal(vw.balance);
            w.pms(vw.post_match_balance_shares);
            s.st(b.ost[p].to_scalars());
        } else if (kind == 10) {
            // the BUNDLE's settlement witness/statement (64/17 scalars, same
            // order as rng_settlement_witness_statement).  Needed because
            // validity_bundle_build mutates the settlement witness after
            // building it (real Schnorr authorities on the input balances),
            // so only the bundle's version links against the bundle's
            // validity proofs.  `party` is ignored.
            const SettlementWitness& sw = b.sw;
            std::vector<Fr> ws;
            for (int i = 0; i < 2; ++i) {
                auto a = sw.p[i].obligation.to_scalars();
                auto bi = sw.p[i].intent.to_scalars();
                auto c = sw.p[i].input_balance.to_scalars();
                auto d = sw.p[i].pre_in_shares.to_scalars();
                auto e = sw.p[i].output_balance.to_scalars();
                auto f = sw.p[i].pre_out_shares.to_scalars();
                ws.insert(ws.end(), a.begin(), a.end());
                ws.insert(ws.end(), bi.begin(), bi.end());
                ws.push_back(sw.p[i].pre_amount_share);
                ws.insert(ws.end(), c.begin(), c.end());
                ws.insert(ws.end(), d.begin(), d.end());
                ws.insert(ws.end(), e.begin(), e.end());
                ws.insert(ws.end(), f.begin(), f.end());
            }
            auto ss = b.sst.to_scalars();
            memcpy(out_w, ws.data(), ws.size() * sizeof(Fr));
            memcpy(out_s, ss.data(), ss.size() * sizeof(Fr));
        } else {
            return RNG_ERR_BAD_ARG;
        }
        return RNG_OK;
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_witness_statement_party: %s\n", e.what());
        return RNG_ERR_BAD_ARG;
    }
}

// Build any circuit from caller-supplied witness/statement scalars (the
// prover-service request shape).  `kind` table in include/rng_prover.h;
// returns null if the witness does not satisfy the circuit.
void* rng_circ_from_scalars(int kind, const uint64_t* witness64,
                            const uint64_t* statement64) {
    try {
        Rd w{(const Fr*)witness64};
        Rd s{(const Fr*)statement64};
        const LinkLayouts& L = link_layouts();
        PlonkCircuit cs;
        switch (kind) {
            case 1:
            case 2: {  // valid deposit / withdrawal (witness 40)
                VdWitness vw;
                vw.old_balance = w.sbal();
                w.opening(vw.opening_elems, vw.opening_indices);
                if (kind == 1) {
                    VdStatement st;
                    st.deposit.from = s.f();
                    st.deposit.token = s.f();
                    st.deposit.amount = s.f();
                    st.merkle_root = s.f();
                    st.old_nullifier = s.f();
                    st.new_commitment = s.f();
                    st.recovery_id = s.f();
                    st.new_amount_share = s.f();
                    vd_apply_constraints(cs, vw, st);
                } else {
                    VwStatement st;
                    st.to = s.f();
                    st.token = s.f();
                    st.amount = s.f();
                    st.merkle_root = s.f();
                    st.old_nullifier = s.f();
                    st.new_commitment = s.f();
                    st.recovery_id = s.f();
                    st.new_amount_share = s.f();
                    vw_apply_constraints(cs, vw, st);
                }
                break;
            }
            case 3: {  // valid order cancellation (witness 34)
                VocWitness vw;
                vw.old_intent = w.sint();
                w.opening(vw.opening_elems, vw.opening_idx);
                VocStatement st;
                st.merkle_root = s.f();
                st.old_intent_nullifier = s.f();
                st.owner = s.f();
                voc_apply_constraints(cs, vw, st);
                break;
            }
            case 4: {  // intent-and-balance validity (witness 91)
                ValidityWitness vw;
                vw.old_intent = w.sint();
                w.opening(vw.intent_opening_elems, vw.intent_opening_idx);
                vw.intent = w.in();
                vw.new_amount_public_share = w.f();
                vw.old_balance = w.sbal();
                w.opening(vw.balance_opening_elems, vw.balance_opening_idx);
                vw.balance = w.bal();
                vw.post_match_balance_shares = w.pms();
                ValidityStatement st;
                st.intent_merkle_root = s.f();
                st.old_intent_nullifier = s.f();
                st.intent_partial_private = s.f();
                st.intent_partial_public = s.f();
                st.intent_recovery_id = s.f();
                st.balance_merkle_root = s.f();
                st.old_balance_nullifier = s.f();
                st.balance_partial_private = s.f();
                st.balance_partial_public = s.f();
                st.balance_recovery_id = s.f();
                validity_apply_constraints(cs, vw, st, (int)L.ib_align, L.pg0, L.pg1);
                break;
            }
            case 5: {  // first-fill validity (witness 69)
                FfWitness vw;
                vw.intent = w.in();
                vw.share_stream = w.cs();
                vw.recovery_stream = w.cs();
                w.frs(vw.private_intent_shares, 5);
                vw.new_amount_public_share = w.f();
                vw.sig = w.sig();
                vw.old_balance = w.sbal();
                vw.balance = w.bal();
                vw.post_match_balance_shares = w.pms();
                w.opening(vw.opening_elems, vw.opening_idx);
                FfStatement st;
                st.merkle_root = s.f();
                s.frs(st.intent_public_share, 4);
                st.intent_private_share_commitment = s.f();
                st.intent_recovery_id = s.f();
                st.balance_partial_private = s.f();
                st.balance_partial_public = s.f();
                st.old_balance_nullifier = s.f();
                st.balance_recovery_id = s.f();
                ff_apply_constraints(cs, vw, st, (int)L.ib_align, L.pg0, L.pg1);
                break;
            }
            case 6: {  // intent-only validity (witness 39)
                IoValidityWitness vw;
                vw.old_intent = w.sint();
                w.opening(vw.opening_elems, vw.opening_idx);
                vw.intent = w.in();
                IoValidityStatement st;
                st.owner = s.f();
                st.merkle_root = s.f();
                st.old_intent_nullifier = s.f();
                st.new_amount_public_share = s.f();
                st.partial_private = s.f();
                st.partial_public = s.f();
                st.recovery_id = s.f();
                io_validity_apply_constraints(cs, vw, st, (int)L.io_align, L.io_off);
                break;
            }
            case 7: {  // intent-only first fill (witness 14)
                IoffWitness vw;
                vw.intent = w.in();
                vw.share_stream = w.cs();
                vw.recovery_stream = w.cs();
                w.frs(vw.private_shares, 5);
                IoffStatement st;
                st.owner = s.f();
                st.intent_private_commitment = s.f();
                st.recovery_id = s.f();
                s.frs(st.intent_public_share, 5);
                ioff_apply_constraints(cs, vw, st, (int)L.io_align, L.io_off);
                break;
            }
            case 8: {  // new output balance (witness 74)
                NobWitness vw;
                vw.new_balance = w.sbal();
                vw.balance = w.bal();
                vw.post_match_balance_shares = w.pms();
                vw.existing_balance = w.sbal();
                w.opening(vw.opening_elems, vw.opening_idx);
                vw.sig = w.sig();
                NobStatement st;
                st.existing_merkle_root = s.f();
                st.existing_nullifier = s.f();
                s.frs(st.pre_match_shares, 5);
                st.partial_private = s.f();
                st.partial_public = s.f();
                st.recovery_id = s.f();
                nob_apply_constraints(cs, vw, st, (int)L.ib_align, L.og0, L.og1);
                break;
            }
            case 9: {  // output-balance validity (witness 51)
                ObValidityWitness vw;
                vw.old_balance = w.sbal();
                w.opening(vw.opening_elems, vw.opening_idx);
                vw.balance = w.bal();
                vw.post_match_balance_shares = w.pms();
                ObValidityStatement st;
                st.merkle_root = s.f();
                st.old_balance_nullifier = s.f();
                st.partial_private = s.f();
                st.partial_public = s.f();
                st.recovery_id = s.f();
                ob_validity_apply_constraints(cs, vw, st, (int)L.ib_align, L.og0, L.og1);
                break;
            }
            case 11: {  // ib public settlement (witness 28)
                SettlementParty p = w.party_no_ob();
                PubSettlementStatement st;
                st.obligation = s.ob();
                st.amount_public_share = s.f();
                st.in_shares = s.pms();
                st.out_shares = s.pms();
                st.relayer_fee_repr = s.f();
                st.protocol_fee_repr = s.f();
                st.relayer_fee_recipient = s.f();
                pub_settlement_apply_constraints(cs, p, st, (int)L.ib_align, L.pg0,
                                                 L.og0);
                break;
            }
            case 12: {  // ib bounded settlement (witness 28)
                SettlementParty p = w.party_no_ob();
                IbBoundedStatement st;
                st.bmr.internal_party_input_token = s.f();
                st.bmr.internal_party_output_token = s.f();
                st.bmr.min_internal_party_amount_in = s.f();
                st.bmr.max_internal_party_amount_in = s.f();
                st.bmr.price_repr = s.f();
                st.bmr.block_deadline = s.f();
                st.amount_public_share = s.f();
                st.in_shares = s.pms();
                st.out_shares = s.pms();
                st.internal_relayer_fee_repr = s.f();
                st.external_relayer_fee_repr = s.f();
                st.relayer_fee_recipient = s.f();
                ib_bounded_apply_constraints(cs, p, st, (int)L.ib_align, L.pg0, L.og0);
                break;
            }
            case 13: {  // io public settlement (witness 5)
                Intent in = w.in();
                IoSettlementStatement st;
                st.obligation = s.ob();
                st.relayer_fee_repr = s.f();
                st.relayer_fee_recipient = s.f();
                io_settlement_apply_constraints(cs, in, st);
                break;
            }
            case 14: {  // io bounded settlement (witness 5)
                Intent in = w.in();
                IoBoundedStatement st;
                st.bmr.internal_party_input_token = s.f();
                st.bmr.internal_party_output_token = s.f();
                st.bmr.min_internal_party_amount_in = s.f();
                st.bmr.max_internal_party_amount_in = s.f();
                st.bmr.price_repr = s.f();
                st.bmr.block_deadline = s.f();
                st.internal_relayer_fee_repr = s.f();
                st.external_relayer_fee_repr = s.f();
                st.relayer_fee_recipient = s.f();
                io_bounded_apply_constraints(cs, in, st, (int)L.io_align, L.io_off);
                break;
            }
            case 15: {  // note redemption (witness 20)
                NoteRedemptionWitness vw;
                w.opening(vw.opening_elems, vw.opening_idx);
                NoteRedemptionStatement st;
                st.note = s.note();
                st.note_root = s.f();
                st.note_nullifier = s.f();
                note_redemption_apply_constraints(cs, vw, st);
                break;
            }
            case 16:
            case 17:
            case 18: {  // fee payments (witness 40 [+1 blinder for 18])
                VdWitness vw;
                vw.old_balance = w.sbal();
                w.opening(vw.opening_elems, vw.opening_indices);
                Fr blinder = (kind == 18) ? w.f() : Fr::zero();
                int field = (kind == 17) ? 6 : 5;
                int note_mode = (kind == 18) ? 1 : 0;
                std::vector<Fr> ss;
                int nst = (note_mode == 0) ? 9 : 7;
                for (int i = 0; i < nst; ++i) ss.push_back(s.f());
                fee_payment_apply_constraints(cs, vw, blinder, field, note_mode,
                                              kind != 17, ss);
                break;
            }
            case 19: {  // private protocol fee (witness 42)
                VdWitness vw;
                vw.old_balance = w.sbal();
                w.opening(vw.opening_elems, vw.opening_indices);
                Fr blinder = w.f();
                Fr enc_k = w.f();
                std::vector<Fr> ss;
                for (int i = 0; i < 14; ++i) ss.push_back(s.f());
                fee_private_protocol_apply_constraints(cs, vw, blinder, enc_k, ss);
                break;
            }
            default:
                fprintf(stderr, "rng_circ_from_scalars: unknown kind %d\n", kind);
                return nullptr;
        }
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_from_scalars(kind=%d): %s\n", kind, why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_from_scalars: %s\n", e.what());
        return nullptr;
    }
}

// VALID ORDER CANCELLATION circuit (valid_order_cancellation.rs)
void* rng_circ_build_valid_order_cancellation(uint64_t seed) {
    try {
        VocWitness w;
        VocStatement st;
        voc_build_witness_statement(seed, w, st);
        PlonkCircuit cs;
        voc_apply_constraints(cs, w, st);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_valid_order_cancellation: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_valid_order_cancellation: %s\n", e.what());
        return nullptr;
    }
}

// circuit builders from caller-supplied witness/statement scalars (the shape
// the external prover service receives — api_types.rs requests; Montgomery
// limbs, field order per the reference structs)
void* rng_circ_vbc_from_scalars(const uint64_t* witness12, const uint64_t* statement13) {
    try {
        VbcWitness w;
        VbcStatement st;
        vbc_witness_from_scalars((const Fr*)witness12, w);
        vbc_statement_from_scalars((const Fr*)statement13, st);
        PlonkCircuit cs;
        vbc_apply_constraints(cs, w, st);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_vbc_from_scalars: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_vbc_from_scalars: %s\n", e.what());
        return nullptr;
    }
}

void* rng_circ_settlement_from_scalars(const uint64_t* witness64,
                                       const uint64_t* statement17) {
    try {
        SettlementWitness w;
        SettlementStatement st;
        settlement_witness_from_scalars((const Fr*)witness64, w);
        settlement_statement_from_scalars((const Fr*)statement17, st);
        PlonkCircuit cs;
        settlement_apply_constraints(cs, w, st);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_settlement_from_scalars: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_settlement_from_scalars: %s\n", e.what());
        return nullptr;
    }
}

// expose the fixed-seed witness/statement generators (bench/test data)
void rng_vbc_witness_statement(uint64_t seed, uint64_t* witness12, uint64_t* statement13) {
    VbcWitness w;
    VbcStatement st;
    vbc_build_witness_statement(seed, w, st);
    auto ws = w.to_scalars();
    auto ss = st.to_scalars();
    memcpy(witness12, ws.data(), ws.size() * sizeof(Fr));
    memcpy(statement13, ss.data(), ss.size() * sizeof(Fr));
}
void rng_settlement_witness_statement(uint64_t seed, uint64_t* witness64,
                                      uint64_t* statement17) {
    SettlementWitness w;
    SettlementStatement st;
    settlement_build_witness_statement(seed, w, st);
    std::vector<Fr> ws;
    for (int i = 0; i < 2; ++i) {
        auto a = w.p[i].obligation.to_scalars();
        auto b = w.p[i].intent.to_scalars();
        auto c = w.p[i].input_balance.to_scalars();
        auto d = w.p[i].pre_in_shares.to_scalars();
        auto e = w.p[i].output_balance.to_scalars();
        auto f = w.p[i].pre_out_shares.to_scalars();
        ws.insert(ws.end(), a.begin(), a.end());
        ws.insert(ws.end(), b.begin(), b.end());
        ws.push_back(w.p[i].pre_amount_share);
        ws.insert(ws.end(), c.begin(), c.end());
        ws.insert(ws.end(), d.begin(), d.end());
        ws.insert(ws.end(), e.begin(), e.end());
        ws.insert(ws.end(), f.begin(), f.end());
    }
    auto ss = st.to_scalars();
    memcpy(witness64, ws.data(), ws.size() * sizeof(Fr));
    memcpy(statement17, ss.data(), ss.size() * sizeof(Fr));
}

// linked test circuit: `count` link-group values derived from value_seed,
// placed at (alignment, offset), plus filler gates scaled by `scale` —
// two different scales give two circuits of different domain size whose
// group values coincide (the cross-circuit linking shape: a validity proof
// linking into the settlement proof across domains).
void* rng_testcirc_build_linked(uint64_t value_seed, uint64_t scale, uint64_t alignment,
                                uint64_t offset, uint64_t count) {
    try {
        PlonkCircuit cs;
        cs.create_link_group("xlink", (int)alignment, (int64_t)offset);
        Lcg vr(value_seed);
        for (uint64_t k = 0; k < count; ++k) {
            Var v = cs.create_variable(vr.fr());
            cs.add_to_link_group(v, "xlink");
        }
        build_mixed_circuit(cs, value_seed + 1000 * scale, scale);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_testcirc_build_linked: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_testcirc_build_linked: %s\n", e.what());
        return nullptr;
    }
}

// `Valid Deposit` circuit builder (zk_circuits/valid_deposit.rs)
void* rng_circ_build_valid_deposit(uint64_t seed) {
    try {
        VdWitness w;
        VdStatement st;
        vd_build_witness_statement(seed, w, st);
        PlonkCircuit cs;
        vd_apply_constraints(cs, w, st);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_valid_deposit: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_valid_deposit: %s\n", e.what());
        return nullptr;
    }
}

// `Valid Withdrawal` circuit builder (zk_circuits/valid_withdrawal.rs)
void* rng_circ_build_valid_withdrawal(uint64_t seed) {
    try {
        VdWitness w;
        VwStatement st;
        vw_build_witness_statement(seed, w, st);
        PlonkCircuit cs;
        vw_apply_constraints(cs, w, st);
        std::string why;
        if (!cs.check_satisfied(&why)) {
            fprintf(stderr, "rng_circ_build_valid_withdrawal: %s\n", why.c_str());
            return nullptr;
        }
        return new CircuitTables(cs.finalize());
    } catch (const std::exception& e) {
        fprintf(stderr, "rng_circ_build_valid_withdrawal: %s\n", e.what());
        return nullptr;
    }
}

uint64_t rng_circ_num_link_groups(void* t) {
    return static_cast<CircuitTables*>(t)->link_groups.size();
}
// out: per group 3 u64 (alignment, grid offset, count), in creation order
void rng_circ_link_groups(void* t_, uint64_t* out) {
    auto* t = static_cast<CircuitTables*>(t_);
    for (size_t i = 0; i < t->link_groups.size(); ++i) {
        out[3 * i] = t->link_groups[i].alignment;
        out[3 * i + 1] = t->link_groups[i].offset;
        out[3 * i + 2] = t->link_groups[i].count;
    }
}

// native Poseidon2 hash (for cross-checks vs the oracle's restatement)
void rng_poseidon_hash(const uint64_t* inputs_mont, uint64_t n, uint64_t* out_mont) {
    std::vector<Fr> in(n);
    memcpy(in.data(), inputs_mont, n * sizeof(Fr));
    Fr r = poseidon_hash(in.data(), n);
    memcpy(out_mont, r.l, 32);
}

uint64_t rng_circ_n(void* t) { return static_cast<CircuitTables*>(t)->n; }
uint64_t rng_circ_npub(void* t) { return static_cast<CircuitTables*>(t)->num_public; }

// selectors: 13*n*4 u64; sigma: 5*n u64; wires: 5*n*4 u64; pubs: npub*4 u64
void rng_circ_get(void* t_, uint64_t* selectors, uint64_t* sigma, uint64_t* wires,
                  uint64_t* pubs) {
    auto* t = static_cast<CircuitTables*>(t_);
    memcpy(selectors, t->selectors.data(), t->selectors.size() * sizeof(Fr));
    memcpy(sigma, t->sigma.data(), t->sigma.size() * 8);
    memcpy(wires, t->wires.data(), t->wires.size() * sizeof(Fr));
    if (!t->public_inputs.empty())
        memcpy(pubs, t->public_inputs.data(), t->public_inputs.size() * sizeof(Fr));
}

void rng_circ_free(void* t) { delete static_cast<CircuitTables*>(t); }
