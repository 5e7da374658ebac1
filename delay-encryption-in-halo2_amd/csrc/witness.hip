// witness.hip -- Circuit::synthesize of the reference's three circuits as VALUES, in C++: what fills the advice columns (and, at keygen,
// the fixed columns and the permutation) before create_proof commits them -- the part of the reference's timed call that precedes the
// first commitment [src/lib.rs:164-318 DelayEncryptCircuit::synthesize; benches/mod_pow.rs:79-120 RSACircuit; src/encryption/chip.rs:
// 131-204 PoseidonEncCircuit].  This file is dehalo_synthesize, one function per stage; what it is made of:
//   bigint_host.hpp     big integers (big_pow_mod's value is read off the pow_mod rows: src/big_integer/utils.rs:2-17)
//   poseidon_host.hpp   Grain LFSR, Cauchy MDS, optimised constants and sparse matrices, the optimised permutation, the native cipher
//   maingate_host.hpp   the MainGate / RangeChip layouter
//   synth_chips.hpp     BigIntChip, PoseidonChip, the rsa / hash / cipher regions
//   synth_pool.hpp      the host threads of a proving call
// The cell layout follows halo2wrong's MainGate / RangeChip instruction by instruction ([UPSTREAM] maingate v2023_04_20, not in the reference tree: one `apply` row
// per instruction, compose / decompose four terms a row, is_equal four rows, is_zero three, assert_equal one), which reproduces the row counts the reference
// publishes (benches/README.md:56-99; tests/test_witness.py): the same rows, in the same order, as dehalo2_amd/witness.py, which the tests compare it with
// bit for bit.  Host code only (no device work): big-integer arithmetic on 64-bit limbs, field arithmetic through hostfield.hpp.
#include <cstring>

#include "../../include/dehalo.h"
#include "guard.hpp"
#include "synth_chips.hpp"

namespace {
using namespace synth;

// permutation::keygen::Assembly::copy [UPSTREAM plonk/permutation/keygen.rs]: cycles over cells, the smaller cycle relabelled
struct Assembly {
    size_t n;
    std::vector<uint64_t> mapping, aux, sizes;
    Assembly(size_t cols, size_t n_) : n(n_), mapping(cols * n_), aux(cols * n_), sizes(cols * n_, 1) {
        for (size_t i = 0; i < mapping.size(); i++) mapping[i] = aux[i] = i;
    }
    void copy(const Copy& c) {
        uint64_t left = c.c0 * n + c.r0, right = c.c1 * n + c.r1;
        if (aux[left] == aux[right]) return;
        if (sizes[aux[left]] < sizes[aux[right]]) std::swap(left, right);
        const uint64_t la = aux[left];
        sizes[la] += sizes[aux[right]];
        uint64_t i = right;
        do {
            aux[i] = la;
            i = mapping[i];
        } while (i != right);
        std::swap(mapping[left], mapping[right]);
    }
};

Fe fe_from(const uint64_t* p) {
    Fe r;
    memcpy(r.v, p, 32);
    return r;
}

// ---- the stages of dehalo_synthesize, in the order it calls them ----
struct SynthInputs {
    const HostField* f;
    size_t n;                                    // 2^k rows
    bool keygen_outputs, range_lookups;
    uint32_t t, rate, r_f, r_p;
    std::vector<Fe> message;
    Fe key[2];                                   // pose_enc
    size_t num_limbs;                            // mod_pow, delay_enc
    Big n_big, x;
};
int read_inputs(const dehalo_circuit_inputs* in, bool any_output, bool keygen_outputs, SynthInputs& si) {
    if (!in || !any_output) return DEHALO_ERR_INVALID;
    si.f = host_field(DEHALO_FIELD_BN254_FR);
    si.keygen_outputs = keygen_outputs;
    si.range_lookups = in->circuit != DEHALO_CIRCUIT_POSE_ENC;
    if (in->circuit > DEHALO_CIRCUIT_POSE_ENC || in->k < 4 || in->k > 24) return DEHALO_ERR_INVALID;
    si.t = in->t ? in->t : 5, si.rate = in->rate ? in->rate : 4, si.r_f = in->r_f ? in->r_f : 8, si.r_p = in->r_p ? in->r_p : 57;
    if (si.t != 5 || si.rate != 4) return DEHALO_ERR_UNSUPPORTED;      // the row layout (linear()) is the T = 5 one the reference instantiates (src/lib.rs:120-121)
    if (in->message_len > 2 || (in->message_len && !in->message)) return DEHALO_ERR_INVALID;
    si.n = (size_t)1 << in->k;
    for (uint32_t i = 0; i < in->message_len; i++) {
        const Fe m = fe_from(in->message + 4 * i);
        if (HostField::geq(m.v, si.f->p)) return DEHALO_ERR_INVALID;
        si.message.push_back(m);
    }
    if (in->circuit == DEHALO_CIRCUIT_POSE_ENC) {
        if (!in->key) return DEHALO_ERR_INVALID;
        si.key[0] = fe_from(in->key), si.key[1] = fe_from(in->key + 4);
        return 0;
    }
    if (!in->n || !in->x || in->bits_len % LIMB_WIDTH || in->bits_len == 0 || in->bits_len > 8192 || in->exp_bits == 0 || in->exp_bits > 64) return DEHALO_ERR_INVALID;
    si.num_limbs = in->bits_len / LIMB_WIDTH;
    si.n_big.assign(in->n, in->n + si.num_limbs), si.x.assign(in->x, in->x + si.num_limbs);
    { Big t0 = si.n_big; big_trim(t0); if (t0.empty()) return DEHALO_ERR_INVALID; }
    if (in->exp_bits < 64 && (in->e >> in->exp_bits)) return DEHALO_ERR_INVALID;
    return 0;
}

struct Trace {
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    void operator()(const char* what) const {
        if (getenv("DEHALO_SYNTH_TRACE")) fprintf(stderr, "synthesize: %-28s +%.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    }
};

struct Laid { uint32_t rsa_rows = 0; Big want; std::vector<Fe> cipher; };      // what the summary reports of the regions

// hash region, then the cipher keyed by the digest's words 1 and 2 (src/lib.rs:216-316)
void hash_and_cipher(Layouter& L, const SynthInputs& si, const std::vector<Cell>& rsa_out, std::vector<Fe>& cipher_vals) {
    const std::shared_ptr<const PoseidonSpec> spec = poseidon_spec(si.f, si.t, si.r_f, si.r_p);
    Cell key_cells[2];
    hash_region(L, *spec, rsa_out, si.rate, key_cells);
    const Fe key_vals[2] = {key_cells[0].val, key_cells[1].val};
    for (auto& c : cipher_region(L, *spec, key_vals, si.message, key_cells, si.rate)) cipher_vals.push_back(c.val);
}

// (a constraint of the reference's circuit that does not hold for these inputs -- x >= n, an exponent wider than exp_bits, a non-zero message --
// throws NotSatisfied: DEHALO_ERR_INVALID, as any exception other than std::bad_alloc)
void lay_out_regions(Layouter& lay, const dehalo_circuit_inputs* in, const SynthInputs& si, const Trace& trace, Laid& out) {
    if (in->circuit == DEHALO_CIRCUIT_POSE_ENC) {
        const std::shared_ptr<const PoseidonSpec> spec = poseidon_spec(si.f, si.t, si.r_f, si.r_p);
        for (auto& c : cipher_region(lay, *spec, si.key, si.message, nullptr, si.rate)) out.cipher.push_back(c.val);
        return;
    }
    const bool with_hash = in->circuit == DEHALO_CIRCUIT_DELAY_ENC;
    lay.range = RangeLens(si.num_limbs);
    // proving: everything behind the exponentiation may be written beside it (BigIntChip::pow_mod_threads), through a cursor at the row where it will end
    const PowTail tail = [&](Layouter& sub, const std::vector<Cell>& powed) {
        const std::vector<Cell> valid = rsa_expected_rows(sub, powed);
        out.rsa_rows = sub.rows();
        if (with_hash) hash_and_cipher(sub, si, valid, out.cipher);
    };
    const RsaOut rsa = rsa_region(lay, si.n_big, in->e, si.x, in->exp_bits, si.num_limbs, si.keygen_outputs ? nullptr : &tail);
    if (!rsa.tail_ran) out.rsa_rows = lay.rows();
    trace(rsa.tail_ran ? "rsa, hash and cipher regions" : "rsa region");
    out.want = rsa.want;
    if (with_hash && !rsa.tail_ran) hash_and_cipher(lay, si, rsa.cells, out.cipher);
}

dehalo_synthesis_info summary(const Layouter& lay, const SynthInputs& si, const Laid& laid) {
    dehalo_synthesis_info inf{};
    inf.rsa_rows = laid.rsa_rows;
    const Big wl = big_limbs(laid.want, std::min<size_t>(si.num_limbs, 128));
    for (size_t i = 0; i < wl.size() && i < 128; i++) inf.rsa_result[i] = wl[i];
    inf.total_rows = lay.rows();
    for (size_t i = 0; i < laid.cipher.size() && i < 3; i++) memcpy(inf.cipher + 4 * i, laid.cipher[i].v, 32);
    inf.cipher_len = (uint32_t)std::min<size_t>(laid.cipher.size(), 3);
    return inf;
}

// ---- into 2^k-row columns
size_t usable_rows(size_t n) {
    const uint32_t bf = 5;      // blinding_factors of both constraint systems: max(3, 2 queries of advice column e) + 2
    return n - (bf + 1);
}
bool rows_fit_and_unused_zeroed(const Layouter& lay, uint64_t* advice, size_t n) {
    if ((size_t)lay.rows() + 1 > usable_rows(n)) return false;      // "not enough rows available" (upstream: Error::NotEnoughRowsAvailable)
    const size_t rows = lay.rows();
    if (advice)      // (the used rows are already in place)
        for (int c = 0; c < 5; c++) memset(advice + ((size_t)c * n + rows) * 4, 0, (n - rows) * 32);
    return true;
}
void export_fixed(const Layouter& lay, const SynthInputs& si, uint64_t* fixed) {
    const uint32_t num_fixed = si.range_lookups ? 15 : 9;
    memset(fixed, 0, (size_t)num_fixed * si.n * 32);
    for (uint32_t c = 0; c < num_fixed; c++) memcpy(fixed + (size_t)c * si.n * 4, lay.fix[c].data(), (size_t)lay.rows() * 32);
}
// RangeChip::load_table rows (tag, value): the disabled row (0, 0), then every value of every bit length
bool range_table_rows(const Layouter& lay, size_t n, uint64_t* fixed) {
    size_t r = 1;
    for (unsigned ti = 0; ti < lay.range.count; ti++)
        for (uint64_t v = 0; v < ((uint64_t)1 << lay.range.bits[ti]); v++, r++) {
            if (r >= usable_rows(n)) return false;
            fixed[((size_t)RC_T_TAG * n + r) * 4] = ti + 1;
            fixed[((size_t)RC_T_VALUE * n + r) * 4] = v;
        }
    return true;
}
bool has_range_rows(const Layouter& lay) {      // range rows in a MainGate-only circuit
    for (int c = 9; c < NUM_FIX; c++)
        for (auto& v : lay.fix[c])
            if (!v.is_zero()) return true;
    return false;
}
void export_mapping(const Layouter& lay, size_t n, uint64_t* mapping) {
    Assembly asm_(6, n);
    for (auto& c : lay.copies) asm_.copy(c);
    memcpy(mapping, asm_.mapping.data(), 6 * n * 8);
}
void export_selectors(const Layouter& lay, size_t n, uint8_t* const* selectors) {
    for (int s = 0; s < 2; s++) {
        if (!selectors[s]) continue;
        memset(selectors[s], 0, n);
        const auto& col = lay.fix[s == 0 ? RC_S_COMPOSITION : RC_S_OVERFLOW];
        for (size_t r = 0; r < lay.rows(); r++) selectors[s][r] = col[r].is_zero() ? 0 : 1;
    }
}

}   // namespace

extern "C" int dehalo_synthesize(const dehalo_circuit_inputs* in, uint64_t* advice, uint64_t* fixed, uint64_t* mapping, uint8_t* const* selectors,
                                 dehalo_synthesis_info* info) {
    return dh_guard(nullptr, [&]() -> int {
        SynthInputs si{};
        if (const int rc = read_inputs(in, advice || fixed || mapping || info, fixed || mapping || selectors, si)) return rc;
        const Trace trace;
        Layouter lay(si.f, si.keygen_outputs, advice, si.n);
        Laid laid;
        lay_out_regions(lay, in, si, trace, laid);
        trace("hash and cipher regions");
        if (info) *info = summary(lay, si, laid);
        if (!rows_fit_and_unused_zeroed(lay, advice, si.n)) return DEHALO_ERR_INVALID;
        trace("unused rows zeroed");
        if (fixed) {
            export_fixed(lay, si, fixed);
            if (si.range_lookups && !range_table_rows(lay, si.n, fixed)) return DEHALO_ERR_INVALID;
        }
        if (!si.range_lookups && si.keygen_outputs && has_range_rows(lay)) return DEHALO_ERR_INVALID;
        if (mapping) export_mapping(lay, si.n, mapping);
        if (selectors && si.range_lookups) export_selectors(lay, si.n, selectors);
        return 0;
    });
}
