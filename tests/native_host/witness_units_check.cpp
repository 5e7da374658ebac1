// The units of witness generation below dehalo_synthesize, each on its own under ASan + UBSan (tests/test_witness.py feeds the cases and compares):
//   div  <u limbs> | <v limbs>     big_divmod and big_mul (csrc/bigint_host.hpp); little-endian hex limbs, zero high limbs allowed.  Prints q, r and u * v.
//   kat  t r_f r_p <t words>       PoseidonSpec::permute (csrc/poseidon_host.hpp) over BN254's scalar field; hex words in, hex words out.
//   range num_limbs                RangeLens (csrc/maingate_host.hpp): the table's bit lengths in tag order, then tag(b) for b = 0..16.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../include/dehalo.h"
#include "../../delay-encryption-in-halo2_amd/csrc/bigint_host.hpp"
#include "../../delay-encryption-in-halo2_amd/csrc/maingate_host.hpp"

using namespace synth;

static std::string hex_of(const uint64_t* limbs, size_t n) {      // one number, most significant limb first
    while (n && limbs[n - 1] == 0) n--;
    if (!n) return "0";
    std::string out;
    char buf[17];
    for (size_t i = n; i-- > 0;) {
        snprintf(buf, sizeof buf, i + 1 == n ? "%llx" : "%016llx", (unsigned long long)limbs[i]);
        out += buf;
    }
    return out;
}

static Fe fe_of_hex(const std::string& s) {      // up to 64 hex digits
    Fe r{{0, 0, 0, 0}};
    for (size_t i = 0; i < s.size(); i++) {
        const size_t pos = s.size() - 1 - i;
        r.v[i / 16] |= (uint64_t)std::stoul(s.substr(pos, 1), nullptr, 16) << (4 * (i % 16));
    }
    return r;
}

static void div_case(std::istringstream& in) {
    Big u, v, *into = &u;
    for (std::string w; in >> w;) {
        if (w == "|") into = &v;
        else into->push_back(std::stoull(w, nullptr, 16));
    }
    Big q, r;
    big_divmod(u, v, q, r);
    const Big p = big_mul(u, v);
    printf("%s %s %s\n", hex_of(q.data(), q.size()).c_str(), hex_of(r.data(), r.size()).c_str(), hex_of(p.data(), p.size()).c_str());
}

static void kat_case(std::istringstream& in) {
    uint32_t t, r_f, r_p;
    in >> t >> r_f >> r_p;
    std::vector<Fe> st;
    for (std::string w; in >> w;) st.push_back(fe_of_hex(w));
    if (st.size() != t) throw std::runtime_error("kat: t words expected");
    const PoseidonSpec spec(host_field(DEHALO_FIELD_BN254_FR), t, r_f, r_p);
    for (const Fe& x : spec.permute(st)) printf("%s ", hex_of(x.v, 4).c_str());
    printf("\n");
}

static void range_case(std::istringstream& in) {
    size_t num_limbs;
    in >> num_limbs;
    const RangeLens lens(num_limbs);
    for (unsigned i = 0; i < lens.count; i++) printf("%u ", lens.bits[i]);
    printf("|");
    for (unsigned b = 0; b <= 16; b++) printf(" %llu", (unsigned long long)lens.tag(b));
    printf("\n");
}

int main() {
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "div") div_case(in);
        else if (what == "kat") kat_case(in);
        else if (what == "range") range_case(in);
        else if (!what.empty()) { fprintf(stderr, "unknown case: %s\n", what.c_str()); return 2; }
    }
    return 0;
}
