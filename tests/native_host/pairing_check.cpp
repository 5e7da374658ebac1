// pairing_check -- csrc/pairing_host.hpp on the CPU (g++, ASan + UBSan; tests/test_pairing_host.py drives it and compares with oracle/pairing.py's verdicts).
// One command per line on stdin, one JSON line per command on stdout:
//   check <curve> <count> <count x 64 bytes hex: G1 affine x | y, Montgomery> <count x 128 bytes hex: G2 raw>     ("-" for an empty list)
//                      {"rc": the status dehalo_pairing_check returns, "is_one": 0 | 1 (-1 when rc != 0)}
//   constants          the derived constants' self-check, the limbs of (q^4 - q^2 + 1) / r as hex (low limb first) and xi^((q - 1) / 6) as raw Montgomery bytes
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../delay-encryption-in-halo2_amd/csrc/pairing_host.hpp"

static std::string hex(const uint8_t* b, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) { s += d[b[i] >> 4]; s += d[b[i] & 15]; }
    return s;
}
static bool unhex(const std::string& s, std::vector<uint8_t>& out, size_t want) {
    if (want == 0) return s == "-";
    if (s.size() != 2 * want) return false;
    out.assign(want, 0);
    for (size_t i = 0; i < 2 * want; i++) {
        const char c = s[i];
        const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
        if (v < 0) return false;
        out[i / 2] = (uint8_t)(out[i / 2] | (v << (i & 1 ? 0 : 4)));
    }
    return true;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "check") {
            int curve = -1;
            size_t count = 0;
            std::string a, b;
            in >> curve >> count >> a >> b;
            std::vector<uint8_t> g1b, g2b;
            if (count > 64 || !unhex(a, g1b, 64 * count) || !unhex(b, g2b, 128 * count)) { printf("{\"bad\": true}\n"); continue; }
            std::vector<uint64_t> g1(8 * count);      // exactly the words the check may read
            if (count) memcpy(g1.data(), g1b.data(), 64 * count);
            int is_one = -1, rc;
            const PairingHost* ph = pairing_host(curve);
            if (!ph) rc = DEHALO_ERR_UNSUPPORTED;
            else rc = ph->check(g1.data(), g2b.data(), count, &is_one);
            printf("{\"rc\": %d, \"is_one\": %d}\n", rc, rc ? -1 : is_one);
        } else if (cmd == "constants") {
            const PairingHost* ph = pairing_host(DEHALO_CURVE_BN254_G1);
            std::string limbs;
            for (uint64_t w : ph->hard) {
                char t[20];
                snprintf(t, sizeof t, "%016llx", (unsigned long long)w);
                limbs += limbs.empty() ? "" : " ";
                limbs += t;
            }
            uint8_t f[64];
            memcpy(f, ph->frob1.a.v, 32); memcpy(f + 32, ph->frob1.b.v, 32);
            printf("{\"ok\": %s, \"hard\": \"%s\", \"frob1\": \"%s\"}\n", ph->ok ? "true" : "false", limbs.c_str(), hex(f, 64).c_str());
        } else if (!cmd.empty()) {
            printf("{\"unknown\": true}\n");
        }
    }
    return 0;
}
