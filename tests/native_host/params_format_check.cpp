// params_format_check -- csrc/params_format.hpp on the CPU (g++, ASan + UBSan; tests/test_params_format_host.py drives it and compares with the Python mirror).
// One command per line on stdin, one JSON line per command on stdout:
//   layout <format> <k>           the layout, or {"ok": false}
//   header <format> <k> <len>     params_parse_header over a buffer of min(len, 4) bytes that holds k: the error's number and text
//   gen                           BN254's G2 generator: on the curve?, its raw bytes, the twist constant's raw bytes
//   mul <scalar hex, canonical>   [s] generator: raw bytes
//   g2 <128 raw bytes hex>        from_raw_checked's status, compress_raw's bytes, and decompress_raw of those: status and raw bytes
//   dec <64 bytes hex>            decompress_raw: status and raw bytes
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../delay-encryption-in-halo2_amd/csrc/params_format.hpp"

static std::string hex(const uint8_t* b, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) { s += d[b[i] >> 4]; s += d[b[i] & 15]; }
    return s;
}
static bool unhex(const std::string& s, std::vector<uint8_t>& out, size_t want) {
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
    const HostField* q = host_field(DEHALO_FIELD_BN254_FQ);
    const G2Host g2(q);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "layout") {
            int format = -1;
            uint32_t k = 0;
            in >> format >> k;
            ParamsLayout L;
            if (!params_layout(format, k, L)) { printf("{\"ok\": false}\n"); continue; }
            printf("{\"ok\": true, \"n\": %zu, \"g1\": %zu, \"g2\": %zu, \"off_g\": %zu, \"off_gl\": %zu, \"off_g2\": %zu, \"off_sg2\": %zu, \"size\": %zu}\n", L.n, L.g1, L.g2, L.off_g,
                   L.off_gl, L.off_g2, L.off_sg2, L.size);
        } else if (cmd == "header") {
            int format = -1;
            uint32_t k = 0;
            unsigned long long len = 0;
            in >> format >> k >> len;
            std::vector<uint8_t> buf(len < 4 ? (size_t)len : 4);      // exactly what the parser may read: ASan sees a byte too many
            for (size_t i = 0; i < buf.size(); i++) buf[i] = (uint8_t)(k >> (8 * i));
            ParamsLayout L;
            const int e = params_parse_header(buf.data(), (size_t)len, format, L);
            printf("{\"error\": %d, \"text\": \"%s\"}\n", e, params_header_error_text(e));
        } else if (cmd == "gen") {
            uint8_t raw[128], b[64];
            const G2Host::Pt G = bn254_g2_generator(q);
            g2.to_raw(G, raw);
            const Fq2 tb = g2.twist_b();
            memcpy(b, tb.a.v, 32); memcpy(b + 32, tb.b.v, 32);
            printf("{\"on_curve\": %s, \"raw\": \"%s\", \"b\": \"%s\"}\n", g2.on_curve(G) ? "true" : "false", hex(raw, 128).c_str(), hex(b, 64).c_str());
        } else if (cmd == "mul") {
            std::string s;
            in >> s;
            std::vector<uint8_t> sb;
            if (!unhex(s, sb, 32)) { printf("{\"bad\": true}\n"); continue; }
            uint64_t sc[4];
            memcpy(sc, sb.data(), 32);
            uint8_t raw[128];
            g2.to_raw(g2.scalar_mul(sc, bn254_g2_generator(q)), raw);
            printf("{\"raw\": \"%s\"}\n", hex(raw, 128).c_str());
        } else if (cmd == "g2") {
            std::string s;
            in >> s;
            std::vector<uint8_t> raw;
            if (!unhex(s, raw, 128)) { printf("{\"bad\": true}\n"); continue; }
            G2Host::Pt P;
            const int chk = g2.from_raw_checked(raw.data(), P);
            uint8_t enc[64], back[128];
            g2.compress_raw(raw.data(), enc);
            const int st = g2.decompress_raw(enc, back);
            printf("{\"check\": %d, \"compressed\": \"%s\", \"status\": %d, \"raw\": \"%s\"}\n", chk, hex(enc, 64).c_str(), st, hex(back, 128).c_str());
        } else if (cmd == "dec") {
            std::string s;
            in >> s;
            std::vector<uint8_t> enc;
            if (!unhex(s, enc, 64)) { printf("{\"bad\": true}\n"); continue; }
            uint8_t back[128];
            const int st = g2.decompress_raw(enc.data(), back);
            printf("{\"status\": %d, \"raw\": \"%s\"}\n", st, hex(back, 128).c_str());
        } else if (!cmd.empty()) {
            printf("{\"unknown\": true}\n");
        }
    }
    return 0;
}
