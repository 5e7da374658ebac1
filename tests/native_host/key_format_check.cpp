// key_format_check -- csrc/key_format.hpp on the CPU (g++, ASan + UBSan; tests/test_key_format_host.py drives it and compares with the Python mirror).
// One command per line on stdin, one JSON line per command on stdout.  A shape is: <nf> <npc> <nsel> <ext_shift>.
//   layout <format> <k> <shape>                                    the layout, or {"ok": false}
//   header <format> <k> <num_fixed> <len> <shape> <pk> <want_k>    key_parse_header over a buffer of min(len, 8) bytes that holds k and num_fixed (want_k < 0:
//                                                                  any k): the error's number and text
//   words <format> <k> <shape> <section> <poly> <value>            a pk-sized buffer with every count and length word right, then the length word of polynomial
//                                                                  <poly> of <section> (poly < 0: the slice's count word) set to <value>: key_check_poly_words
//   texts                                                          the section names and the element / point failure texts
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../delay-encryption-in-halo2_amd/csrc/key_format.hpp"

static KeyShape read_shape(std::istringstream& in) {
    KeyShape sh;
    unsigned long long nf = 0, npc = 0, nsel = 0;
    uint32_t ext = 0;
    in >> nf >> npc >> nsel >> ext;
    sh.nf = (size_t)nf; sh.npc = (size_t)npc; sh.nsel = (size_t)nsel; sh.ext_shift = ext;
    return sh;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "layout") {
            int format = -1;
            uint32_t k = 0;
            in >> format >> k;
            const KeyShape sh = read_shape(in);
            KeyLayout L;
            if (!key_layout(format, k, sh, L)) { printf("{\"ok\": false}\n"); continue; }
            printf("{\"ok\": true, \"k\": %u, \"n\": %zu, \"m\": %zu, \"point\": %zu, \"off_fixed_c\": %zu, \"off_perm_c\": %zu, \"off_selectors\": %zu, \"sel_bytes\": %zu, "
                   "\"vk_size\": %zu, \"pk_size\": %zu, \"polys\": {",
                   L.k, L.n, L.m, L.point, L.off_fixed_c, L.off_perm_c, L.off_selectors, L.sel_bytes, L.vk_size, L.pk_size);
            for (int s = KEY_L0; s < KEY_SECTIONS; s++) {
                const KeyPolys& P = L.polys[s];
                printf("%s\"%s\": [%zu, %zu, %zu, %s]", s == KEY_L0 ? "" : ", ", key_section_name(s), P.off, P.count, P.len, P.slice ? "true" : "false");
            }
            printf("}}\n");
        } else if (cmd == "header") {
            int format = -1, pk = 0;
            uint32_t k = 0, nf_file = 0;
            unsigned long long len = 0;
            long long want = -1;
            in >> format >> k >> nf_file >> len;
            const KeyShape sh = read_shape(in);
            in >> pk >> want;
            std::vector<uint8_t> buf(len < 8 ? (size_t)len : 8);      // exactly what the parser may read: ASan sees a byte too many
            uint8_t head[8];
            key_put_u32_be(head, k);
            key_put_u32_be(head + 4, nf_file);
            for (size_t i = 0; i < buf.size(); i++) buf[i] = head[i];
            KeyLayout L;
            const int e = key_parse_header(buf.data(), (size_t)len, format, sh, want < 0 ? DEHALO_KEEP_K : (uint32_t)want, pk != 0, L);
            printf("{\"error\": %d, \"text\": \"%s\"}\n", e, key_header_error_text(e));
        } else if (cmd == "words") {
            int format = -1, section = 0;
            uint32_t k = 0, value = 0;
            long long poly = -1;
            in >> format >> k;
            const KeyShape sh = read_shape(in);
            in >> section >> poly >> value;
            KeyLayout L;
            if (!key_layout(format, k, sh, L) || L.pk_size > ((size_t)1 << 24) || section < KEY_L0 || section >= KEY_SECTIONS) { printf("{\"ok\": false}\n"); continue; }
            std::vector<uint8_t> buf(L.pk_size, 0);      // exactly the key's size
            for (int s = KEY_L0; s < KEY_SECTIONS; s++) {
                const KeyPolys& P = L.polys[s];
                if (P.slice) key_put_u32_be(buf.data() + P.off, (uint32_t)P.count);
                for (size_t i = 0; i < P.count; i++) key_put_u32_be(buf.data() + P.poly_off(i), (uint32_t)P.len);
            }
            const KeyPolys& T = L.polys[section];
            if (poly < 0 ? !T.slice : (size_t)poly >= T.count) { printf("{\"ok\": false}\n"); continue; }
            key_put_u32_be(buf.data() + (poly < 0 ? T.off : T.poly_off((size_t)poly)), value);
            int bad = -1;
            const int e = key_check_poly_words(buf.data(), L, bad);
            printf("{\"ok\": true, \"error\": %d, \"text\": \"%s\", \"section\": \"%s\"}\n", e, key_header_error_text(e), key_section_name(bad));
        } else if (cmd == "texts") {
            printf("{\"sections\": [");
            for (int s = 0; s < KEY_SECTIONS; s++) printf("%s\"%s\"", s ? ", " : "", key_section_name(s));
            printf("], \"element_processed\": \"%s\", \"element_raw\": \"%s\", \"points_processed\": [\"%s\", \"%s\", \"%s\"], \"points_raw\": [\"%s\", \"%s\"]}\n",
                   key_element_error_text(true, KEY_FIXED_POLYS, 7).c_str(), key_element_error_text(false, KEY_PERM_COSETS, 12345678901ull).c_str(),
                   point_status_text(1, true), point_status_text(2, true), point_status_text(4, true), point_status_text(1, false),
                   point_status_text(2, false));
        } else if (!cmd.empty()) {
            printf("{\"unknown\": true}\n");
        }
    }
    return 0;
}
