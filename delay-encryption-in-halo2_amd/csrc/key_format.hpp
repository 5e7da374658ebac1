// key_format.hpp -- VerifyingKey and ProvingKey on disk in upstream's three SerdeFormats [UPSTREAM halo2_proofs @ v2023_04_20 plonk.rs, poly.rs, helpers.rs;
// halo2curves 0.3.x SerdeObject]: where every section of
//   vk   = k: u32 BE | num_fixed: u32 BE | fixed commitments | permutation commitments | selectors (2^k bits each, packed LSB first)
//   pk   = vk | l0 | l_last | l_active_row | slice(fixed_values) | slice(fixed_polys) | slice(fixed_cosets) | slice(perm values) | slice(perm polys) | slice(perm cosets)
//   poly = len: u32 BE | len elements          slice = count: u32 BE | count polys
// lies per format, and the validation of untrusted bytes against the circuit: the header, the total length, every count and length word.  A commitment is 32 B
// (Processed: the point codec's compressed form) or 64 B (both raw formats: Montgomery limbs), a field element 32 B in every format (Processed: the canonical
// integer, little-endian; raw: Montgomery limbs), so the formats differ in length by 32 B per commitment only.  What the bytes of a point or an element MEAN is
// the device's (gfft.cuh: the point codec; scalar_codec.cuh: its scalar twin).
// Host only, no HIP header: keygen.hip includes it, and tests/native_host/key_format_check.cpp drives it on the CPU against the Python mirror (keygen.py) -- this
// is the parser of untrusted bytes.  The formats restate upstream from memory, as the other formats here do.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/dehalo.h"
#include "g1_host.hpp"      // serde_format_known, point_status_text

// what the circuit fixes of a key's shape: fixed columns, permutation columns, selectors serialised with the vk, and extended_k - k (from the degree)
struct KeyShape {
    size_t nf = 0, npc = 0, nsel = 0;
    uint32_t ext_shift = 0;
};

// the sections that hold points or elements, in file order
enum KeySection {
    KEY_FIXED_COMMITMENTS = 0, KEY_PERM_COMMITMENTS, KEY_L0, KEY_L_LAST, KEY_L_ACTIVE_ROW, KEY_FIXED_VALUES, KEY_FIXED_POLYS, KEY_FIXED_COSETS, KEY_PERM_VALUES,
    KEY_PERM_POLYS, KEY_PERM_COSETS, KEY_SECTIONS
};
inline const char* key_section_name(int s) {
    static const char* const name[] = {"fixed commitments", "permutation commitments", "l0", "l_last", "l_active_row", "fixed_values", "fixed_polys", "fixed_cosets",
                                       "permutation values", "permutation polys", "permutation cosets"};
    return s >= 0 && s < KEY_SECTIONS ? name[s] : "";
}

// the sections over the extended domain: kept in the kernels' internal form on the device, in upstream's standard form on disk
inline bool key_section_extended(int s) { return (s >= KEY_L0 && s <= KEY_L_ACTIVE_ROW) || s == KEY_FIXED_COSETS || s == KEY_PERM_COSETS; }
// the most elements one call of the scalar codec takes (count < 2^29, include/dehalo.h): a larger group of polynomials is converted or checked in pieces
constexpr size_t KEY_CODEC_MOST = (size_t)1 << 28;

// One polynomial section: `count` polynomials of `len` elements.  A slice starts with its count word at `off`; a lone polynomial (l0, l_last, l_active_row) has
// none.  Polynomial i's length word is at poly_off(i), its elements 4 bytes further.
struct KeyPolys {
    size_t off = 0, count = 0, len = 0;
    bool slice = false;
    size_t poly_off(size_t i) const { return off + (slice ? 4 : 0) + i * (4 + 32 * len); }
    size_t bytes() const { return (slice ? 4 : 0) + count * (4 + 32 * len); }
};

struct KeyLayout {
    uint32_t k = 0;
    size_t n = 0, m = 0, point = 0;                      // rows, extended rows, bytes per commitment
    size_t off_fixed_c = 0, off_perm_c = 0, off_selectors = 0, sel_bytes = 0, vk_size = 0;
    KeyPolys polys[KEY_SECTIONS];                        // [KEY_L0 .. KEY_PERM_COSETS]; the two commitment lists have no entry
    size_t pk_size = 0;
};
constexpr uint32_t KEY_MAX_K = 28;

// false for an unknown format, k > 28, an extended domain above 2^32 rows (its length word is a u32) or a size beyond size_t
inline bool key_layout(int format, uint32_t k, const KeyShape& sh, KeyLayout& L) {
    if (!serde_format_known(format) || k > KEY_MAX_K || sh.ext_shift > 32 || k + sh.ext_shift > 32) return false;
    const uint64_t n = (uint64_t)1 << k, m = n << sh.ext_shift;
    if (m > 0xffffffffull || sh.nf > 0xffffffffull || sh.npc > 0xffffffffull || sh.nsel > 0xffffffffull) return false;
    const uint64_t point = format == DEHALO_SERDE_PROCESSED ? 32 : 64;
    L.k = k; L.n = (size_t)n; L.m = (size_t)m; L.point = (size_t)point;
    L.sel_bytes = (size_t)((n + 7) / 8);
    unsigned __int128 o = 8;
    L.off_fixed_c = (size_t)o; o += (unsigned __int128)point * sh.nf;
    L.off_perm_c = (size_t)o; o += (unsigned __int128)point * sh.npc;
    L.off_selectors = (size_t)o; o += (unsigned __int128)L.sel_bytes * sh.nsel;
    if (o > (unsigned __int128)SIZE_MAX) return false;
    L.vk_size = (size_t)o;
    const size_t cnt[KEY_SECTIONS] = {0, 0, 1, 1, 1, sh.nf, sh.nf, sh.nf, sh.npc, sh.npc, sh.npc};
    const uint64_t len[KEY_SECTIONS] = {0, 0, m, m, m, n, n, m, n, n, m};
    for (int s = KEY_L0; s < KEY_SECTIONS; s++) {
        KeyPolys& P = L.polys[s];
        P.off = (size_t)o; P.count = cnt[s]; P.len = (size_t)len[s]; P.slice = s >= KEY_FIXED_VALUES;
        o += (P.slice ? 4 : 0) + (unsigned __int128)cnt[s] * (4 + 32 * (unsigned __int128)len[s]);
        if (o > (unsigned __int128)SIZE_MAX) return false;
    }
    L.pk_size = (size_t)o;
    return true;
}

enum KeyHeaderError {
    KEY_HEADER_OK = 0, KEY_HEADER_FORMAT, KEY_HEADER_SHORT, KEY_HEADER_K, KEY_HEADER_K_DIFFERS, KEY_HEADER_NUM_FIXED, KEY_HEADER_LENGTH, KEY_HEADER_POLY_COUNT,
    KEY_HEADER_POLY_LENGTH
};
inline const char* key_header_error_text(int e) {
    static const char* const text[] = {"", "unknown format", "length: unexpected end of input", "k out of range", "k differs from the params'",
                                       "fixed-column count: the key's number of fixed commitments differs from the circuit's fixed columns",
                                       "length does not match the circuit (unexpected end of input or trailing bytes)",
                                       "polynomial count differs from the circuit's", "polynomial length differs from the domain's"};
    return e >= 0 && e <= KEY_HEADER_POLY_LENGTH ? text[e] : "";
}
inline uint32_t key_u32_be(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline void key_put_u32_be(uint8_t* o, uint32_t v) { for (int i = 0; i < 4; i++) o[i] = (uint8_t)(v >> (8 * (3 - i))); }

// k of `len` bytes that claim to be a key in `format`: reads bytes[0 .. 4), and only when len >= 8 (a key has both header words)
inline KeyHeaderError key_peek_k(const uint8_t* bytes, size_t len, int format, uint32_t& k) {
    if (!serde_format_known(format)) return KEY_HEADER_FORMAT;
    if (len < 8) return KEY_HEADER_SHORT;
    k = key_u32_be(bytes);
    return k > KEY_MAX_K ? KEY_HEADER_K : KEY_HEADER_OK;
}

// The header of a vk (pk = false) or pk against the circuit's shape: reads bytes[0 .. 8) only; k must be want_k unless that is DEHALO_KEEP_K, the fixed-column
// count the circuit's, and the length exactly the layout's.
inline KeyHeaderError key_parse_header(const uint8_t* bytes, size_t len, int format, const KeyShape& sh, uint32_t want_k, bool pk, KeyLayout& L) {
    uint32_t k = 0;
    const KeyHeaderError e = key_peek_k(bytes, len, format, k);
    if (e != KEY_HEADER_OK) return e;
    if (want_k != DEHALO_KEEP_K && k != want_k) return KEY_HEADER_K_DIFFERS;
    if (!key_layout(format, k, sh, L)) return KEY_HEADER_K;
    if ((size_t)key_u32_be(bytes + 4) != sh.nf) return KEY_HEADER_NUM_FIXED;
    if (len != (pk ? L.pk_size : L.vk_size)) return KEY_HEADER_LENGTH;
    return KEY_HEADER_OK;
}

// Every count and length word of a pk whose header passed (so all of them lie inside the buffer): the first that differs, with its section
inline KeyHeaderError key_check_poly_words(const uint8_t* bytes, const KeyLayout& L, int& section) {
    for (int s = KEY_L0; s < KEY_SECTIONS; s++) {
        const KeyPolys& P = L.polys[s];
        section = s;
        if (P.slice && (size_t)key_u32_be(bytes + P.off) != P.count) return KEY_HEADER_POLY_COUNT;
        for (size_t i = 0; i < P.count; i++)
            if ((size_t)key_u32_be(bytes + P.poly_off(i)) != P.len) return KEY_HEADER_POLY_LENGTH;
    }
    section = -1;
    return KEY_HEADER_OK;
}

inline std::string key_element_error_text(bool encodings, int section, uint64_t index) {
    return std::string(encodings ? "an element is not below the modulus" : "an element's stored word is not below the modulus") + ": " + key_section_name(section) + ", element " +
           std::to_string(index);
}
