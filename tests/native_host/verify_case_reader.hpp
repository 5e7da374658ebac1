// verify_case_reader.hpp -- what verify_host_check.cpp and verify_ipa_host_check.cpp read their case files with: little-endian words off the file's bytes, and
// the constraint system both files carry --
//   num_advice, num_fixed, num_instance, minimum_degree, nodes, constants, gates, lookups, permutation columns, advice / fixed / instance queries, challenges,
//     shuffles : 14 x u32 | nodes (kind, a, b, rotation) | constants 32 B each | gates | lookup_lens | lookup_inputs | lookup_tables | permutation columns, advice,
//     fixed, instance queries (kind, index, rotation) | advice_phases u8 | challenge_phases u8 | shuffle_lens | shuffle_inputs | shuffle_tables
#pragma once
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../include/dehalo.h"

struct Reader {
    std::vector<uint8_t> data;
    size_t pos = 0;
    bool ok = true;
    explicit Reader(const char* path) {
        std::ifstream in(path, std::ios::binary);
        data.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    }
    const uint8_t* take(size_t n) {
        static const uint8_t none = 0;
        if (n > data.size() - pos) { ok = false; return &none; }
        const uint8_t* p = data.data() + pos;
        pos += n;
        return n ? p : &none;
    }
    void copy(void* dst, size_t n) {
        const uint8_t* p = take(n);
        if (ok && n) memcpy(dst, p, n);
    }
    uint32_t u32() {
        const uint8_t* p = take(4);
        return ok ? (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24) : 0;
    }
    // n values of T, a 32-bit word or a struct of them
    template <class T> std::vector<T> words(size_t n) {
        std::vector<T> v;
        for (size_t i = 0; i < n && ok; i++) {
            uint32_t w[sizeof(T) / 4];
            for (uint32_t& x : w) x = u32();
            v.emplace_back();
            memcpy(&v.back(), w, sizeof(T));
        }
        return v;
    }
    // n bytes; a count larger than the whole file reads as none
    std::vector<uint8_t> bytes(size_t n) {
        std::vector<uint8_t> v(n <= data.size() ? n : 0);
        copy(v.data(), v.size());
        return v;
    }
};

// a dehalo_constraint_system and the arrays it points into (so: made in place, never copied)
struct CaseCS {
    dehalo_constraint_system d{};
    std::vector<dehalo_expr_node> nodes;
    std::vector<uint64_t> constants;
    std::vector<uint32_t> gates, lookup_lens, lookup_inputs, lookup_tables, shuffle_lens, shuffle_inputs, shuffle_tables;
    std::vector<dehalo_column_query> perm, aq, fq, iq;
    std::vector<uint8_t> advice_phases, challenge_phases;
    // false: the file ends inside it
    bool read(Reader& r) {
        for (uint32_t* count : {&d.num_advice, &d.num_fixed, &d.num_instance, &d.minimum_degree, &d.num_nodes, &d.num_constants, &d.num_gates, &d.num_lookups,
                                &d.num_permutation_columns, &d.num_advice_queries, &d.num_fixed_queries, &d.num_instance_queries, &d.num_challenges, &d.num_shuffles})
            *count = r.u32();
        if (!r.ok) return false;
        nodes = r.words<dehalo_expr_node>(d.num_nodes);
        constants.assign(4 * (size_t)d.num_constants + 1, 0);
        r.copy(constants.data(), 32 * (size_t)d.num_constants);
        gates = r.words<uint32_t>(d.num_gates);
        lookup_lens = r.words<uint32_t>(d.num_lookups);
        size_t tl = 0, ts = 0;
        for (uint32_t l : lookup_lens) tl += l;
        lookup_inputs = r.words<uint32_t>(tl);
        lookup_tables = r.words<uint32_t>(tl);
        perm = r.words<dehalo_column_query>(d.num_permutation_columns);
        aq = r.words<dehalo_column_query>(d.num_advice_queries);
        fq = r.words<dehalo_column_query>(d.num_fixed_queries);
        iq = r.words<dehalo_column_query>(d.num_instance_queries);
        advice_phases = r.bytes(d.num_advice);
        challenge_phases = r.bytes(d.num_challenges);
        shuffle_lens = r.words<uint32_t>(d.num_shuffles);
        for (uint32_t l : shuffle_lens) ts += l;
        shuffle_inputs = r.words<uint32_t>(ts);
        shuffle_tables = r.words<uint32_t>(ts);
        d.nodes = nodes.data(); d.constants = constants.data(); d.gates = gates.data();
        d.lookup_lens = lookup_lens.data(); d.lookup_inputs = lookup_inputs.data(); d.lookup_tables = lookup_tables.data();
        d.permutation_columns = perm.data(); d.advice_queries = aq.data(); d.fixed_queries = fq.data(); d.instance_queries = iq.data();
        d.advice_phases = advice_phases.data(); d.challenge_phases = challenge_phases.data();
        d.shuffle_lens = shuffle_lens.data(); d.shuffle_inputs = shuffle_inputs.data(); d.shuffle_tables = shuffle_tables.data();
        return r.ok;
    }
};
