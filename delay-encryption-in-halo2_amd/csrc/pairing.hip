// pairing.hip -- dehalo_pairing_table_* and dehalo_pairing_checks*: line tables of fixed G2 points, made on the host (pairing_host.hpp), and the kernel that
// runs many independent pairing checks over them in one launch (pairing.cuh).  A host table (ctx = NULL) runs the same tables through PairingHost::table_checks:
// a mode the caller chooses, never a fallback.  C entry points run under dh_guard, as everywhere.
#include <memory>

#include "internal.hpp"
#include "pairing.cuh"
#include "pairing_host.hpp"

static_assert(PAIRING_STEPS == PairingHost::LINE_STEPS, "the kernel walks the host's table");
static_assert(PAIRING_MAX_PAIRS == DEHALO_PAIRING_MAX_PAIRS, "the kernel's LDS holds the header's maximum");

struct dehalo_pairing_table {
    dehalo_ctx* ctx = nullptr;      // null: a host table
    int curve = 0;
    uint32_t pairs = 0, one_mask = 0, hard_bits = 0;      // one_mask: bit j = Q_j is the identity
    std::vector<PairingHost::LineTable> host;
    DevMem lines;       // pairs x 102 x {lam.a, lam.b, mu.a, mu.b}, standard Montgomery
    DevMem consts;      // 12 words: conj(frob[k]) frob[k] for k < 6, a | b; then the hard exponent, 16 u64
};

extern "C" uint32_t dehalo_pairing_checks_per_block(const dehalo_pairing_table*) { return PAIRING_WAVES; }

extern "C" int dehalo_pairing_table_create(dehalo_ctx* ctx, int curve, const uint8_t* g2_raw, uint32_t pairs, dehalo_pairing_table** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!out || !g2_raw || curve_scalar_field(curve) < 0) return dh_fail(ctx, DEHALO_ERR_INVALID, "pairing_table_create: null argument or unknown curve");
        const PairingHost* ph = pairing_host(curve);
        if (!ph || !ph->ok) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "pairing_table_create: no pairing on this curve");
        if (pairs == 0 || pairs > DEHALO_PAIRING_MAX_PAIRS) return dh_fail(ctx, DEHALO_ERR_INVALID, "pairing_table_create: pairs out of range");
        std::unique_ptr<dehalo_pairing_table> t(new dehalo_pairing_table);
        t->ctx = ctx; t->curve = curve; t->pairs = pairs;
        t->host.resize(pairs);
        for (uint32_t j = 0; j < pairs; j++) {
            G2Host::Pt Q;
            if (ph->load_g2(g2_raw + 128 * (size_t)j, Q) != PairingHost::G2_OK)
                return dh_fail(ctx, DEHALO_ERR_INVALID, "pairing_table_create: a G2 point is off the twist, outside the order-r subgroup or holds a word not below q");
            if (!ph->line_table(Q, t->host[j])) return dh_fail(ctx, DEHALO_ERR_INVALID, "pairing_table_create: a degenerate step in a G2 point's Miller loop");
            if (t->host[j].one) t->one_mask |= 1u << j;
        }
        if (!ctx) { *out = t.release(); return 0; }
        // the device's copy: the lines, then the constants of the final exponentiation
        std::vector<Fe> lines(4 * PairingHost::LINE_STEPS * (size_t)pairs, Fe{});
        for (uint32_t j = 0; j < pairs; j++)
            for (size_t i = 0; i < t->host[j].lines.size(); i++) {
                lines[2 * (PairingHost::LINE_STEPS * 2 * (size_t)j + i)] = t->host[j].lines[i].a;
                lines[2 * (PairingHost::LINE_STEPS * 2 * (size_t)j + i) + 1] = t->host[j].lines[i].b;
            }
        std::vector<Fe> consts(16, Fe{});
        for (int k = 0; k < 6; k++) {
            const Fq2 g = ph->e2.mul(ph->conj2(ph->frob[k]), ph->frob[k]);
            consts[2 * k] = g.a;
            consts[2 * k + 1] = g.b;
        }
        if (ph->hard.size() > 16) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "pairing_table_create: the hard exponent is longer than 1024 bits");
        memcpy(&consts[12], ph->hard.data(), 8 * ph->hard.size());
        for (size_t b = 64 * ph->hard.size(); b-- > 0;)
            if ((ph->hard[b >> 6] >> (b & 63)) & 1) { t->hard_bits = (uint32_t)b + 1; break; }
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        TRY(t->lines.alloc(ctx, lines.size(), false));
        TRY(t->consts.alloc(ctx, consts.size(), false));
        TRY(dehalo_upload(ctx, lines.data(), 32 * lines.size(), t->lines.p));
        TRY(dehalo_upload(ctx, consts.data(), 32 * consts.size(), t->consts.p));
        *out = t.release();
        return 0;
    });
}

extern "C" void dehalo_pairing_table_release(dehalo_pairing_table* t) {
    if (!t) return;
    (void)dh_guard(nullptr, [&]() -> int {
        if (t->ctx) {
            std::lock_guard<std::recursive_mutex> lk(t->ctx->mu);
            (void)hipSetDevice(t->ctx->device);
            (void)hipStreamSynchronize(t->ctx->stream.get());      // (a launch on the context's stream may still read the table)
            delete t;
        } else delete t;
        return 0;
    });
}

// what both calls refuse; 0 with checks = 0 means "nothing to do"
static int pairing_checks_args(dehalo_ctx* ctx, const dehalo_pairing_table* t, const void* g1, uint32_t checks, const void* status) {
    if (!t) return dh_fail(ctx, DEHALO_ERR_INVALID, "pairing_checks: null table");
    if (checks > DEHALO_PAIRING_MAX_CHECKS) return dh_fail(ctx, DEHALO_ERR_INVALID, "pairing_checks: too many checks in one call");
    if (checks && (!g1 || !status)) return dh_fail(ctx, DEHALO_ERR_INVALID, "pairing_checks: null argument");
    return 0;
}

static int pairing_launch(dehalo_ctx* ctx, const dehalo_pairing_table* t, const fe* d_g1, uint32_t checks, uint8_t* d_status, fe* d_gt, hipStream_t s) {
    const unsigned __int128 loop = (unsigned __int128)6 * BN254_X + 2;
    const uint32_t blocks = (checks + PAIRING_WAVES - 1) / PAIRING_WAVES;
    k_pairing_checks<<<blocks, PAIRING_BLOCK, 0, s>>>(t->lines.p, t->pairs, t->one_mask, t->consts.p, t->hard_bits, (uint64_t)loop, d_g1, checks, d_status, d_gt);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int dehalo_pairing_checks_device(dehalo_ctx* ctx, const dehalo_pairing_table* t, const uint64_t* d_g1_affine_xy, uint32_t checks, uint8_t* d_status,
                                            uint64_t* d_gt, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    TRY(pairing_checks_args(ctx, t, d_g1_affine_xy, checks, d_status));
    if (!t->ctx) return dh_fail(ctx, DEHALO_ERR_INVALID, "pairing_checks_device: a host table (made without a context)");
    if (t->ctx->device != ctx->device) return dh_fail(ctx, DEHALO_ERR_INVALID, "pairing_checks_device: the table lives on another device");
    if (checks == 0) return 0;
    return dh_device(ctx, stream, [&](hipStream_t s) -> int { return pairing_launch(ctx, t, (const fe*)d_g1_affine_xy, checks, d_status, (fe*)d_gt, s); });
}

extern "C" int dehalo_pairing_checks(const dehalo_pairing_table* t, const uint64_t* g1_affine_xy, uint32_t checks, uint8_t* status, uint64_t* gt) {
    dehalo_ctx* ctx = t ? t->ctx : nullptr;
    TRY(pairing_checks_args(ctx, t, g1_affine_xy, checks, status));
    if (checks == 0) return 0;
    if (!ctx) {
        return dh_guard(nullptr, [&]() -> int {
            pairing_host(t->curve)->table_checks(t->host, g1_affine_xy, checks, status, gt);
            return 0;
        });
    }
    return dh_device(ctx, nullptr, [&](hipStream_t s) -> int {
        const size_t points = (size_t)checks * t->pairs;
        DevMem g1, out;
        DevArray<uint8_t> st;
        TRY(g1.alloc(ctx, 2 * points, false));
        TRY(st.alloc(ctx, checks, false));
        if (gt) TRY(out.alloc(ctx, 12 * (size_t)checks, false));
        TRY(dehalo_upload(ctx, g1_affine_xy, 64 * points, g1.p));
        TRY(pairing_launch(ctx, t, g1.p, checks, st.p, out.p, s));
        TRY(dehalo_download(ctx, st.p, checks, status));
        if (gt) TRY(dehalo_download(ctx, out.p, 384 * (size_t)checks, gt));
        return 0;
    });
}
