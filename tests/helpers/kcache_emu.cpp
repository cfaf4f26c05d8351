// TEST HELPER: the generated rate function of a caching unit (rmt_kinetics or rmt_kinetics_node, -DKIN_FN=...,
// -DKIN_EXTRA=2 with the gain's denominator, 3 with rscale in front of it) and the node function around it, compiled for the host with a cache type
// whose `enabled` is true - the cached section and the callers' cache-only paths, which the host emulation discards.
// Reads records from stdin:
//   "M row_0 .. row_(RMT_NM-1)"         the member row of the N records that follow
//   "K T_ref T P x_0 .. x_(S-1)"        the rate function: a full evaluation (MODE 0) at T_ref moves the reference point,
//                                       then the cached one (MODE 2) at T and a full one at T into a second cache; prints
//                                       "valid flags r2_0 .. r2_(R-1) r0_0 .. r0_(R-1) ginv2 ginv0"
//   "N P up_0 .. up_(V-1) yref_0 .. yref_(V-1) y_0 .. y_(V-1)"
//                                       the node function rmt_node_pre / rmt_node_post: without a cache at y, with a
//                                       cache in full at yref and from the cache at y, with a second cache in full at y;
//                                       prints "valid flags kplain_0 .. kfull_0 .. kcached_0 .."
// Numbers are printed as hexadecimal floats.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#define RMT_HOST_EMULATION 1
#define __device__
#define __forceinline__ inline
#define __restrict__
#ifndef INFINITY
#define INFINITY __builtin_inf()
#endif
using std::trunc;
#include RMT_GENERATED_SOURCE

struct HostKC {
    static constexpr bool enabled = true;
    real s[RMT_KC_SLOTS > 0 ? RMT_KC_SLOTS : 1];
    bool valid;
    real get(const int k) const { return s[k]; }
    void put(const int k, const real v) { s[k] = v; }
    void leave(const bool out) { valid = valid && !out; }
};

#ifndef KIN_EXTRA
#define KIN_EXTRA 0
#endif

static bool read_n(real* v, int n) {
    for (int i = 0; i < n; ++i) {
        double t;
        if (std::scanf("%lf", &t) != 1) return false;
        v[i] = real(t);
    }
    return true;
}

int main() {
    char what[4];
    double row[RMT_NM] = {0.0};
    RmtMember m;
    while (std::scanf("%3s", what) == 1) {
        rmt_flags_t f;
        rmt_flags_clear(f);
        HostKC kc, kc0;
        kc.valid = kc0.valid = true;
        if (what[0] == 'M') {
            for (int i = 0; i < RMT_NM; ++i)
                if (std::scanf("%lf", &row[i]) != 1) return 2;
            rmt_load_member(row, m);
            continue;
        }
#if RMT_MODEL == 0
        if (what[0] == 'N') {
            real P[1], up[RMT_V], yr[RMT_V], y[RMT_V], kp[RMT_V], kf[RMT_V], kc2[RMT_V], kt[RMT_V];
            if (!read_n(P, 1) || !read_n(up, RMT_V) || !read_n(yr, RMT_V) || !read_n(y, RMT_V)) return 2;
            RmtNode nd, ndr;
            (void)rmt_node_pre(m, y, nd);
            (void)rmt_node_pre(m, yr, ndr);
            rmt_node_post(m, nd, y, up, preal(P[0]), kp, f);
            rmt_node_post<rmt_flags_t, false, HostKC, 0>(m, ndr, yr, up, preal(P[0]), kt, f, nullptr, &kc);
            rmt_node_post<rmt_flags_t, false, HostKC, 2>(m, nd, y, up, preal(P[0]), kc2, f, nullptr, &kc);
            rmt_node_post<rmt_flags_t, false, HostKC, 0>(m, nd, y, up, preal(P[0]), kf, f, nullptr, &kc0);
            std::printf("%d %u", kc.valid ? 1 : 0, rmt_flags_bits(f));
            for (int i = 0; i < RMT_V; ++i) std::printf(" %a", (double)kp[i]);
            for (int i = 0; i < RMT_V; ++i) std::printf(" %a", (double)kf[i]);
            for (int i = 0; i < RMT_V; ++i) std::printf(" %a", (double)kc2[i]);
            std::printf("\n");
            continue;
        }
#endif
        if (what[0] != 'K') return 3;
        real tp[3];
        if (!read_n(tp, 3)) return 2;
        const real tref = tp[0], T = tp[1], P = tp[2];
        real x[RMT_S], C[RMT_S], U[1] = {real(0)}, r0[RMT_R], r2[RMT_R], rr[RMT_R];
        if (!read_n(x, RMT_S)) return 2;
        for (int i = 0; i < RMT_S; ++i) C[i] = real(0);
        real g2 = real(0), g0 = real(0), gr = real(0);
        const real gden = real(1234.5);
        (void)gden; (void)gr;
#if KIN_EXTRA == 3      // rscale (the member row's FM) and the gain's denominator
        KIN_FN<rmt_flags_t, HostKC, 0>(tref, real(1) / tref, P, x, C, U, rr, f, kc, m.inv_macote, gden, gr);
        KIN_FN<rmt_flags_t, HostKC, 2>(T, real(1) / T, P, x, C, U, r2, f, kc, m.inv_macote, gden, g2);
        KIN_FN<rmt_flags_t, HostKC, 0>(T, real(1) / T, P, x, C, U, r0, f, kc0, m.inv_macote, gden, g0);
#elif KIN_EXTRA == 2    // the gain's denominator only
        KIN_FN<rmt_flags_t, HostKC, 0>(tref, real(1) / tref, P, x, C, U, rr, f, kc, gden, gr);
        KIN_FN<rmt_flags_t, HostKC, 2>(T, real(1) / T, P, x, C, U, r2, f, kc, gden, g2);
        KIN_FN<rmt_flags_t, HostKC, 0>(T, real(1) / T, P, x, C, U, r0, f, kc0, gden, g0);
#else
        KIN_FN<rmt_flags_t, HostKC, 0>(tref, real(1) / tref, P, x, C, U, rr, f, kc);
        KIN_FN<rmt_flags_t, HostKC, 2>(T, real(1) / T, P, x, C, U, r2, f, kc);
        KIN_FN<rmt_flags_t, HostKC, 0>(T, real(1) / T, P, x, C, U, r0, f, kc0);
#endif
        std::printf("%d %u", kc.valid ? 1 : 0, rmt_flags_bits(f));
        for (int q = 0; q < RMT_R; ++q) std::printf(" %a", (double)r2[q]);
        for (int q = 0; q < RMT_R; ++q) std::printf(" %a", (double)r0[q]);
        std::printf(" %a %a\n", (double)g2, (double)g0);
    }
    return 0;
}
