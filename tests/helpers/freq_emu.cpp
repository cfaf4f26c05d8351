// TEST HELPER: the per-node code of the frequency sweep (rmt_sens_eval and rmt_freq_node, csrc/kernels/73_sensitivity.inc and
// 74_frequency.inc) compiled for the host from the generated source of a frequency unit (RMT_FREQ), and the sweep of ONE
// reactor at a list of frequencies around it - the loop of the kernel rmt_n2_steady_freq, which itself is device code.
// Reads records from stdin:
//   "M row_0 .. row_(RMT_NM-1)"           the member row of the records that follow
//   "A N a_0 .. a_(N-1) d_0 .. d_(N-1)"   the profile table of the R and W records that follow (RMT_PROFILE)
//   "J P act dtm y_0 .. y_(V-1)"          the node's blocks as rmt_sens_eval forms them: prints "a" (V*V, row-major,
//                                         a = -df/dy), "fP" (V), "ftm", "daz" (V), "az"
//   "R N tol max_iter"                    the steady-state march (the loop of rmt_n2_steady_march): prints "state" V*N numbers
//   "W N F w_0 .. w_(F-1) kind_0 index_0 .. kind_(NP-1) index_(NP-1) y (V*N numbers, y[v][z])"
//                                         the sweep: prints "out" F*NP*(V+1)*N*2 numbers ([f][p][v][z][re, im], row V =
//                                         dP_z) and "end" F numbers: the node the sweep of that frequency stopped at (-1: none)
// Numbers are printed as hexadecimal floats.
#include "rmt_host_unit.h"

#if !RMT_FREQ
#error "generate the source with RMT_FREQ (n2.freq_plan)"
#endif

static bool read_reals(real* v, int n) {
    for (int i = 0; i < n; ++i) {
        double t;
        if (std::scanf("%lf", &t) != 1) return false;
        v[i] = real(t);
    }
    return true;
}

static void print_reals(const char* tag, const real* v, size_t n) {
    std::printf("%s", tag);
    for (size_t i = 0; i < n; ++i) std::printf(" %a", (double)v[i]);
    std::printf("\n");
}

static void at_node(RmtMember& m, const std::vector<double>& tab, int N, int z) {
#if RMT_PROFILE
    m.act = real(tab.empty() ? 1.0 : tab[(size_t)z]);
    m.dtm = real(tab.empty() ? 0.0 : tab[(size_t)N + z]);
#else
    (void)m; (void)tab; (void)N; (void)z;
#endif
}

int main() {
    char what[4];
    double row[RMT_NM] = {0.0};
    RmtMember m;
    std::vector<double> tab;
    int tabN = 0;
    bool have = false;
    while (std::scanf("%3s", what) == 1) {
        if (what[0] == 'M') {
            for (int i = 0; i < RMT_NM; ++i)
                if (std::scanf("%lf", &row[i]) != 1) return 2;
            rmt_load_member(row, m);
            have = true;
            continue;
        }
        if (what[0] == 'A') {
            if (std::scanf("%d", &tabN) != 1 || tabN < 1) return 2;
            tab.assign((size_t)2 * tabN, 0.0);
            for (size_t i = 0; i < tab.size(); ++i)
                if (std::scanf("%lf", &tab[i]) != 1) return 2;
            continue;
        }
        if (!have) return 4;
        rmt_flags_t flag;
        rmt_flags_clear(flag);
        if (what[0] == 'J') {
            double P, act, dtm;
            real y[RMT_V];
            if (std::scanf("%lf %lf %lf", &P, &act, &dtm) != 3 || !read_reals(y, RMT_V)) return 2;
#if RMT_PROFILE
            m.act = real(act);
            m.dtm = real(dtm);
#endif
            RmtSensNode sn;
            rmt_sens_eval(m, y, preal(P), sn, flag);
            print_reals("a", &sn.ainv[0][0], RMT_V * RMT_V);
            print_reals("fP", sn.fP, RMT_V);
            print_reals("ftm", &sn.ftm, 1);
            print_reals("daz", sn.daz, RMT_V);
            const real az = real(sn.az);
            print_reals("az", &az, 1);
            continue;
        }
        int N;
        if (std::scanf("%d", &N) != 1 || N < 1) return 2;
        if (!tab.empty() && tabN != N) return 5;
        if (what[0] == 'R') {
            double tol;
            long long max_iter;
            if (std::scanf("%lf %lld", &tol, &max_iter) != 2) return 2;
            std::vector<real> Y((size_t)RMT_V * N, real(0));
            real up[RMT_V], yz[RMT_V];
            for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(m.cin[i], RMT_EPS);
#if !RMT_ISO
            up[RMT_S] = m.theta_in;
#endif
            preal P = m.p0;
            for (int z = 0; z < N; ++z) {
                for (int i = 0; i < RMT_V; ++i) yz[i] = up[i];
                at_node(m, tab, N, z);
                const RmtSteadyNode nd = rmt_steady_node(m, up, P, yz, tol, max_iter, flag);
                if (nd.fail) return 6;
                for (int i = 0; i < RMT_V; ++i) Y[(size_t)i * N + z] = yz[i];
                for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(yz[i], RMT_EPS);
#if !RMT_ISO
                up[RMT_S] = yz[RMT_S];
#endif
                P = rmt_pressure_next(m, nd.a, P);
            }
            print_reals("state", Y.data(), (size_t)RMT_V * N);
            continue;
        }
        if (what[0] != 'W') return 3;
        int F;
        if (std::scanf("%d", &F) != 1 || F < 1) return 2;
        std::vector<double> omegas((size_t)F);
        for (int f = 0; f < F; ++f)
            if (std::scanf("%lf", &omegas[(size_t)f]) != 1) return 2;
        RmtSensDesc desc;
        std::memset(&desc, 0, sizeof(desc));
        for (int p = 0; p < RMT_FREQ_NP; ++p)
            if (std::scanf("%d %d", &desc.kind[p], &desc.index[p]) != 2) return 2;
        std::vector<real> Y((size_t)RMT_V * N);
        if (!read_reals(Y.data(), RMT_V * N)) return 2;
        const size_t per = (size_t)RMT_FREQ_NP * (RMT_V + 1) * N * 2;
        std::vector<real> out((size_t)F * per, real(0));
        std::vector<real> failed((size_t)F, real(-1));
        for (int f = 0; f < F; ++f) {
            real* of = out.data() + (size_t)f * per;
            real sdr[RMT_FREQ_NP][RMT_V], sdi[RMT_FREQ_NP][RMT_V];
            preal pir[RMT_FREQ_NP], pii[RMT_FREQ_NP];
            for (int p = 0; p < RMT_FREQ_NP; ++p) {
                rmt_sens_seed(m, desc.kind[p], desc.index[p], sdr[p], pir[p]);
                pii[p] = preal(0);
                for (int i = 0; i < RMT_V; ++i) sdi[p][i] = real(0);
            }
            preal P = m.p0;
            for (int z = 0; z < N; ++z) {
                real yz[RMT_V];
                for (int i = 0; i < RMT_V; ++i) yz[i] = Y[(size_t)i * N + z];
                at_node(m, tab, N, z);
                RmtSensNode sn;
                rmt_sens_eval(m, yz, P, sn, flag);
                preal pzr[RMT_FREQ_NP], pzi[RMT_FREQ_NP];
                for (int p = 0; p < RMT_FREQ_NP; ++p) {
                    pzr[p] = pir[p];
                    pzi[p] = pii[p];
                }
                real sr[RMT_FREQ_NP][RMT_V], si[RMT_FREQ_NP][RMT_V];
                const bool ok = rmt_freq_node(m, sn, yz, P, real(omegas[(size_t)f]), desc, sdr, sdi, pir, pii, sr, si);
                for (int p = 0; p < RMT_FREQ_NP; ++p)
                    for (int i = 0; i <= RMT_V; ++i) {
                        real* o = of + (((size_t)p * (RMT_V + 1) + i) * N + z) * 2;
                        o[0] = !ok ? real(__builtin_nan("")) : (i < RMT_V ? sr[p][i < RMT_V ? i : 0] : real(pzr[p]));
                        o[1] = !ok ? real(__builtin_nan("")) : (i < RMT_V ? si[p][i < RMT_V ? i : 0] : real(pzi[p]));
                    }
                if (!ok) {
                    failed[(size_t)f] = real(z);
                    break;
                }
                P = rmt_pressure_next(m, sn.az, P);
            }
        }
        print_reals("out", out.data(), out.size());
        print_reals("end", failed.data(), failed.size());
    }
    return 0;
}
