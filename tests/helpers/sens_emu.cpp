// TEST HELPER: the per-node code of the sensitivity sweep (rmt_sens_eval / rmt_sens_factor / rmt_sens_solve,
// csrc/kernels/73_sensitivity.inc) compiled for the host from the generated source of a sensitivity unit (RMT_SENS), and
// the sweep of ONE reactor around it - the loop of the kernel rmt_n2_steady_sens, which itself is device code.
// Reads records from stdin (act, dtm: the node's catalyst activity and coolant offset, read but unused without RMT_PROFILE):
//   "M row_0 .. row_(RMT_NM-1)"           the member row of the records that follow
//   "A N a_0 .. a_(N-1) d_0 .. d_(N-1)"   the profile table of the R and S records that follow (RMT_PROFILE)
//   "F P act dtm y_0 .. y_(V-1) up_0 .. up_(V-1)"   the node function: prints "f f_0 .. f_(V-1) az-1 az": the Ergun
//                                         coefficient less one, RE-FORMED here as -alpha_k M/T from rmt_node_pre's own
//                                         M/T (nd.MoT) without the cancellation against 1 - the double az has lost those
//                                         digits, no precision of the subtraction brings them back - and az as
//                                         rmt_node_pre returns it, so that the caller can hold the two together
//   "J P act dtm y_0 .. y_(V-1)"          the analytic columns: prints "a" (V*V, row-major, a = -df/dy), "fP" (V), "ftm",
//                                         "fU" (NUU*V), "daz" (V), "az", and "ajac" (V*V): a as rmt_node_jac forms it
//                                         (rmt_sens_eval restates that function: the two must agree bit for bit)
//   "R N tol max_iter"                    the steady-state march (the loop of rmt_n2_steady_march): prints "state" V*N numbers
//   "S N kind_0 index_0 .. kind_(NP-1) index_(NP-1) y (V*N numbers, y[v][z])"
//                                         the sweep: prints "out" NP*(V+1)*N numbers ([p][v][z], row V = dP_z/dp) and
//                                         "end failed_node" (-1: none)
// Numbers are printed as hexadecimal floats.
#include "rmt_host_unit.h"

#if !RMT_SENS
#error "generate the source with RMT_SENS (n2.sens_plan)"
#endif

static bool read_reals(real* v, int n) {
    for (int i = 0; i < n; ++i) {
        double t;
        if (std::scanf("%lf", &t) != 1) return false;
        v[i] = real(t);
    }
    return true;
}

static void print_reals(const char* tag, const real* v, int n) {
    std::printf("%s", tag);
    for (int i = 0; i < n; ++i) std::printf(" %a", (double)v[i]);
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
        if (what[0] == 'F' || what[0] == 'J') {
            double P, act, dtm;
            real y[RMT_V], up[RMT_V];
            if (std::scanf("%lf %lf %lf", &P, &act, &dtm) != 3 || !read_reals(y, RMT_V)) return 2;
#if RMT_PROFILE
            m.act = real(act);
            m.dtm = real(dtm);
#endif
            if (what[0] == 'F') {
                if (!read_reals(up, RMT_V)) return 2;
                real f[RMT_V + 2], a[RMT_V][RMT_V];
                f[RMT_V + 1] = real(rmt_steady_eval(m, up, preal(P), y, f, a, flag));
                RmtNode nd;
                (void)rmt_node_pre(m, y, nd);
                f[RMT_V] = real(-(m.alpha_k * preal(nd.MoT)));
                print_reals("f", f, RMT_V + 2);
                continue;
            }
            RmtSensNode sn;
            rmt_sens_eval(m, y, preal(P), sn, flag);
            print_reals("a", &sn.ainv[0][0], RMT_V * RMT_V);
            print_reals("fP", sn.fP, RMT_V);
            print_reals("ftm", &sn.ftm, 1);
            print_reals("fU", &sn.fU[0][0], RMT_SENS_NUU * RMT_V);
            print_reals("daz", sn.daz, RMT_V);
            const real az = real(sn.az);
            print_reals("az", &az, 1);
            {
                real f[RMT_V], a[RMT_V][RMT_V], up[RMT_V];
                for (int i = 0; i < RMT_V; ++i) up[i] = y[i];
                (void)rmt_steady_eval(m, up, preal(P), y, f, a, flag);
                print_reals("ajac", &a[0][0], RMT_V * RMT_V);
            }
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
            print_reals("state", Y.data(), RMT_V * N);
            continue;
        }
        if (what[0] != 'S') return 3;
        int kind[RMT_SENS_NP], index[RMT_SENS_NP];
        for (int p = 0; p < RMT_SENS_NP; ++p)
            if (std::scanf("%d %d", &kind[p], &index[p]) != 2) return 2;
        std::vector<real> Y((size_t)RMT_V * N);
        if (!read_reals(Y.data(), RMT_V * N)) return 2;
        std::vector<real> out((size_t)RMT_SENS_NP * (RMT_V + 1) * N, real(0));
        real sd[RMT_SENS_NP][RMT_V];
        preal pi[RMT_SENS_NP];
        for (int p = 0; p < RMT_SENS_NP; ++p) rmt_sens_seed(m, kind[p], index[p], sd[p], pi[p]);
        preal P = m.p0;
        int failed = -1;
        for (int z = 0; z < N && failed < 0; ++z) {
            real yz[RMT_V];
            for (int i = 0; i < RMT_V; ++i) yz[i] = Y[(size_t)i * N + z];
            at_node(m, tab, N, z);
            RmtSensNode sn;
            bool ok = rmt_sens_factor(m, yz, P, sn, flag);
            for (int p = 0; p < RMT_SENS_NP; ++p) {
                real s[RMT_V];
                const preal piz = pi[p];
                ok = rmt_sens_solve(m, sn, yz, P, kind[p], index[p], sd[p], pi[p], s) && ok;
                real* op = out.data() + (size_t)p * (RMT_V + 1) * N + z;
                for (int i = 0; i < RMT_V; ++i) op[(size_t)i * N] = s[i];
                op[(size_t)RMT_V * N] = real(piz);
            }
            if (!ok) {
                for (int p = 0; p < RMT_SENS_NP; ++p)
                    for (int i = 0; i <= RMT_V; ++i) out[((size_t)p * (RMT_V + 1) + i) * N + z] = real(__builtin_nan(""));
                failed = z;
            } else {
                P = rmt_pressure_next(m, sn.az, P);
            }
        }
        print_reals("out", out.data(), (int)out.size());
        std::printf("end %d\n", failed);
    }
    return 0;
}
