// TEST HELPER: the node function of a PROFILED unit (RMT_PROFILE, csrc/kernels/12_profile.inc) compiled for the host from
// the generated source, walked node by node as oracle/hostemu_driver.cpp walks it - with the two profile fields of every
// node set from a table, the way the device callers do.  Reads records from stdin (numbers as hexadecimal or decimal
// floats), prints hexadecimal floats:
//   "M row_0 .. row_(RMT_NM-1)"       the member row of the records that follow
//   "T N a_0 .. a_(N-1) d_0 .. d_(N-1)"   the member's table: N catalyst activities, then N coolant offsets
//   "F y_0 .. y_(V*N-1)"              right-hand side at the state y[v][z]: prints "rhs" and V*N numbers
//   "J y_0 .. y_(V*N-1)"              (units with rmt_node_jac) per node the analytic -d f_z/d y_z and its forward
//                                     differences under the same table: prints "jan" and "jfd", N*V*V numbers each
//   "R tol max_iter"                  (march units) the steady-state march with the table: the output of
//                                     steady_march_emu.cpp's record R
#include "rmt_host_unit.h"

#if !RMT_PROFILE
#error "generate the source with RMT_PROFILE"
#endif

static bool read_state(std::vector<double>& y, int N) {
    y.assign((size_t)RMT_V * N, 0.0);
    for (size_t i = 0; i < y.size(); ++i)
        if (std::scanf("%lf", &y[i]) != 1) return false;
    return true;
}

static void inlet(const RmtMember& m, real* up) {
    for (int i = 0; i < RMT_S; ++i) up[i] = m.cin[i];
#if !RMT_ISO
    up[RMT_S] = m.theta_in;
#endif
}

static void next_up(const real* ys, real* up) {
    for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(ys[i], RMT_EPS);
#if !RMT_ISO
    up[RMT_S] = ys[RMT_S];
#endif
}

int main() {
    char what[4];
    double row[RMT_NM] = {0.0};
    RmtMember m;
    bool have = false;
    int N = 0;
    std::vector<double> act, dtm, y;
    while (std::scanf("%3s", what) == 1) {
        if (what[0] == 'M') {
            for (int i = 0; i < RMT_NM; ++i)
                if (std::scanf("%lf", &row[i]) != 1) return 2;
            rmt_load_member(row, m);
            have = true;
            continue;
        }
        if (what[0] == 'T') {
            if (std::scanf("%d", &N) != 1 || N < 1) return 2;
            act.assign(N, 1.0);
            dtm.assign(N, 0.0);
            for (int i = 0; i < N; ++i)
                if (std::scanf("%lf", &act[i]) != 1) return 2;
            for (int i = 0; i < N; ++i)
                if (std::scanf("%lf", &dtm[i]) != 1) return 2;
            continue;
        }
        if (!have || N < 1) return 4;
        rmt_flags_t flag;
        rmt_flags_clear(flag);
        if (what[0] == 'F') {
            if (!read_state(y, N)) return 2;
            std::vector<double> f((size_t)RMT_V * N, 0.0);
            preal P = m.p0;
            real up[RMT_V];
            inlet(m, up);
            for (int z = 0; z < N; ++z) {
                real ys[RMT_V], k[RMT_V];
                for (int i = 0; i < RMT_V; ++i) ys[i] = real(y[(size_t)i * N + z]);
                RmtNode nd;
                const preal a = rmt_node_pre(m, ys, nd);
                nd.act = real(act[z]);
                nd.dtm = real(dtm[z]);
                rmt_node_post(m, nd, ys, up, P, k, flag);
                for (int i = 0; i < RMT_V; ++i) f[(size_t)i * N + z] = (double)k[i];
                P = rmt_pressure_next(m, a, P);
                next_up(ys, up);
            }
            std::printf("rhs");
            for (size_t i = 0; i < f.size(); ++i) std::printf(" %a", f[i]);
            std::printf("\nflags %u\n", rmt_flags_bits(flag));
            continue;
        }
#if RMT_WITH_ROS4 || RMT_WITH_MARCH
        if (what[0] == 'J') {
            if (!read_state(y, N)) return 2;
            std::vector<double> jan((size_t)N * RMT_V * RMT_V), jfd((size_t)N * RMT_V * RMT_V);
            rmt_noflags_t nof;
            preal P = m.p0;
            real up[RMT_V];
            inlet(m, up);
            for (int z = 0; z < N; ++z) {
                real ys[RMT_V], k[RMT_V], kr[RMT_V];
                for (int i = 0; i < RMT_V; ++i) ys[i] = real(y[(size_t)i * N + z]);
                RmtNode nd;
                const preal a0 = rmt_node_pre(m, ys, nd);
                nd.act = real(act[z]);
                nd.dtm = real(dtm[z]);
                rmt_node_post(m, nd, ys, up, P, k, nof);
                real a[RMT_V][RMT_V], r[RMT_R];
                rmt_node_jac(m, nd, ys, P, a, r, nof);
                // (the rates rmt_node_jac hands over give the same node function: the stiff stepper's stage 1)
                rmt_node_post<rmt_noflags_t, true>(m, nd, ys, up, P, kr, nof, r);
                for (int i = 0; i < RMT_V; ++i)
                    if (std::fabs((double)(kr[i] - k[i])) > 1e-9 * (std::fabs((double)k[i]) + 1e-300) + 1e-13) return 5;
                for (int rr = 0; rr < RMT_V; ++rr)
                    for (int c = 0; c < RMT_V; ++c) jan[((size_t)z * RMT_V + rr) * RMT_V + c] = (double)a[rr][c];
                for (int c = 0; c < RMT_V; ++c) {
                    real yp[RMT_V], kp[RMT_V];
                    for (int i = 0; i < RMT_V; ++i) yp[i] = ys[i];
                    const real d = real(1.5e-8) * rmt_max(rmt_abs(ys[c]), real(1e-3));
                    yp[c] += d;
                    RmtNode ndp;
                    (void)rmt_node_pre(m, yp, ndp);
                    ndp.act = real(act[z]);
                    ndp.dtm = real(dtm[z]);
                    rmt_node_post(m, ndp, yp, up, P, kp, nof);
                    for (int rr = 0; rr < RMT_V; ++rr)
                        jfd[((size_t)z * RMT_V + rr) * RMT_V + c] = -(double)(kp[rr] - k[rr]) / (double)(yp[c] - ys[c]);
                }
                P = rmt_pressure_next(m, a0, P);
                next_up(ys, up);
            }
            std::printf("jan");
            for (size_t i = 0; i < jan.size(); ++i) std::printf(" %a", jan[i]);
            std::printf("\njfd");
            for (size_t i = 0; i < jfd.size(); ++i) std::printf(" %a", jfd[i]);
            std::printf("\n");
            continue;
        }
#endif
#if RMT_WITH_MARCH
        if (what[0] == 'R') {
            double tol;
            long long max_iter;
            if (std::scanf("%lf %lld", &tol, &max_iter) != 2) return 2;
            std::vector<double> Y((size_t)RMT_V * N, 0.0);
            real up[RMT_V], yz[RMT_V];
            for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(m.cin[i], RMT_EPS);
#if !RMT_ISO
            up[RMT_S] = m.theta_in;
#endif
            preal P = m.p0;
            double worst = 0.0;
            long long itmax = 0, ndamped = 0;
            unsigned fail = 0u;
            for (int z = 0; z < N; ++z) {
                for (int i = 0; i < RMT_V; ++i) yz[i] = up[i];
                m.act = real(act[z]);                  // the node this march is solving, as the kernel sets it
                m.dtm = real(dtm[z]);
                const RmtSteadyNode nd = rmt_steady_node(m, up, P, yz, tol, max_iter, flag);
                std::printf("node %d %u %d %d %d %a\n", z, nd.fail, nd.iters, nd.rejected, nd.nonfinite, nd.res);
                itmax = nd.iters > itmax ? nd.iters : itmax;
                ndamped += nd.rejected > 0 ? 1 : 0;
                if (nd.fail) { fail = nd.fail; break; }
                worst = std::fmax(worst, nd.res);
                for (int i = 0; i < RMT_V; ++i) Y[(size_t)i * N + z] = (double)yz[i];
                next_up(yz, up);
                P = rmt_pressure_next(m, nd.a, P);
            }
            std::printf("state");
            for (size_t i = 0; i < Y.size(); ++i) std::printf(" %a", Y[i]);
            std::printf("\nend %u %u %a %lld %lld\n", fail, rmt_flags_bits(flag), worst, itmax, ndamped);
            continue;
        }
#endif
        return 3;
    }
    return 0;
}
