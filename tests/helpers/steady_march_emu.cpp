// TEST HELPER: the node solver of the steady-state march (rmt_steady_node, csrc/kernels/71_steady_march.inc) compiled for
// the host from the generated source of a march unit (RMT_WITH_MARCH), and the march of ONE reactor around it - the loop
// of the kernel rmt_n2_steady_march, which itself is device code.
// Reads records from stdin:
//   "M row_0 .. row_(RMT_NM-1)"     the member row of the records that follow
//   "R N tol max_iter"              march N nodes from the inlet; prints per node
//                                   "node z fail iters rejected nonfinite res" and then "state" followed by the V*N
//                                   numbers of y[v][z] (row-major) and "end fail flags worst itmax ndamped"
//   "Z P tol max_iter up_0 .. up_(V-1)"   ONE node started from its upstream state; prints
//                                   "node 0 fail iters rejected nonfinite res" and "state y_0 .. y_(V-1)"
// Numbers are printed as hexadecimal floats.
#include "rmt_host_unit.h"

#if !RMT_WITH_MARCH
#error "generate the source with RMT_WITH_MARCH"
#endif

static void print_node(int z, const RmtSteadyNode& nd) {
    std::printf("node %d %u %d %d %d %a\n", z, nd.fail, nd.iters, nd.rejected, nd.nonfinite, nd.res);
}

int main() {
    char what[4];
    double row[RMT_NM] = {0.0};
    RmtMember m;
    bool have = false;
    while (std::scanf("%3s", what) == 1) {
        if (what[0] == 'M') {
            for (int i = 0; i < RMT_NM; ++i)
                if (std::scanf("%lf", &row[i]) != 1) return 2;
            rmt_load_member(row, m);
            have = true;
            continue;
        }
        if (!have) return 4;
        rmt_flags_t flag;
        rmt_flags_clear(flag);
        if (what[0] == 'Z') {
            double P, tol;
            long long max_iter;
            real up[RMT_V], y[RMT_V];
            if (std::scanf("%lf %lf %lld", &P, &tol, &max_iter) != 3) return 2;
            for (int i = 0; i < RMT_V; ++i) {
                double t;
                if (std::scanf("%lf", &t) != 1) return 2;
                up[i] = y[i] = real(t);
            }
            const RmtSteadyNode nd = rmt_steady_node(m, up, preal(P), y, tol, max_iter, flag);
            print_node(0, nd);
            std::printf("state");
            for (int i = 0; i < RMT_V; ++i) std::printf(" %a", (double)y[i]);
            std::printf("\n");
            continue;
        }
        if (what[0] != 'R') return 3;
        int N;
        double tol;
        long long max_iter;
        if (std::scanf("%d %lf %lld", &N, &tol, &max_iter) != 3 || N < 1) return 2;
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
            const RmtSteadyNode nd = rmt_steady_node(m, up, P, yz, tol, max_iter, flag);
            print_node(z, nd);
            itmax = nd.iters > itmax ? nd.iters : itmax;
            ndamped += nd.rejected > 0 ? 1 : 0;
            if (nd.fail) { fail = nd.fail; break; }
            worst = std::fmax(worst, nd.res);
            for (int i = 0; i < RMT_V; ++i) Y[(size_t)i * N + z] = (double)yz[i];
            for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(yz[i], RMT_EPS);
#if !RMT_ISO
            up[RMT_S] = yz[RMT_S];
#endif
            P = rmt_pressure_next(m, nd.a, P);
        }
        std::printf("state");
        for (size_t i = 0; i < Y.size(); ++i) std::printf(" %a", Y[i]);
        std::printf("\nend %u %u %a %lld %lld\n", fail, rmt_flags_bits(flag), worst, itmax, ndamped);
    }
    return 0;
}
