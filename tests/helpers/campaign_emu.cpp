// TEST HELPER: the campaign loop of ONE reactor (solver-config "deactivation", csrc/kernels/72_campaign.inc) compiled for
// the host from the generated source of a campaign unit (RMT_CAMPAIGN): the node solver rmt_steady_node and the update
// rmt_campaign_update are the product's, the loop around them restates the kernel rmt_n2_campaign_step, which itself is
// device code.  Reads records from stdin (numbers as hexadecimal or decimal floats), prints hexadecimal floats:
//   "M row_0 .. row_(RMT_NM-1)"            the member row
//   "T N a_0 .. a_(N-1) d_0 .. d_(N-1)"    the fresh table: N catalyst activities, then N coolant offsets
//   "L k_ref Ed Tref m a_inf"              the law
//   "C tol max_iter K dt_0 .. dt_(K-1)"    K launches, launch k marches with the activities as they are and moves them
//                                          over dt_k; per launch it prints
//                                            "step k fail flags worst itmax peak peaknode mean min"
//                                            "iters i_0 .. i_(N-1)"      pseudo-time steps per node
//                                            "act a_0 .. a_(N-1)"        the activities the march READ
//                                            "state y_0 .. y_(V*N-1)"    y[v][z] row-major
//                                          and stops at the first launch that fails
//   "U a T dt"                             one call of rmt_campaign_update with the law: prints "upd value"
#include "rmt_host_unit.h"

#if !RMT_CAMPAIGN
#error "generate the source with RMT_CAMPAIGN"
#endif

int main() {
    char what[4];
    double row[RMT_NM] = {0.0}, law[RMT_CAMPAIGN_LAW] = {0.0};
    RmtMember m;
    bool have = false, have_law = false;
    int N = 0;
    std::vector<double> act, dtm;
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
        if (what[0] == 'L') {
            for (int i = 0; i < RMT_CAMPAIGN_LAW; ++i)
                if (std::scanf("%lf", &law[i]) != 1) return 2;
            have_law = true;
            continue;
        }
        if (!have_law) return 4;
        if (what[0] == 'U') {
            double a, T, dt;
            if (std::scanf("%lf %lf %lf", &a, &T, &dt) != 3) return 2;
            std::printf("upd %a\n", rmt_campaign_update(a, T, law, dt));
            continue;
        }
        if (what[0] != 'C') return 3;
        if (!have || N < 1) return 4;
        double tol;
        long long max_iter;
        int K;
        if (std::scanf("%lf %lld %d", &tol, &max_iter, &K) != 3 || K < 1) return 2;
        std::vector<double> dts(K);
        for (int k = 0; k < K; ++k)
            if (std::scanf("%lf", &dts[k]) != 1) return 2;
        for (int k = 0; k < K; ++k) {
            rmt_flags_t flag;
            rmt_flags_clear(flag);
            std::vector<double> Y((size_t)RMT_V * N, 0.0), read(act);
            std::vector<int> iters(N, 0);
            real up[RMT_V], yz[RMT_V];
            for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(m.cin[i], RMT_EPS);
#if !RMT_ISO
            up[RMT_S] = m.theta_in;
#endif
            preal P = m.p0;
            double worst = 0.0, peak = (double)m.theta_in, asum = 0.0, amin = INFINITY;
            long long itmax = 0;
            int peakz = 0, z = 0;
            unsigned fail = 0u;
            for (; z < N; ++z) {
                for (int i = 0; i < RMT_V; ++i) yz[i] = up[i];
                const double an = act[z];
                m.act = real(an);
                m.dtm = real(dtm[z]);
                const RmtSteadyNode nd = rmt_steady_node(m, up, P, yz, tol, max_iter, flag);
                iters[z] = nd.iters;
                itmax = nd.iters > itmax ? nd.iters : itmax;
                if (nd.fail) { fail = nd.fail; break; }
                worst = std::fmax(worst, nd.res);
                for (int i = 0; i < RMT_V; ++i) Y[(size_t)i * N + z] = (double)yz[i];
#if !RMT_ISO
                const double th = (double)yz[RMT_S];
#else
                const double th = (double)m.theta_in;
#endif
                act[z] = rmt_campaign_update(an, (double)m.tf * (1.0 + th), law, dts[k]);
                if (z == 0 || th > peak) { peak = th; peakz = z; }
                asum += an;
                amin = std::fmin(amin, an);
                for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(yz[i], RMT_EPS);
#if !RMT_ISO
                up[RMT_S] = yz[RMT_S];
#endif
                P = rmt_pressure_next(m, nd.a, P);
            }
            std::printf("step %d %u %u %a %lld %a %d %a %a\n", k, fail, rmt_flags_bits(flag), worst, itmax, peak, peakz,
                        z > 0 ? asum / z : 0.0, amin);
            std::printf("iters");
            for (int i = 0; i < N; ++i) std::printf(" %d", iters[i]);
            std::printf("\nact");
            for (int i = 0; i < N; ++i) std::printf(" %a", read[i]);
            std::printf("\nstate");
            for (size_t i = 0; i < Y.size(); ++i) std::printf(" %a", Y[i]);
            std::printf("\n");
            if (fail) break;
        }
    }
    return 0;
}
