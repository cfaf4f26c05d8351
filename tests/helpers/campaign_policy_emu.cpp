// TEST HELPER: the policy step of ONE reactor (solver-config "deactivation" "policy", csrc/kernels/72_campaign.inc under
// RMT_CAMPAIGN_POLICY) compiled for the host from the generated source of a policy unit: the node solver rmt_steady_node
// and the update rmt_campaign_update are the product's, the state machine around them restates the kernel
// rmt_n2_campaign_policy_step, which itself is device code.  Reads records from stdin (numbers as hexadecimal or decimal
// floats), prints hexadecimal floats:
//   "M row_0 .. row_(RMT_NM-1)"            the member row
//   "T N a_0 .. a_(N-1) d_0 .. d_(N-1)"    the fresh table: N catalyst activities, then N coolant offsets
//   "L k_ref Ed Tref m a_inf"              the law
//   "P target lo hi tol comp max_evals carried"   the policy row, the held component, the evaluation limit and the level
//                                                 step 0 carries in
//   "C tol max_iter K dt_0 .. dt_(K-1)"    K launches; per launch it prints
//                                            "step k fail flags worst itmax peak peaknode mean min"
//                                            "policy level held evaluations saturated"
//                                            "marches T_0 r_0 T_1 r_1 .."   every march of the step: its level and r
//                                            "act a_0 .. a_(N-1)"        the activities the marches READ
//                                            "state y_0 .. y_(V*N-1)"    y[v][z] row-major, the last march
//                                          and stops at the first launch that fails (fail: the node solver's bits, or 64 =
//                                          the bracket collapsed, 128 = the evaluation limit)
#include "rmt_host_unit.h"

#if !RMT_CAMPAIGN || !RMT_CAMPAIGN_POLICY
#error "generate the source with RMT_CAMPAIGN and RMT_CAMPAIGN_POLICY"
#endif

struct March {
    std::vector<double> Y;
    double worst = 0.0, peak = 0.0, asum = 0.0, amin = INFINITY, held = 0.0;
    long long itmax = 0;
    int peakz = 0, z = 0;
    unsigned fail = 0u;
};

// one march of the bed at the coolant level T with the activities as they are (the loop of rmt_n2_campaign_step without its
// update)
static March march(RmtMember& m, const double T, const std::vector<double>& act, const std::vector<double>& dtm, const int N,
                   const double tol, const long long max_iter, const int comp, rmt_flags_t& flag) {
    March o;
    o.Y.assign((size_t)RMT_V * N, 0.0);
    m.tm = real(T);
    real up[RMT_V], yz[RMT_V];
    for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(m.cin[i], RMT_EPS);
    up[RMT_S] = m.theta_in;
    for (int i = 0; i < RMT_V; ++i) yz[i] = up[i];
    preal P = m.p0;
    o.peak = (double)m.theta_in;
    for (; o.z < N; ++o.z) {
        const int z = o.z;
        for (int i = 0; i < RMT_V; ++i) yz[i] = up[i];
        const double an = act[z];
        m.act = real(an);
        m.dtm = real(dtm[z]);
        const RmtSteadyNode nd = rmt_steady_node(m, up, P, yz, tol, max_iter, flag);
        o.itmax = nd.iters > o.itmax ? nd.iters : o.itmax;
        if (nd.fail) { o.fail = nd.fail; break; }
        o.worst = std::fmax(o.worst, nd.res);
        for (int i = 0; i < RMT_V; ++i) o.Y[(size_t)i * N + z] = (double)yz[i];
        const double th = (double)yz[RMT_S];
        if (z == 0 || th > o.peak) { o.peak = th; o.peakz = z; }
        o.asum += an;
        o.amin = std::fmin(o.amin, an);
        for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(yz[i], RMT_EPS);
        up[RMT_S] = yz[RMT_S];
        P = rmt_pressure_next(m, nd.a, P);
    }
    double sum = 0.0;
    for (int i = 0; i < RMT_S; ++i) sum += (double)yz[i];
    o.held = (double)yz[comp] / sum;
    return o;
}

int main() {
    char what[4];
    double row[RMT_NM] = {0.0}, law[RMT_CAMPAIGN_LAW] = {0.0}, pol[RMT_POLICY_ROW] = {0.0}, carried = 0.0;
    RmtMember m;
    bool have = false, have_law = false, have_pol = false;
    int N = 0, comp = 0, max_evals = 0;
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
        if (what[0] == 'P') {
            for (int i = 0; i < RMT_POLICY_ROW; ++i)
                if (std::scanf("%lf", &pol[i]) != 1) return 2;
            if (std::scanf("%d %d %lf", &comp, &max_evals, &carried) != 3 || comp < 0 || comp >= RMT_S) return 2;
            have_pol = true;
            continue;
        }
        if (what[0] != 'C') return 3;
        if (!have || !have_law || !have_pol || N < 1) return 4;
        double tol;
        long long max_iter;
        int K;
        if (std::scanf("%lf %lld %d", &tol, &max_iter, &K) != 3 || K < 1) return 2;
        std::vector<double> dts(K);
        for (int k = 0; k < K; ++k)
            if (std::scanf("%lf", &dts[k]) != 1) return 2;
        const double target = pol[0], lo = pol[1], hi = pol[2], ptol = pol[3];
        for (int k = 0; k < K; ++k) {
            rmt_flags_t flag;
            rmt_flags_clear(flag);
            std::vector<double> trace;              // T_0 r_0 T_1 r_1 ..
            double a = lo, b = hi, ra = 0.0, rb = 0.0, T = lo;
            int phase = RMT_POLICY_AT_LO, side = 0, nev = 0, sat = 0;
            unsigned fail = 0u;
            bool accepted = false;
            March o;
            for (;;) {
                o = march(m, T, act, dtm, N, tol, max_iter, comp, flag);
                if (o.fail) { fail = o.fail; break; }
                const double r = o.held - target;
                trace.push_back(T);
                trace.push_back(r);
                ++nev;
                bool again = false;
                if (phase == RMT_POLICY_AT_LO) {
                    ra = r;
                    if (lo == hi) { sat = -1; accepted = true; }
                    else { T = hi; phase = RMT_POLICY_AT_HI; again = true; }
                } else if (phase == RMT_POLICY_AT_HI) {
                    rb = r;
                    if (!(ra * rb < 0.0)) {
                        if (std::fabs(rb) < std::fabs(ra)) { sat = 1; accepted = true; }
                        else { sat = -1; T = lo; phase = RMT_POLICY_AGAIN; again = true; }
                    } else if (carried > lo && carried < hi) {
                        T = carried;
                        phase = RMT_POLICY_AT_CARRIED;
                        again = true;
                    } else {
                        phase = RMT_POLICY_ILLINOIS;
                        T = a - ra * (b - a) / (rb - ra);
                        if (!(T > a && T < b)) T = 0.5 * (a + b);
                        again = true;
                    }
                } else if (phase == RMT_POLICY_AGAIN) {
                    accepted = true;
                } else if (std::fabs(r) <= ptol) {
                    sat = 0;
                    accepted = true;
                } else {
                    if (r * rb > 0.0) {
                        b = T;
                        rb = r;
                        if (phase == RMT_POLICY_ILLINOIS && side == 1) ra *= 0.5;
                        side = 1;
                    } else {
                        a = T;
                        ra = r;
                        if (phase == RMT_POLICY_ILLINOIS && side == -1) rb *= 0.5;
                        side = -1;
                    }
                    if (phase == RMT_POLICY_AT_CARRIED) side = 0;
                    phase = RMT_POLICY_ILLINOIS;
                    if (b - a < RMT_POLICY_MIN_BRACKET) { fail = RMT_FLAG_POLICY_BRACKET; sat = 2; }
                    else if (nev >= max_evals) { fail = RMT_FLAG_POLICY_EVALS; sat = 3; }
                    else {
                        T = a - ra * (b - a) / (rb - ra);
                        if (!(T > a && T < b)) T = 0.5 * (a + b);
                        again = true;
                    }
                }
                if (!again) break;
            }
            const std::vector<double> read(act);
            if (accepted) {
                for (int n = 0; n < N; ++n)
                    act[n] = rmt_campaign_update(act[n], (double)m.tf * (1.0 + o.Y[(size_t)RMT_S * N + n]), law, dts[k]);
                carried = T;
            }
            std::printf("step %d %u %u %a %lld %a %d %a %a\n", k, fail, rmt_flags_bits(flag), o.worst, o.itmax, o.peak, o.peakz,
                        o.z > 0 ? o.asum / o.z : 0.0, o.amin);
            std::printf("policy %a %a %d %d\n", T, o.held, nev, sat);
            std::printf("marches");
            for (size_t i = 0; i < trace.size(); ++i) std::printf(" %a", trace[i]);
            std::printf("\nact");
            for (int i = 0; i < N; ++i) std::printf(" %a", read[i]);
            std::printf("\nstate");
            for (size_t i = 0; i < o.Y.size(); ++i) std::printf(" %a", o.Y[i]);
            std::printf("\n");
            if (fail) break;
        }
    }
    return 0;
}
