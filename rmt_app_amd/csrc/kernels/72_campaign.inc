//>>> RMT_CAMPAIGN  (plan.Mechanism.source generates every unit but the campaign unit, n2.campaign_plan, WITHOUT the lines
//                   from here to the closing mark: their source and cache key are what they are without this file)
#if RMT_CAMPAIGN_POLICY && !RMT_CAMPAIGN
#error "RMT_CAMPAIGN_POLICY: only together with RMT_CAMPAIGN (the policy unit is the campaign unit plus this define)"
#endif
#if RMT_CAMPAIGN
// ===================================================================== time on stream: catalyst deactivation (batched)
// solver-config "deactivation" (host: rmt_app_amd/campaign.py).  Deactivation runs over hours to months, the bed's own
// transient over seconds: the bed is quasi-steady, a campaign is a sequence of steady states f(y; a(t)) = 0 with
//     da_n/dt = -k_d(T_n) (a_n - a_inf)^m,   k_d(T) = k_ref exp(-(Ed/R)(1/T - 1/Tref))
// between them.  One launch of rmt_n2_campaign_step is ONE march of the bed with the activities as they are (the loop of
// rmt_n2_steady_march, rmt_steady_node unchanged, every node started from its converged upstream state) that, at every
// node whose solve has converged, moves a_n over dt with the frozen-temperature exact solution of the law - in place, in
// the handle's own table [E][2][N].  dt = 0 leaves every a_n as it is bit for bit: the output at the last time is one
// more launch of the same kernel.
#if RMT_CAMPAIGN != 1
#error "RMT_CAMPAIGN: 1 (the campaign step of the steady-state march) or undefined"
#endif
#if !RMT_WITH_MARCH || !RMT_PROFILE
#error "RMT_CAMPAIGN: needs RMT_WITH_MARCH and RMT_PROFILE (the march on a profiled bed)"
#endif
#define RMT_CAMPAIGN_LAW 5                 // doubles per member: {k_ref [1/s], Ed [J/mol], Tref [K], m, a_inf}
#define RMT_CAMPAIGN_LOG (RMT_V + 6)       // doubles per member and step: outlet state [V], peak theta, its node, mean and
                                           // minimum activity (as read), worst scaled node residual, largest step count

// a(t + dt) of one node at the frozen temperature T [K]: with b = max(a - a_inf, 0)
//     m == 1:  b <- b exp(-k_d dt)                                  written  a + b expm1(-k_d dt)
//     else:    b <- b (1 + (m-1) k_d dt b^(m-1))^(-1/(m-1))         written  a - b (1 - (...)^(-1/(m-1)))
// The written forms return a itself when dt = 0 (expm1(-0) = -0, pow(1, .) = 1), a <= a_inf does not move, and the result
// stays in [a_inf, a].  Also compiled for the host.
__device__ __forceinline__ double rmt_campaign_update(const double a, const double T, const double* __restrict__ law,
                                                      const double dt) {
    const double b = a - law[4];
    if (!(b > 0.0)) return a;
    const double x = law[0] * rmt_exp(-(law[1] / 8.314472) * (1.0 / T - 1.0 / law[2])) * dt;
    const double q = law[3] - 1.0;
    if (q == 0.0) return a + b * rmt_expm1(-x);
    return a - b * (1.0 - rmt_pow(1.0 + q * x * rmt_pow(b, q), -1.0 / q));
}

#ifndef RMT_HOST_EMULATION
// kernel: rmt_n2_steady_march with the activity update fused in.  `tab` is the handle's profile table (the buffer
// rmt_profile_tab points to), read AND written here: lane e touches only its own rows tab[e][0][*] (a_n, updated in place
// behind the node's solve) and tab[e][1][*] (delta_n, read).  log[e][RMT_CAMPAIGN_LOG] describes the bed as it was marched,
// that is at the START of the step: the activities as read.  stats and the status bits are the march's.  A member whose
// node fails stops there, keeps its activities from that node on, and is flagged.
extern "C" __global__ __launch_bounds__(64) void rmt_n2_campaign_step(
        real* __restrict__ y /* [E][V][N] */, const double* __restrict__ members, const int N, const int E,
        const double tol, const long long max_iter, double* __restrict__ stats, unsigned* __restrict__ flags,
        double* __restrict__ tab /* [E][2][N] */, const double* __restrict__ laws /* [E][5] */, const double dt,
        double* __restrict__ log /* [E][V+6] */) {
    rmt_math_init();
    const int e = blockIdx.x * 64 + (int)threadIdx.x;
    const bool live = e < E;
    const int el = live ? e : 0;                  // dead lanes read member 0 and write nothing
    RmtMember m;
    rmt_load_member(members + (size_t)el * RMT_NM, m);
    double* __restrict__ te = tab + (size_t)el * 2 * (size_t)N;      // (m.prof stays unbound: nothing here reads through it)
    double law[RMT_CAMPAIGN_LAW];
#pragma unroll
    for (int i = 0; i < RMT_CAMPAIGN_LAW; ++i) law[i] = laws[(size_t)el * RMT_CAMPAIGN_LAW + i];
    real up[RMT_V], yz[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(m.cin[i], RMT_EPS);
#if !RMT_ISO
    up[RMT_S] = m.theta_in;
#endif
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) yz[i] = up[i];
    preal P = m.p0;
    rmt_flags_t flag;
    rmt_flags_clear(flag);
    real* ye = y + (size_t)el * RMT_V * N;
    double worst = 0.0, peak = (double)m.theta_in, asum = 0.0, amin = __builtin_inf();
    long long itmax = 0, ndamped = 0;
    int z = 0, failed = -1, peakz = 0;
    unsigned lf = 0u;
    bool active = live && N > 0;
    while (__any(active)) {
        if (active) {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) yz[i] = up[i];
            const double an = te[z];                      // (active: z < N)
            m.act = real(an);
            m.dtm = real(te[N + z]);
            const RmtSteadyNode nd = rmt_steady_node(m, up, P, yz, tol, max_iter, flag);
            itmax = nd.iters > itmax ? (long long)nd.iters : itmax;
            ndamped += nd.rejected > 0 ? 1 : 0;
            if (nd.fail) {
                lf |= nd.fail;
                failed = z;
                active = false;
            } else {
                worst = fmax(worst, nd.res);
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) ye[(size_t)i * N + z] = yz[i];
#if !RMT_ISO
                const double th = (double)yz[RMT_S];
#else
                const double th = (double)m.theta_in;
#endif
                te[z] = rmt_campaign_update(an, (double)m.tf * (1.0 + th), law, dt);
                if (z == 0 || th > peak) {
                    peak = th;
                    peakz = z;
                }
                asum += an;
                amin = fmin(amin, an);
#pragma unroll
                for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(yz[i], RMT_EPS);
#if !RMT_ISO
                up[RMT_S] = yz[RMT_S];
#endif
                P = rmt_pressure_next(m, nd.a, P);
                if (++z >= N) active = false;
            }
        }
    }
    if (live) {
        lf |= rmt_march_lane_bits(flag);
        double* __restrict__ le = log + (size_t)e * RMT_CAMPAIGN_LOG;
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) le[i] = (double)yz[i];            // (the last node solved: the outlet unless failed)
        le[RMT_V + 0] = peak;
        le[RMT_V + 1] = (double)peakz;
        le[RMT_V + 2] = z > 0 ? asum / (double)z : 0.0;
        le[RMT_V + 3] = amin;
        le[RMT_V + 4] = worst;
        le[RMT_V + 5] = (double)itmax;
        stats[(size_t)e * 4 + 0] = worst;
        stats[(size_t)e * 4 + 1] = (double)failed;
        ((long long*)stats)[(size_t)e * 4 + 2] = itmax;
        ((long long*)stats)[(size_t)e * 4 + 3] = ndamped;
        if (lf) atomicOr(&flags[e], lf);
    }
}
#endif  // RMT_HOST_EMULATION

#if RMT_CAMPAIGN_POLICY
// ===================================================================== constant-yield operation: the coolant policy
// solver-config "deactivation" "policy" (host: rmt_app_amd/campaign.py, DESIGN 3p').  Per member and step the common
// coolant level T (the member field tm; the zones of the table keep their offsets delta_n) is moved within [lo, hi] so that
//     r(T) = x_c,outlet(T) - target = 0,
// x_c the outlet mole fraction of component c.  Every value of r is a whole march of the bed with the activities as they
// stand.  The scheme (campaign.policy_emulate restates it in numpy):
//   1. march at lo and at hi (once when lo == hi);
//   2. r(lo) r(hi) < 0 does not hold: the limit with the smaller |r| is accepted (a tie: lo), the step is saturated;
//   3. else a march at the carried level (the previous step's accepted one) when it lies strictly inside shrinks the
//      bracket, then Illinois regula falsi on [a, b] until |r| <= tolerance;
//   4. b - a < RMT_POLICY_MIN_BRACKET with |r| > tolerance: RMT_FLAG_POLICY_BRACKET (the outlet jumps there: a node
//      changed branch); 5. max_evals marches without |r| <= tolerance: RMT_FLAG_POLICY_EVALS;
//   6. the accepted level is the last one marched (a saturated step that accepts lo marches it once more), so y and the log
//      row are those of the accepted level; 7. then a pass over the nodes moves a_n at T_n read back from y.
// The sign of dr/dT is taken from the bracket and not assumed; where the bracket holds several roots the one Illinois
// reaches from the limits is taken.
#if RMT_CAMPAIGN_POLICY != 1
#error "RMT_CAMPAIGN_POLICY: 1 (the coolant policy of the campaign step) or undefined"
#endif
#if RMT_ISO
#error "RMT_CAMPAIGN_POLICY: the manipulated coolant level needs a wall (not an iso-thermal unit)"
#endif
#define RMT_POLICY_ROW 4                   // doubles per member: {target, lo [K], hi [K], tolerance}
#define RMT_POLICY_LOG 4                   // doubles per member and step: {level [K], held x_c, marches, saturated -1 | 0 | +1
                                           // (a step that failed: 2 = the bracket collapsed, 3 = the evaluation limit)}
#define RMT_POLICY_MIN_BRACKET 1e-9        // K
#define RMT_FLAG_POLICY_BRACKET 64u        // the bracket fell below RMT_POLICY_MIN_BRACKET with |r| > tolerance
#define RMT_FLAG_POLICY_EVALS 128u         // max_evals marches in one step without |r| <= tolerance
// what the march in flight is for
#define RMT_POLICY_AT_LO 0
#define RMT_POLICY_AT_HI 1
#define RMT_POLICY_AT_CARRIED 2
#define RMT_POLICY_ILLINOIS 3
#define RMT_POLICY_AGAIN 4                 // the accepted level once more (it was not the last one marched)

#ifndef RMT_HOST_EMULATION
// kernel: rmt_n2_campaign_step with the root-find around the march, one reactor per lane.  ONE flat state machine around a
// single call of rmt_steady_node: in every trip of the wave loop each active lane solves one node of whatever march it is
// in; a lane that leaves the last node forms r, advances its own root-find state and starts its next march at node 0 (or
// ends).  Lanes in different marches share the node solver's instruction stream.  `tab` is read during the marches and
// written by the pass behind them, by lanes that accepted a level only: a member whose node solve fails in any march, whose
// bracket collapses or that reaches max_evals stops, keeps its activities and is flagged (stats[1]: the node, or -1).
// level[e]: the carried coolant level, read here and replaced by the accepted one.  log as rmt_n2_campaign_step (the
// accepted march), plog[e][RMT_POLICY_LOG] beside it.
extern "C" __global__ __launch_bounds__(64) void rmt_n2_campaign_policy_step(
        real* __restrict__ y /* [E][V][N] */, const double* __restrict__ members, const int N, const int E,
        const double tol, const long long max_iter, double* __restrict__ stats, unsigned* __restrict__ flags,
        double* __restrict__ tab /* [E][2][N] */, const double* __restrict__ laws /* [E][5] */, const double dt,
        double* __restrict__ log /* [E][V+6] */, const double* __restrict__ rows /* [E][4] */,
        double* __restrict__ level /* [E] */, double* __restrict__ plog /* [E][4] */, const int comp, const int max_evals) {
    rmt_math_init();
    const int e = blockIdx.x * 64 + (int)threadIdx.x;
    const bool live = e < E;
    const int el = live ? e : 0;                  // dead lanes read member 0 and write nothing
    RmtMember m;
    rmt_load_member(members + (size_t)el * RMT_NM, m);
    double* __restrict__ te = tab + (size_t)el * 2 * (size_t)N;
    const double target = rows[(size_t)el * RMT_POLICY_ROW + 0], lo = rows[(size_t)el * RMT_POLICY_ROW + 1],
                 hi = rows[(size_t)el * RMT_POLICY_ROW + 2], ptol = rows[(size_t)el * RMT_POLICY_ROW + 3];
    const double carried = level[el];
    // the root-find state of this lane: the bracket [a, b] with r at its ends, the level of the march in flight
    double a = lo, b = hi, ra = 0.0, rb = 0.0, T = lo, held = 0.0;
    int phase = RMT_POLICY_AT_LO, side = 0, nev = 0, sat = 0;
    m.tm = real(T);
    real up[RMT_V], yz[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(m.cin[i], RMT_EPS);
    up[RMT_S] = m.theta_in;
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) yz[i] = up[i];
    preal P = m.p0;
    rmt_flags_t flag;
    rmt_flags_clear(flag);
    real* ye = y + (size_t)el * RMT_V * N;
    double worst = 0.0, peak = (double)m.theta_in, asum = 0.0, amin = __builtin_inf();
    long long itmax = 0, ndamped = 0;
    int z = 0, failed = -1, peakz = 0;
    unsigned lf = 0u;
    bool active = live && N > 0, accepted = false;
    while (__any(active)) {
        if (active) {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) yz[i] = up[i];
            const double an = te[z];                      // (active: z < N)
            m.act = real(an);
            m.dtm = real(te[N + z]);
            const RmtSteadyNode nd = rmt_steady_node(m, up, P, yz, tol, max_iter, flag);
            itmax = nd.iters > itmax ? (long long)nd.iters : itmax;
            ndamped += nd.rejected > 0 ? 1 : 0;
            if (nd.fail) {
                lf |= nd.fail;
                failed = z;
                active = false;
            } else {
                worst = fmax(worst, nd.res);
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) ye[(size_t)i * N + z] = yz[i];
                const double th = (double)yz[RMT_S];
                if (z == 0 || th > peak) {
                    peak = th;
                    peakz = z;
                }
                asum += an;
                amin = fmin(amin, an);
#pragma unroll
                for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(yz[i], RMT_EPS);
                up[RMT_S] = yz[RMT_S];
                P = rmt_pressure_next(m, nd.a, P);
                if (++z >= N) {
                    // ---- this march is complete: r, then the lane's next move
                    double sum = 0.0, xc = 0.0;
#pragma unroll
                    for (int i = 0; i < RMT_S; ++i) {
                        sum += (double)yz[i];
                        xc = i == comp ? (double)yz[i] : xc;
                    }
                    held = xc / sum;
                    const double r = held - target;
                    ++nev;
                    bool again = false;           // true: another march, at T
                    if (phase == RMT_POLICY_AT_LO) {
                        ra = r;
                        if (lo == hi) {
                            sat = -1;
                            accepted = true;
                        } else {
                            T = hi;
                            phase = RMT_POLICY_AT_HI;
                            again = true;
                        }
                    } else if (phase == RMT_POLICY_AT_HI) {
                        rb = r;
                        if (!(ra * rb < 0.0)) {                       // no sign change: saturated at the better limit
                            if (fabs(rb) < fabs(ra)) {
                                sat = 1;
                                accepted = true;
                            } else {
                                sat = -1;
                                T = lo;
                                phase = RMT_POLICY_AGAIN;
                                again = true;
                            }
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
                    } else if (fabs(r) <= ptol) {                     // (at the carried level or inside Illinois)
                        sat = 0;
                        accepted = true;
                    } else {
                        if (r * rb > 0.0) {                           // r has the sign of r(b): T replaces b
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
                        if (b - a < RMT_POLICY_MIN_BRACKET) {
                            lf |= RMT_FLAG_POLICY_BRACKET;
                            sat = 2;
                        } else if (nev >= max_evals) {
                            lf |= RMT_FLAG_POLICY_EVALS;
                            sat = 3;
                        } else {
                            T = a - ra * (b - a) / (rb - ra);
                            if (!(T > a && T < b)) T = 0.5 * (a + b);
                            again = true;
                        }
                    }
                    if (again) {                                      // the next march of this lane starts at the inlet
                        m.tm = real(T);
                        z = 0;
#pragma unroll
                        for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(m.cin[i], RMT_EPS);
                        up[RMT_S] = m.theta_in;
                        P = m.p0;
                        worst = 0.0;
                        peak = (double)m.theta_in;
                        peakz = 0;
                        asum = 0.0;
                        amin = __builtin_inf();
                        itmax = 0;
                        ndamped = 0;
                    } else {
                        active = false;
                    }
                }
            }
        }
    }
    if (live) {
        if (accepted) {
            const double* __restrict__ law = laws + (size_t)e * RMT_CAMPAIGN_LAW;
            for (int n = 0; n < N; ++n)            // (T_n of the accepted march, as the lane stored it)
                te[n] = rmt_campaign_update(te[n], (double)m.tf * (1.0 + (double)ye[(size_t)RMT_S * N + n]), law, dt);
            level[e] = T;
        }
        lf |= rmt_march_lane_bits(flag);
        double* __restrict__ le = log + (size_t)e * RMT_CAMPAIGN_LOG;
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) le[i] = (double)yz[i];            // (the last node solved: the outlet unless failed)
        le[RMT_V + 0] = peak;
        le[RMT_V + 1] = (double)peakz;
        le[RMT_V + 2] = z > 0 ? asum / (double)z : 0.0;
        le[RMT_V + 3] = amin;
        le[RMT_V + 4] = worst;
        le[RMT_V + 5] = (double)itmax;
        double* __restrict__ pe = plog + (size_t)e * RMT_POLICY_LOG;
        pe[0] = T;
        pe[1] = held;
        pe[2] = (double)nev;
        pe[3] = (double)sat;
        stats[(size_t)e * 4 + 0] = worst;
        stats[(size_t)e * 4 + 1] = (double)failed;
        ((long long*)stats)[(size_t)e * 4 + 2] = itmax;
        ((long long*)stats)[(size_t)e * 4 + 3] = ndamped;
        if (lf) atomicOr(&flags[e], lf);
    }
}
#endif  // RMT_HOST_EMULATION
#endif  // RMT_CAMPAIGN_POLICY
#endif  // RMT_CAMPAIGN
//<<< RMT_CAMPAIGN
