#if RMT_WITH_MARCH
// ===================================================================== steady state of model N2 by marching (batched)
// solver-config "initial": "steady" (host: rmt_app_amd/initial.py).  The discretisation is first-order upwind without
// dispersion and the Ergun recurrence runs downstream, so the discrete steady state f(y*) = 0 is block lower-bidiagonal:
// node z sees its own state, the clamped state of node z-1 (or the inlet) and the pressure P_z, which follows from the
// nodes before it.  y* is found by marching from the inlet with one V x V nonlinear solve per node.
#if RMT_MODEL != 0 || RMT_FP32
#error "RMT_WITH_MARCH: model N2 in fp64 only"
#endif
// A pseudo-time step is rejected when the scaled residual grows by more than this factor.  The node's own transient is
// NOT monotone in the residual (fast equilibrium reactions, products that start at the clamp): with a factor of 2 node 0
// of the DME cases needs 370 - 390 steps, most of them at a step size the rejections keep small, and the nodes behind
// it 40 - 70; with two decades 17 - 28 and 9 - 13 (host emulation, 20 nodes).  The factor only stops a runaway.
#ifndef RMT_MARCH_REJECT_GROWTH
#define RMT_MARCH_REJECT_GROWTH 100.0
#endif
// This many consecutive updates within the tolerance, at steps no shorter than the residence time, end a node whose
// residual does not come down to the tolerance: it is at the noise of its own evaluation.  Fast equilibrium reactions put
// that noise (the cancellation of two large rates) at a scaled residual of 1e-10 .. 1.3e-10 in the DME cases, while the
// updates are 1e-16 .. 1e-15 of the state: Newton's iteration has nothing left to remove.
#ifndef RMT_MARCH_CALM_STEPS
#define RMT_MARCH_CALM_STEPS 3
#endif
#ifndef RMT_MARCH_FLOOR
#define RMT_MARCH_FLOOR 1e-6         // a variable smaller than this is scaled as if it had this size
#endif

struct RmtSteadyNode {
    preal a;            // Ergun coefficient of the converged state: P_{z+1} = a P_z + beta
    double res;         // scaled residual max_i |f_i| / (F1 inv_dz max(|y_i|, floor)) of the converged state
    int iters;          // pseudo-time steps taken, the rejected ones included
    int rejected;       // ... of them rejected (h <- h / 4)
    int nonfinite;      // ... of them with a non-finite trial state or residual
    unsigned fail;      // 0, or RMT_FLAG_STEP (max_iter reached) | RMT_FLAG_NONFINITE (the last trial was not finite / singular)
};

// f(y; up, P) of one node and a = -df/dy at frozen (up, P): ONE rate evaluation serves both (rmt_node_jac hands its rates to
// rmt_node_post).  Returns the node's Ergun coefficient.
template <typename FL>
__device__ __forceinline__ preal rmt_steady_eval(const RmtMember& m, const real* __restrict__ up, const preal P,
                                                 const real* __restrict__ y, real* __restrict__ f,
                                                 real (&a)[RMT_V][RMT_V], FL& fl) {
    RmtNode nd;
    const preal az = rmt_node_pre(m, y, nd);
#if RMT_PROFILE
    nd.act = m.act;                   // the node this lane is solving (the kernel below reads the table per node)
    nd.dtm = m.dtm;
#endif
    real r[RMT_R];
    rmt_node_jac(m, nd, y, P, a, r, fl);
    rmt_node_post<FL, true>(m, nd, y, up, P, f, fl, r);
    return az;
}

__device__ __forceinline__ double rmt_steady_scaled(const real* __restrict__ f, const real* __restrict__ y, const double iconv) {
    double w = 0.0;
    bool nan = false;
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) {
        const double s = fabs((double)f[i]) * iconv / fmax(fabs((double)y[i]), RMT_MARCH_FLOOR);
        nan |= !(s == s);
        w = fmax(w, s);
    }
    return nan ? __builtin_nan("") : w;       // (fmax drops a NaN operand)
}

// One node: pseudo-transient continuation on the node's own relaxation dy/dtau = f(y; up, P) - linearly implicit Euler
// steps (I/h - J) d = f from the upstream state, h_0 = the cell residence time 1/(F1 inv_dz).  A step is rejected
// (h <- h/4) when the new residual is not finite, a species goes negative, the pivot is not positive or the scaled
// residual grows by more than RMT_MARCH_REJECT_GROWTH; else h follows the residual ratio (switched evolution relaxation,
// growth at most 10 x), so the
// iteration turns into Newton's and ends quadratically.  Plain Newton from the upstream state does NOT work: at node 0 the
// products sit at the clamp RMT_EPS, where rmt_node_jac's act[j] is zero, and the iteration diverges within a few steps.
// Converged: scaled residual <= tol AND the last update |d_i| <= tol max(|y_i|, floor) - or RMT_MARCH_CALM_STEPS updates in
// a row within that bound at steps no shorter than the residence time.  On entry y = the start (the
// converged upstream state), on exit the converged state; `fl` receives the Python-exception tests of the converged
// iterate only.
template <typename FL>
__device__ __forceinline__ RmtSteadyNode rmt_steady_node(const RmtMember& m, const real* __restrict__ up, const preal P,
                                                         real* __restrict__ y, const double tol, const long long max_iter,
                                                         FL& fl) {
    RmtSteadyNode out;
    out.iters = out.rejected = out.nonfinite = 0;
    out.fail = 0u;
    const double conv = (double)(m.f1 * m.inv_dz), iconv = 1.0 / conv;
    double h = iconv;
    real f[RMT_V], a[RMT_V][RMT_V];
    FL cur;
    rmt_flags_clear(cur);
    out.a = rmt_steady_eval(m, up, P, y, f, a, cur);
    out.res = rmt_steady_scaled(f, y, iconv);
    if (!(out.res == out.res) || __builtin_isinf(out.res)) {      // the start itself is not finite: nothing to damp
        out.nonfinite = 1;
        out.fail = RMT_FLAG_NONFINITE;
        return out;
    }
    bool done = false, lastbad = false;
    int calm = 0;
    while (!done) {
        if ((long long)out.iters >= max_iter) {
            out.fail = RMT_FLAG_STEP | (lastbad ? RMT_FLAG_NONFINITE : 0u);
            break;
        }
        ++out.iters;
        const real ih = real(1.0 / h);
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) a[i][i] += ih;
        const real pv = rmt_invert_n<RMT_V>(a);
        real yn[RMT_V], d[RMT_V], fn[RMT_V];
        bool bad = !(pv > real(0)), neg = false;
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) {
            real acc = real(0);
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) acc += a[r][c] * f[c];
            d[r] = acc;
            yn[r] = y[r] + acc;
            bad |= !__builtin_isfinite((double)yn[r]);
            if (r < RMT_S) neg |= yn[r] < real(0);
        }
        FL trial;
        rmt_flags_clear(trial);
        preal an = preal(1);
        double resn = __builtin_nan("");
        if (!bad && !neg) {
            an = rmt_steady_eval(m, up, P, yn, fn, a, trial);
            resn = rmt_steady_scaled(fn, yn, iconv);
            bad = !(resn == resn) || __builtin_isinf(resn);
        }
        if (bad || neg || resn > RMT_MARCH_REJECT_GROWTH * out.res) {
            ++out.rejected;
            out.nonfinite += bad ? 1 : 0;
            lastbad = bad;
            h *= 0.25;
            FL again;               // the matrix was overwritten: f and a at y again (rare)
            rmt_flags_clear(again);
            (void)rmt_steady_eval(m, up, P, y, f, a, again);
            continue;
        }
        lastbad = false;
        bool small = true;
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) {
            small = small && fabs((double)d[i]) <= tol * fmax(fabs((double)yn[i]), RMT_MARCH_FLOOR);
            y[i] = yn[i];
            f[i] = fn[i];
        }
        calm = (small && h * conv >= 1.0) ? calm + 1 : 0;      // (a step cut below the residence time proves nothing by its size)
        // switched evolution relaxation: h follows the residual ratio, growth at most 10 x, a cut at most by half
        h *= (resn < out.res) ? fmin(10.0, out.res / resn) : fmax(0.5, out.res / resn);
        out.res = resn;
        out.a = an;
        cur = trial;
        done = (small && resn <= tol) || calm >= RMT_MARCH_CALM_STEPS;
    }
    if (done) rmt_flags_merge(fl, cur);
    return out;
}

#ifndef RMT_HOST_EMULATION
// the status bits of ONE lane (a lane is a reactor here; the workgroup is one wave, the masks of rmt_flags_t are its lanes)
__device__ __forceinline__ unsigned rmt_march_lane_bits(const rmt_flags_t& f) {
#if RMT_FLAGS_MODE == 0
    const unsigned lane = threadIdx.x & 63u;
    return (((f.dom >> lane) & 1ull) ? RMT_FLAG_DOMAIN : 0u) | (((f.div0 >> lane) & 1ull) ? RMT_FLAG_DIV0 : 0u) |
           (((f.ovf >> lane) & 1ull) ? RMT_FLAG_OVERFLOW : 0u);
#else
    return rmt_flags_bits(f);
#endif
}

// kernel: one reactor per lane (the shape of rmt_n1_ros4), the lane walks z = 0..N-1 carrying the clamped upstream state
// and the pressure in registers and writes y[e][v][z] as it goes (stride-N stores: this runs once per run).  Member rows
// come through rmt_load_member: a forced row (RMT_FORCING) is read at its reference time, its tail is not looked at.
// stats[e] = {worst scaled node residual, node that failed (-1: none), largest per-node step count, nodes that needed a
// rejected step}; a member that fails keeps what it had downstream of the failed node and gets RMT_FLAG_STEP /
// RMT_FLAG_NONFINITE.
extern "C" __global__ __launch_bounds__(64) void rmt_n2_steady_march(
        real* __restrict__ y /* [E][V][N] */, const double* __restrict__ members, const int N, const int E,
        const double tol, const long long max_iter, double* __restrict__ stats, unsigned* __restrict__ flags) {
    rmt_math_init();
    const int e = blockIdx.x * 64 + (int)threadIdx.x;
    const bool live = e < E;
    RmtMember m;
    rmt_load_member(members + (size_t)(live ? e : 0) * RMT_NM, m);      // dead lanes read member 0 and write nothing
    RMT_PROFILE_BIND(m, live ? e : 0, N)
    real up[RMT_V], yz[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(m.cin[i], RMT_EPS);
#if !RMT_ISO
    up[RMT_S] = m.theta_in;
#endif
    preal P = m.p0;
    rmt_flags_t flag;
    rmt_flags_clear(flag);
    real* ye = y + (size_t)(live ? e : 0) * RMT_V * N;
    double worst = 0.0;
    long long itmax = 0, ndamped = 0;
    int z = 0, failed = -1;
    unsigned lf = 0u;
    bool active = live && N > 0;
    while (__any(active)) {
        if (active) {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) yz[i] = up[i];
#if RMT_PROFILE
            m.act = real(m.prof[z]);                      // (active: z < N)
            m.dtm = real(m.prof[N + z]);
#endif
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
        stats[(size_t)e * 4 + 0] = worst;
        stats[(size_t)e * 4 + 1] = (double)failed;
        ((long long*)stats)[(size_t)e * 4 + 2] = itmax;
        ((long long*)stats)[(size_t)e * 4 + 3] = ndamped;
        if (lf) atomicOr(&flags[e], lf);
    }
}
#endif  // RMT_HOST_EMULATION
#endif  // RMT_WITH_MARCH
