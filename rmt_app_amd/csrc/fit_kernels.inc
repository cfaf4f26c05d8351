// Kinetic parameter estimation from steady-state data (solver-config "fit", rmt_app_amd/fit.py): the reduction over the
// experiments and one Levenberg-Marquardt step, between the sensitivity sweep of one iteration and the march of the next,
// without the host.  Mechanism-independent and a translation unit of its own (NOT part of the stepper template
// kernels/*.inc): compiled once with hipRTC (rmt_n2_fit_source -> rmt_n2_compile, WITH -ffp-contract=off: every operation
// is one correctly rounded fp64 operation, so numpy reproduces the kernels - fit.emulate_residuals, fit.emulate_update)
// and loaded by rmt_n2_fit_create.  rmt_n2_fit_step enqueues the two kernels below back to back.
//
// rmt_n2_fit_residuals_f64: one wave per experiment, experiments walked grid-stride.  Lane q < MQ evaluates entry q of the
//   experiment's measurement table {code, value, weight}: the prediction, the weighted residual r_q = (pred - value) w and
//   its row of the Jacobian J_q[p] = d pred / d p_p w from the sensitivity buffer (the arithmetic of
//   sensitivity.result_entry: mole fractions of the clamped outlet state, zero derivative at the clamp; the peak temperature
//   at the node of the discrete maximum, ties to the lowest node, a NaN never wins).  Lane j < 45 then adds up entry j of
//   contrib = {C = 1/2 sum r^2, g = J^T r [8], upper triangle of J^T J [36]} over q in index order; entry 45 = failed.
// rmt_n2_fit_update_f64: ONE workgroup of one wave.  Lane j < 46 sums column j of contrib over the experiments in index
//   order (no atomics: the sums do not depend on the geometry of the first kernel), lane 0 evaluates the LM law in fp64
//   (small matrices in LDS, nothing in scratch) and writes the state and the log slice, all lanes write the trial values
//   into the fitted user columns of every member's device row.
// rmt_n2_fit_residuals_ex_f64, rmt_n2_fit_update_ex_f64 (rmt_n2_fit_step_ex): the same two bodies (template<bool EX>) with
//   measurements along the bed - code S+2 the temperature, S+3+i the mole fraction of species i at the entry's record
//   {n0, f} of the position table: (1-f) q(n0) + f q(n0+1), the Jacobian row likewise - log-scaled parameters (theta = ln p:
//   column j of J times the member's own value of the constant) and bounds (active set, projected step: see the update).
// No atomics, no scratch; every store is an ordinary vector store.
#define RMT_FIT_BLOCK 256
#define RMT_FIT_MAXP 8
#define RMT_FIT_TRI 36            // upper triangle of an 8 x 8 matrix, row by row
#define RMT_FIT_CONTRIB 46        // C, g[8], H[36], failed
#define RMT_FIT_STATE 80          // see below
#define RMT_FIT_LOG 68            // C_trial, C_cur, lambda, nu, accepted, converged, failed, status, p_trial[8], p_cur[8], g[8], H[36]
#define RMT_FIT_EPS 1e-30         // the clamp of the concentrations (RMT_EPS of the template)
#define RMT_FIT_FLOOR 1e-300
// state: 0 started, 1 C_cur, 2 lambda, 3 nu, 4 converged, 5 passes, 6 status, 7 predicted reduction of the trial,
//        8 p_cur[8], 16 p_trial[8], 24 g_cur[8], 32 H_cur[36], 68 delta[8], 76..79 reserved
#define RMT_FIT_ST_PCUR 8
#define RMT_FIT_ST_PTRIAL 16
#define RMT_FIT_ST_G 24
#define RMT_FIT_ST_H 32
#define RMT_FIT_ST_DELTA 68
// the extended update: state words 76, 77 and log words 68, 69 = the parameters of the current point on their lower / upper
// bound, one bit each
#define RMT_FIT_LOG_EX 70
#define RMT_FIT_ST_LOWER 76
#define RMT_FIT_ST_UPPER 77
// status bits
#define RMT_FIT_FIRST_FAILED 1    // the first pass had a failed experiment (or a cost that is not finite)
#define RMT_FIT_NOT_POSITIVE 2    // H + lambda D had a non-positive pivot after 8 increases of lambda
// member row (kernels/00_config_math.inc)
#define RMT_FIT_M_CMAX 0
#define RMT_FIT_M_TF 1
#define RMT_FIT_M_USER 16         // + S: the first user column

// index of (a, b), a <= b, in the upper triangle
__device__ __forceinline__ int rmt_fit_tri(int a, int b) { return a*RMT_FIT_MAXP - a*(a - 1)/2 + (b - a); }

// largest element of p[0..N) and its lowest index, for the 64 lanes of one wave (every lane returns both); the wave
// reduction of rmt_ctl_row_max (control_kernels.inc) with the index carried along: plain >, so a NaN never wins, and
// among equal values the lower node; node 0 when no element compares greater than -inf
__device__ __forceinline__ double rmt_fit_row_max(const double* __restrict__ p, int N, int lane, int& at) {
    double vmax = -__builtin_huge_val();
    int imax = 0;
    for (int j = lane; j < N; j += 64) {
        const double x = p[j];
        if (x > vmax) { vmax = x; imax = j; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double o = __shfl_xor(vmax, m, 64);
        const int oi = __shfl_xor(imax, m, 64);
        if (o > vmax || (o == vmax && oi < imax)) { vmax = o; imax = oi; }
    }
    at = imax;
    return vmax;
}

__device__ __forceinline__ bool rmt_fit_finite(double x) { return x - x == 0.0; }

// the user columns of the fitted constants and their scale (1: log), by value
struct RmtFitCols { int col[RMT_FIT_MAXP]; };
struct RmtFitScale { int col[RMT_FIT_MAXP]; int log[RMT_FIT_MAXP]; };

// total concentration and the concentration of species `code` of the clamped state of node n
__device__ __forceinline__ void rmt_fit_node(const double* __restrict__ ye, int S, int N, int n, int code, double cmax,
                                             double& ctot, double& cs) {
    ctot = 0.0;
    cs = 0.0;
    for (int i = 0; i < S; ++i) {
        const double yi = ye[(size_t)i*(size_t)N + (size_t)n];
        const double c = (yi > RMT_FIT_EPS ? yi : RMT_FIT_EPS)*cmax;
        ctot += c;
        if (i == code) cs = c;
    }
}

// d (mole fraction of species `code` at node n) / d p from one parameter's rows sp; zero derivative at the clamp
__device__ __forceinline__ double rmt_fit_node_dx(const double* __restrict__ ye, const double* __restrict__ sp, int S, int N,
                                                  int n, int code, double cmax, double ctot, double cs) {
    double dsum = 0.0;
    for (int i = 0; i < S; ++i) {
        const size_t at = (size_t)i*(size_t)N + (size_t)n;
        const double d = ye[at] > RMT_FIT_EPS ? sp[at]*cmax : 0.0;
        dsum += d;
    }
    const size_t at = (size_t)code*(size_t)N + (size_t)n;
    const double ds = ye[at] > RMT_FIT_EPS ? sp[at]*cmax : 0.0;
    return ds/ctot - (cs*dsum)/(ctot*ctot);
}

// y [E][V][N]; sens [E][P][V+1][N] (rmt_n2_steady_sens); stats [E][4] (the march's: entry 1 = the failed node, -1 none);
// rows [E][width]; meas [E][MQ][3]; pred [E][MQ]; contrib [E][RMT_FIT_CONTRIB].  1 <= P <= 8, 1 <= MQ <= 64.
// EX: pos [E][MQ][2] = {n0, f} of the entries measured along the bed; scale: the fitted columns and their log flags.
template <bool EX>
__device__ __forceinline__ void rmt_fit_residuals(
    const double* __restrict__ y, const double* __restrict__ sens, const double* __restrict__ stats,
    const double* __restrict__ rows, const double* __restrict__ meas, double* __restrict__ pred,
    double* __restrict__ contrib, int E, int S, int V, int N, int P, int MQ, int width,
    const double* __restrict__ pos, const RmtFitScale& scale) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, waves = (int)blockDim.x >> 6;
    // which entry of contrib this lane adds up: 0 the cost, 1..8 g[ja], 9..44 H[ja][jb]
    int ja = 0, jb = 0;
    if (lane >= 1 && lane <= RMT_FIT_MAXP) {
        ja = lane - 1;
    } else if (lane > RMT_FIT_MAXP && lane < RMT_FIT_CONTRIB - 1) {
        int k = lane - 1 - RMT_FIT_MAXP;
        while (k >= RMT_FIT_MAXP - ja) { k -= RMT_FIT_MAXP - ja; ++ja; }
        jb = ja + k;
    }
    for (long long e = (long long)blockIdx.x*waves + wave; e < E; e += (long long)gridDim.x*waves) {
        const double* __restrict__ ye = y + (size_t)e*(size_t)V*(size_t)N;
        const double* __restrict__ se = sens + (size_t)e*(size_t)P*(size_t)(V + 1)*(size_t)N;
        const double* __restrict__ row = rows + (size_t)e*(size_t)width;
        const double cmax = row[RMT_FIT_M_CMAX], tf = row[RMT_FIT_M_TF];
        const size_t prow = (size_t)(V + 1)*(size_t)N;              // one parameter's rows
        int peak = 0;
        if (V > S) (void)rmt_fit_row_max(ye + (size_t)S*(size_t)N, N, lane, peak);
        double r = 0.0, J[RMT_FIT_MAXP];
#pragma unroll
        for (int p = 0; p < RMT_FIT_MAXP; ++p) J[p] = 0.0;
        bool bad = false;
        if (lane < MQ) {
            const double* __restrict__ mq = meas + ((size_t)e*(size_t)MQ + (size_t)lane)*3;
            const int code = (int)mq[0];
            const double value = mq[1], w = mq[2];
            double pv = 0.0;
            if (w != 0.0) {
                if (code >= 0 && code < S) {
                    double ctot, cs;
                    rmt_fit_node(ye, S, N, N - 1, code, cmax, ctot, cs);
                    pv = cs/ctot;
#pragma unroll
                    for (int p = 0; p < RMT_FIT_MAXP; ++p)
                        if (p < P) J[p] = rmt_fit_node_dx(ye, se + (size_t)p*prow, S, N, N - 1, code, cmax, ctot, cs)*w;
                } else if (V > S && (code == S || code == S + 1)) {
                    const size_t at = (size_t)S*(size_t)N + (size_t)(code == S ? N - 1 : peak);
                    pv = ye[at]*tf + tf;
#pragma unroll
                    for (int p = 0; p < RMT_FIT_MAXP; ++p)
                        if (p < P) J[p] = (se[(size_t)p*prow + at]*tf)*w;
                } else if (EX && code >= S + 2 && code < 2*S + 3 && (V > S || code > S + 2)) {
                    const double* __restrict__ pq = pos + ((size_t)e*(size_t)MQ + (size_t)lane)*2;
                    const int n0 = (int)pq[0];
                    const double f = pq[1], f0 = 1.0 - f;
                    if (n0 < 0 || n0 > N - 2) {
                        pv = __builtin_nan("");                    // a record outside the mesh: the member fails
                    } else if (code == S + 2) {
                        const size_t at = (size_t)S*(size_t)N + (size_t)n0;
                        pv = f0*(ye[at]*tf + tf) + f*(ye[at + 1]*tf + tf);
#pragma unroll
                        for (int p = 0; p < RMT_FIT_MAXP; ++p)
                            if (p < P) J[p] = (f0*(se[(size_t)p*prow + at]*tf) + f*(se[(size_t)p*prow + at + 1]*tf))*w;
                    } else {
                        const int sp = code - S - 3;
                        double ct0, cs0, ct1, cs1;
                        rmt_fit_node(ye, S, N, n0, sp, cmax, ct0, cs0);
                        rmt_fit_node(ye, S, N, n0 + 1, sp, cmax, ct1, cs1);
                        pv = f0*(cs0/ct0) + f*(cs1/ct1);
#pragma unroll
                        for (int p = 0; p < RMT_FIT_MAXP; ++p)
                            if (p < P)
                                J[p] = (f0*rmt_fit_node_dx(ye, se + (size_t)p*prow, S, N, n0, sp, cmax, ct0, cs0) +
                                        f*rmt_fit_node_dx(ye, se + (size_t)p*prow, S, N, n0 + 1, sp, cmax, ct1, cs1))*w;
                    }
                } else {
                    pv = __builtin_nan("");                        // a code the table must not hold: the member fails
                }
                if (EX) {
                    // theta = ln p: d/d theta = p d/d p, p the member's own value of the constant
#pragma unroll
                    for (int p = 0; p < RMT_FIT_MAXP; ++p)
                        if (p < P && scale.log[p]) J[p] = J[p]*row[RMT_FIT_M_USER + S + scale.col[p]];
                }
                r = (pv - value)*w;
                bad = !rmt_fit_finite(pv) || !rmt_fit_finite(r);
#pragma unroll
                for (int p = 0; p < RMT_FIT_MAXP; ++p) bad = bad || !rmt_fit_finite(J[p]);
            }
            pred[(size_t)e*(size_t)MQ + (size_t)lane] = pv;
        }
        // entry `lane` of contrib: the sum over the quantities in index order
        double acc = 0.0;
        for (int q = 0; q < MQ; ++q) {
            const double rq = __shfl(r, q, 64);
            double va = 0.0, vb = 0.0;
#pragma unroll
            for (int p = 0; p < RMT_FIT_MAXP; ++p) {
                const double jq = __shfl(J[p], q, 64);
                va = ja == p ? jq : va;
                vb = jb == p ? jq : vb;
            }
            const double term = lane == 0 ? rq*rq : lane <= RMT_FIT_MAXP ? va*rq : va*vb;
            acc += term;
        }
        if (lane == 0) acc = 0.5*acc;
        if (lane < RMT_FIT_CONTRIB - 1) bad = bad || !rmt_fit_finite(acc);
        const bool failed = __any(bad) || stats[(size_t)e*4 + 1] >= 0.0;
        if (lane == RMT_FIT_CONTRIB - 1) acc = failed ? 1.0 : 0.0;
        if (lane < RMT_FIT_CONTRIB) contrib[(size_t)e*RMT_FIT_CONTRIB + (size_t)lane] = acc;
    }
}

extern "C" __global__ __launch_bounds__(RMT_FIT_BLOCK) void rmt_n2_fit_residuals_f64(
    const double* __restrict__ y, const double* __restrict__ sens, const double* __restrict__ stats,
    const double* __restrict__ rows, const double* __restrict__ meas, double* __restrict__ pred,
    double* __restrict__ contrib, int E, int S, int V, int N, int P, int MQ, int width) {
    rmt_fit_residuals<false>(y, sens, stats, rows, meas, pred, contrib, E, S, V, N, P, MQ, width, nullptr, RmtFitScale());
}

extern "C" __global__ __launch_bounds__(RMT_FIT_BLOCK) void rmt_n2_fit_residuals_ex_f64(
    const double* __restrict__ y, const double* __restrict__ sens, const double* __restrict__ stats,
    const double* __restrict__ rows, const double* __restrict__ meas, double* __restrict__ pred,
    double* __restrict__ contrib, int E, int S, int V, int N, int P, int MQ, int width,
    const double* __restrict__ pos, RmtFitScale scale) {
    rmt_fit_residuals<true>(y, sens, stats, rows, meas, pred, contrib, E, S, V, N, P, MQ, width, pos, scale);
}

// Cholesky factor of the P x P matrix a (row-major, stride 8, lower triangle written in place) - false at a pivot that
// is not positive (a NaN included)
__device__ __forceinline__ bool rmt_fit_cholesky(double* a, int P) {
    for (int j = 0; j < P; ++j) {
        double d = a[j*RMT_FIT_MAXP + j];
        for (int k = 0; k < j; ++k) d = d - a[j*RMT_FIT_MAXP + k]*a[j*RMT_FIT_MAXP + k];
        if (!(d > 0.0)) return false;
        const double l = __builtin_sqrt(d);
        a[j*RMT_FIT_MAXP + j] = l;
        for (int i = j + 1; i < P; ++i) {
            double s = a[i*RMT_FIT_MAXP + j];
            for (int k = 0; k < j; ++k) s = s - a[i*RMT_FIT_MAXP + k]*a[j*RMT_FIT_MAXP + k];
            a[i*RMT_FIT_MAXP + j] = s/l;
        }
    }
    return true;
}

// contrib [E][46]; rows [E][width] (written: the user columns cols[j] of every member); state [RMT_FIT_STATE], zero before
// the first pass; log [RMT_FIT_LOG], this pass's slice.  The columns travel by value.
// EX: log [RMT_FIT_LOG_EX]; the law in theta_j = p_j, ln p_j for a log-scaled parameter (box.log), inside the box: the
// bounds in p (plo, phi) and in theta (lo, hi: the logarithms are taken on the host), -inf / +inf where open.  In order:
//  1. the active set A = {j: p_j <= plo_j and g_j > 0, or p_j >= phi_j and g_j < 0}: row and column j of H + lambda D become
//     the unit vector, g_j = 0; all parameters in A: converged;
//  2. the step, then theta + delta clamped into [lo, hi]: delta_c;
//  3. the predicted reduction: nothing clamped - 1/2 delta^T (lambda D delta - g) as without bounds; else the model's own
//     -(g^T delta_c + 1/2 delta_c^T H delta_c), and one that is not > 0 counts as a failed pivot (lambda <- 10 lambda);
//  4. converged when max_j |delta_c,j| / s_j <= tolerance, s_j = max(|p_j|, 1e-300), 1 for a log parameter;
//  5. the trial: p + delta_c, p exp(delta_c) for a log parameter, the bound itself where the step was clamped - kept in
//     [plo, phi] so that a rounding in exp cannot leave the box.
struct RmtFitBox { double plo[RMT_FIT_MAXP], phi[RMT_FIT_MAXP], lo[RMT_FIT_MAXP], hi[RMT_FIT_MAXP]; int log[RMT_FIT_MAXP]; };

template <bool EX>
__device__ __forceinline__ void rmt_fit_update(
    const double* __restrict__ contrib, double* __restrict__ rows, double* __restrict__ state, double* __restrict__ log,
    int E, int S, int P, int width, const RmtFitCols& cols, double tolerance, double damping0, const RmtFitBox& box) {
    __shared__ double s_sum[RMT_FIT_CONTRIB], s_a[RMT_FIT_MAXP*RMT_FIT_MAXP], s_g[RMT_FIT_MAXP], s_h[RMT_FIT_TRI],
        s_d[RMT_FIT_MAXP], s_x[RMT_FIT_MAXP], s_pc[RMT_FIT_MAXP], s_pt[RMT_FIT_MAXP];
    __shared__ int s_col[RMT_FIT_MAXP];
    // (EX only; a kernel that does not touch them allocates none of it)
    __shared__ double s_box[4*RMT_FIT_MAXP], s_th[RMT_FIT_MAXP];
    __shared__ int s_log[RMT_FIT_MAXP], s_side[RMT_FIT_MAXP];
    const int lane = (int)threadIdx.x;
    if (EX && lane < RMT_FIT_MAXP) {
        s_box[lane] = box.plo[lane];
        s_box[RMT_FIT_MAXP + lane] = box.phi[lane];
        s_box[2*RMT_FIT_MAXP + lane] = box.lo[lane];
        s_box[3*RMT_FIT_MAXP + lane] = box.hi[lane];
        s_log[lane] = box.log[lane];
    }
    const double* const s_plo = s_box;
    const double* const s_phi = s_box + RMT_FIT_MAXP;
    const double* const s_lo = s_box + 2*RMT_FIT_MAXP;
    const double* const s_hi = s_box + 3*RMT_FIT_MAXP;
    if (lane < RMT_FIT_CONTRIB) {
        // (eight independent loads in flight, added in index order: the sum is the sequential one)
        double acc = 0.0;
        const double* __restrict__ c = contrib + lane;
        int e = 0;
        for (; e + 8 <= E; e += 8) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = c[(size_t)(e + k)*RMT_FIT_CONTRIB];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc += v[k];
        }
        for (; e < E; ++e) acc += c[(size_t)e*RMT_FIT_CONTRIB];
        s_sum[lane] = acc;
    }
    if (lane < RMT_FIT_MAXP) s_col[lane] = cols.col[lane];
    __syncthreads();
    if (lane == 0) {
        const double Ct = s_sum[0], nfail = s_sum[RMT_FIT_CONTRIB - 1];
        double Ccur = state[1], lam = state[2], nu = state[3], conv = state[4], status = state[6], red = state[7];
        const bool started = state[0] != 0.0;
        double accepted = 0.0;
        for (int j = 0; j < RMT_FIT_MAXP; ++j) {
            s_pc[j] = started ? state[RMT_FIT_ST_PCUR + j] : (j < P ? rows[RMT_FIT_M_USER + S + s_col[j]] : 0.0);
            s_pt[j] = started ? state[RMT_FIT_ST_PTRIAL + j] : s_pc[j];
        }
        if (conv == 0.0 && status == 0.0) {          // (converged, or given up: frozen - only the log slice is written)
            const bool ok = rmt_fit_finite(Ct) && nfail == 0.0;
            bool take;
            if (!started) {
                take = true;
                if (!ok) status = (double)((int)status | RMT_FIT_FIRST_FAILED);
                lam = damping0;
                nu = 2.0;
            } else {
                take = ok && Ct < Ccur;
                if (take) {
                    const double rho = (Ccur - Ct)/red;
                    const double t = 2.0*rho - 1.0;
                    double f = 1.0 - t*t*t;
                    if (!(f > 1.0/3.0)) f = 1.0/3.0;
                    lam = lam*f;
                    nu = 2.0;
                } else {
                    lam = lam*nu;
                    nu = 2.0*nu;
                }
            }
            if (take) {
                accepted = 1.0;
                Ccur = Ct;
                for (int j = 0; j < RMT_FIT_MAXP; ++j) {
                    s_pc[j] = s_pt[j];
                    state[RMT_FIT_ST_G + j] = s_sum[1 + j];
                }
                for (int k = 0; k < RMT_FIT_TRI; ++k) state[RMT_FIT_ST_H + k] = s_sum[1 + RMT_FIT_MAXP + k];
            }
            for (int j = 0; j < RMT_FIT_MAXP; ++j) s_g[j] = state[RMT_FIT_ST_G + j];
            for (int k = 0; k < RMT_FIT_TRI; ++k) s_h[k] = state[RMT_FIT_ST_H + k];
            int act = 0;
            if (EX) {
                int lower = 0, upper = 0;
                for (int j = 0; j < P; ++j) {
                    if (s_pc[j] <= s_plo[j] && s_g[j] > 0.0) lower |= 1 << j;
                    if (s_pc[j] >= s_phi[j] && s_g[j] < 0.0) upper |= 1 << j;
                }
                act = lower | upper;
                for (int j = 0; j < P; ++j)
                    if ((act >> j) & 1) s_g[j] = 0.0;
                state[RMT_FIT_ST_LOWER] = (double)lower;
                state[RMT_FIT_ST_UPPER] = (double)upper;
            }
            if (Ccur == 0.0 || (EX && act == (1 << P) - 1)) conv = 1.0;
            if (conv == 0.0 && ((int)status & RMT_FIT_FIRST_FAILED) == 0) {
                for (int j = 0; j < P; ++j) {
                    const double hjj = s_h[rmt_fit_tri(j, j)];
                    s_d[j] = hjj > RMT_FIT_FLOOR ? hjj : RMT_FIT_FLOOR;
                    if (EX) s_th[j] = s_log[j] ? ::log(s_pc[j]) : s_pc[j];   // (`log` is the slice here)
                }
                bool solved = false, clamped = false;
                for (int tries = 0; tries <= 8 && !solved; ++tries) {
                    if (tries) lam = 10.0*lam;
                    for (int i = 0; i < P; ++i)
                        for (int j = 0; j <= i; ++j) {
                            if (EX && (((act >> i) | (act >> j)) & 1))
                                s_a[i*RMT_FIT_MAXP + j] = i == j ? 1.0 : 0.0;
                            else
                                s_a[i*RMT_FIT_MAXP + j] = i == j ? s_h[rmt_fit_tri(j, i)] + lam*s_d[i] : s_h[rmt_fit_tri(j, i)];
                        }
                    if (!rmt_fit_cholesky(s_a, P)) continue;
                    // L z = -g, L^T delta = z
                    for (int i = 0; i < P; ++i) {
                        double s = -s_g[i];
                        for (int k = 0; k < i; ++k) s = s - s_a[i*RMT_FIT_MAXP + k]*s_x[k];
                        s_x[i] = s/s_a[i*RMT_FIT_MAXP + i];
                    }
                    for (int i = P - 1; i >= 0; --i) {
                        double s = s_x[i];
                        for (int k = i + 1; k < P; ++k) s = s - s_a[k*RMT_FIT_MAXP + i]*s_x[k];
                        s_x[i] = s/s_a[i*RMT_FIT_MAXP + i];
                    }
                    if (EX) {
                        clamped = false;
                        for (int j = 0; j < P; ++j) {
                            const double t = s_th[j] + s_x[j];
                            s_side[j] = 0;
                            if (t < s_lo[j]) {
                                s_side[j] = -1;             // (already on the bound: no step, whatever ln rounds to)
                                s_x[j] = s_pc[j] <= s_plo[j] ? 0.0 : s_lo[j] - s_th[j];
                            } else if (t > s_hi[j]) {
                                s_side[j] = 1;
                                s_x[j] = s_pc[j] >= s_phi[j] ? 0.0 : s_hi[j] - s_th[j];
                            }
                            clamped = clamped || s_side[j] != 0;
                        }
                        if (clamped) {
                            // the model's own decrease along the clamped step
                            double gd = 0.0, hd = 0.0;
                            for (int i = 0; i < P; ++i) {
                                gd += s_g[i]*s_x[i];
                                double hrow = 0.0;
                                for (int j = 0; j < P; ++j) hrow += s_h[i <= j ? rmt_fit_tri(i, j) : rmt_fit_tri(j, i)]*s_x[j];
                                hd += s_x[i]*hrow;
                            }
                            red = -(gd + 0.5*hd);
                            if (!(red > 0.0)) continue;
                        }
                    }
                    solved = true;
                }
                if (!solved) {
                    status = (double)((int)status | RMT_FIT_NOT_POSITIVE);
                } else {
                    double q = 0.0, step = 0.0;
                    for (int j = 0; j < P; ++j) {
                        q += s_x[j]*((lam*s_d[j])*s_x[j] - s_g[j]);
                        const double a = __builtin_fabs(s_pc[j]);
                        const double rel = EX && s_log[j] ? __builtin_fabs(s_x[j])
                                                          : __builtin_fabs(s_x[j])/(a > RMT_FIT_FLOOR ? a : RMT_FIT_FLOOR);
                        if (!(rel <= step)) step = rel;             // (a NaN stays and never converges)
                    }
                    if (!(EX && clamped)) red = 0.5*q;
                    if (step <= tolerance) conv = 1.0;
                    for (int j = 0; j < P; ++j) {
                        double v;
                        if (EX) {
                            if (s_side[j]) v = s_side[j] < 0 ? s_plo[j] : s_phi[j];
                            else v = s_log[j] ? s_pc[j]*::exp(s_x[j]) : s_pc[j] + s_x[j];
                            v = v < s_plo[j] ? s_plo[j] : v;
                            v = v > s_phi[j] ? s_phi[j] : v;
                        } else {
                            v = s_pc[j] + s_x[j];
                        }
                        s_pt[j] = v;
                        state[RMT_FIT_ST_DELTA + j] = s_x[j];
                    }
                }
            }
            if (conv != 0.0 || status != 0.0)
                for (int j = 0; j < RMT_FIT_MAXP; ++j) s_pt[j] = s_pc[j];
            state[0] = 1.0;
            state[1] = Ccur;
            state[2] = lam;
            state[3] = nu;
            state[4] = conv;
            state[5] = state[5] + 1.0;
            state[6] = status;
            state[7] = red;
            for (int j = 0; j < RMT_FIT_MAXP; ++j) {
                state[RMT_FIT_ST_PCUR + j] = s_pc[j];
                state[RMT_FIT_ST_PTRIAL + j] = s_pt[j];
            }
        }
        log[0] = Ct;
        log[1] = Ccur;
        log[2] = lam;
        log[3] = nu;
        log[4] = accepted;
        log[5] = conv;
        log[6] = nfail;
        log[7] = status;
        for (int j = 0; j < RMT_FIT_MAXP; ++j) {
            log[8 + j] = s_pt[j];
            log[16 + j] = s_pc[j];
            log[24 + j] = s_sum[1 + j];
        }
        for (int k = 0; k < RMT_FIT_TRI; ++k) log[32 + k] = s_sum[1 + RMT_FIT_MAXP + k];
        if (EX) {
            log[RMT_FIT_LOG] = state[RMT_FIT_ST_LOWER];
            log[RMT_FIT_LOG + 1] = state[RMT_FIT_ST_UPPER];
        }
    }
    __syncthreads();
    // the trial values into the fitted user columns of every member's row
    for (int k = lane; k < E*P; k += (int)blockDim.x) {
        const int e = k/P, j = k - e*P;
        rows[(size_t)e*(size_t)width + (size_t)(RMT_FIT_M_USER + S + s_col[j])] = s_pt[j];
    }
}

extern "C" __global__ __launch_bounds__(64) void rmt_n2_fit_update_f64(
    const double* __restrict__ contrib, double* __restrict__ rows, double* __restrict__ state, double* __restrict__ log,
    int E, int S, int P, int width, RmtFitCols cols, double tolerance, double damping0) {
    rmt_fit_update<false>(contrib, rows, state, log, E, S, P, width, cols, tolerance, damping0, RmtFitBox());
}

extern "C" __global__ __launch_bounds__(64) void rmt_n2_fit_update_ex_f64(
    const double* __restrict__ contrib, double* __restrict__ rows, double* __restrict__ state, double* __restrict__ log,
    int E, int S, int P, int width, RmtFitCols cols, double tolerance, double damping0, RmtFitBox box) {
    rmt_fit_update<true>(contrib, rows, state, log, E, S, P, width, cols, tolerance, damping0, box);
}
