//>>> RMT_SENS  (plan.Mechanism.source generates every unit but the sensitivity unit, n2.sens_plan, WITHOUT the lines
// from this mark to the closing one: their sources and cache keys are what they are without this file)
#if RMT_SENS
// ===================================================================== parametric sensitivities of the N2 steady state
// solver-config "sensitivity" (host: rmt_app_amd/sensitivity.py).  The discrete steady state f(y*) = 0 the march found
// (71_steady_march.inc) is block lower-bidiagonal, so its tangent system is a downstream march as well: with
// a_z = -df/dy at the converged node (y*_z, up_z, P_z), for every parameter p
//     a_z s_z = U D_{z-1} s_{z-1} + (df/dP) pi_z + df/dp,          pi_{z+1} = az_z pi_z + P_z (d az/dy . s_z)
// s_z = dy*_z/dp, pi_z = dP_z/dp, U = diag(conv, .., conv, FT inv_dz) (the upwind coupling), D the derivative of the
// clamp (1 for theta, y_i > RMT_EPS for a species) and az = 1 - alpha_k M/T the node's Ergun coefficient.  Everything
// is analytic: df/dy, df/dP and df/du_k come from ONE evaluation of the generated rmt_kinetics_jacs (rmt_kinetics_jac
// plus the partials by P and by the per-reactor inputs u<k>), the rest is differentiated by hand, term by term as
// rmt_node_jac does it.  a_z is inverted once per node (no 1/h shift) and applied to all right-hand sides.
// The parameters are the member-row values the march read: TM, THETA_IN, P0, CIN_i, and the user columns u<k>.
#if RMT_SENS != 1
#error "RMT_SENS: 1 (the sensitivity sweep behind the steady-state march) or undefined"
#endif
#if !RMT_WITH_MARCH
#error "RMT_SENS: needs RMT_WITH_MARCH (the sensitivity unit is the march unit plus RMT_SENS and RMT_SENS_NP)"
#endif
#ifndef RMT_SENS_NP
#error "RMT_SENS: RMT_SENS_NP (the number of parameters, 1..8) must be defined"
#endif
#if RMT_SENS_NP < 1 || RMT_SENS_NP > 8
#error "RMT_SENS_NP: 1..8"
#endif
#define RMT_SENS_TM 0          // "medium-temperature": member field TM
#define RMT_SENS_TIN 1         // "inlet-temperature":  member field THETA_IN
#define RMT_SENS_PIN 2         // "inlet-pressure":     member field P0
#define RMT_SENS_CIN 3         // "inlet-concentration": member field CIN[index]
#define RMT_SENS_USER 4        // "rate-constant":      user column u<index>
#define RMT_SENS_NUU (RMT_NU > 0 ? RMT_NU : 1)
struct RmtSensDesc {
    int kind[8], index[8];     // per parameter; entries from RMT_SENS_NP on are not looked at
};

// What one node contributes, parameter-independent: the inverse of a = -df/dy (pivot: its smallest |pivot|), the columns
// df/dP, df/du_k and the energy row's d/dTM, the node's Ergun coefficient and its gradient.
struct RmtSensNode {
    real ainv[RMT_V][RMT_V];
    real fP[RMT_V], fU[RMT_SENS_NUU][RMT_V], daz[RMT_V];
    real ftm, pivot;
    preal az;
};

// a = -df/dy and the parameter columns at (y, P) - rmt_node_jac with its intermediate values kept (a is NOT yet inverted)
template <typename FL>
__device__ __forceinline__ void rmt_sens_eval(const RmtMember& m, const real* __restrict__ ys, const preal Pz,
                                              RmtSensNode& sn, FL& flag) {
    RmtNode nd;
    sn.az = rmt_node_pre(m, ys, nd);
#if RMT_PROFILE
    nd.act = m.act;                   // the node this lane is at (the kernel below reads the table per node)
    nd.dtm = m.dtm;
#endif
    real (&a)[RMT_V][RMT_V] = sn.ainv;
    const real P = real(Pz);
    real r[RMT_R], drdT[RMT_R], drdx[RMT_R][RMT_S], drdC[RMT_R][RMT_S], drdP[RMT_R], drdU[RMT_R][RMT_SENS_NUU];
    rmt_kinetics_jacs(nd.T, nd.invT, P, nd.x, nd.C, m.user, r, drdT, drdx, drdC, drdP, drdU, flag);
#if RMT_PROFILE
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) {                     // catalyst activity: every rate and every partial of it
        r[q] *= nd.act;
        drdP[q] *= nd.act;
#pragma unroll
        for (int k = 0; k < RMT_SENS_NUU; ++k) drdU[q][k] *= nd.act;
    }
#endif
    real ctot = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) ctot += nd.C[i];
    const real ict = rmt_rcp(ctot);
    real act[RMT_S];                                       // d C_j / d c_j: cmax where the clamp is inactive
#pragma unroll
    for (int j = 0; j < RMT_S; ++j) act[j] = (ys[j] > RMT_EPS) ? m.cmax * ict : real(0);
    real G[RMT_R][RMT_V];                                  // G[q][c] = d r_q / d y_c
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) {
        real sx = real(0);
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) sx += nd.x[i] * drdx[q][i];
#pragma unroll
        for (int j = 0; j < RMT_S; ++j) G[q][j] = act[j] * (drdC[q][j] * ctot + (drdx[q][j] - sx));
#if !RMT_ISO
        G[q][RMT_S] = m.tf * drdT[q];
#endif
#if RMT_PROFILE
#pragma unroll
        for (int c = 0; c < RMT_V; ++c) G[q][c] *= nd.act;
#endif
    }
    // species rows: k_i = -F1 (c_i - up_i) inv_dz + FM sum_q nu_qi r_q
    const real fm = m.inv_macote;
#pragma unroll
    for (int c = 0; c < RMT_V; ++c) {
        real col[RMT_R], src[RMT_S];
#pragma unroll
        for (int q = 0; q < RMT_R; ++q) col[q] = G[q][c];
        rmt_species_source(col, src);
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) a[i][c] = -(fm * src[i]);
    }
    {
        real src[RMT_S];
        rmt_species_source(drdP, src);
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) sn.fP[i] = fm * src[i];
#pragma unroll
        for (int k = 0; k < RMT_SENS_NUU; ++k) {
            real col[RMT_R];
#pragma unroll
            for (int q = 0; q < RMT_R; ++q) col[q] = drdU[q][k];
            rmt_species_source(col, src);
#pragma unroll
            for (int i = 0; i < RMT_S; ++i) sn.fU[k][i] = fm * src[i];
        }
    }
    const real conv = m.f1 * m.inv_dz;
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) a[i][i] += conv;
    // the Ergun coefficient az = 1 - alpha_k M/T:  dM_j = act_j (1e-3 MW_j - M),  d(M/T)/d theta = -M Tf / T^2
#pragma unroll
    for (int j = 0; j < RMT_S; ++j)
        sn.daz[j] = -(real(m.alpha_k) * (act[j] * (real(1e-3) * RMT_MW[j] - nd.M)) * nd.invT);
    sn.ftm = real(0);
#if !RMT_ISO
    sn.daz[RMT_S] = real(m.alpha_k) * nd.M * m.tf * (nd.invT * nd.invT);
    // energy row: k_T = -FT (theta - up_T) inv_dz + gain (qm - qr), gain = GAIN_K / (P (M/T) cpm)
    const real T = nd.T;
    real cpbar[RMT_S], dcpb[RMT_S];
    real cpm = real(0), dcpm = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) {
        cpbar[i] = rmt_cp_mean(i, T);
        dcpb[i] = rmt_cp_mean_dT(i, T);
        cpm += nd.x[i] * cpbar[i];
        dcpm += nd.x[i] * dcpb[i];
    }
    real dcp[RMT_R], ddcp[RMT_R];
    rmt_reaction_dcp(cpbar, dcp);
    rmt_reaction_dcp(dcpb, ddcp);
    real qr = real(0), dqrT = real(0), dqrP = real(0);
    real hq[RMT_R];
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) {
        hq[q] = dcp[q] * (T - RMT_TREF) + RMT_DH25[q];
        qr += r[q] * hq[q];
        dqrT += G[q][RMT_S] * hq[q] + r[q] * (m.tf * (dcp[q] + (T - RMT_TREF) * ddcp[q]));
        dqrP += drdP[q] * hq[q];
    }
    const bool wall = !(m.tm == real(0));
#if RMT_PROFILE
    const real qm = wall ? m.ua * ((m.tm + nd.dtm) - T) : real(0);
#else
    const real qm = wall ? m.ua * (m.tm - T) : real(0);
#endif
    const real dqmT = wall ? -(m.ua * m.tf) : real(0);
    const real icpm = rmt_rcp(cpm);
    const real iP = rmt_rcp(P);
    const real gain = m.inv_hecote * rmt_rcp(P * nd.MoT) * icpm;
    const real drive = gain * (qm - qr);                  // gain (qm - qr)
    const real iM = rmt_rcp(nd.M);
#pragma unroll
    for (int j = 0; j < RMT_S; ++j) {
        // d ln gain / d c_j = -(dM_j / M + dcpm_j / cpm),  dM_j = act_j (1e-3 MW_j - M),  dcpm_j = act_j (cpbar_j - cpm)
        const real dlg = -act[j] * ((real(1e-3) * RMT_MW[j] - nd.M) * iM + (cpbar[j] - cpm) * icpm);
        real gq = real(0);
#pragma unroll
        for (int q = 0; q < RMT_R; ++q) gq += hq[q] * G[q][j];
        a[RMT_S][j] = -(dlg * drive - gain * gq);
    }
    {
        const real dlgT = m.tf * (nd.invT - dcpm * icpm);   // d ln gain / d theta: M/T -> +Tf/T, cpm -> -Tf cpm'/cpm
        a[RMT_S][RMT_S] = m.ft * m.inv_dz - (dlgT * drive + gain * (dqmT - dqrT));
    }
    sn.fP[RMT_S] = -(drive * iP) - gain * dqrP;             // d ln gain / dP = -1/P
#pragma unroll
    for (int k = 0; k < RMT_SENS_NUU; ++k) {
        real dq = real(0);
#pragma unroll
        for (int q = 0; q < RMT_R; ++q) dq += drdU[q][k] * hq[q];
        sn.fU[k][RMT_S] = -(gain * dq);
    }
    sn.ftm = wall ? gain * m.ua : real(0);                  // a wall that is off (TM == 0) stays off
#endif
}

// ... and the inverse in place.  False when the node is singular (a pivot that is not positive, or not finite).
template <typename FL>
__device__ __forceinline__ bool rmt_sens_factor(const RmtMember& m, const real* __restrict__ ys, const preal Pz,
                                                RmtSensNode& sn, FL& flag) {
    rmt_sens_eval(m, ys, Pz, sn, flag);
    sn.pivot = rmt_invert_n<RMT_V>(sn.ainv);
    return sn.pivot > real(0) && __builtin_isfinite((double)sn.pivot);
}

// The seed of one parameter: sd = D_{-1} s_{-1} (the inlet values are the node "before" node 0) and pi_0.  A feed component
// at the clamp (CIN_i <= RMT_EPS) has zero sensitivity: the inlet value the march used is RMT_EPS, whatever CIN_i is.
__device__ __forceinline__ void rmt_sens_seed(const RmtMember& m, const int kind, const int index, real* __restrict__ sd,
                                              preal& pi) {
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) sd[i] = (kind == RMT_SENS_CIN && index == i && m.cin[i] > RMT_EPS) ? real(1) : real(0);
#if !RMT_ISO
    sd[RMT_S] = (kind == RMT_SENS_TIN) ? real(1) : real(0);
#endif
    pi = (kind == RMT_SENS_PIN) ? preal(1) : preal(0);
}

// One parameter at one node: s = a^-1 (U sd + fP pi + df/dp); then sd <- D s and pi <- az pi + P (d az/dy . s) for the
// node behind.  False when s is not finite.
__device__ __forceinline__ bool rmt_sens_solve(const RmtMember& m, const RmtSensNode& sn, const real* __restrict__ ys,
                                               const preal Pz, const int kind, const int index, real* __restrict__ sd,
                                               preal& pi, real* __restrict__ s) {
    real rhs[RMT_V];
    const real conv = m.f1 * m.inv_dz, pr = real(pi);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) rhs[i] = conv * sd[i] + sn.fP[i] * pr;
#if !RMT_ISO
    rhs[RMT_S] = (m.ft * m.inv_dz) * sd[RMT_S] + sn.fP[RMT_S] * pr + (kind == RMT_SENS_TM ? sn.ftm : real(0));
#endif
#pragma unroll
    for (int k = 0; k < RMT_NU; ++k) {
        if (kind == RMT_SENS_USER && index == k) {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) rhs[i] += sn.fU[k][i];
        }
    }
    bool ok = true;
    preal dot = preal(0);
#pragma unroll
    for (int r = 0; r < RMT_V; ++r) {
        real acc = real(0);
#pragma unroll
        for (int c = 0; c < RMT_V; ++c) acc += sn.ainv[r][c] * rhs[c];
        s[r] = acc;
        ok = ok && __builtin_isfinite((double)acc);
        dot += preal(sn.daz[r]) * preal(acc);
    }
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) sd[i] = (ys[i] > RMT_EPS) ? s[i] : real(0);
#if !RMT_ISO
    sd[RMT_S] = s[RMT_S];
#endif
    pi = sn.az * pi + Pz * dot;
    return ok && __builtin_isfinite((double)pi);
}

#ifndef RMT_HOST_EMULATION
// kernel: one reactor per lane, the shape of rmt_n2_steady_march; the lane walks z = 0..N-1 over the converged state
// y[e][v][z], re-forms P_z by the march's recurrence and carries sd[NP][V] and pi[NP] in registers.
// out[e][p][v][z], v < V: d y*_v,z / dp in the scaled units of the state and of the member row; out[e][p][V][z] = d P_z / dp
// (stride-N stores: this runs once per run); np: the caller's parameter count, which must be RMT_SENS_NP.  A member with a singular node (or a non-finite result) gets
// RMT_FLAG_NONFINITE, NaN in all its rows at that node, and stops there: what is behind keeps what the buffer held.
extern "C" __global__ __launch_bounds__(64) void rmt_n2_steady_sens(
        const real* __restrict__ y /* [E][V][N] */, const double* __restrict__ members, const int N, const int E,
        const int np, const RmtSensDesc desc, double* __restrict__ out /* [E][NP][V+1][N] */, unsigned* __restrict__ flags) {
    rmt_math_init();
    const int e = blockIdx.x * 64 + (int)threadIdx.x;
    const bool live = e < E;
    if (np != RMT_SENS_NP) {          // the caller sized `out` for another unit: write nothing but the flag
        if (live) atomicOr(&flags[e], RMT_FLAG_NONFINITE);
        return;
    }
    RmtMember m;
    rmt_load_member(members + (size_t)(live ? e : 0) * RMT_NM, m);      // dead lanes read member 0 and write nothing
    RMT_PROFILE_BIND(m, live ? e : 0, N)
    real sd[RMT_SENS_NP][RMT_V];
    preal pi[RMT_SENS_NP];
#pragma unroll
    for (int p = 0; p < RMT_SENS_NP; ++p) rmt_sens_seed(m, desc.kind[p], desc.index[p], sd[p], pi[p]);
    preal P = m.p0;
    rmt_flags_t flag;                 // (the march reported the Python-exception tests of this very state already)
    rmt_flags_clear(flag);
    const real* ye = y + (size_t)(live ? e : 0) * RMT_V * N;
    double* oe = out + (size_t)(live ? e : 0) * RMT_SENS_NP * (RMT_V + 1) * N;
    int z = 0;
    bool failed = false;
    bool active = live && N > 0;
    while (__any(active)) {
        if (active) {
            real yz[RMT_V];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) yz[i] = ye[(size_t)i * N + z];
#if RMT_PROFILE
            m.act = real(m.prof[z]);                      // (active: z < N)
            m.dtm = real(m.prof[N + z]);
#endif
            RmtSensNode sn;
            bool ok = rmt_sens_factor(m, yz, P, sn, flag);
#pragma unroll
            for (int p = 0; p < RMT_SENS_NP; ++p) {
                double* op = oe + (size_t)p * (RMT_V + 1) * N + z;
                real s[RMT_V];
                const preal piz = pi[p];
                const bool okp = rmt_sens_solve(m, sn, yz, P, desc.kind[p], desc.index[p], sd[p], pi[p], s);
                ok = ok && okp;
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) op[(size_t)i * N] = (double)s[i];
                op[(size_t)RMT_V * N] = (double)piz;
            }
            if (!ok) {
#pragma unroll
                for (int p = 0; p < RMT_SENS_NP; ++p)
#pragma unroll
                    for (int i = 0; i <= RMT_V; ++i) oe[((size_t)p * (RMT_V + 1) + i) * N + z] = __builtin_nan("");
                failed = true;
                active = false;
            } else {
                P = rmt_pressure_next(m, sn.az, P);
                if (++z >= N) active = false;
            }
        }
    }
    if (live && failed) atomicOr(&flags[e], RMT_FLAG_NONFINITE);
}
#endif  // RMT_HOST_EMULATION
#endif  // RMT_SENS
