// ------------------------------------------------------------------ steady-state model N1: node function
// SURVEY.md section 8(f) rank 1: PackedBedHomoReactorClass.runN1 / modelEquationN1
// (pbHomoReactor.py:2694-3314), the steady sibling of N2 - an ODE in the dimensionless length z*
// for u = [c_1..c_S, P*, theta] - integrated by the reference with solve_ivp(LSODA) at
// t_eval = linspace(0, 1, zNo+1) (:2931).  Along z the chemistry is as stiff as in time, so the
// same Rosenbrock(4,3) scheme is used, here with a dense (S+2)^2 finite-difference Jacobian and ONE
// REACTOR PER LANE (an ensemble of N1 profiles); steps are clipped to the output grid.
//   member row (doubles, host: plan.member_constants_n1): see M1_* below.
// The per-lane stepper rmt_n1_ros4 (70_n1.inc) integrates any steady model through the three functions rmt_n1_init,
// rmt_n1_rhs and rmt_n1_rhs_jac; the generation-time define RMT_SS_MODEL picks their bodies: absent or 0 = model N1
// (this file), 7 = model M7, 1 = model M1 (23_node_steady.inc).  Every steady model keeps the member-row width
// 16 + S + NU, with the user parameters in the last NU columns.
#ifndef RMT_SS_MODEL
#define RMT_SS_MODEL 0
#endif
#define RMT_NM1 (16 + RMT_S + RMT_NU)
#define M1_USER (16 + RMT_S)
__device__ __forceinline__ void rmt_n1_user(const double* __restrict__ mr, real (&U)[RMT_NU > 0 ? RMT_NU : 1]) {
    U[0] = real(0);
#pragma unroll
    for (int k = 0; k < RMT_NU; ++k) U[k] = real(mr[M1_USER + k]);
}
#if RMT_SS_MODEL == 0
#define RMT_V1 (RMT_S + 1 + (RMT_ISO ? 0 : 1))
#define M1_CMAX 0
#define M1_TF 1
#define M1_PF 2          // = P0
#define M1_SPCO0 3
#define M1_ERGA 4        // 150 mu ergB/dp^2 * zf/Pf      (times SuGaVe)
#define M1_ERGC 5        // 1.75 ergD/dp * zf/Pf          (times rho SuGaVe^2)
#define M1_SUGAVE0 6
#define M1_RHO_K 7       // 1/(R GaDe0)
#define M1_INV_CP0 8
#define M1_EPS 9
#define M1_INV_MACOTE 10
#define M1_INV_HECOTE 11
#define M1_UA 12
#define M1_TM 13
#define M1_GADE0 14
#define M1_CIN 16

// RMT_N1_SCALE_FIX 1 = the reference's MODEL_SETTING['GaMaCoTe0'] != "MAX" branch of model N1: species i is scaled by
// ITS OWN feed concentration - real value u_i SpCoi0[i] (pbHomoReactor.py:3159-3162), GaMaCoTe0[i] = (vf/zf) SpCoi0[i]
// (:2819-2821) - while the initial values stay SpCoi0[i]/max(SpCoi0) (:2834).  With cin_i = SpCoi0[i]/Cmax (the row's
// M1_CIN columns) both follow from the existing row: scale_i = cmax cin_i, 1/GaMaCoTe0[i] = INV_MACOTE / cin_i.
#ifndef RMT_N1_SCALE_FIX
#define RMT_N1_SCALE_FIX 0
#endif
__device__ __forceinline__ real rmt_n1_scale(const double* __restrict__ mr, const real cmax, const int i) {
#if RMT_N1_SCALE_FIX
    return cmax * real(mr[M1_CIN + i]);
#else
    (void)mr; (void)i;
    return cmax;
#endif
}
__device__ __forceinline__ real rmt_n1_inv_macote(const double* __restrict__ mr, const int i) {
#if RMT_N1_SCALE_FIX
    return rmt_div(real(mr[M1_INV_MACOTE]), real(mr[M1_CIN + i]));
#else
    (void)i;
    return real(mr[M1_INV_MACOTE]);
#endif
}
// initial state u(z* = 0): c_i = SpCoi0[i]/Cmax, P* = 1, theta = 0 (pbHomoReactor.py:2831-2839)
__device__ __forceinline__ void rmt_n1_init(const double* __restrict__ mr, real (&u)[RMT_V1]) {
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) u[i] = real(mr[M1_CIN + i]);              // :2831-2839
    u[RMT_S] = real(1);
#if !RMT_ISO
    u[RMT_S + 1] = real(0);
#endif
}
template <typename FL>
__device__ __forceinline__ void rmt_n1_rhs(const double* __restrict__ mr, const real (&u)[RMT_V1],
                                           real (&du)[RMT_V1], FL& flag) {
    const real cmax = real(mr[M1_CMAX]), tf = real(mr[M1_TF]), pf = real(mr[M1_PF]);
    real C[RMT_S], x[RMT_S];
    real ctot = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { C[i] = u[i] * rmt_n1_scale(mr, cmax, i); ctot += C[i]; }      // :3123, :3159-3162 (no clamp in N1)
    const real inv_ctot = rmt_rcp(ctot);
    real mw = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { x[i] = C[i] * inv_ctot; mw += x[i] * RMT_MW[i]; }
    const real M = mw * real(1e-3);
    const real P = u[RMT_S] * pf;                                              // :3135
#if RMT_ISO
    const real T = tf;
#else
    const real T = u[RMT_S + 1] * tf + tf;
#endif
    // interstitial velocity from the EOS (rmtUtility.py:404-421): InGaVe* = (Ctot/SpCo0)(P0/P)
    const real vstar = rmt_div(ctot * pf, real(mr[M1_SPCO0]) * P);
    const real su = vstar * real(mr[M1_SUGAVE0]);
    const real rho = rmt_div(P * M, real(8.314472) * T);                        // rmtThermo.py:353
    const real rho_s = rho * rmt_rcp(real(mr[M1_GADE0]));
    du[RMT_S] = -(real(mr[M1_ERGA]) * su + real(mr[M1_ERGC]) * rho * su * su);  // :3206-3220
    real r[RMT_R], U[RMT_NU > 0 ? RMT_NU : 1];
    rmt_n1_user(mr, U);
    rmt_nocache_t nc;
    rmt_kinetics(T, rmt_rcp(T), P, x, C, U, r, flag, nc);
    real src[RMT_S];
    rmt_species_source(r, src);
    const real iv = rmt_rcp(vstar);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) du[i] = iv * src[i] * rmt_n1_inv_macote(mr, i);   // :3283-3289
#if !RMT_ISO
    real cpbar[RMT_S], cpm = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { cpbar[i] = rmt_cp_mean(i, T); cpm += x[i] * cpbar[i]; }
    real dcp[RMT_R];
    rmt_reaction_dcp(cpbar, dcp);
    real qr = real(0);
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) qr += r[q] * (dcp[q] * (T - RMT_TREF) + RMT_DH25[q]);
    const real tm = real(mr[M1_TM]);
    const real qm = (tm == real(0)) ? real(0) : real(mr[M1_UA]) * (tm - T);
    const real cp_eff = cpm * real(mr[M1_INV_CP0]) * real(mr[M1_EPS]);
    du[RMT_S + 1] = rmt_div((qm - qr) * real(mr[M1_INV_HECOTE]), rho_s * cp_eff * vstar);   // :3284,3298
#endif
}

#if RMT_WITH_N1
#ifndef RMT_N1_JAC_FD
#define RMT_N1_JAC_FD 0          // 1: the (S+2)^2 Jacobian by forward differences of rmt_n1_rhs (the round-1 form)
#endif
// rmt_n1_rhs AND a[r][c] = -d du_r / d u_c, analytic (the rates' partials by T, P, x_i, C_i come from the generated
// rmt_kinetics_jacp; the rest is differentiated by hand, term by term as rmt_n1_rhs writes it): one evaluation instead
// of the V1 + 1 of the forward differences.  With ln v* = ln(K Ctot / P), ln rho = ln(P M / (R T)):
//   d ln v*/dc_j = cmax/Ctot,  d ln v*/dp = -1/p;   d ln rho/dc_j = dM_j/M,  d ln rho/dp = 1/p,  d ln rho/dtheta = -Tf/T
//   f_P = -(A su + C rho su^2)            df_P = -(A su dlnv + C rho su^2 (dlnrho + 2 dlnv))
//   f_i = kappa src_i(r) / v*              df_i = kappa src_i(dr) / v* - f_i dlnv
//   f_T = h (qm - qr) / (rho_s cp_eff v*)  df_T = h (dqm - dqr) / Dn - f_T (dlnrho + dlncpm + dlnv)
template <typename FL>
__device__ __forceinline__ void rmt_n1_rhs_jac(const double* __restrict__ mr, const real (&u)[RMT_V1],
                                               real (&du)[RMT_V1], real (&a)[RMT_V1][RMT_V1], FL& flag) {
    const real cmax = real(mr[M1_CMAX]), tf = real(mr[M1_TF]), pf = real(mr[M1_PF]);
    real C[RMT_S], x[RMT_S], sc[RMT_S];                  // sc_j = d C_j / d u_j (cmax, or the species' own scale)
    real ctot = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { sc[i] = rmt_n1_scale(mr, cmax, i); C[i] = u[i] * sc[i]; ctot += C[i]; }
    const real inv_ctot = rmt_rcp(ctot);
    real mw = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { x[i] = C[i] * inv_ctot; mw += x[i] * RMT_MW[i]; }
    const real M = mw * real(1e-3);
    const real P = u[RMT_S] * pf;
#if RMT_ISO
    const real T = tf;
#else
    const real T = u[RMT_S + 1] * tf + tf;
#endif
    const real vstar = rmt_div(ctot * pf, real(mr[M1_SPCO0]) * P);
    const real su = vstar * real(mr[M1_SUGAVE0]);
    const real rho = rmt_div(P * M, real(8.314472) * T);
    const real rho_s = rho * rmt_rcp(real(mr[M1_GADE0]));
    const real ea = real(mr[M1_ERGA]) * su, ec = real(mr[M1_ERGC]) * rho * su * su;
    du[RMT_S] = -(ea + ec);
    real r[RMT_R], drdT[RMT_R], drdx[RMT_R][RMT_S], drdC[RMT_R][RMT_S], drdP[RMT_R], U[RMT_NU > 0 ? RMT_NU : 1];
    rmt_n1_user(mr, U);
    rmt_kinetics_jacp(T, rmt_rcp(T), P, x, C, U, r, drdT, drdx, drdC, drdP, flag);
    real src[RMT_S];
    rmt_species_source(r, src);
    const real iv = rmt_rcp(vstar);
    real kap[RMT_S];
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) {
        const real im = rmt_n1_inv_macote(mr, i);
        kap[i] = iv * im;
        du[i] = iv * src[i] * im;
    }
    // logarithmic derivatives by column: species j, pressure (index S), temperature (index S + 1)
    const real ip = rmt_rcp(u[RMT_S]), iM = rmt_rcp(M);
    real cj[RMT_S];
    real dlnv[RMT_V1], dlnrho[RMT_V1];
#pragma unroll
    for (int j = 0; j < RMT_S; ++j) {
        cj[j] = sc[j] * inv_ctot;
        dlnv[j] = cj[j];
        dlnrho[j] = cj[j] * (real(1e-3) * RMT_MW[j] - M) * iM;
    }
    dlnv[RMT_S] = -ip;
    dlnrho[RMT_S] = ip;
#if !RMT_ISO
    dlnv[RMT_S + 1] = real(0);
    dlnrho[RMT_S + 1] = -tf * rmt_rcp(T);
#endif
    // G[q][c] = d r_q / d u_c
    real G[RMT_R][RMT_V1];
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) {
        real sx = real(0);
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) sx += x[i] * drdx[q][i];
#pragma unroll
        for (int j = 0; j < RMT_S; ++j) G[q][j] = sc[j] * (drdC[q][j] + (drdx[q][j] - sx) * inv_ctot);
        G[q][RMT_S] = pf * drdP[q];
#if !RMT_ISO
        G[q][RMT_S + 1] = tf * drdT[q];
#endif
    }
#if !RMT_ISO
    real cpbar[RMT_S], dcpb[RMT_S], cpm = real(0), dcpm = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) {
        cpbar[i] = rmt_cp_mean(i, T);
        dcpb[i] = rmt_cp_mean_dT(i, T);
        cpm += x[i] * cpbar[i];
        dcpm += x[i] * dcpb[i];
    }
    real dcp[RMT_R], ddcp[RMT_R], hq[RMT_R];
    rmt_reaction_dcp(cpbar, dcp);
    rmt_reaction_dcp(dcpb, ddcp);
    real qr = real(0), dqrT = real(0);
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) {
        hq[q] = dcp[q] * (T - RMT_TREF) + RMT_DH25[q];
        qr += r[q] * hq[q];
        dqrT += r[q] * (tf * (dcp[q] + (T - RMT_TREF) * ddcp[q]));
    }
    const real tm = real(mr[M1_TM]);
    const bool wall = !(tm == real(0));
    const real qm = wall ? real(mr[M1_UA]) * (tm - T) : real(0);
    const real cp_eff = cpm * real(mr[M1_INV_CP0]) * real(mr[M1_EPS]);
    const real iDn = rmt_rcp(rho_s * cp_eff * vstar);
    const real hh = real(mr[M1_INV_HECOTE]);
    du[RMT_S + 1] = rmt_div((qm - qr) * hh, rho_s * cp_eff * vstar);
    const real icpm = rmt_rcp(cpm);
#endif
#pragma unroll
    for (int c = 0; c < RMT_V1; ++c) {
        real col[RMT_R], dsrc[RMT_S];
#pragma unroll
        for (int q = 0; q < RMT_R; ++q) col[q] = G[q][c];
        rmt_species_source(col, dsrc);
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) a[i][c] = -(kap[i] * dsrc[i] - du[i] * dlnv[c]);
        a[RMT_S][c] = ea * dlnv[c] + ec * (dlnrho[c] + real(2) * dlnv[c]);
#if !RMT_ISO
        real dqr = real(0);
#pragma unroll
        for (int q = 0; q < RMT_R; ++q) dqr += col[q] * hq[q];
        real dqm = real(0), dlncpm = real(0);
        if (c < RMT_S) dlncpm = cj[c < RMT_S ? c : 0] * (cpbar[c < RMT_S ? c : 0] - cpm) * icpm;
        if (c == RMT_S + 1) {
            dqr += dqrT;
            dqm = wall ? -(real(mr[M1_UA]) * tf) : real(0);
            dlncpm = tf * dcpm * icpm;
        }
        a[RMT_S + 1][c] = -(hh * (dqm - dqr) * iDn - du[RMT_S + 1] * (dlnrho[c] + dlncpm + dlnv[c]));
#endif
    }
}
#endif   // RMT_WITH_N1
#endif   // RMT_SS_MODEL == 0

