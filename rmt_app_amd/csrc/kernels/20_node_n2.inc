#if RMT_MODEL == 0
// ------------------------------------------------------------------ node physics
// (the switches of the node function's cuts and their defaults: 10_member.inc, in front of RmtMember)
// Phase A (before the pressure scan): clamp, real concentrations, mole fractions, T, mixture MW,
// Ergun affine coefficient.  pbHomoReactor.py:3897-3928, 3960-3979.
struct RmtNode {
    real x[RMT_S];
    real C[RMT_S];
    real T, M;
    real invT;     // 1/T: M/T below and every c/T, c/(R T) of the kinetics
    real MoT;      // M/T, shared by the Ergun coefficient and the EOS density
#if RMT_NODE_CS
    real ict;      // 1/sum cs; x holds cs, MoT is 1e3 M/T and M is not formed
#endif
#if RMT_PROFILE
    real act, dtm; // catalyst activity and coolant offset of this node (12_profile.inc); rmt_node_pre: the identity (1, 0)
#endif
};

// rmt_node_pre in two halves around its reciprocal, so that rmt_rhs_block can take the reciprocals of a lane's two nodes
// from one (RMT_NODE_PAIR_RCP): _sum returns sum(state) * T, _fin takes its reciprocal.
__device__ __forceinline__ real rmt_node_pre_sum(const RmtMember& m, const real* __restrict__ ys, RmtNode& nd,
                                                 real& ctot) {
    ctot = real(0);
#if RMT_PROFILE
    nd.act = real(1);                                     // a caller that knows its node overwrites the two
    nd.dtm = real(0);
#endif
#if RMT_NODE_X_CC
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) {                     // ctot, inv_ctot below: of the clamped state (no cmax)
        nd.x[i] = rmt_max(ys[i], RMT_EPS);                // :3899 (cs_i; scaled to x_i in _fin unless RMT_NODE_CS)
        nd.C[i] = nd.x[i] * m.cmax;                       // :3903 (MAX scaling; no reader here: removed)
        ctot += nd.x[i];
    }
#else
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) {
        const real cc = rmt_max(ys[i], RMT_EPS);          // :3899
        nd.C[i] = cc * m.cmax;                            // :3903 (MAX scaling)
        ctot += nd.C[i];
    }
#endif
#if RMT_ISO
    nd.T = m.tf;
#else
    nd.T = ys[RMT_S] * m.tf + m.tf;                       // :3914
#endif
    return ctot * nd.T;
}

#ifndef RMT_NODE_RCP_MERGE
#define RMT_NODE_RCP_MERGE 1
#endif
__device__ __forceinline__ preal rmt_node_pre_fin(const RmtMember& m, RmtNode& nd, const real ctot, const real inv_ct_T) {
    // 1/sum(C) and 1/T from ONE reciprocal of their product (v_rcp_f64 issues at a quarter of the FMA rate and each
    // reciprocal carries two Newton steps: 3 multiplications instead of a second one; both factors are O(1)..O(1e3))
#if RMT_NODE_RCP_MERGE
    const real inv_ctot = inv_ct_T * nd.T;
    nd.invT = inv_ct_T * ctot;
    const real ict_T = inv_ct_T;
#else
    (void)inv_ct_T;
    const real inv_ctot = rmt_rcp(ctot);
    nd.invT = rmt_rcp(nd.T);
    const real ict_T = inv_ctot * nd.invT;
#endif
    (void)ict_T;
    real mw = real(0);
#if RMT_NODE_CS
    nd.ict = inv_ctot;
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) mw += nd.x[i] * RMT_MW[i];
    nd.M = real(0);
    const preal mot = preal(mw) * preal(ict_T);           // 1e3 M/T
    nd.MoT = real(mot);
    return preal(1) - m.alpha_k * mot;                    // (alpha_k carries the 1e-3: rmt_load_member)
#else
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) {
#if RMT_NODE_X_CC
        nd.x[i] = nd.x[i] * inv_ctot;                     // :3927
#else
        nd.x[i] = nd.C[i] * inv_ctot;                     // :3927
#endif
        mw += nd.x[i] * RMT_MW[i];
    }
    nd.M = mw * real(1e-3);                               // :3960  [kg/mol]
    // P[z+1] = P[z] + dz*(-(ergA*ergB + 1.75*rho*v^2/dp*ergD)),  rho = P*M/(R*T)   (:3964-3979)
    const preal mot = preal(nd.M) * preal(nd.invT);
    nd.MoT = real(mot);
    return preal(1) - m.alpha_k * mot;
#endif
}

__device__ __forceinline__ preal rmt_node_pre(const RmtMember& m, const real* __restrict__ ys,
                                              RmtNode& nd) {
    real ctot;
    const real ct_T = rmt_node_pre_sum(m, ys, nd, ctot);
#if RMT_NODE_RCP_MERGE
    return rmt_node_pre_fin(m, nd, ctot, rmt_rcp(ct_T));
#else
    return rmt_node_pre_fin(m, nd, ctot, real(0));
#endif
}

// Phase B (pressure known): kinetics, species source, Cp, heat of reaction, wall exchange,
// upwind balances.  pbHomoReactor.py:3989-4128.  `up` = clamped state of node z-1 (or inlet).
template <typename FL, bool HAVE_R = false, typename KC = rmt_nocache_t, int KMODE = 0>
__device__ __forceinline__ void rmt_node_post(const RmtMember& m, const RmtNode& nd,
                                              const real* __restrict__ ys,
                                              const real* __restrict__ up, const preal Pz,
                                              real* __restrict__ k, FL& flag, const real* __restrict__ rin = nullptr,
                                              KC* kc = nullptr) {
    // A caller with a cache gets the unit's rmt_kinetics_node where there is one (plan.Mechanism.node_kinetics: literal
    // prefactors and FM inside the cached constants, the gain's reciprocal from the rate laws' division group); a caller
    // without one the plain rmt_kinetics - the plain twin of a caching stepper returns bit for bit what a cache-less
    // build of the same geometry returns.
    constexpr bool KNODE = KC::enabled && !HAVE_R && (RMT_KIN_NODE != 0);
    constexpr bool FMR = KNODE && (RMT_KIN_RATES_FM != 0);        // the rates arrive scaled by FM
    constexpr bool GDEN = KNODE && (RMT_KIN_GAIN_DEN != 0);       // 1/gden comes back from the rate function
#if RMT_NODE_CS
    const real P = real(Pz) * nd.ict;                     // P / sum cs: with x := cs the partial pressures are x_i P as before
#else
    const real P = real(Pz);
#endif
    // (1) convective parts first: after this the stage state and the upstream values are dead,
    //     which keeps the register footprint of the kinetics small.
#if RMT_NODE_CONV_FOLD
    const real conv = m.f1 * m.inv_dz;
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) {
        // FMR: only the difference now, k_i = conv (up_i - y_i) + src_i in one fma behind the rates
        if constexpr (FMR) k[i] = up[i] - ys[i];
        else k[i] = conv * (up[i] - ys[i]);                             // :4086-4098, convective term
    }
#else
#pragma unroll
    for (int i = 0; i < RMT_S; ++i)
        k[i] = -m.f1 * ((ys[i] - up[i]) * m.inv_dz);                    // :4086-4098, convective term
#endif
#if !RMT_ISO
    const real T = nd.T;
#if RMT_NODE_CONV_FOLD
    k[RMT_S] = (m.ft * m.inv_dz) * (up[RMT_S] - ys[RMT_S]);             // :4104-4116
#else
    k[RMT_S] = -m.ft * ((ys[RMT_S] - up[RMT_S]) * m.inv_dz);            // :4104-4116
#endif
    // (2) everything of the energy balance that does not need the rates
    real hq[RMT_R];
    real cpm = real(0);
    {
        real cpbar[RMT_S];
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) {
            cpbar[i] = rmt_cp_mean(i, T);                               // rmtThermo.py:52-75
            cpm += nd.x[i] * cpbar[i];                                  // :4013
        }
        real dcp[RMT_R];
        rmt_reaction_dcp(cpbar, dcp);                                   // sparse nu cpbar
#pragma unroll
        for (int q = 0; q < RMT_R; ++q) hq[q] = dcp[q] * (T - RMT_TREF) + RMT_DH25[q];   // :4025-4028
    }
#if RMT_PROFILE
    const real qm = (m.tm == real(0)) ? real(0) : (FMR ? m.qm_kf : m.ua) * ((m.tm + nd.dtm) - T);   // coolant of this zone
#else
    const real qm = (m.tm == real(0)) ? real(0) : (FMR ? m.qm_kf : m.ua) * (m.tm - T);    // rmtUtility.py:438-445
#endif
    // const_T2/GaHeCoTe0 (:4077, 4118) = F1/(GaHeCoTe0 rho* Cp*), rho* = P M/(R T GaDe0) (:3964-3966),
    // Cp* = Cp/Cp0 (:4016): the four per-reactor constants arrive as ONE (member field GAIN_K; m.gain_k / gain_kf: with the
    // factors of the cuts, rmt_load_member).  RMT_NODE_CS: P is P / sum cs, MoT is 1e3 M/T and cpm is sum cs_i cpbar_i -
    // the product is 1e3 times the plain one
    const real gden = (P * nd.MoT) * cpm;
    real ginv = real(0);
    if constexpr (!GDEN) ginv = rmt_rcp(gden);
#endif
    // (3) kinetics and the source terms
    real r[RMT_R];
    if (HAVE_R) {                 // rates already evaluated (together with their partials, by rmt_node_jac)
#pragma unroll
        for (int q = 0; q < RMT_R; ++q) r[q] = rin[q];
    } else {
        if constexpr (KC::enabled) {      // :3989-3992; KMODE 2: the temperature-only constants from the node's cache
#if RMT_KIN_NODE
#if RMT_KIN_RATES_FM
#define RMT_KIN_NODE_FM , m.inv_macote
#else
#define RMT_KIN_NODE_FM
#endif
#if RMT_KIN_GAIN_DEN
            rmt_kinetics_node<FL, KC, KMODE>(nd.T, nd.invT, P, nd.x, nd.C, m.user, r, flag, *kc RMT_KIN_NODE_FM, gden, ginv);
#else
            rmt_kinetics_node<FL, KC, KMODE>(nd.T, nd.invT, P, nd.x, nd.C, m.user, r, flag, *kc RMT_KIN_NODE_FM);
#endif
#undef RMT_KIN_NODE_FM
#else
            rmt_kinetics<FL, KC, KMODE>(nd.T, nd.invT, P, nd.x, nd.C, m.user, r, flag, *kc);
#endif
        } else {
            rmt_nocache_t nc;
            rmt_kinetics(nd.T, nd.invT, P, nd.x, nd.C, m.user, r, flag, nc);    // :3989-3992
        }
#if RMT_PROFILE
        // catalyst activity: every rate of this node, whichever rate function returned it (with FMR they carry FM as well).
        // Rates handed in (HAVE_R) come from rmt_node_jac, which has scaled them already
#pragma unroll
        for (int q = 0; q < RMT_R; ++q) r[q] *= nd.act;
#endif
    }
    real src[RMT_S];
    rmt_species_source(r, src);                                         // :4000 (sparse nu^T r)
    const real fm = m.inv_macote;                                       // member field FM = F1/GaMaCoTe0
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) {
#if RMT_NODE_CONV_FOLD
        if constexpr (FMR) k[i] = conv * k[i] + src[i];                 // :4086-4098 (src carries FM)
        else k[i] += fm * src[i];                                       // :4098
#else
        if constexpr (FMR) k[i] += src[i];
        else k[i] += fm * src[i];
#endif
    }
#if !RMT_ISO
    const real gain = (FMR ? m.gain_kf : m.gain_k) * ginv;
    real qr = real(0);
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) qr += r[q] * hq[q];                 // :4032
    k[RMT_S] += gain * (qm - qr);                                       // :4118-4126 (FMR: qm and qr carry FM, gain 1/FM)
#endif
}

__device__ __forceinline__ preal rmt_pressure_next(const RmtMember& m, const preal a, const preal P) {
    return a * P + m.beta;                                // :3979
}

#if RMT_WITH_ROS4 || RMT_WITH_MARCH
#ifndef RMT_ROS_JAC_FD
#define RMT_ROS_JAC_FD 0         // 1: node Jacobian by V forward differences of the node function (the round-1 form)
#endif
// Analytic node Jacobian of the stiff stepper: a[r][c] = -d f_r / d y_c of rmt_node_post at frozen
// (P, upstream state), y = (c_1..c_S, theta).  Chain rule through C_j = cmax max(c_j, eps),
// x_i = C_i / sum C, T = Tf theta + Tf around the generated rmt_kinetics_jac (rates + their partials by
// T, x_i, C_i from symbolic differentiation of the lowered DAG, lowering.Lowered.gradient); the rest of the
// node function is differentiated by hand below, term by term as rmt_node_post writes it.
// ~700 fp64 operations for the DME mechanism against ~2100 of the V forward differences it replaces.
template <typename FL>
__device__ __forceinline__ void rmt_node_jac(const RmtMember& m, const RmtNode& nd, const real* __restrict__ ys,
                                             const preal Pz, real (&a)[RMT_V][RMT_V], real* __restrict__ rout,
                                             FL& flag) {
    const real P = real(Pz);
    real r[RMT_R], drdT[RMT_R], drdx[RMT_R][RMT_S], drdC[RMT_R][RMT_S];
    rmt_kinetics_jac(nd.T, nd.invT, P, nd.x, nd.C, m.user, r, drdT, drdx, drdC, flag);
#if RMT_PROFILE
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) r[q] *= nd.act;       // catalyst activity: the scaled rates leave in rout, G below
#endif
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) rout[q] = r[q];
    real ctot = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) ctot += nd.C[i];
    const real ict = rmt_rcp(ctot);
    real act[RMT_S];                                       // d C_j / d c_j: cmax where the clamp is inactive
#pragma unroll
    for (int j = 0; j < RMT_S; ++j) act[j] = (ys[j] > RMT_EPS) ? m.cmax * ict : real(0);
    // G[q][c] = d r_q / d y_c
    real G[RMT_R][RMT_V];
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
    const real conv = m.f1 * m.inv_dz;
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) a[i][i] += conv;
#if !RMT_ISO
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
    real qr = real(0), dqrT = real(0);
    real hq[RMT_R];
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) {
        hq[q] = dcp[q] * (T - RMT_TREF) + RMT_DH25[q];
        qr += r[q] * hq[q];
        dqrT += G[q][RMT_S] * hq[q] + r[q] * (m.tf * (dcp[q] + (T - RMT_TREF) * ddcp[q]));
    }
    const bool wall = !(m.tm == real(0));
#if RMT_PROFILE
    const real qm = wall ? m.ua * ((m.tm + nd.dtm) - T) : real(0);
#else
    const real qm = wall ? m.ua * (m.tm - T) : real(0);
#endif
    const real dqmT = wall ? -(m.ua * m.tf) : real(0);
    const real icpm = rmt_rcp(cpm);
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
#endif
}
#endif   // RMT_WITH_ROS4 || RMT_WITH_MARCH

