// ------------------------------------------------------------------ steady-state models M7 and M1: node functions
// The homogeneous steady packed-bed models of PackedBedReactorClass that take the user's reaction-rate lambdas, the
// dimensional siblings of N1: ODEs along the bed, integrated by the reference with solve_ivp (LSODA) on
// t_eval = linspace(0, ReLe, n).  Here rmt_n1_ros4 integrates them in the scaled length z* = z/ReLe on [0, 1] with
// the bodies below of rmt_n1_init / rmt_n1_rhs / rmt_n1_rhs_jac (RMT_SS_MODEL 7 or 1; model N1 is 22_node_n1.inc).
// Both call the rate lambdas with (T, P, MoFri, CoSpi) in K, Pa and mol/m^3, unscaled (pbReactor.py:507-510,
// :465-470), and use the feed's mixture-viscosity in Ergun with GaDe = MiMoWe*CoSp (rmtThermo.py:338-350).
#if RMT_SS_MODEL == 7 || RMT_SS_MODEL == 1
#if RMT_ISO
#error "the steady models M7 and M1 are non-iso-thermal"
#endif
#define RMT_RGAS real(8.314472)          // PyREMOT/core/constants.py:8

#if RMT_SS_MODEL == 7
// ---- model M7 = PackedBedReactorClass.runM3 / modelEquationM3 (pbReactor.py:1170-1369, :1371-1575)
// unknowns u = [c_1..c_S, theta, p] with C_i = CMAX c_i [mol/m^3], T = T0 (1 + theta), P = P0 p; z* = z/ReLe.
// member row (doubles, host: plan.member_constants_m7):
//   0 CMAX = max SpCoi0       1 T0          2 P0          3 SPCO0 = sum SpCoi0
//   4 ERGA = ReLe/P0 150 GaMiVi ergB/PaDi^2   (times SuGaVe)          5 ERGC = ReLe/P0 1.75 ergD/PaDi (times GaDe SuGaVe^2)
//   6 INGAVE0 = VoFlRa0/(CrSeAr BeVoFr)       7 EPS = BeVoFr          8 KC = ReLe/CMAX        9 KT = ReLe/T0
//   10 UA = OvHeTrCo EfHeTrAr                 11 TM = MeTe            16.. CIN = SpCoi0/CMAX  16+S.. user parameters
#define RMT_V1 (RMT_S + 2)
#define M7_CMAX 0
#define M7_T0 1
#define M7_P0 2
#define M7_SPCO0 3
#define M7_ERGA 4
#define M7_ERGC 5
#define M7_INGAVE0 6
#define M7_EPS 7
#define M7_KC 8
#define M7_KT 9
#define M7_UA 10
#define M7_TM 11
#define M7_CIN 16
// IV = [SpCoi0, T, P] (:1244-1247)
__device__ __forceinline__ void rmt_n1_init(const double* __restrict__ mr, real (&u)[RMT_V1]) {
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) u[i] = real(mr[M7_CIN + i]);
    u[RMT_S] = real(0);
    u[RMT_S + 1] = real(1);
}
template <typename FL>
__device__ __forceinline__ void rmt_n1_rhs(const double* __restrict__ mr, const real (&u)[RMT_V1],
                                           real (&du)[RMT_V1], FL& flag) {
    const real cmax = real(mr[M7_CMAX]), t0 = real(mr[M7_T0]), p0 = real(mr[M7_P0]);
    real C[RMT_S], x[RMT_S];
    real ctot = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { C[i] = u[i] * cmax; ctot += C[i]; }                 // CoSp, :1451-1458
    const real inv_ctot = rmt_rcp(ctot);
    real mw = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { x[i] = C[i] * inv_ctot; mw += x[i] * RMT_MW[i]; }   // :1461-1462
    const real T = u[RMT_S] * t0 + t0;
    const real P = u[RMT_S + 1] * p0;
    // calGaVeFromEOS(InGaVe0, SpCo0, CoSp, P0, P): no temperature factor (rmtUtility.py:405-421); SuGaVe = InGaVe eps
    const real su = real(mr[M7_INGAVE0]) * rmt_div(ctot, real(mr[M7_SPCO0])) * rmt_div(p0, P) * real(mr[M7_EPS]);
    const real mofl = ctot * su;                                                          // MoFl, :1471-1477
    const real gade = mw * real(1e-3) * ctot;                                             // :1483-1486
    du[RMT_S + 1] = -(real(mr[M7_ERGA]) * su + real(mr[M7_ERGC]) * gade * su * su);        // Ergun, :1493-1497
    real r[RMT_R], U[RMT_NU > 0 ? RMT_NU : 1];
    rmt_n1_user(mr, U);
    rmt_nocache_t nc;
    rmt_kinetics(T, rmt_rcp(T), P, x, C, U, r, flag, nc);                                 // :1507-1510
    real src[RMT_S];
    rmt_species_source(r, src);                                                           // :1518-1519
    const real iv = rmt_rcp(su);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) du[i] = real(mr[M7_KC]) * src[i] * iv;                // dC_i/dz = ri/SuGaVe, :1563-1565
    real cpbar[RMT_S], cpm = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { cpbar[i] = rmt_cp_mean(i, T); cpm += x[i] * cpbar[i]; }  // :1527-1531
    real dcp[RMT_R];
    rmt_reaction_dcp(cpbar, dcp);
    real qr = real(0);
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) qr += r[q] * (dcp[q] * (T - RMT_TREF) + RMT_DH25[q]);  // OvHeReT, :1536-1540
    const real qm = real(mr[M7_UA]) * (real(mr[M7_TM]) - T);                               // Qm = Ua (Tm - T), :1545-1553
    du[RMT_S] = real(mr[M7_KT]) * rmt_div(qm - qr, mofl * cpm);                             // :1560, :1568
}

#if RMT_WITH_N1
// rmt_n1_rhs AND a[r][c] = -d du_r / d u_c (analytic; the rates' partials come from rmt_kinetics_jacp).  By column c
// (species j, theta at S, p at S+1), with C_j = CMAX c_j:
//   d ln su/dc_j = CMAX/CoSp, d ln su/dp = -1/p;    d ln GaDe/dc_j = CMAX MW_j 1e-3/GaDe;    MoFl = CoSp su
//   f_i = KC src_i/su          df_i = KC src_i(dr)/su - f_i dlnsu
//   f_p = -(A su + B GaDe su^2)  df_p = -(A su dlnsu + B GaDe su^2 (dlnGaDe + 2 dlnsu))
//   f_T = KT (Qm - Qr)/(MoFl cpm)  df_T = KT (dQm - dQr)/(MoFl cpm) - f_T (dlnMoFl + dlncpm)
template <typename FL>
__device__ __forceinline__ void rmt_n1_rhs_jac(const double* __restrict__ mr, const real (&u)[RMT_V1],
                                               real (&du)[RMT_V1], real (&a)[RMT_V1][RMT_V1], FL& flag) {
    const real cmax = real(mr[M7_CMAX]), t0 = real(mr[M7_T0]), p0 = real(mr[M7_P0]);
    real C[RMT_S], x[RMT_S];
    real ctot = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { C[i] = u[i] * cmax; ctot += C[i]; }
    const real inv_ctot = rmt_rcp(ctot);
    real mw = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { x[i] = C[i] * inv_ctot; mw += x[i] * RMT_MW[i]; }
    const real T = u[RMT_S] * t0 + t0;
    const real P = u[RMT_S + 1] * p0;
    const real su = real(mr[M7_INGAVE0]) * rmt_div(ctot, real(mr[M7_SPCO0])) * rmt_div(p0, P) * real(mr[M7_EPS]);
    const real mofl = ctot * su;
    const real gade = mw * real(1e-3) * ctot;
    const real ea = real(mr[M7_ERGA]) * su, ec = real(mr[M7_ERGC]) * gade * su * su;
    du[RMT_S + 1] = -(ea + ec);
    real r[RMT_R], drdT[RMT_R], drdx[RMT_R][RMT_S], drdC[RMT_R][RMT_S], drdP[RMT_R], U[RMT_NU > 0 ? RMT_NU : 1];
    rmt_n1_user(mr, U);
    rmt_kinetics_jacp(T, rmt_rcp(T), P, x, C, U, r, drdT, drdx, drdC, drdP, flag);
    real src[RMT_S];
    rmt_species_source(r, src);
    const real iv = rmt_rcp(su), kc = real(mr[M7_KC]);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) du[i] = kc * src[i] * iv;
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
        dqrT += r[q] * (t0 * (dcp[q] + (T - RMT_TREF) * ddcp[q]));
    }
    const real ua = real(mr[M7_UA]);
    const real qm = ua * (real(mr[M7_TM]) - T);
    const real iD = rmt_rcp(mofl * cpm), kt = real(mr[M7_KT]);
    du[RMT_S] = kt * rmt_div(qm - qr, mofl * cpm);
    // logarithmic derivatives by column
    const real ip = rmt_rcp(u[RMT_S + 1]), icpm = rmt_rcp(cpm), igade = rmt_rcp(gade);
    real dlnsu[RMT_V1], dlnrho[RMT_V1], dlnD[RMT_V1];
#pragma unroll
    for (int j = 0; j < RMT_S; ++j) {
        const real cj = cmax * inv_ctot;
        dlnsu[j] = cj;
        dlnrho[j] = cmax * real(1e-3) * RMT_MW[j] * igade;
        dlnD[j] = real(2) * cj + cj * (cpbar[j] - cpm) * icpm;           // d ln(MoFl cpm)
    }
    dlnsu[RMT_S] = real(0);
    dlnrho[RMT_S] = real(0);
    dlnD[RMT_S] = t0 * dcpm * icpm;
    dlnsu[RMT_S + 1] = -ip;
    dlnrho[RMT_S + 1] = real(0);
    dlnD[RMT_S + 1] = -ip;
    // G[q][c] = d r_q / d u_c
    real G[RMT_R][RMT_V1];
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) {
        real sx = real(0);
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) sx += x[i] * drdx[q][i];
#pragma unroll
        for (int j = 0; j < RMT_S; ++j) G[q][j] = cmax * (drdC[q][j] + (drdx[q][j] - sx) * inv_ctot);
        G[q][RMT_S] = t0 * drdT[q];
        G[q][RMT_S + 1] = p0 * drdP[q];
    }
#pragma unroll
    for (int c = 0; c < RMT_V1; ++c) {
        real col[RMT_R], dsrc[RMT_S];
#pragma unroll
        for (int q = 0; q < RMT_R; ++q) col[q] = G[q][c];
        rmt_species_source(col, dsrc);
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) a[i][c] = -(kc * dsrc[i] * iv - du[i] * dlnsu[c]);
        a[RMT_S + 1][c] = ea * dlnsu[c] + ec * (dlnrho[c] + real(2) * dlnsu[c]);
        real dqr = real(0), dqm = real(0);
#pragma unroll
        for (int q = 0; q < RMT_R; ++q) dqr += col[q] * hq[q];
        if (c == RMT_S) {
            dqr += dqrT;
            dqm = -(ua * t0);
        }
        a[RMT_S][c] = -(kt * (dqm - dqr) * iD - du[RMT_S] * dlnD[c]);
    }
}
#endif   // RMT_WITH_N1

#else    // RMT_SS_MODEL == 1
// ---- model M1 = PackedBedReactorClass.runM1 / modelEquationM1 (pbReactor.py:141-352, :354-547)
// unknowns u = [f_1..f_S, phi, theta, p] with F_i = FTOT f_i [mol/s], F* = FL0 phi [mol/m^2.s], T = T0 (1 + theta),
// P = P0 p; z* = z/ReLe.
// member row (doubles, host: plan.member_constants_m1):
//   0 FTOT = sum F_i(0)       1 T0          2 P0          3 FL0 = F*(0) = MoFlRa/CrSeAr
//   4 ERGA = ReLe/P0 150 GaMiVi ergB/PaDi^2   (times SuGaVe)          5 ERGC = ReLe/P0 1.75 ergD/PaDi (times GaDe SuGaVe^2)
//   6 EPS = BeVoFr            7 KF = ReLe CrSeAr/FTOT                 8 KFL = ReLe/FL0        9 KT = ReLe/T0
//   10 UA = OvHeTrCo 4/ReInDi (EfHeTrAr overridden, :211)             11 TM = MeTe
//   16.. CIN = F_i(0)/FTOT    16+S.. user parameters
#define RMT_V1 (RMT_S + 3)
#define SM1_FTOT 0
#define SM1_T0 1
#define SM1_P0 2
#define SM1_FL0 3
#define SM1_ERGA 4
#define SM1_ERGC 5
#define SM1_EPS 6
#define SM1_KF 7
#define SM1_KFL 8
#define SM1_KT 9
#define SM1_UA 10
#define SM1_TM 11
#define SM1_CIN 16
// IV = [MoFlRai, MoFl, T, P] (:223-227)
__device__ __forceinline__ void rmt_n1_init(const double* __restrict__ mr, real (&u)[RMT_V1]) {
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) u[i] = real(mr[SM1_CIN + i]);
    u[RMT_S] = real(1);
    u[RMT_S + 1] = real(0);
    u[RMT_S + 2] = real(1);
}
template <typename FL>
__device__ __forceinline__ void rmt_n1_rhs(const double* __restrict__ mr, const real (&u)[RMT_V1],
                                           real (&du)[RMT_V1], FL& flag) {
    const real t0 = real(mr[SM1_T0]), p0 = real(mr[SM1_P0]);
    real fs = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) fs += u[i];                                           // MoFlRa / FTOT, :423
    const real T = u[RMT_S + 1] * t0 + t0;
    const real P = u[RMT_S + 2] * p0;
    // calVolumetricFlowrateIG + calConcentrationIG: C_i = F_i/((R T/P) sum F) (rmtThermo.py:315-335)
    const real ivol = rmt_rcp(rmt_div(RMT_RGAS * T, P) * fs);
    real C[RMT_S], x[RMT_S];
    real ctot = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { C[i] = u[i] * ivol; ctot += C[i]; }                 // :426-431
    const real inv_ctot = rmt_rcp(ctot);
    real mw = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { x[i] = C[i] * inv_ctot; mw += x[i] * RMT_MW[i]; }   // :434, :443
    const real fl = u[RMT_S] * real(mr[SM1_FL0]);
    // calSuperficialGasVelocityFromEOS(MoFl, P, T) = MoFl T R/P (rmtUtility.py:343-357); SuGaVe = InGaVe eps, :438-440
    const real su = rmt_div(fl * T * RMT_RGAS, P) * real(mr[SM1_EPS]);
    const real gade = mw * real(1e-3) * ctot;                                             // :446
    du[RMT_S + 2] = -(real(mr[SM1_ERGA]) * su + real(mr[SM1_ERGC]) * gade * su * su);     // Ergun, :450-454
    real r[RMT_R], U[RMT_NU > 0 ? RMT_NU : 1];
    rmt_n1_user(mr, U);
    rmt_nocache_t nc;
    rmt_kinetics(T, rmt_rcp(T), P, x, C, U, r, flag, nc);                                 // :465-471
    real src[RMT_S];
    rmt_species_source(r, src);                                                           // :486-487
    real ovr = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { du[i] = real(mr[SM1_KF]) * src[i]; ovr += src[i]; }  // dF_i/dz = CrSeAr ri, :532-534
    du[RMT_S] = real(mr[SM1_KFL]) * ovr;                                                  // dF*/dz = sum ri, :490, :536
    real cpbar[RMT_S], cpm = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { cpbar[i] = rmt_cp_mean(i, T); cpm += x[i] * cpbar[i]; }  // :495-499
    real dcp[RMT_R];
    rmt_reaction_dcp(cpbar, dcp);
    real qr = real(0);
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) qr += r[q] * (dcp[q] * (T - RMT_TREF) + RMT_DH25[q]);  // OvHeReT, :504-508
    // calHeatExchangeBetweenReactorMedium: 0 when Tm == 0 (rmtUtility.py:424-452)
    const real tm = real(mr[SM1_TM]);
    const real qm = (tm == real(0)) ? real(0) : real(mr[SM1_UA]) * (tm - T);
    du[RMT_S + 1] = real(mr[SM1_KT]) * rmt_div(qm - qr, fl * cpm);                        // const_T1 = MoFl Cp, :528, :540
}

#if RMT_WITH_N1
// rmt_n1_rhs AND a[r][c] = -d du_r / d u_c (analytic).  By column c (species j, phi at S, theta at S+1, p at S+2), with
// K = P/(R T), C_i = K x_i, x_i = f_i/fs:
//   dC_i/df_j = (delta_ij - x_i) K/fs,  dC_i/dtheta = -C_i T0/T,  dC_i/dp = C_i/p;  dx_i/df_j = (delta_ij - x_i)/fs
//   d ln su: 1/phi, T0/T, -1/p;   d ln GaDe = d ln(K M): (MW_j 1e-3 - M)/(M fs), -T0/T, 1/p
//   f_i = KF src_i,  f_phi = KFL sum src,  f_T = KT (Qm - Qr)/(F* cpm),  f_p = -(A su + B GaDe su^2)
template <typename FL>
__device__ __forceinline__ void rmt_n1_rhs_jac(const double* __restrict__ mr, const real (&u)[RMT_V1],
                                               real (&du)[RMT_V1], real (&a)[RMT_V1][RMT_V1], FL& flag) {
    const real t0 = real(mr[SM1_T0]), p0 = real(mr[SM1_P0]);
    real fs = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) fs += u[i];
    const real T = u[RMT_S + 1] * t0 + t0;
    const real P = u[RMT_S + 2] * p0;
    const real ivol = rmt_rcp(rmt_div(RMT_RGAS * T, P) * fs);
    real C[RMT_S], x[RMT_S];
    real ctot = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { C[i] = u[i] * ivol; ctot += C[i]; }
    const real inv_ctot = rmt_rcp(ctot);
    real mw = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { x[i] = C[i] * inv_ctot; mw += x[i] * RMT_MW[i]; }
    const real fl = u[RMT_S] * real(mr[SM1_FL0]);
    const real su = rmt_div(fl * T * RMT_RGAS, P) * real(mr[SM1_EPS]);
    const real gade = mw * real(1e-3) * ctot;
    const real ea = real(mr[SM1_ERGA]) * su, ec = real(mr[SM1_ERGC]) * gade * su * su;
    du[RMT_S + 2] = -(ea + ec);
    real r[RMT_R], drdT[RMT_R], drdx[RMT_R][RMT_S], drdC[RMT_R][RMT_S], drdP[RMT_R], U[RMT_NU > 0 ? RMT_NU : 1];
    rmt_n1_user(mr, U);
    rmt_kinetics_jacp(T, rmt_rcp(T), P, x, C, U, r, drdT, drdx, drdC, drdP, flag);
    real src[RMT_S];
    rmt_species_source(r, src);
    const real kf = real(mr[SM1_KF]), kfl = real(mr[SM1_KFL]), kt = real(mr[SM1_KT]);
    real ovr = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) { du[i] = kf * src[i]; ovr += src[i]; }
    du[RMT_S] = kfl * ovr;
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
        dqrT += r[q] * (t0 * (dcp[q] + (T - RMT_TREF) * ddcp[q]));
    }
    const real tm = real(mr[SM1_TM]);
    const bool wall = !(tm == real(0));
    const real qm = wall ? real(mr[SM1_UA]) * (tm - T) : real(0);
    const real iD = rmt_rcp(fl * cpm);
    du[RMT_S + 1] = kt * rmt_div(qm - qr, fl * cpm);
    // logarithmic derivatives by column
    const real ifs = rmt_rcp(fs), iphi = rmt_rcp(u[RMT_S]), ip = rmt_rcp(u[RMT_S + 2]), tT = t0 * rmt_rcp(T);
    const real M = mw * real(1e-3), iM = rmt_rcp(M), icpm = rmt_rcp(cpm);
    real dlnsu[RMT_V1], dlnrho[RMT_V1], dlnD[RMT_V1];
#pragma unroll
    for (int j = 0; j < RMT_S; ++j) {
        dlnsu[j] = real(0);
        dlnrho[j] = (real(1e-3) * RMT_MW[j] - M) * iM * ifs;
        dlnD[j] = (cpbar[j] - cpm) * icpm * ifs;                         // d ln(F* cpm)
    }
    dlnsu[RMT_S] = iphi;
    dlnrho[RMT_S] = real(0);
    dlnD[RMT_S] = iphi;
    dlnsu[RMT_S + 1] = tT;
    dlnrho[RMT_S + 1] = -tT;
    dlnD[RMT_S + 1] = t0 * dcpm * icpm;
    dlnsu[RMT_S + 2] = -ip;
    dlnrho[RMT_S + 2] = ip;
    dlnD[RMT_S + 2] = real(0);
    // G[q][c] = d r_q / d u_c
    real G[RMT_R][RMT_V1];
#pragma unroll
    for (int q = 0; q < RMT_R; ++q) {
        real sx = real(0), sC = real(0);
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) { sx += x[i] * drdx[q][i]; sC += C[i] * drdC[q][i]; }
#pragma unroll
        for (int j = 0; j < RMT_S; ++j) G[q][j] = (drdx[q][j] - sx) * ifs + drdC[q][j] * ivol - sC * ifs;
        G[q][RMT_S] = real(0);
        G[q][RMT_S + 1] = t0 * drdT[q] - sC * tT;
        G[q][RMT_S + 2] = p0 * drdP[q] + sC * ip;
    }
#pragma unroll
    for (int c = 0; c < RMT_V1; ++c) {
        real col[RMT_R], dsrc[RMT_S];
#pragma unroll
        for (int q = 0; q < RMT_R; ++q) col[q] = G[q][c];
        rmt_species_source(col, dsrc);
        real dsum = real(0);
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) { a[i][c] = -(kf * dsrc[i]); dsum += dsrc[i]; }
        a[RMT_S][c] = -(kfl * dsum);
        a[RMT_S + 2][c] = ea * dlnsu[c] + ec * (dlnrho[c] + real(2) * dlnsu[c]);
        real dqr = real(0), dqm = real(0);
#pragma unroll
        for (int q = 0; q < RMT_R; ++q) dqr += col[q] * hq[q];
        if (c == RMT_S + 1) {
            dqr += dqrT;
            dqm = wall ? -(real(mr[SM1_UA]) * t0) : real(0);
        }
        a[RMT_S + 1][c] = -(kt * (dqm - dqr) * iD - du[RMT_S + 1] * dlnD[c]);
    }
}
#endif   // RMT_WITH_N1
#endif   // RMT_SS_MODEL 7 / 1
#endif   // RMT_SS_MODEL == 7 || RMT_SS_MODEL == 1
