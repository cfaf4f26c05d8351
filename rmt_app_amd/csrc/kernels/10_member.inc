// Cache argument of the generated kinetics (lowering.Lowered.kcache_plan): a caller without a cache passes this
// and the cached section is discarded at compile time; the on-chip steppers pass RmtKC (30_lanes_links.inc).
template <int V_> struct rmt_int_t { static constexpr int value = V_; };
struct rmt_nocache_t {
    static constexpr bool enabled = false;
    static constexpr bool valid = true;
    __device__ __forceinline__ real get(const int) const { return real(0); }
    __device__ __forceinline__ void put(const int, const real) const {}
    __device__ __forceinline__ void leave(const bool) const {}
};

RMT_KINETICS_SOURCE

// Two cuts of the node function's multiplications (each its own switch, default on; profiles/node_cuts.md):
//  RMT_NODE_CONV_FOLD     the convective term as (F1 inv_dz)(up - y): the product is a per-reactor constant - a literal
//                         where the member fields are literals (RMT_MC_*), else formed once per call
//  RMT_NODE_X_FROM_STATE  x_i = cc_i / sum cc from the clamped state itself (C_i = cmax cc_i scales numerator and
//                         denominator alike), only where the kinetics never read C (RMT_KIN_USES_C 0, from the lowering)
//                         and the unit has no rmt_node_jac (the stiff stepper differentiates x_i = C_i / sum C as written)
#ifndef RMT_NODE_CONV_FOLD
#define RMT_NODE_CONV_FOLD 1
#endif
#ifndef RMT_NODE_X_FROM_STATE
#define RMT_NODE_X_FROM_STATE 1
#endif
#ifndef RMT_KIN_USES_C
#define RMT_KIN_USES_C 1
#endif
#define RMT_NODE_X_CC (RMT_NODE_X_FROM_STATE && !RMT_KIN_USES_C && !RMT_WITH_ROS4 && !RMT_WITH_MARCH)
// Four more (profiles/node_cuts.md, DESIGN.md section 3j), each its own switch, default on:
//  RMT_NODE_NO_X          no mole fractions at all where the rates depend on (x, P) only through the partial pressures
//                         x_i P (RMT_KIN_XP_INVARIANT, from the lowering) and under the conditions of RMT_NODE_X_CC:
//                         nd.x holds the clamped state cs_i, the kinetics get P / sum cs, the mixture sums run over cs_i
//                         (M/T = (sum cs_i MW_i) / (sum cs T), the 1e-3 in alpha_k and the gain constant; the factor
//                         1/sum cs of cpm cancels against the one of P in the gain)
//  RMT_KC_FOLD, RMT_KIN_FOLD_FM, RMT_KIN_GAIN_RCP   switches of the generator (plan.Mechanism.node_kinetics), which
//                         announces rmt_kinetics_node by RMT_KIN_NODE / RMT_KIN_RATES_FM / RMT_KIN_GAIN_DEN
//  RMT_NODE_PAIR_RCP      one reciprocal for the two nodes of a lane (40_rhs_block.inc)
#ifndef RMT_NODE_NO_X
#define RMT_NODE_NO_X 1
#endif
#ifndef RMT_KIN_XP_INVARIANT
#define RMT_KIN_XP_INVARIANT 0
#endif
#define RMT_NODE_CS (RMT_NODE_NO_X && RMT_KIN_XP_INVARIANT && RMT_NODE_X_CC && !RMT_ISO)
#ifndef RMT_KIN_NODE
#define RMT_KIN_NODE 0
#define RMT_KIN_RATES_FM 0
#define RMT_KIN_GAIN_DEN 0
#endif
#ifndef RMT_NODE_PAIR_RCP
#define RMT_NODE_PAIR_RCP 1
#endif

// ------------------------------------------------------------------ per-member constants
struct RmtMember {
    real cmax, tf, theta_in, rho_k, inv_cp0, f1, ft, inv_dz, inv_macote, inv_hecote, ua, tm;
    real gain_k, gain_kf, qm_kf;     // inv_hecote and ua with the constant factors of the node function's cuts (rmt_load_member)
    preal p0, alpha_k, beta;
    real cin[RMT_S];
    real user[RMT_NU > 0 ? RMT_NU : 1];
#if RMT_PROFILE
    // axial profile (12_profile.inc): the member's table [2][prof_n] = {activity a_n, coolant offset delta_n}, bound by the
    // kernel (rmt_profile_bind), and the two values of the node a per-lane march is solving (identity unless it sets them)
    const double* prof;
    int prof_n;
    real act, dtm;
#endif
};

// A member field whose value is identical for every reactor of the launch can be baked into the
// kernel as a literal (prelude: #define RMT_MC_<FIELD> value): literals are rematerialised with
// s_mov instead of occupying (and spilling) SGPRs for the whole time loop.
__device__ __forceinline__ void rmt_load_member(const double* __restrict__ row, RmtMember& m) {
#ifdef RMT_MC_CMAX
    m.cmax = real(RMT_MC_CMAX);
#else
    m.cmax = real(row[M_CMAX]);
#endif
#ifdef RMT_MC_TF
    m.tf = real(RMT_MC_TF);
#else
    m.tf = real(row[M_TF]);
#endif
#ifdef RMT_MC_THETA_IN
    m.theta_in = real(RMT_MC_THETA_IN);
#else
    m.theta_in = real(row[M_THETA_IN]);
#endif
#ifdef RMT_MC_RHO_K
    m.rho_k = real(RMT_MC_RHO_K);
#else
    m.rho_k = real(row[M_RHO_K]);
#endif
#ifdef RMT_MC_INV_CP0
    m.inv_cp0 = real(RMT_MC_INV_CP0);
#else
    m.inv_cp0 = real(row[M_INV_CP0]);
#endif
#ifdef RMT_MC_F1
    m.f1 = real(RMT_MC_F1);
#else
    m.f1 = real(row[M_F1]);
#endif
#ifdef RMT_MC_FT
    m.ft = real(RMT_MC_FT);
#else
    m.ft = real(row[M_FT]);
#endif
#ifdef RMT_MC_INV_DZ
    m.inv_dz = real(RMT_MC_INV_DZ);
#else
    m.inv_dz = real(row[M_INV_DZ]);
#endif
#ifdef RMT_MC_INV_MACOTE
    m.inv_macote = real(RMT_MC_INV_MACOTE);
#else
    m.inv_macote = real(row[M_INV_MACOTE]);
#endif
#ifdef RMT_MC_INV_HECOTE
    m.inv_hecote = real(RMT_MC_INV_HECOTE);
#else
    m.inv_hecote = real(row[M_INV_HECOTE]);
#endif
#ifdef RMT_MC_UA
    m.ua = real(RMT_MC_UA);
#else
    m.ua = real(row[M_UA]);
#endif
#ifdef RMT_MC_TM
    m.tm = real(RMT_MC_TM);
#else
    m.tm = real(row[M_TM]);
#endif
#ifdef RMT_MC_P0
    m.p0 = RMT_MC_P0;
#else
    m.p0 = row[M_P0];
#endif
#ifdef RMT_MC_ALPHA_K
    m.alpha_k = RMT_MC_ALPHA_K;
#else
    m.alpha_k = row[M_ALPHA_K];
#endif
#ifdef RMT_MC_BETA
    m.beta = RMT_MC_BETA;
#else
    m.beta = row[M_BETA];
#endif
    // constant factors of the node function's cuts, once per launch (all of them 1 with the cuts off):
    // RMT_NODE_CS        1e-3 of the mixture molar mass: out of the node's M/T into alpha_k and the gain constant gain_k
    // RMT_KIN_RATES_FM   callers with a cache get their rates scaled by FM: for them the wall term carries
    //                    it too (qm_kf = UA FM) and the gain 1/FM (gain_kf)
    m.gain_k = m.inv_hecote;
#if RMT_MODEL == 0 && RMT_NODE_CS
    m.alpha_k = m.alpha_k * preal(1e-3);
    m.gain_k = m.gain_k * real(1e3);
#endif
    m.gain_kf = m.gain_k;
    m.qm_kf = m.ua;
#if RMT_MODEL == 0 && RMT_KIN_RATES_FM
    m.gain_kf = m.gain_k / m.inv_macote;
    m.qm_kf = m.ua * m.inv_macote;
#endif
#ifdef RMT_MC_CIN
    {
        const double cin_[RMT_S] = RMT_MC_CIN;
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) m.cin[i] = real(cin_[i]);
    }
#else
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) m.cin[i] = real(row[M_CIN + i]);
#endif
#pragma unroll
    for (int k = 0; k < RMT_NU; ++k) m.user[k] = real(row[M_USER + k]);
#if RMT_NU == 0
    m.user[0] = real(0);
#endif
#if RMT_PROFILE
    m.prof = nullptr;
    m.prof_n = 0;
    m.act = real(1);
    m.dtm = real(0);
#endif
}

