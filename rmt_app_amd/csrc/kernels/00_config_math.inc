// =====================================================================================
// rmt N2 device template (gfx950 / CDNA4, wave64).  Compiled at run time by hipRTC after a
// host-generated prelude that defines:
//
//   RMT_S, RMT_R            species / reactions            RMT_ISO   1 = iso-thermal (V = S)
//   RMT_FP32                1 = state & kinetics in fp32   RMT_BLOCK threads per workgroup
//   RMT_NPT                 nodes per thread of the register-resident steppers
//   typedef ... real;       double or float
//   RMT_MW[S]               molecular weights [g/mol]
//   rmt_species_source(r,s) s = nu^T r, rmt_reaction_dcp(cp,d) d = nu cp   (sparse, unrolled)
//   rmt_cp_mean(i,T)        0.5*(Cp_i(Tref)+Cp_i(T)) with only the non-zero polynomial terms
//   RMT_DH25[R]             standard heats of reaction [J/mol]
//   rmt_kinetics(T,1/T,P,x,C,U,r,flag) lowered user rate lambdas (U = the reactor's user parameters)
//
// What it computes: the method-of-lines right-hand side of PyREMOT's model N2
// (modelEquationN2, PyREMOT/docs/pbHomoReactor.py:3706-4134; equations restated in SURVEY.md
// Appendix A) for one axial mesh node per lane (RMT_NPT consecutive nodes per lane), and
// explicit time steppers on top of it (RK4 tableau of PyREMOT/solvers/odeSolver.py:17-40;
// Dormand-Prince 5(4) with per-reactor step control).
//
// Layout: state y[E][V][N] (the reference's row-major (V,N) flattening per reactor, reactors
// stacked), per-member constants members[E][RMT_NM] (see M_* below).  One workgroup integrates
// one reactor: the sequential Ergun pressure march  P[z+1] = a_z P[z] + b  (:3979) is an affine
// prefix scan (wave shuffles + one LDS exchange per stage), the upwind neighbour z-1 comes from
// lane-1 (shuffle) or the previous wave (same LDS exchange).  No inter-workgroup communication.
// =====================================================================================

#define RMT_V (RMT_S + (RMT_ISO ? 0 : 1))
#ifndef RMT_MEMBER_LDS
#define RMT_MEMBER_LDS 0
#endif
#ifndef RMT_STAGE_UNROLL
#define RMT_STAGE_UNROLL 1
#endif
// Python-exception tests (log(<=0), x/0, exp overflow ...) run on RK stage 1 only by default: an
// exception inside a trial stage ends in a non-finite state (RMT_FLAG_NONFINITE; the lean division and exp
// turn an intermediate inf into NaN, so 1/(1+inf) does not come back finite) - but it is then reported as
// FloatingPointError, not as the OverflowError / ZeroDivisionError / ValueError the reference raises.
// RMT_CHECK_ALL_STAGES 1 (solver-config "strict-flags") tests every stage, like the reference's
// Python path raises wherever it happens (+8 % VALU instructions).
#ifndef RMT_CHECK_ALL_STAGES
#define RMT_CHECK_ALL_STAGES 0
#endif
// optional kernel families (their unrolled VxV linear algebra dominates the JIT time)
#ifndef RMT_WITH_ROS4
#define RMT_WITH_ROS4 0
#endif
#ifndef RMT_WITH_N1
#define RMT_WITH_N1 0
#endif
// RMT_WITH_MARCH: the steady-state march of model N2 (71_steady_march.inc, solver-config "initial"); brings the analytic
// node Jacobian of the stiff stepper (rmt_node_jac, rmt_kinetics_jac) without the stiff stepper's kernels
#ifndef RMT_WITH_MARCH
#define RMT_WITH_MARCH 0
#endif
// stiff stepper with ONE NODE ON FOUR LANES (61_ros4_quad.inc): set by the host for mechanisms wider than 8 variables
#ifndef RMT_ROS_QUAD
#define RMT_ROS_QUAD 0
#endif
// RMT_MODEL 0: the dimensionless dynamic model N2 (pbHomoReactor.py:3706-4134)
// RMT_MODEL 2: the dimensional dynamic model M2 (pbReactor.py:845-1165): same steppers, its own
//              node functions and a NONLINEAR pressure march (Newton on the affine scan)
#ifndef RMT_MODEL
#define RMT_MODEL 0
#endif
#if RMT_MODEL == 2 && RMT_ISO
#error "model M2 has no iso-thermal variant"
#endif
#ifndef RMT_M2_NEWTON
#define RMT_M2_NEWTON 3
#endif
#define RMT_NW (RMT_BLOCK / 64)
// per-reactor kinetic parameters: scalar reaction-rates.VARS entries that differ between the members of an
// ensemble (host: plan.Mechanism(params=...)); the generated kinetics read them as U[k]
#ifndef RMT_NU
#define RMT_NU 0
#endif
// RMT_FORCING 1 (solver-config "schedule", 11_forcing.inc): the member row grows by a tail of four doubles;
// RMT_FORCING 2 (the schedule also moves the feed composition): by S more, the slopes of the inlet values M_CIN
#ifndef RMT_FORCING
#define RMT_FORCING 0
#endif
// RMT_PROFILE 1 (solver-config "axial-profile", 12_profile.inc): catalyst activity and coolant offset per mesh node, read
// from a table beside the member rows; the rows themselves keep their layout
#ifndef RMT_PROFILE
#define RMT_PROFILE 0
#endif
#if RMT_FORCING == 2
#define RMT_NM (16 + RMT_S + RMT_NU + 4 + RMT_S)
#elif RMT_FORCING
#define RMT_NM (16 + RMT_S + RMT_NU + 4)
#else
#define RMT_NM (16 + RMT_S + RMT_NU)
#endif

#define RMT_FLAG_DOMAIN 1u
#define RMT_FLAG_DIV0 2u
#define RMT_FLAG_OVERFLOW 4u
#define RMT_FLAG_NONFINITE 8u
#define RMT_FLAG_STEP 16u
#define RMT_FLAG_PRESSURE 32u   // M2: Newton iteration of the pressure march did not converge

// member row layout (doubles); host side: rmt_app_amd/plan.py MEMBER_FIELDS
#define M_CMAX 0        // max(SpCoi0)                     [mol/m^3]
#define M_TF 1          // feed temperature                [K]
#define M_P0 2          // inlet pressure                  [Pa]
#define M_THETA_IN 3    // (T0-Tf)/Tf
#define M_ALPHA_K 4     // dz*1.75*vf^2*ergD/(dp*R):   a_z = 1 - ALPHA_K*M_z/T_z
#define M_BETA 5        // -dz*ergA*ergB
#define M_RHO_K 6       // 1/(R*GaDe0):                rho* = P*M/T*RHO_K
#define M_INV_CP0 7     // 1/GaCpMeanMix0
#define M_F1 8          // vf/(eps*zf)
#define M_FT 9          // vf/zf
#define M_INV_DZ 10     // N-1
#define M_INV_MACOTE 11 // model N2: FM = F1/GaMaCoTe0
#define M_INV_HECOTE 12 // model N2: GAIN_K = F1*R*GaDe0*GaCpMeanMix0/GaHeCoTe0 (RHO_K, INV_CP0 are folded in)
#define M_UA 13         // U*a
#define M_TM 14         // medium temperature, 0 = adiabatic
#define M_CIN 16        // S inlet values SpCoi0[i]/Cmax
#define M_USER (16 + RMT_S)   // RMT_NU user parameters (always read at run time)
#if RMT_FORCING
#define M_FORCE (16 + RMT_S + RMT_NU)   // t_ref, d THETA_IN/dt, d P0/dt, d TM/dt of this launch (P0, THETA_IN, TM: the values at t_ref)
#define M_FORCE_CIN (M_FORCE + 4)       // RMT_FORCING 2: d CIN_i/dt, S doubles (M_CIN: the values at t_ref)
#endif

typedef double preal;   // the pressure scan is always carried in fp64

#define RMT_EPS real(1e-30)
#define RMT_TREF real(298.15)

// ------------------------------------------------------------------ math wrappers
__device__ __forceinline__ double rmt_expm1(double x) { return expm1(x); }
__device__ __forceinline__ double rmt_log10(double x) { return log10(x); }
__device__ __forceinline__ double rmt_log2(double x) { return log2(x); }
__device__ __forceinline__ double rmt_log1p(double x) { return log1p(x); }
#ifndef RMT_FAST_MATH_SQRT
#define RMT_FAST_MATH_SQRT 1
#endif
#if !(RMT_FAST_MATH_SQRT) || defined(RMT_HOST_EMULATION)
__device__ __forceinline__ double rmt_sqrt(double x) { return sqrt(x); }
#else
// v_rsq_f64, one Goldschmidt step, one residual correction: 11 VALU instructions against the library's 20 (which scales
// arguments below 2^-767, passes +inf through and corrects twice) and BIT-IDENTICAL to it on 4.2 million random normal
// arguments between 2^-300 and 2^300 (tools/microbench/sqrt_acc.hip on an MI355X).  sqrt(0) = 0, a negative argument
// gives NaN (the tested stages flag it as Python's ValueError before that), +inf gives NaN instead of +inf.
__device__ __forceinline__ double rmt_sqrt(double x) {
    const double r = __builtin_amdgcn_rsq(x);
    double g = x * r, h = 0.5 * r;
    const double e = fma(-h, g, 0.5);
    g = fma(g, e, g);
    h = fma(h, e, h);
    g = fma(fma(-g, g, x), h, g);
    return (x == 0.0) ? 0.0 : g;
}
#endif
__device__ __forceinline__ double rmt_abs(double x) { return fabs(x); }
__device__ __forceinline__ double rmt_pow(double x, double y) { return pow(x, y); }
__device__ __forceinline__ double rmt_sin(double x) { return sin(x); }
__device__ __forceinline__ double rmt_cos(double x) { return cos(x); }
__device__ __forceinline__ double rmt_tan(double x) { return tan(x); }
__device__ __forceinline__ double rmt_tanh(double x) { return tanh(x); }
__device__ __forceinline__ double rmt_sinh(double x) { return sinh(x); }
__device__ __forceinline__ double rmt_cosh(double x) { return cosh(x); }
__device__ __forceinline__ double rmt_atan(double x) { return atan(x); }
__device__ __forceinline__ double rmt_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ double rmt_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float rmt_expm1(float x) { return expm1f(x); }
__device__ __forceinline__ float rmt_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ float rmt_abs(float x) { return fabsf(x); }
__device__ __forceinline__ float rmt_pow(float x, float y) { return powf(x, y); }
__device__ __forceinline__ float rmt_sin(float x) { return sinf(x); }
__device__ __forceinline__ float rmt_cos(float x) { return cosf(x); }
__device__ __forceinline__ float rmt_tan(float x) { return tanf(x); }
__device__ __forceinline__ float rmt_tanh(float x) { return tanhf(x); }
__device__ __forceinline__ float rmt_sinh(float x) { return sinhf(x); }
__device__ __forceinline__ float rmt_cosh(float x) { return coshf(x); }
__device__ __forceinline__ float rmt_atan(float x) { return atanf(x); }
__device__ __forceinline__ float rmt_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float rmt_max(float a, float b) { return fmaxf(a, b); }

// ---- status flags ---------------------------------------------------------------------------
// The generated kinetics test the conditions on which Python would raise (log(<=0), x/0, exp
// overflow ...) through RMT_CHECK_POS / _NONNEG / _DEN / _EXP (and the generic RMT_CHECK).
// RMT_FLAGS_MODE 0 (device default): one v_cmp into an SGPR pair OR-ed into a wave-wide lane mask
//   with a scalar instruction; masks are collapsed to status bits at the end of the launch.
// RMT_FLAGS_MODE 1 (host emulation; selectable on the device): one fp64 min/max into per-lane
//   running extremes.  On gfx950 this cost 8 more live VGPRs and pushed the 512x2 kernel into
//   scratch (10.1 -> 6.9 G node-steps/s), so it is not the default there.
#define RMT_EXP_LIMIT 709.782712893384
#ifndef RMT_FLAGS_MODE
#ifdef RMT_HOST_EMULATION
#define RMT_FLAGS_MODE 1
#else
#define RMT_FLAGS_MODE 0
#endif
#endif
#if RMT_FLAGS_MODE == 1
struct rmt_flags_t {
    real pos_min;       // smallest argument that must be  > 0  (log)
    real nn_min;        // smallest argument that must be >= 0  (sqrt)
    real den_min;       // smallest |denominator|
    real exp_max;       // largest exp() argument
    unsigned bits;      // anything else (pow domain), per lane
};
__device__ __forceinline__ void rmt_flags_clear(rmt_flags_t& f) {
    f.pos_min = f.nn_min = f.den_min = real(__builtin_inf());
    f.exp_max = real(-__builtin_inf());
    f.bits = 0u;
}
__device__ __forceinline__ void rmt_flags_merge(rmt_flags_t& into, const rmt_flags_t& f) {
    into.pos_min = rmt_min(into.pos_min, f.pos_min);
    into.nn_min = rmt_min(into.nn_min, f.nn_min);
    into.den_min = rmt_min(into.den_min, f.den_min);
    into.exp_max = rmt_max(into.exp_max, f.exp_max);
    into.bits |= f.bits;
}
__device__ __forceinline__ unsigned rmt_flags_bits(const rmt_flags_t& f) {
    return f.bits | ((f.pos_min <= real(0) || f.nn_min < real(0)) ? RMT_FLAG_DOMAIN : 0u) |
           ((f.den_min == real(0)) ? RMT_FLAG_DIV0 : 0u) |
           ((f.exp_max > real(RMT_EXP_LIMIT)) ? RMT_FLAG_OVERFLOW : 0u);
}
#define RMT_CHECK_POS(f, x) (f).pos_min = rmt_min((f).pos_min, (x))
#define RMT_CHECK_NONNEG(f, x) (f).nn_min = rmt_min((f).nn_min, (x))
#define RMT_CHECK_DEN(f, x) (f).den_min = rmt_min((f).den_min, rmt_abs(x))
#define RMT_CHECK_EXP(f, x) (f).exp_max = rmt_max((f).exp_max, (x))
#define RMT_CHECK(f, cond, bit) (f).bits |= ((cond) ? (bit) : 0u)
#else
#if RMT_MODEL == 2
struct rmt_flags_t { unsigned long long dom, div0, ovf, prs; };
#define RMT_PRS(x) x
#else
struct rmt_flags_t { unsigned long long dom, div0, ovf; };
#define RMT_PRS(x)
#endif
template <unsigned BIT>
__device__ __forceinline__ void rmt_check(rmt_flags_t& f, const bool c) {
    const unsigned long long m = __ballot(c);
    if (BIT == RMT_FLAG_DOMAIN) f.dom |= m;
    else if (BIT == RMT_FLAG_DIV0) f.div0 |= m;
    RMT_PRS(else if (BIT == RMT_FLAG_PRESSURE) f.prs |= m;)
    else f.ovf |= m;
}
__device__ __forceinline__ void rmt_flags_clear(rmt_flags_t& f) { f.dom = f.div0 = f.ovf = 0ull; RMT_PRS(f.prs = 0ull;) }
__device__ __forceinline__ void rmt_flags_merge(rmt_flags_t& into, const rmt_flags_t& f) {
    into.dom |= f.dom;
    into.div0 |= f.div0;
    into.ovf |= f.ovf;
    RMT_PRS(into.prs |= f.prs;)
}
__device__ __forceinline__ unsigned rmt_flags_bits(const rmt_flags_t& f) {
    return (f.dom ? RMT_FLAG_DOMAIN : 0u) | (f.div0 ? RMT_FLAG_DIV0 : 0u) | (f.ovf ? RMT_FLAG_OVERFLOW : 0u)
           RMT_PRS(| (f.prs ? RMT_FLAG_PRESSURE : 0u));
}
#define RMT_CHECK(f, cond, bit) rmt_check<bit>(f, (cond))
#define RMT_CHECK_POS(f, x) rmt_check<RMT_FLAG_DOMAIN>(f, (x) <= real(0))
#define RMT_CHECK_NONNEG(f, x) rmt_check<RMT_FLAG_DOMAIN>(f, (x) < real(0))
#define RMT_CHECK_DEN(f, x) rmt_check<RMT_FLAG_DIV0>(f, (x) == real(0))
#define RMT_CHECK_EXP(f, x) rmt_check<RMT_FLAG_OVERFLOW>(f, (x) > real(RMT_EXP_LIMIT))
#endif
// "do not check" argument: the generated kinetics are templated on the flags type, so passing this
// instead of an rmt_flags_t removes every test at compile time (used for RK stages 2-4 - an
// exception there still surfaces as a non-finite state - and for finite-difference evaluations)
struct rmt_noflags_t {};
#undef RMT_CHECK_POS
#undef RMT_CHECK_NONNEG
#undef RMT_CHECK_DEN
#undef RMT_CHECK_EXP
#undef RMT_CHECK
#if RMT_FLAGS_MODE == 1
__device__ __forceinline__ void rmt_chk_pos(rmt_flags_t& f, const real x) { f.pos_min = rmt_min(f.pos_min, x); }
__device__ __forceinline__ void rmt_chk_nonneg(rmt_flags_t& f, const real x) { f.nn_min = rmt_min(f.nn_min, x); }
__device__ __forceinline__ void rmt_chk_den(rmt_flags_t& f, const real x) { f.den_min = rmt_min(f.den_min, rmt_abs(x)); }
__device__ __forceinline__ void rmt_chk_exp(rmt_flags_t& f, const real x) { f.exp_max = rmt_max(f.exp_max, x); }
__device__ __forceinline__ void rmt_chk(rmt_flags_t& f, const bool c, const unsigned bit) { f.bits |= c ? bit : 0u; }
#else
__device__ __forceinline__ void rmt_chk_pos(rmt_flags_t& f, const real x) { rmt_check<RMT_FLAG_DOMAIN>(f, x <= real(0)); }
__device__ __forceinline__ void rmt_chk_nonneg(rmt_flags_t& f, const real x) { rmt_check<RMT_FLAG_DOMAIN>(f, x < real(0)); }
__device__ __forceinline__ void rmt_chk_den(rmt_flags_t& f, const real x) { rmt_check<RMT_FLAG_DIV0>(f, x == real(0)); }
__device__ __forceinline__ void rmt_chk_exp(rmt_flags_t& f, const real x) { rmt_check<RMT_FLAG_OVERFLOW>(f, x > real(RMT_EXP_LIMIT)); }
__device__ __forceinline__ void rmt_chk(rmt_flags_t& f, const bool c, const unsigned bit) {
    const unsigned long long m = __ballot(c);
    if (bit == RMT_FLAG_DOMAIN) f.dom |= m;
    else if (bit == RMT_FLAG_DIV0) f.div0 |= m;
    RMT_PRS(else if (bit == RMT_FLAG_PRESSURE) f.prs |= m;)
    else f.ovf |= m;
}
#endif
#if RMT_FLAGS_MODE == 0
// The tests of ONE right-hand-side evaluation as running extremes (one fp64 min / max per test, no compare mask in SGPRs -
// the masks of ~40 tests per stage were spilled to VGPR lanes and read back, ~100 lane moves per step), folded into the
// launch-long lane masks of an rmt_flags_t by four compares when the evaluation is over.  The extremes live for one
// call only, so they do not cost the registers RMT_FLAGS_MODE 1 did.
struct rmt_callflags_t {
    real pos_min, nn_min, den_min, exp_max;
    unsigned long long other[3];          // generic RMT_CHECKs (pow domain ...): masks, rare
};
__device__ __forceinline__ void rmt_callflags_clear(rmt_callflags_t& f) {
    f.pos_min = f.nn_min = f.den_min = real(__builtin_inf());
    f.exp_max = real(-__builtin_inf());
    f.other[0] = f.other[1] = f.other[2] = 0ull;
}
__device__ __forceinline__ void rmt_chk_pos(rmt_callflags_t& f, const real x) { f.pos_min = rmt_min(f.pos_min, x); }
__device__ __forceinline__ void rmt_chk_nonneg(rmt_callflags_t& f, const real x) { f.nn_min = rmt_min(f.nn_min, x); }
__device__ __forceinline__ void rmt_chk_den(rmt_callflags_t& f, const real x) { f.den_min = rmt_min(f.den_min, rmt_abs(x)); }
__device__ __forceinline__ void rmt_chk_exp(rmt_callflags_t& f, const real x) { f.exp_max = rmt_max(f.exp_max, x); }
__device__ __forceinline__ void rmt_chk(rmt_callflags_t& f, const bool c, const unsigned bit) {
    f.other[bit == RMT_FLAG_DOMAIN ? 0 : (bit == RMT_FLAG_DIV0 ? 1 : 2)] |= __ballot(c);
}
// (NaN arguments: min / max drop a NaN operand, a compare with NaN is false as well - the same tests fail to fire either
// way, and the non-finite state is caught by RMT_FLAG_NONFINITE)
__device__ __forceinline__ void rmt_flags_fold(rmt_flags_t& into, const rmt_callflags_t& f) {
    into.dom |= __ballot(f.pos_min <= real(0) || f.nn_min < real(0)) | f.other[0];
    into.div0 |= __ballot(f.den_min == real(0)) | f.other[1];
    into.ovf |= __ballot(f.exp_max > real(RMT_EXP_LIMIT)) | f.other[2];
}
#endif
__device__ __forceinline__ void rmt_chk_pos(rmt_noflags_t&, const real) {}
__device__ __forceinline__ void rmt_chk_nonneg(rmt_noflags_t&, const real) {}
__device__ __forceinline__ void rmt_chk_den(rmt_noflags_t&, const real) {}
__device__ __forceinline__ void rmt_chk_exp(rmt_noflags_t&, const real) {}
__device__ __forceinline__ void rmt_chk(rmt_noflags_t&, const bool, const unsigned) {}
#define RMT_CHECK_POS(f, x) rmt_chk_pos(f, (x))
#define RMT_CHECK_NONNEG(f, x) rmt_chk_nonneg(f, (x))
#define RMT_CHECK_DEN(f, x) rmt_chk_den(f, (x))
#define RMT_CHECK_EXP(f, x) rmt_chk_exp(f, (x))
#define RMT_CHECK(f, cond, bit) rmt_chk(f, (cond), (bit))

// ---- lean fp64 division / reciprocal / log (RMT_FAST_MATH, default on) -----------------------
// gfx950 costs in fp64 VALU ops (llvm-objdump of the ocml versions): x/y 11 (+v_rcp_f64), log 76,
// log10 83, exp 19, sqrt 14.  The versions below drop the scale/fixup and double-double work that
// only matters for denormal/huge operands or the last half ulp: rcp 5, div 8, log ~30 ops, each
// accurate to ~1 ulp on normal numbers - far inside the 1e-12 parity budget of the RHS.
#ifndef RMT_FAST_MATH
#define RMT_FAST_MATH 1
#endif
#if RMT_FAST_MATH && !defined(RMT_HOST_EMULATION)
__device__ __forceinline__ double rmt_rcp(double b) {
    double r = __builtin_amdgcn_rcp(b);
    r = fma(fma(-b, r, 1.0), r, r);
    r = fma(fma(-b, r, 1.0), r, r);
    return r;
}
__device__ __forceinline__ double rmt_div(double a, double b) {
    double r = __builtin_amdgcn_rcp(b);
    r = fma(fma(-b, r, 1.0), r, r);       // one Newton step (~2^-46) is enough here: the residual
    const double q = a * r;               // correction below squares the error of q
    return fma(fma(-b, q, a), r, q);
}
__device__ __forceinline__ double rmt_log(double x) {     // after fdlibm e_log.c (x > 0, finite)
#ifdef RMT_TIMING_CHEAP_LOG          // cost attribution only (results are wrong)
    return x * 1e-2;
#endif
    int e = __builtin_amdgcn_frexp_exp(x);
    double m = __builtin_amdgcn_frexp_mant(x);            // [0.5, 1)
    const bool lo = m < 0.70710678118654752440;
    m = lo ? m + m : m;
    e = lo ? e - 1 : e;
    const double f = m - 1.0;
    const double s = rmt_div(f, 2.0 + f);
    const double dk = (double)e;
    const double z = s * s, w = z * z;
    const double t1 = w * fma(w, fma(w, 1.531383769920937332e-01, 2.222219843214978396e-01), 3.999999999940941908e-01);
    const double t2 = z * fma(w, fma(w, fma(w, 1.479819860511658591e-01, 1.818357216161805012e-01),
                                     2.857142874366239149e-01), 6.666666666666735130e-01);
    const double R = t2 + t1;
    const double hfsq = 0.5 * f * f;
    return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
}
#else
__device__ __forceinline__ double rmt_rcp(double b) { return 1.0 / b; }
__device__ __forceinline__ double rmt_div(double a, double b) { return a / b; }
__device__ __forceinline__ double rmt_log(double x) { return log(x); }
#endif
#if RMT_FAST_MATH && !defined(RMT_HOST_EMULATION)
// exp(x) = 2^m * 2^(j/64) * e^r,  k = rint(x*64/ln2) = 64 m + j,  |r| <= ln2/128: a 64-entry table
// (staged in LDS by rmt_math_init) and a degree-5 polynomial - 12 fp64 ops against 19 + 6 range
// selects in the ocml version (the exp is ~40 % of the DME kernel's fp64 work).  Overflow is
// flagged by the generated checks before the call; results below 2^-1022 flush through ldexp.
#ifndef RMT_EXP_BITS
#define RMT_EXP_BITS 11          // 2^11-entry table of 2^(j/2048) in LDS (16 KiB): cubic polynomial suffices
#endif
__shared__ double rmt_exp_lds[1 << RMT_EXP_BITS];
__device__ static const double RMT_EXP_TAB[64] = {
    0x1.0000000000000p+0, 0x1.02c9a3e778061p+0, 0x1.059b0d3158574p+0, 0x1.0874518759bc8p+0,
    0x1.0b5586cf9890fp+0, 0x1.0e3ec32d3d1a2p+0, 0x1.11301d0125b51p+0, 0x1.1429aaea92de0p+0,
    0x1.172b83c7d517bp+0, 0x1.1a35beb6fcb75p+0, 0x1.1d4873168b9aap+0, 0x1.2063b88628cd6p+0,
    0x1.2387a6e756238p+0, 0x1.26b4565e27cddp+0, 0x1.29e9df51fdee1p+0, 0x1.2d285a6e4030bp+0,
    0x1.306fe0a31b715p+0, 0x1.33c08b26416ffp+0, 0x1.371a7373aa9cbp+0, 0x1.3a7db34e59ff7p+0,
    0x1.3dea64c123422p+0, 0x1.4160a21f72e2ap+0, 0x1.44e086061892dp+0, 0x1.486a2b5c13cd0p+0,
    0x1.4bfdad5362a27p+0, 0x1.4f9b2769d2ca7p+0, 0x1.5342b569d4f82p+0, 0x1.56f4736b527dap+0,
    0x1.5ab07dd485429p+0, 0x1.5e76f15ad2148p+0, 0x1.6247eb03a5585p+0, 0x1.6623882552225p+0,
    0x1.6a09e667f3bcdp+0, 0x1.6dfb23c651a2fp+0, 0x1.71f75e8ec5f74p+0, 0x1.75feb564267c9p+0,
    0x1.7a11473eb0187p+0, 0x1.7e2f336cf4e62p+0, 0x1.82589994cce13p+0, 0x1.868d99b4492edp+0,
    0x1.8ace5422aa0dbp+0, 0x1.8f1ae99157736p+0, 0x1.93737b0cdc5e5p+0, 0x1.97d829fde4e50p+0,
    0x1.9c49182a3f090p+0, 0x1.a0c667b5de565p+0, 0x1.a5503b23e255dp+0, 0x1.a9e6b5579fdbfp+0,
    0x1.ae89f995ad3adp+0, 0x1.b33a2b84f15fbp+0, 0x1.b7f76f2fb5e47p+0, 0x1.bcc1e904bc1d2p+0,
    0x1.c199bdd85529cp+0, 0x1.c67f12e57d14bp+0, 0x1.cb720dcef9069p+0, 0x1.d072d4a07897cp+0,
    0x1.d5818dcfba487p+0, 0x1.da9e603db3285p+0, 0x1.dfc97337b9b5fp+0, 0x1.e502ee78b3ff6p+0,
    0x1.ea4afa2a490dap+0, 0x1.efa1bee615a27p+0, 0x1.f50765b6e4540p+0, 0x1.fa7c1819e90d8p+0,
};
#if RMT_EXP_BITS == 11
__device__ static const double RMT_EXP_TAB_LO[32] = {      // 2^(i/2048)
    0x1.0000000000000p+0, 0x1.00162f3904052p+0, 0x1.002c605e2e8cfp+0, 0x1.0042936faa3d8p+0,
    0x1.0058c86da1c0ap+0, 0x1.006eff583fc3dp+0, 0x1.0085382faef83p+0, 0x1.009b72f41a12bp+0,
    0x1.00b1afa5abcbfp+0, 0x1.00c7ee448ee02p+0, 0x1.00de2ed0ee0f5p+0, 0x1.00f4714af41d3p+0,
    0x1.010ab5b2cbd11p+0, 0x1.0120fc089ff63p+0, 0x1.0137444c9b5b5p+0, 0x1.014d8e7ee8d2fp+0,
    0x1.0163da9fb3335p+0, 0x1.017a28af25567p+0, 0x1.019078ad6a19fp+0, 0x1.01a6ca9aac5f3p+0,
    0x1.01bd1e77170b4p+0, 0x1.01d37442d5070p+0, 0x1.01e9cbfe113efp+0, 0x1.020025a8f6a35p+0,
    0x1.02168143b0281p+0, 0x1.022cdece68c4fp+0, 0x1.02433e494b755p+0, 0x1.02599fb483385p+0,
    0x1.027003103b10ep+0, 0x1.0286685c9e059p+0, 0x1.029ccf99d720ap+0, 0x1.02b338c811703p+0,
};
__device__ __forceinline__ void rmt_math_init() {
    for (int j = threadIdx.x; j < 2048; j += blockDim.x)   // 2^(j/2048) = 2^((j>>5)/64) * 2^((j&31)/2048), <= 1.5 ulp
        rmt_exp_lds[j] = RMT_EXP_TAB[j >> 5] * RMT_EXP_TAB_LO[j & 31];
    __syncthreads();
}
__device__ __forceinline__ double rmt_exp(double x) {
#ifdef RMT_TIMING_CHEAP_EXP          // cost attribution only (results are wrong): what the nine exp of a node-RHS cost
    return 1.0 + x * 1e-3;
#endif
    // round-to-nearest integer by adding 1.5*2^52: the integer sits in the low word of the sum
    const double ks = fma(x, 2954.639443740597, 6755399441055744.0);     // 2048/ln2
    const int k = __double2loint(ks);
    const double kd = ks - 6755399441055744.0;
    double r = fma(-kd, 3.384507717577858e-04, x);                      // ln2/2048 hi
    r = fma(-kd, 1.1323470770733884e-20, r);                            // ln2/2048 lo
    const double q = r * r;                                             // |r| <= 1.7e-4: r^4/24 < 4e-17
    const double p = fma(q, fma(r, 1.6666666666666666e-01, 0.5), r);    // e^r - 1
    const double t = rmt_exp_lds[k & 2047];
    return __builtin_ldexp(fma(t, p, t), k >> 11);
}
#else
__device__ __forceinline__ void rmt_math_init() {
    if (threadIdx.x < 64) rmt_exp_lds[threadIdx.x] = RMT_EXP_TAB[threadIdx.x];
    __syncthreads();
}
__device__ __forceinline__ double rmt_exp(double x) {
    const double kd = __builtin_rint(x * 92.33248261689366);            // 64/ln2
    const int k = (int)kd;
    double r = fma(-kd, 0.010830424696249145, x);                       // ln2/64 hi
    r = fma(-kd, 3.623510646634843e-19, r);                             // ln2/64 lo
    double p = fma(r, 8.3333333333333332e-03, 4.1666666666666664e-02);  // 1/120, 1/24
    p = fma(p, r, 1.6666666666666666e-01);
    p = fma(p, r, 0.5);
    p = p * r;
    p = fma(p, r, r);                                                   // e^r - 1
    const double t = rmt_exp_lds[k & 63];
    return __builtin_ldexp(fma(t, p, t), k >> 6);
}
#endif
__device__ __forceinline__ double rmt_exp10(double x) { return rmt_exp(x * 2.302585092994046); }
__device__ __forceinline__ double rmt_exp2(double x) { return rmt_exp(x * 0.6931471805599453); }
// RMT_KC_SMALL_EXP 1 (host: n2.kcache_choice): a kernel that caches EVERY table-driven exp of the mechanism evaluates
// them in full only when its reference point moves, so it keeps the 64-entry table (512 B of LDS instead of 16 KiB - the
// room the cache of the equilibrium constants needs) and pays two more multiply-adds per full evaluation.  Its own
// array: a kernel is charged for the tables it references.  rmt_exp_sel<true> = the exp of such a kernel.
#ifndef RMT_KC_SMALL_EXP
#define RMT_KC_SMALL_EXP 0
#endif
#if RMT_KC_SMALL_EXP && RMT_EXP_BITS == 11
__shared__ double rmt_exp_lds6[64];
__device__ __forceinline__ void rmt_math_init6() {
    if (threadIdx.x < 64) rmt_exp_lds6[threadIdx.x] = RMT_EXP_TAB[threadIdx.x];
    __syncthreads();
}
__device__ __forceinline__ double rmt_exp6(double x) {
    const double ks = fma(x, 92.33248261689366, 6755399441055744.0);     // 64/ln2; the integer in the low word
    const int k = __double2loint(ks);
    const double kd = ks - 6755399441055744.0;
    double r = fma(-kd, 0.010830424696249145, x);                       // ln2/64 hi
    r = fma(-kd, 3.623510646634843e-19, r);                             // ln2/64 lo
    double p = fma(r, 8.3333333333333332e-03, 4.1666666666666664e-02);  // 1/120, 1/24
    p = fma(p, r, 1.6666666666666666e-01);
    p = fma(p, r, 0.5);
    p = p * r;
    p = fma(p, r, r);                                                   // e^r - 1
    const double t = rmt_exp_lds6[k & 63];
    return __builtin_ldexp(fma(t, p, t), k >> 6);
}
#else
__device__ __forceinline__ void rmt_math_init6() { rmt_math_init(); }
__device__ __forceinline__ double rmt_exp6(double x) { return rmt_exp(x); }
#endif
template <bool CACHING> __device__ __forceinline__ double rmt_exp_sel(double x) {
    if constexpr (CACHING) return rmt_exp6(x);
    else return rmt_exp(x);
}
template <bool CACHING> __device__ __forceinline__ double rmt_exp10_sel(double x) { return rmt_exp_sel<CACHING>(x * 2.302585092994046); }
template <bool CACHING> __device__ __forceinline__ double rmt_exp2_sel(double x) { return rmt_exp_sel<CACHING>(x * 0.6931471805599453); }
#else
__device__ __forceinline__ void rmt_math_init() {}
__device__ __forceinline__ void rmt_math_init6() {}
__device__ __forceinline__ double rmt_exp(double x) { return exp(x); }
__device__ __forceinline__ double rmt_exp10(double x) { return exp10(x); }
__device__ __forceinline__ double rmt_exp2(double x) { return exp2(x); }
template <bool CACHING> __device__ __forceinline__ double rmt_exp_sel(double x) { return exp(x); }
template <bool CACHING> __device__ __forceinline__ double rmt_exp10_sel(double x) { return exp10(x); }
template <bool CACHING> __device__ __forceinline__ double rmt_exp2_sel(double x) { return exp2(x); }
#endif
#if RMT_FAST_MATH && !defined(RMT_HOST_EMULATION)
// fp32: the hardware transcendental instructions (v_rcp_f32, v_exp_f32, v_log_f32, v_sqrt_f32; ~1 ulp)
__device__ __forceinline__ float rmt_rcp(float b) { return __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ float rmt_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ float rmt_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
__device__ __forceinline__ float rmt_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float rmt_exp10(float x) { return __builtin_amdgcn_exp2f(x * 3.32192809488736235f); }
__device__ __forceinline__ float rmt_log(float x) { return __builtin_amdgcn_logf(x) * 0.693147180559945309f; }
__device__ __forceinline__ float rmt_log2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float rmt_log10(float x) { return __builtin_amdgcn_logf(x) * 0.301029995663981195f; }
__device__ __forceinline__ float rmt_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
#else
__device__ __forceinline__ float rmt_rcp(float b) { return 1.0f / b; }
__device__ __forceinline__ float rmt_div(float a, float b) { return a / b; }
__device__ __forceinline__ float rmt_exp(float x) { return expf(x); }
__device__ __forceinline__ float rmt_exp2(float x) { return exp2f(x); }
__device__ __forceinline__ float rmt_exp10(float x) { return exp10f(x); }
__device__ __forceinline__ float rmt_log(float x) { return logf(x); }
__device__ __forceinline__ float rmt_log2(float x) { return log2f(x); }
__device__ __forceinline__ float rmt_log10(float x) { return log10f(x); }
__device__ __forceinline__ float rmt_sqrt(float x) { return sqrtf(x); }
#endif

// ---- dense inverse of a small matrix, in place (Gauss-Jordan without pivoting; returns the smallest |pivot|: 0 or NaN =
// singular).  One matrix per lane: the steady-state kernels (70_n1.inc, 71_steady_march.inc); also compiled for the host.
template <int NV>
__device__ __forceinline__ real rmt_invert_n(real (&a)[NV][NV]) {
    real pmin = real(__builtin_inf());
#pragma unroll
    for (int p = 0; p < NV; ++p) {
        pmin = rmt_min(pmin, rmt_abs(a[p][p]));
        const real ip = rmt_rcp(a[p][p]);
        a[p][p] = real(1);
#pragma unroll
        for (int c = 0; c < NV; ++c) a[p][c] *= ip;
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            if (r != p) {
                const real f = a[r][p];
                a[r][p] = real(0);
#pragma unroll
                for (int c = 0; c < NV; ++c) a[r][c] -= f * a[p][c];
            }
        }
    }
    return pmin;
}

