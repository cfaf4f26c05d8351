// ------------------------------------------------------------------ time-varying inlet / coolant conditions
// solver-config "schedule" (host: rmt_app_amd/schedule.py): the inlet temperature, the inlet pressure and the medium
// temperature of a reactor are piecewise-linear functions of time.  The host splits the integration at every breakpoint,
// so inside ONE launch each of the three is one linear function of t, and a code object generated with RMT_FORCING 1
// evaluates it at the stage time of every RHS evaluation: the member row carries, behind its ordinary fields - which hold
// the values at t_ref, the start of the launch - a tail of four doubles {t_ref, d THETA_IN/dt, d P0/dt, d TM/dt}
// (M_FORCE; the host refreshes the rows before each launch).  Nothing else of the member depends on the three: the
// scaling constants and the pre-combined fields stay those of the member's own input.
// RMT_FORCING 2: the schedule also moves the feed composition ("inlet-concentration").  The inlet values M_CIN =
// C_in,i/Cmax hold the values at t_ref and the tail grows by their S slopes (M_FORCE_CIN); Cmax and every other scaling
// constant stay the member's own, so only node 0's upstream concentration changes.  Everything RMT_FORCING 1 does stays.
// A build without the define contains none of this and has the member row of 16 + S + NU doubles.
#if RMT_FORCING
#if RMT_FORCING != 1 && RMT_FORCING != 2
#error "RMT_FORCING: 1 (inlet temperature, inlet pressure, medium temperature) or 2 (the same plus the feed composition)"
#endif
#if RMT_MODEL != 0 || RMT_FP32 || RMT_MEMBER_LDS
#error "RMT_FORCING: model N2 in fp64 with the member in registers only"
#endif
#if defined(RMT_MC_THETA_IN) || defined(RMT_MC_P0) || defined(RMT_MC_TM)
#error "RMT_FORCING: the forced member fields must not be baked into the kernel as literals (specialize=False)"
#endif
#if RMT_FORCING == 2 && defined(RMT_MC_CIN)
#error "RMT_FORCING 2: the forced inlet composition must not be baked into the kernel as a literal (RMT_MC_CIN)"
#endif
#if defined(RMT_UP_LDS) && RMT_UP_LDS
#error "RMT_FORCING: the LDS neighbour exchange keeps a constant inlet slot"
#endif
// m.theta_in, m.p0, m.tm <- value + slope (t - t_ref).  `row` and `t` are wave-uniform: three fp64 multiply-adds on uniform
// values (CDNA has no scalar fp64 arithmetic, so they run on the vector unit), the seven row entries come by scalar loads
// at the place of use instead of staying in registers over the step loop.  p0 stays in preal.
// The results go back to SGPRs (v_readfirstlane), where the unforced member keeps these fields: as VGPR-resident values
// they cost the 512 x 2 on-chip steppers, which sit at their register wall, six more live VGPRs across the whole RHS.
#ifndef RMT_FORCING_SGPR
#define RMT_FORCING_SGPR 1
#endif
__device__ __forceinline__ double rmt_forcing_uniform(const double v) {
#if RMT_FORCING_SGPR
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
#else
    return v;
#endif
}
// the three boundary values of RMT_FORCING 1 alone (the on-chip steppers, which never read m.cin inside their step loop)
__device__ __forceinline__ void rmt_forcing_apply3(RmtMember& m, const double* __restrict__ row, const double t) {
    const double dt = t - row[M_FORCE];
    m.theta_in = real(rmt_forcing_uniform(row[M_THETA_IN] + row[M_FORCE + 1] * dt));
    m.p0 = rmt_forcing_uniform(row[M_P0] + row[M_FORCE + 2] * dt);
    m.tm = real(rmt_forcing_uniform(row[M_TM] + row[M_FORCE + 3] * dt));
}
// RMT_FORCING 2: m.cin moves too - the stiff stepper hands it to node 0 through rmt_carry_inlet (60_ros4.inc)
__device__ __forceinline__ void rmt_forcing_apply(RmtMember& m, const double* __restrict__ row, const double t) {
    rmt_forcing_apply3(m, row, t);
#if RMT_FORCING == 2
    const double dt = t - row[M_FORCE];
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) m.cin[i] = real(rmt_forcing_uniform(row[M_CIN + i] + row[M_FORCE_CIN + i] * dt));
#endif
}
// the same a time `del` later, exactly (the forcing is linear): for the time derivative of the stiff stepper
__device__ __forceinline__ void rmt_forcing_shift(RmtMember& m, const double* __restrict__ row, const double del) {
    m.theta_in = real(rmt_forcing_uniform((double)m.theta_in + row[M_FORCE + 1] * del));
    m.p0 = rmt_forcing_uniform(m.p0 + row[M_FORCE + 2] * del);
    m.tm = real(rmt_forcing_uniform((double)m.tm + row[M_FORCE + 3] * del));
#if RMT_FORCING == 2
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) m.cin[i] = real(rmt_forcing_uniform((double)m.cin[i] + row[M_FORCE_CIN + i] * del));
#endif
}
// true when nothing moves during this launch (a hold between two breakpoints): workgroup-uniform
__device__ __forceinline__ bool rmt_forcing_constant(const double* __restrict__ row) {
    bool c = row[M_FORCE + 1] == 0.0 && row[M_FORCE + 2] == 0.0 && row[M_FORCE + 3] == 0.0;
#if RMT_FORCING == 2
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) c = c && row[M_FORCE_CIN + i] == 0.0;
#endif
    return c;
}
// One stage of an explicit stepper: the member at the stage time, and the inlet hand-over that goes with it - the carry
// {P0, upstream state of node 0} of the memory-resident forms, and `inlet` (the LDS slot sh.inlet of the on-chip forms,
// nullptr elsewhere).  Slot RMT_S of sh.inlet changes, and under RMT_FORCING 2 the slots 0..S-1 as well.  All RMT_V slots
// have ONE writer and ONE reader (40_rhs_block.inc, the branch !CARRY_OUT && CHAIN == 0 reads them in one loop): thread 0
// writes them ahead of the barrier inside the RHS evaluation and thread 0 (lane 0 of wave 0) is also their only reader,
// behind that barrier: no race, no new barrier, for the composition as for theta_in.
// The composition of the on-chip forms is formed where thread 0 writes the slot - scalar loads of value and slope, one
// fp64 multiply-add each, straight to LDS - and never enters RmtMember: S more wave-uniform values live across the RHS
// would spill in the 512 x 2 kernels.  The memory-resident forms (inlet == nullptr: thread 0 fills the stage hand-overs
// of the whole step ahead of the node blocks) write carry.up[0..S-1] the same way.
template <typename CARRY>
__device__ __forceinline__ void rmt_forcing_stage(RmtMember& m, CARRY& carry, const double* __restrict__ row,
                                                  const double t, real* inlet) {
    rmt_forcing_apply3(m, row, t);
    carry.P = m.p0;
#if RMT_FORCING == 2
    if (inlet) {
        if (threadIdx.x == 0) {
            // (a zero offset into the row passes through an empty asm: loads that depend on it cannot be hoisted out of the
            // stage loop, where 2 S loop-invariant doubles would occupy SGPRs - and their spills VGPRs - across every RHS)
            int off = 0;
            asm volatile("" : "+s"(off));
            const double* r = row + off;
            const double dt = t - r[M_FORCE];
#pragma unroll
            for (int i = 0; i < RMT_S; ++i) inlet[i] = real(r[M_CIN + i] + r[M_FORCE_CIN + i] * dt);
        }
    } else {
        const double dt = t - row[M_FORCE];
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) carry.up[i] = real(row[M_CIN + i] + row[M_FORCE_CIN + i] * dt);
    }
#endif
#if !RMT_ISO
    carry.up[RMT_S] = m.theta_in;
    if (inlet && threadIdx.x == 0) inlet[RMT_S] = m.theta_in;
#else
    (void)inlet;
#endif
}
// stage abscissae: classic RK4, Dormand-Prince 5(4), and Hairer & Wanner's RODAS4 with its time weights d_i (gamma_i):
// stage i of the non-autonomous Rosenbrock method evaluates f(t + c_i h, Y_i) and its right-hand side gains h d_i f_t
__device__ __forceinline__ double rmt_rk4_c(const int s) { return s == 0 ? 0.0 : (s == 3 ? 1.0 : 0.5); }
__device__ __forceinline__ double rmt_dp_c(const int s) {      // s = 0..6
    return s == 0 ? 0.0 : s == 1 ? 0.2 : s == 2 ? 0.3 : s == 3 ? 0.8 : s == 4 ? 8.0 / 9.0 : 1.0;
}
template <int STAGE> struct rmt_rodas_t {      // STAGE = 1..6
    static constexpr double c = STAGE == 1 ? 0.0 : STAGE == 2 ? 0.386 : STAGE == 3 ? 0.21 : STAGE == 4 ? 0.63 : 1.0;
    static constexpr double d = STAGE == 1 ? 0.25 : STAGE == 2 ? -0.1043 : STAGE == 3 ? 0.1035
                                : STAGE == 4 ? -0.3620000000000023e-01 : 0.0;
};
__device__ __forceinline__ double rmt_rodas_c(const int st) {      // st = 0..5
    return st == 0 ? 0.0 : st == 1 ? 0.386 : st == 2 ? 0.21 : st == 3 ? 0.63 : 1.0;
}
// the time derivative f_t is a forward difference over RMT_FT_FRAC of the step: exact in theta_in, tm and the inlet
// composition (f is affine in all of them: they enter the upwind difference of node 0 and the wall term only), O(del) only
// in the curvature of f along p0
#ifndef RMT_FT_FRAC
#define RMT_FT_FRAC (1.0 / 256.0)
#endif
#endif   // RMT_FORCING

