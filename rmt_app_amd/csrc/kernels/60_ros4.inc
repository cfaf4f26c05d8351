#if RMT_WITH_ROS4
// ===================================================================== kernel: stiff integrator (Rosenbrock), state in memory
// SURVEY.md section 8(f) rank 2.  The explicit steppers are stability-limited to dt ~ 3e-6 s on
// the hot DME bed (250 000 steps for 0.5 s).  This kernel is a linearly-implicit 4th-order
// Rosenbrock method with an embedded 3rd-order error estimate - the Kaps-Rentrop scheme with
// Shampine's parameters (gamma = 1/2; 3 RHS evaluations, 4 linear solves per step) - and
// per-reactor step control like rmt_n2_rk45_mem.
//   Jacobian: the method of lines RHS of node z depends on its own state, on the clamped state of
// node z-1 (upwind) and - weakly - on all upstream nodes through the pressure march.  J is taken
// as block lower-bidiagonal: D_z = d f_z / d y_z by forward differences of the node function at
// frozen (P_z, upstream state), L_z = d f_z / d y_{z-1} = diag(F1/dz or FT/dz) (0 where the clamp
// is active); the pressure coupling is dropped (measured: same step counts and accuracy as the
// full finite-difference Jacobian, tools/ros_prototype.py).
//   Solve (I/(gamma h) - J) x = b: per node x_z = Ainv_z (b_z + L_z x_{z-1}), Ainv_z the explicit
// VxV inverse (Gauss-Jordan in registers); the upstream coupling is resolved by Jacobi sweeps
// x <- p + Ainv L x_up whose contraction factor is <= c/(1/(gamma h) + c), c = F1/dz (h is capped
// so that this is <= 1/2); node blocks are walked in order, so the block boundary value is exact.
// work = 8 vector arrays [E][V][N] (F, G1..G4, stage state, new state, b) + Ainv [E][V*V][N] +
// per-node clamp masks.
#define RMT_ROS_GAM 0.5
#ifndef RMT_ROS_MAX_FRAC
#define RMT_ROS_MAX_FRAC 0.1
#endif
// relative accuracy of the Jacobi-sweep solves in units of rtol, from the worst-case contraction bound (the
// inert directions; the reacting ones converge much faster).  Measured (tools/ros4_solve_tol_scan.py,
// profiles/round2_time_to_solution.md): outlet / profile errors against the tight goldens and the step counts are
// identical to three digits for 1e-2 ... 1; 0.3 keeps a margin and saves 5 of 27 sweeps at rtol 1e-6.
#ifndef RMT_ROS_SOLVE_TOL
#define RMT_ROS_SOLVE_TOL 0.3
#endif
// largest contraction factor of the sweeps the step size may produce: rho = c/(1/(gamma h) + c) <= RMT_ROS_RHO_MAX,
// i.e. h <= rho/((1 - rho) gamma c), c = F1/dz.  A larger rho lets an accuracy-limited step grow past the
// convective scale at the price of log(tol)/log(rho) sweeps per solve.
#ifndef RMT_ROS_RHO_MAX
#define RMT_ROS_RHO_MAX 0.5
#endif
#ifndef RMT_ROS_MAX_SWEEPS
#define RMT_ROS_MAX_SWEEPS 60
#endif
// Jacobi steps per sweep of the RODAS4 path = how many steps old a cross-wave / cross-chunk boundary value can
// be (rmt_rodas_bs runs two-step sweeps; the solve's step count is padded by RMT_ROS_XCH - 1 for the staleness
// and rounded up to whole sweeps)
#ifndef RMT_ROS_XCH
#define RMT_ROS_XCH 2
#endif
// the chained stiff stepper runs without back-pressure on its links: a producer is at most one step attempt ahead of
// its consumer (every chunk waits for the decision), and an attempt sends 6 stage records + 6 x (sweeps / XCH + 1)
// boundary iterates + the error norm - that must stay below the ring depth or the producer laps unread entries
static_assert(6 * (RMT_ROS_MAX_SWEEPS + RMT_ROS_XCH) + 1 < RMT_RING,
              "RMT_ROS_MAX_SWEEPS: one step attempt of the chained stiff stepper must fit the link ring");
#ifdef RMT_ROS_FIX_SWEEPS
static_assert(6 * (RMT_ROS_FIX_SWEEPS + RMT_ROS_XCH) + 1 < RMT_RING,
              "RMT_ROS_FIX_SWEEPS: one step attempt of the chained stiff stepper must fit the link ring");
#endif
__device__ __forceinline__ void rmt_shift_up(RmtShared& sh, const int buf, const real (&x)[RMT_V],
                                             real (&xup)[RMT_V], real (&carry_out)[RMT_V],
                                             const bool want_out = true) {
    // the value upstream of the block sits in sh.xb[*][0] (rmt_sweep_carry), so lane 0 of EVERY wave reads row
    // `wave` - no select between a register-held carry and LDS inside the sweep loop
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) xup[i] = rmt_lane_up1(x[i]);
    if (lane == 63) {
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) sh.xb[buf][wave + 1][i] = x[i];
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) xup[i] = sh.xb[buf][wave][i];
    }
    if (want_out) {                                      // (workgroup-uniform: only the last pass of a solve)
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) carry_out[i] = sh.xb[buf][RMT_NW][i];
    }
}
// before the sweeps of a solve: the carry from the previous node block into row 0 of both exchange buffers
// (written and later read by wave 0 only; the first sweep's barrier orders it against nothing else)
__device__ __forceinline__ void rmt_sweep_carry(RmtShared& sh, const real (&carry_in)[RMT_V]) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) { sh.xb[0][0][i] = carry_in[i]; sh.xb[1][0][i] = carry_in[i]; }
    }
}

// The same exchange when the reactor is chained over workgroups (tagged-word links): the first block of a
// chunk takes the value upstream of its first node from the upstream chunk's message of THIS sweep - that
// chunk's boundary iterate before its update, i.e. plain synchronous Jacobi across the chunk boundary - and
// the last block of a chunk sends its own.  Wave 0 receives and the last wave sends, both before the barrier.
__device__ __forceinline__ void rmt_shift_up_chain(RmtShared& sh, const int buf, const real (&x)[RMT_V],
                                                   real (&xup)[RMT_V], real (&carry_out)[RMT_V],
                                                   const bool exchange, RmtChainCtx& ctx) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) xup[i] = rmt_lane_up1(x[i]);
    if (lane == 63) {
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) sh.xb[buf][wave + 1][i] = x[i];
    }
    if (exchange) {                                      // (workgroup-uniform: every pass but the last of a solve)
        if (ctx.has_out) {
            if (wave == RMT_NW - 1) {
                if (lane < RMT_V) sh.cst[buf][lane] = (double)sh.xb[buf][RMT_NW][lane];
                rmt_link_send(rmt_ring_entry(ctx.ring_out, ctx.seq_out), ctx.seq_out, sh.cst[buf], RMT_V);
            }
            ctx.seq_out = rmt_seq_next(ctx.seq_out);
        }
        if (ctx.has_in) {
            if (wave == 0) {
                ctx.dead |= rmt_link_recv(rmt_ring_entry(ctx.ring_in, ctx.seq_in), ctx.seq_in, sh.cin[buf], RMT_V,
                                          ctx.abort_word, ctx.dead);
                if (lane < RMT_V) sh.xb[buf][0][lane] = real(sh.cin[buf][lane]);
            }
            ctx.seq_in = rmt_seq_next(ctx.seq_in);
        }
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) xup[i] = sh.xb[buf][wave][i];
    }
    if (!exchange) {
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) carry_out[i] = sh.xb[buf][RMT_NW][i];
    }
}

// in-place inverse of a VxV matrix held in registers (Gauss-Jordan, no pivoting: the matrix is
// I/(gamma h) - D with a dominant positive diagonal); returns the smallest |pivot|
__device__ __forceinline__ real rmt_invert(real (&a)[RMT_V][RMT_V]) {
    real pmin = real(__builtin_inf());
#pragma unroll
    for (int p = 0; p < RMT_V; ++p) {
        pmin = rmt_min(pmin, rmt_abs(a[p][p]));
        const real ip = rmt_rcp(a[p][p]);
        a[p][p] = real(1);
#pragma unroll
        for (int c = 0; c < RMT_V; ++c) a[p][c] *= ip;
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) {
            if (r != p) {
                const real f = a[r][p];
                a[r][p] = real(0);
#pragma unroll
                for (int c = 0; c < RMT_V; ++c) a[r][c] -= f * a[p][c];
            }
        }
    }
    return pmin;
}

// ---- fused stage ------------------------------------------------------------------------------
// One Rosenbrock stage for ALL node blocks of the reactor: stage state -> f -> right-hand side ->
// (I/(gamma h) - J)^-1 -> G_STAGE, block by block, with the stage state, B and (stage 1) the block
// inverse kept in registers instead of being written to memory and read back by the next pass.
// Per step and node block this leaves 4 dependent memory round trips + the final update instead of
// the 14 of a pass-per-operation layout (the kernel runs ONE wave per SIMD, so every round trip is
// exposed; PMC of that first layout: 31 % VALU, 50 % waits).  Kaps-Rentrop pair = RMT_ROS_SCHEME 0.
template <int STAGE>
__device__ __forceinline__ void rmt_ros_stage(const RmtMember& m, RmtShared& sh, int& ph,
                                              const real* ye, real* F, const real* G1, const real* G2,
                                              const real* G3, real* Gout, real* ainv, unsigned* mask,
                                              real* coup, const int N, const real inv_gh, const real ih,
                                              const int sweeps, rmt_flags_t& flag, real& pivmin) {
    // Kaps-Rentrop / Shampine parameters (gamma = 1/2), as in the kernel below
    const real A21 = real(2.0), A31 = real(48.0 / 25), A32 = real(6.0 / 25), C21 = real(-8.0),
               C31 = real(372.0 / 25), C32 = real(12.0 / 5), C41 = real(-112.0 / 125),
               C42 = real(-54.0 / 125), C43 = real(-2.0 / 5);
    RmtCarry carry;
    rmt_carry_inlet(m, carry);
    real xc[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) xc[i] = real(0);             // nothing upstream of node 0
#if RMT_MODEL == 0
    const real cs = m.f1 * m.inv_dz, ct = m.ft * m.inv_dz;       // d f_z / d y_{z-1}
#endif
    for (int base = 0; base < N; base += RMT_BLOCK) {
        const int node = base + (int)threadIdx.x;
        const bool valid = node < N;
        real g1[RMT_V], g2[RMT_V], g3[RMT_V], ys[1][RMT_V], k[1][RMT_V];
        rmt_safe_state(m, ys[0]);
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) {
            const size_t o = (size_t)i * N + node;
            g1[i] = (STAGE >= 2 && valid) ? G1[o] : real(0);
            g2[i] = (STAGE >= 3 && valid) ? G2[o] : real(0);
            g3[i] = (STAGE >= 4 && valid) ? G3[o] : real(0);
            if (STAGE <= 3 && valid) {
                const real y0 = ye[o];
                ys[0][i] = (STAGE == 1) ? y0 : (STAGE == 2) ? y0 + A21 * g1[i] : y0 + A31 * g1[i] + A32 * g2[i];
            }
            if (STAGE == 4) k[0][i] = valid ? F[o] : real(0);    // stage 4 reuses f of stage 3
        }
        real a[RMT_V][RMT_V], l[RMT_V];
        unsigned mk = 0u;
        if (STAGE <= 3) {
            RmtLocal lc[1];
            RMT_PROFILE_AT(carry, base)
            rmt_rhs_block<1, true, false>(m, sh, ph, ys, valid ? 1 : 0, carry, k, flag, nullptr,
                                          STAGE == 1 ? lc : nullptr);
            ph ^= 1;
            if (STAGE == 3 && valid) {
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) F[(size_t)i * N + node] = k[0][i];
            }
            if (STAGE == 1) {
                rmt_noflags_t scratch_flag;
#if RMT_MODEL == 0 && !RMT_ROS_JAC_FD
                {
                    RmtNode ndj;
                    real rj[RMT_R];
                    (void)rmt_node_pre(m, ys[0], ndj);
                    RMT_PROFILE_NODE(m, ndj, node)
                    rmt_node_jac(m, ndj, ys[0], lc[0].P, a, rj, scratch_flag);
                }
#else
#pragma unroll
                for (int c = 0; c < RMT_V; ++c) {                // column c of D_z by a forward difference
                    real yp[RMT_V], kp[RMT_V];
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) yp[i] = ys[0][i];
                    const real d = real(RMT_FP32 ? 3e-4 : 1.5e-8) * rmt_max(rmt_abs(ys[0][c]), real(1e-3));
                    yp[c] += d;
                    const real id = rmt_rcp(yp[c] - ys[0][c]);
                    RmtNode ndp;
                    (void)rmt_node_pre(m, yp, ndp);
                    RMT_PROFILE_NODE(m, ndp, node)
                    rmt_node_post(m, ndp, yp, lc[0].up, lc[0].P, kp, scratch_flag);
#pragma unroll
                    for (int r = 0; r < RMT_V; ++r) a[r][c] = -(kp[r] - k[0][r]) * id;
                }
#endif
                if (node > 0) {                                  // upwind coupling active? (clamp, :4093)
#pragma unroll
                    for (int i = 0; i < RMT_S; ++i) mk |= (lc[0].up[i] > RMT_EPS) ? (1u << i) : 0u;
#if !RMT_ISO
                    mk |= 1u << RMT_S;
#endif
                }
#if RMT_MODEL != 0
                {   // d f_r / d up_r (diagonal; f is linear in `up`): node dependent in model M2
                    real upp[RMT_V], kp[RMT_V], dd[RMT_V];
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) {
                        dd[i] = real(RMT_FP32 ? 3e-4 : 1.5e-8) * rmt_max(rmt_abs(lc[0].up[i]), real(1e-3));
                        upp[i] = lc[0].up[i] + dd[i];
                        dd[i] = upp[i] - lc[0].up[i];
                    }
                    RmtNode nd0;
                    (void)rmt_node_pre(m, ys[0], nd0);
                    rmt_node_post(m, nd0, ys[0], upp, lc[0].P, kp, scratch_flag);
#pragma unroll
                    for (int r = 0; r < RMT_V; ++r) {
                        l[r] = (kp[r] - k[0][r]) * rmt_rcp(dd[r]);
                        if (valid) coup[(size_t)r * N + node] = l[r];
                        l[r] = ((mk >> r) & 1u) ? l[r] : real(0);
                    }
                }
#endif
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) a[i][i] += inv_gh;  // A = I/(gamma h) - D
                const real pv = rmt_invert(a);
                if (valid) {
                    pivmin = rmt_min(pivmin, pv);
#pragma unroll
                    for (int r = 0; r < RMT_V; ++r)
#pragma unroll
                        for (int c = 0; c < RMT_V; ++c) ainv[(size_t)(r * RMT_V + c) * N + node] = a[r][c];
                    mask[node] = mk;
                }
            }
        }
        if (STAGE >= 2) {
            if (valid) mk = mask[node];
#pragma unroll
            for (int r = 0; r < RMT_V; ++r) {
#pragma unroll
                for (int c = 0; c < RMT_V; ++c) a[r][c] = valid ? ainv[(size_t)(r * RMT_V + c) * N + node] : real(0);
#if RMT_MODEL != 0
                l[r] = (((mk >> r) & 1u) && valid) ? coup[(size_t)r * N + node] : real(0);
#endif
            }
        }
#if RMT_MODEL == 0
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) l[r] = ((mk >> r) & 1u) ? ((r < RMT_S) ? cs : ct) : real(0);
#endif
        // right-hand side of the stage, p = Ainv b, then the Jacobi sweeps over the upwind coupling
        real p[RMT_V], xv[RMT_V];
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) {
            real bv = k[0][r];
            if (STAGE == 2) bv += C21 * g1[r] * ih;
            if (STAGE == 3) bv += (C31 * g1[r] + C32 * g2[r]) * ih;
            if (STAGE == 4) bv += (C41 * g1[r] + C42 * g2[r] + C43 * g3[r]) * ih;
            xv[r] = valid ? bv : real(0);
        }
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) {
            real acc = real(0);
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) acc += a[r][c] * xv[c];
            p[r] = valid ? acc : real(0);
        }
#pragma unroll
        for (int r = 0; r < RMT_V; ++r)
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) a[r][c] = valid ? a[r][c] * l[c] : real(0);
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) xv[r] = p[r];
        real cout[RMT_V];
        rmt_sweep_carry(sh, xc);
        for (int it = 0; it <= sweeps; ++it, ph ^= 1) {           // last pass only publishes the boundary
            real xup[RMT_V];
            rmt_shift_up(sh, ph, xv, xup, cout, it == sweeps);
            if (it < sweeps) {
#pragma unroll
                for (int r = 0; r < RMT_V; ++r) {
                    real acc = p[r];
#pragma unroll
                    for (int c = 0; c < RMT_V; ++c) acc += a[r][c] * xup[c];
                    xv[r] = acc;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) xc[i] = cout[i];
        if (valid) {
#pragma unroll
            for (int r = 0; r < RMT_V; ++r) Gout[(size_t)r * N + node] = xv[r];
        }
    }
}

// ---- RODAS4 ------------------------------------------------------------------------------------
// Default scheme of the stiff stepper (RMT_ROS_SCHEME 1): Hairer & Wanner's RODAS4, a 6-stage,
// stiffly accurate, L-stable Rosenbrock method of order 4 with an embedded 3rd-order solution
// (coefficients in the k-form used by e.g. Numerical Recipes 3rd ed. "StepperRoss"; gamma = 1/4):
//     Y_i = y + sum_j a_ij G_j,   (I/(gamma h) - J) G_i = f(Y_i) + sum_j c_ij G_j / h,   i = 1..6,
//     Y_6 = Y_5 + G_5,   y_new = Y_6 + G_6,   error estimate = G_6.
// On the reference's DME case it needs 5x fewer linear solves than the Kaps-Rentrop pair for the
// same outlet accuracy, with a smooth error and almost no rejected steps (tools/ros_method_study.py,
// profiles/round1_ros_scheme.md), and being L-stable it does not ring after long steps.
#ifndef RMT_ROS_SCHEME
#define RMT_ROS_SCHEME 1
#endif
#define RMT_RODAS_GAM 0.25
#if RMT_FORCING && (RMT_ROS_SCHEME != 1 || RMT_ROS_QUAD)
#error "RMT_FORCING: the stiff stepper carries the forcing in its RODAS4 one-node-per-lane form only"
#endif
// ---- RODAS4, node blocks outermost ---------------------------------------------------------------
// Walking all node blocks once per stage (the layout of rmt_ros_stage) parks G_1..G_5 and the block
// inverses in memory (5 V + V^2 doubles per node written and read back every step).  Information
// only travels downstream, and stage i of block b needs nothing but stage i of block b-1, so the
// loops can be swapped: for every node block run ALL six stages back to back, with one carry
// {pressure, upstream state, upstream G_i} PER STAGE handed from block to block through LDS.  The
// inverse then never leaves the registers, the G_j of the block live in LDS (5 V block doubles), and
// a step touches memory twice per node: read y, write y_new (stage-outermost, with G_j and the
// inverses in memory: 0.086 s for the 256 x 1024 x 0.5 s job; this order: 0.064 s).
// RMT_FORCING (11_forcing.inc): the stepper is non-autonomous.  Stage i evaluates f(t + c_i h, Y_i) - member and inlet
// hand-over at that time - and its right-hand side gains h d_i f_t; f_t = (f(t + del, y_n) - f(t, y_n))/del comes from ONE
// more RHS pass per node block and step attempt, ahead of the block's stage 1, with a {pressure, upstream state} hand-over
// of its own (slot 6: a changed p0 moves the pressure of every node downstream).  A launch whose forcing is constant (a
// hold between two breakpoints) skips the pass and adds nothing.
#if RMT_FORCING
#define RMT_ROS_NCARRY 7
#define RMT_M_ARG m_launch
#define RMT_F_DECL , const double* __restrict__ frow, const double ft, const double fh, const bool fconst, real (&ftv)[RMT_V]
#define RMT_F_PASS , frow, ft, fh, fconst, ftv
#else
#define RMT_ROS_NCARRY 6
#define RMT_M_ARG m
#define RMT_F_DECL
#define RMT_F_PASS
#endif
struct RmtRodasCarry {
    double P[RMT_ROS_NCARRY];
    real up[RMT_ROS_NCARRY][RMT_V];
    real xc[6][RMT_V];
};

// ---- Jacobi sweeps, two steps at a time --------------------------------------------------------------
// The stage equation of node z is x_z = p_z + M_z x_{z-1} with p = A^-1 b, M = A^-1 diag(l) (l = d f_z / d y_{z-1},
// the upwind coupling); a Jacobi sweep moves information one node downstream.  Substituting the equation of
// node z-1 gives x_z = q_z + N_z x_{z-2} with
//     q_z = p_z + M_z p_{z-1}   (one matrix-vector product per stage),
//     N_z = M_z M_{z-1}         (one VxV matrix product per node block and STEP: the Jacobian is frozen over the stages),
// and one sweep of THIS recurrence is two Jacobi steps for the price of one: V^2 FMAs and two lane shifts,
// without the l-scaling.  Lane 0 of each wave has no lane-1 to take M_{z-1} and p_{z-1} from; it keeps the
// one-step form with the boundary value x_{z-1} that the previous wave (block, chunk) publishes - in the same
// code, by shifting in the identity for M_{z-1} and zero for p_{z-1} - and lane 1 then finds x_{z-2} = that same
// boundary value.  With the boundary refreshed before every sweep the iterates are those of plain Jacobi with
// the boundary refreshed every second step (the scheme measured in round 2 as RMT_ROS_XCH 2), at 0.47 of the
// instructions; profiles/round2_issue_model.md says why the instruction count is what matters here.
// (Round 2 also tried the sweeps on a packed-fp32 correction: same errors, +1.5 %, removed.)
#ifndef RMT_ROS_TWOSTEP
#define RMT_ROS_TWOSTEP 1
#endif
template <int STAGE, int CH = 0>
__device__ __forceinline__ void rmt_rodas_bs(const RmtMember& RMT_M_ARG, RmtShared& sh, RmtRodasCarry& rc, int& ph,
                                             real (*s_g)[RMT_V][RMT_BLOCK], const real (&y0)[RMT_V],
                                             const bool valid, const int node, real (&a)[RMT_V][RMT_V],
                                             real (&l)[RMT_V], unsigned& mk, real (&ynew)[RMT_V],
                                             const real inv_gh, const real ih, const int sweeps,
                                             rmt_flags_t& flag, real& pivmin, const double rtol,
                                             const double atol, double& errloc, bool& bad,
                                             RmtChainCtx* ctx, real (&nn)[RMT_V][RMT_V] RMT_F_DECL) {
#if RMT_FORCING
    RmtMember m = m_launch;                              // the member at this stage's time t + c_i h
    rmt_forcing_apply(m, frow, ft + rmt_rodas_t<STAGE>::c * fh);
#endif
    const real A[6][5] = {{0, 0, 0, 0, 0}, {real(1.544), 0, 0, 0, 0},
        {real(0.9466785280815826), real(0.2557011698983284), 0, 0, 0},
        {real(3.314825187068521), real(2.896124015972201), real(0.9986419139977817), 0, 0},
        {real(1.221224509226641), real(6.019134481288629), real(12.53708332932087), real(-0.6878860361058950), 0},
        {real(1.221224509226641), real(6.019134481288629), real(12.53708332932087), real(-0.6878860361058950), real(1)}};
    const real Cc[6][5] = {{0, 0, 0, 0, 0}, {real(-5.6688), 0, 0, 0, 0},
        {real(-2.430093356833875), real(-0.2063599157091915), 0, 0, 0},
        {real(-0.1073529058151375), real(-9.594562251023355), real(-20.47028614809616), 0, 0},
        {real(7.496443313967647), real(-10.24680431464352), real(-33.99990352819905), real(11.70890893206160), 0},
        {real(8.083246795921522), real(-7.981132988064893), real(-31.52159432874371), real(16.31930543123136),
         real(-6.058818238834054)}};
    const int tid = threadIdx.x;
    real ys[1][RMT_V], k[1][RMT_V], cg[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) {
        real st = y0[i], cc = real(0);
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            if (q < STAGE - 1) {
                const real g = s_g[q][i][tid];
                st += A[STAGE - 1][q] * g;
                cc += Cc[STAGE - 1][q] * g;
            }
        }
        ys[0][i] = st;                                   // (lanes beyond the end hold the safe inlet state)
        cg[i] = cc * ih;
    }
    RmtCarry carry;                                      // this stage's hand-over from the previous block
    carry.P = rc.P[STAGE - 1];
    real xc[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) { carry.up[i] = rc.up[STAGE - 1][i]; xc[i] = rc.xc[STAGE - 1][i]; }
    RMT_PROFILE_AT(carry, node - tid)                    // the block's first node
    RmtLocal lc[1];
    // Python-exception tests on stage 1 (f at the accepted state y_n) like the explicit steppers; the later
    // stages are evaluated test-free unless RMT_CHECK_ALL_STAGES (a failure there still ends non-finite -> rejected)
    rmt_noflags_t nof_stage;
    (void)nof_stage;
#if !RMT_ROS_JAC_FD
    // stage 1 also returns the analytic node Jacobian -D_z (one evaluation of the rates AND their partials)
    if (STAGE == 1 || RMT_CHECK_ALL_STAGES)
        rmt_rhs_block<1, true, CH>(m, sh, ph, ys, valid ? 1 : 0, carry, k, flag, ctx, STAGE == 1 ? lc : nullptr,
                                   nullptr, 0, STAGE == 1 ? a : nullptr);
    else
        rmt_rhs_block<1, true, CH>(m, sh, ph, ys, valid ? 1 : 0, carry, k, nof_stage, ctx);
#else
    if (STAGE == 1 || RMT_CHECK_ALL_STAGES)
        rmt_rhs_block<1, true, CH>(m, sh, ph, ys, valid ? 1 : 0, carry, k, flag, ctx, STAGE == 1 ? lc : nullptr);
    else
        rmt_rhs_block<1, true, CH>(m, sh, ph, ys, valid ? 1 : 0, carry, k, nof_stage, ctx);
#endif
    ph ^= 1;
#if RMT_FORCING
    if (STAGE == 1) {                                    // ftv arrives as f(t + del, y_n); k = f(t, y_n)
        const real idel = fconst ? real(0) : real(1.0 / (RMT_FT_FRAC * fh));
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) ftv[r] = fconst ? real(0) : (ftv[r] - k[0][r]) * idel;
    }
#endif
    if (STAGE == 1) {
        rmt_noflags_t scratch_flag;
        (void)scratch_flag;
#if !RMT_ROS_JAC_FD
#else
#pragma unroll
        for (int c = 0; c < RMT_V; ++c) {                        // column c of D_z by a forward difference
            real yp[RMT_V], kp[RMT_V];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) yp[i] = ys[0][i];
            const real d = real(RMT_FP32 ? 3e-4 : 1.5e-8) * rmt_max(rmt_abs(ys[0][c]), real(1e-3));
            yp[c] += d;
            const real id = rmt_rcp(yp[c] - ys[0][c]);
            RmtNode ndp;
            (void)rmt_node_pre(m, yp, ndp);
            RMT_PROFILE_NODE(m, ndp, node)
            rmt_node_post(m, ndp, yp, lc[0].up, lc[0].P, kp, scratch_flag);
#pragma unroll
            for (int r = 0; r < RMT_V; ++r) a[r][c] = -(kp[r] - k[0][r]) * id;
        }
#endif
        mk = 0u;
        if (node > 0) {                                          // upwind coupling active? (clamp)
#pragma unroll
            for (int i = 0; i < RMT_S; ++i) mk |= (lc[0].up[i] > RMT_EPS) ? (1u << i) : 0u;
#if !RMT_ISO
            mk |= 1u << RMT_S;
#endif
        }
#if RMT_MODEL != 0 && !RMT_ROS_JAC_FD
        {   // d f_r / d up_r (diagonal; f is linear in `up`): node dependent in model M2, returned with the Jacobian
#pragma unroll
            for (int r = 0; r < RMT_V; ++r) l[r] = (((mk >> r) & 1u) && valid) ? lc[0].lco[r] : real(0);
        }
#elif RMT_MODEL != 0
        {   // d f_r / d up_r by a forward difference
            real upp[RMT_V], kp[RMT_V], dd[RMT_V];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) {
                dd[i] = real(RMT_FP32 ? 3e-4 : 1.5e-8) * rmt_max(rmt_abs(lc[0].up[i]), real(1e-3));
                upp[i] = lc[0].up[i] + dd[i];
                dd[i] = upp[i] - lc[0].up[i];
            }
            RmtNode nd0;
            (void)rmt_node_pre(m, ys[0], nd0);
            rmt_node_post(m, nd0, ys[0], upp, lc[0].P, kp, scratch_flag);
#pragma unroll
            for (int r = 0; r < RMT_V; ++r)
                l[r] = (((mk >> r) & 1u) && valid) ? (kp[r] - k[0][r]) * rmt_rcp(dd[r]) : real(0);
        }
#else
        {
            const real cs = m.f1 * m.inv_dz, ct = m.ft * m.inv_dz;   // d f_z / d y_{z-1}
#pragma unroll
            for (int r = 0; r < RMT_V; ++r) l[r] = (((mk >> r) & 1u) && valid) ? ((r < RMT_S) ? cs : ct) : real(0);
        }
#endif
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) a[i][i] += inv_gh;       // A = I/(gamma h) - D
        const real pv = rmt_invert(a);
        if (valid) pivmin = rmt_min(pivmin, pv);
        else {
#pragma unroll
            for (int r = 0; r < RMT_V; ++r)
#pragma unroll
                for (int c = 0; c < RMT_V; ++c) a[r][c] = real(0);
        }
        // N = M_z M_{z-1}, column by column: column c of diag(l_z) M_{z-1} = l_z .* (A_{z-1}^-1)[:, c] l_{z-1}[c]
        // (lane 0 of a wave: the identity instead of M_{z-1}, see above)
        if (RMT_ROS_TWOSTEP) {
            const real one0 = ((tid & 63) == 0) ? real(1) : real(0);
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) {
                const real lu = rmt_lane_up1(l[c]);
                real col[RMT_V];
#pragma unroll
                for (int kk = 0; kk < RMT_V; ++kk) {
                    real v = rmt_lane_up1(a[kk][c]) * lu;
                    if (kk == c) v += one0;
                    col[kk] = v * l[kk];
                }
#pragma unroll
                for (int r = 0; r < RMT_V; ++r) {
                    real acc = real(0);
#pragma unroll
                    for (int kk = 0; kk < RMT_V; ++kk) acc += a[r][kk] * col[kk];
                    nn[r][c] = acc;
                }
            }
        }
    }
    // right-hand side of the stage, p = Ainv b, Jacobi sweeps x <- p + Ainv (l .* x_up)
    real p[RMT_V], xv[RMT_V];
#pragma unroll
    for (int r = 0; r < RMT_V; ++r) xv[r] = valid ? k[0][r] + cg[r] : real(0);
#if RMT_FORCING
    if (rmt_rodas_t<STAGE>::d != 0.0 && !fconst) {       // + h d_i f_t
        const real hd = real(rmt_rodas_t<STAGE>::d * fh);
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) xv[r] = valid ? xv[r] + hd * ftv[r] : real(0);
    }
#endif
#pragma unroll
    for (int r = 0; r < RMT_V; ++r) {
        real acc = real(0);
#pragma unroll
        for (int c = 0; c < RMT_V; ++c) acc += a[r][c] * xv[c];
        p[r] = acc;
    }
#pragma unroll
    for (int r = 0; r < RMT_V; ++r) xv[r] = p[r];
    real cout[RMT_V];
    rmt_sweep_carry(sh, xc);                                      // (a chunk's first block: overwritten per sweep by the link)
    real u[RMT_V];
    if (RMT_ROS_TWOSTEP) {
    // q = p + M p_up; the sweeps start from x = p (two-step sweep k then yields Jacobi iterate 2k)
    real q[RMT_V];
    {
        real pu[RMT_V];
#pragma unroll
        for (int c = 0; c < RMT_V; ++c) pu[c] = rmt_lane_up1(p[c]) * l[c];
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) {
            real acc = p[r];
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) acc += a[r][c] * pu[c];
            q[r] = acc;
        }
    }
    // `sweeps` (even, see where it is computed) counts Jacobi steps.  Per two-step sweep: the boundary values
    // cross the waves (LDS + one barrier; the link of a chained reactor), u = x shifted by one lane with lane 0
    // = the boundary value, then u shifted once more IN PLACE by a DPP move that leaves lane 0 untouched.
    for (int it = 0; it < sweeps; it += 2) {
        if (CH == 2) rmt_shift_up_chain(sh, ph, xv, u, cout, true, *ctx);
        else rmt_shift_up(sh, ph, xv, u, cout, false);
        ph ^= 1;
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) u[i] = rmt_lane_up1_keep(u[i], u[i]);
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) {
            real acc = q[r];
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) acc += nn[r][c] * u[c];
            xv[r] = acc;
        }
    }
    } else {
    // one Jacobi step per sweep, boundary refreshed every second one: lanes >= 1 take the upstream iterate by a
    // DPP move that leaves lane 0 (the boundary value of the last exchange) untouched
    for (int it = 0; it < sweeps; it += 2) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (half == 0) {
                if (CH == 2) rmt_shift_up_chain(sh, ph, xv, u, cout, true, *ctx);
                else rmt_shift_up(sh, ph, xv, u, cout, false);
                ph ^= 1;
            } else {
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) u[i] = rmt_lane_up1_keep(u[i], xv[i]);
            }
            real xs[RMT_V];
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) xs[c] = u[c] * l[c];
#pragma unroll
            for (int r = 0; r < RMT_V; ++r) {
                real acc = p[r];
#pragma unroll
                for (int c = 0; c < RMT_V; ++c) acc += a[r][c] * xs[c];
                xv[r] = acc;
            }
        }
    }
    }
    // last pass: only publishes the boundary (the value handed to the next node block)
    if (CH == 2) rmt_shift_up_chain(sh, ph, xv, u, cout, false, *ctx);
    else rmt_shift_up(sh, ph, xv, u, cout, true);
    ph ^= 1;
    // hand-over to the next block: the values are identical in every thread, one writes them to LDS
    // (every reader of this stage's slot has passed the barriers above; the next one is behind more)
    if (tid == 0) {
        rc.P[STAGE - 1] = carry.P;
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) { rc.up[STAGE - 1][i] = carry.up[i]; rc.xc[STAGE - 1][i] = cout[i]; }
    }
    if (STAGE < 6) {
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) s_g[STAGE - 1][r][tid] = xv[r];
    } else {
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) {
            const double yn = (double)ys[0][r] + (double)xv[r];
            ynew[r] = real(yn);
            if (valid) {
                bad |= !__builtin_isfinite(yn);
                errloc = fmax(errloc, fabs((double)xv[r]) / (atol + rtol * fmax(fabs((double)y0[r]), fabs(yn))));
            }
        }
    }
}

__device__ __forceinline__ void rmt_rodas_blocks(const RmtMember& m, RmtShared& sh, RmtRodasCarry& rc, int& ph,
                                                 real (*s_g)[RMT_V][RMT_BLOCK], const real* ye, real* yout,
                                                 const int N, const real inv_gh, const real ih,
                                                 const int sweeps, rmt_flags_t& flag, real& pivmin,
                                                 const double rtol, const double atol, double& errloc,
                                                 bool& bad
#if RMT_FORCING
                                                 , const double* __restrict__ frow, const double ft, const double fh
#endif
                                                 ) {
#if RMT_FORCING
    const bool fconst = rmt_forcing_constant(frow);
#endif
    __syncthreads();                                     // the previous step's readers of rc are done
    if (threadIdx.x == 0) {
#pragma unroll
        for (int st = 0; st < 6; ++st) {
            RmtCarry c0;
#if RMT_FORCING
            RmtMember ms = m;                            // each stage: the inlet at its own time
            rmt_forcing_apply(ms, frow, ft + rmt_rodas_c(st) * fh);
            rmt_carry_inlet(ms, c0);
#else
            rmt_carry_inlet(m, c0);
#endif
            rc.P[st] = c0.P;
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) { rc.up[st][i] = c0.up[i]; rc.xc[st][i] = real(0); }
        }
#if RMT_FORCING
        {                                                // slot 6: the pass that yields f(t + del, y_n)
            RmtCarry c0;
            RmtMember ms = m;
            rmt_forcing_apply(ms, frow, ft);
            rmt_forcing_shift(ms, frow, RMT_FT_FRAC * fh);
            rmt_carry_inlet(ms, c0);
            rc.P[6] = c0.P;
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) rc.up[6][i] = c0.up[i];
        }
#endif
    }
    __syncthreads();
    for (int base = 0; base < N; base += RMT_BLOCK) {
        const int node = base + (int)threadIdx.x;
        const bool valid = node < N;
        real y0[RMT_V], ynew[RMT_V], a[RMT_V][RMT_V], l[RMT_V];
        real nn[RMT_V][RMT_V];
        unsigned mk = 0u;
        rmt_safe_state(m, y0);
        if (valid) {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) y0[i] = ye[(size_t)i * N + node];
        }
#if RMT_FORCING
        real ftv[RMT_V];
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) ftv[i] = real(0);
        if (!fconst) {                                   // (workgroup-uniform) f(t + del, y_n) of this block, test-free
            RmtMember md = m;
            rmt_forcing_apply(md, frow, ft);
            rmt_forcing_shift(md, frow, RMT_FT_FRAC * fh);
            RmtCarry carry;
            carry.P = rc.P[6];
            real ysd[1][RMT_V], kd[1][RMT_V];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) { carry.up[i] = rc.up[6][i]; ysd[0][i] = y0[i]; }
            RMT_PROFILE_AT(carry, base)
            rmt_noflags_t nof_ft;
            rmt_rhs_block<1, true, 0>(md, sh, ph, ysd, valid ? 1 : 0, carry, kd, nof_ft);
            ph ^= 1;
            if (threadIdx.x == 0) {                      // (every reader of slot 6 is past the barrier inside)
                rc.P[6] = carry.P;
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) rc.up[6][i] = carry.up[i];
            }
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) ftv[i] = kd[0][i];
        }
#endif
        rmt_rodas_bs<1>(m, sh, rc, ph, s_g, y0, valid, node, a, l, mk, ynew, inv_gh, ih, sweeps, flag, pivmin, rtol, atol, errloc, bad, nullptr, nn RMT_F_PASS);
        rmt_rodas_bs<2>(m, sh, rc, ph, s_g, y0, valid, node, a, l, mk, ynew, inv_gh, ih, sweeps, flag, pivmin, rtol, atol, errloc, bad, nullptr, nn RMT_F_PASS);
        rmt_rodas_bs<3>(m, sh, rc, ph, s_g, y0, valid, node, a, l, mk, ynew, inv_gh, ih, sweeps, flag, pivmin, rtol, atol, errloc, bad, nullptr, nn RMT_F_PASS);
        rmt_rodas_bs<4>(m, sh, rc, ph, s_g, y0, valid, node, a, l, mk, ynew, inv_gh, ih, sweeps, flag, pivmin, rtol, atol, errloc, bad, nullptr, nn RMT_F_PASS);
        rmt_rodas_bs<5>(m, sh, rc, ph, s_g, y0, valid, node, a, l, mk, ynew, inv_gh, ih, sweeps, flag, pivmin, rtol, atol, errloc, bad, nullptr, nn RMT_F_PASS);
        rmt_rodas_bs<6>(m, sh, rc, ph, s_g, y0, valid, node, a, l, mk, ynew, inv_gh, ih, sweeps, flag, pivmin, rtol, atol, errloc, bad, nullptr, nn RMT_F_PASS);
        if (valid) {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) yout[(size_t)i * N + node] = ynew[i];
        }
    }
}

// bound of the upwind coupling d f_z / d y_{z-1} (sets the contraction factor of the Jacobi sweeps and the step cap)
__device__ __forceinline__ double rmt_ros_coupling_bound(const RmtMember& m) {
#if RMT_MODEL == 0
    return (double)rmt_max(m.f1, m.ft) * (double)m.inv_dz;
#else
    double c0 = 0.0;              // model M2: from the feed state, (SuGaVe0/eps)/dz, with 25 % head-room
    for (int i = 0; i < RMT_S; ++i) c0 += (double)m.cin[i];
    return 1.25 * (double)m.f1 * ((double)m.rho_k * c0 / (double)m.p0) * (double)m.inv_dz;
#endif
}
#ifndef RMT_ROS_WAVES
#define RMT_ROS_WAVES 1          // min waves per SIMD asked from the register allocator
#endif
#if !RMT_ROS_QUAD             // (quad layout: the kernels of the same names live in 61_ros4_quad.inc)
extern "C" __global__ __launch_bounds__(RMT_BLOCK, RMT_ROS_WAVES) void rmt_n2_ros4_mem(
        real* __restrict__ y, real* __restrict__ work, unsigned* __restrict__ maskbuf,
        const double* __restrict__ members, const int N, const int E, const double t0,
        const double t1, const double rtol, const double atol, const double h0,
        const long long max_steps, double* __restrict__ stats, unsigned* __restrict__ flags) {
    __shared__ RmtShared sh;
#if RMT_ROS_SCHEME == 1
    __shared__ real s_g[5][RMT_V][RMT_BLOCK];       // G_1..G_5 of the current node block
    __shared__ RmtRodasCarry s_rc;                  // per-stage hand-over between node blocks
#endif
    rmt_math_init();
    const int e = blockIdx.x;
    RmtMember m;
    rmt_load_member(members + (size_t)e * RMT_NM, m);
    RMT_PROFILE_BIND(m, e, N)
    const size_t per = (size_t)RMT_V * N, tot = per * E;
    real* ye = y + e * per;
    real* F = work + 0 * tot + e * per;
    real* G1 = work + 1 * tot + e * per;
    real* G2 = work + 2 * tot + e * per;
    real* G3 = work + 3 * tot + e * per;
    real* G4 = work + 4 * tot + e * per;
    real* YS = work + 5 * tot + e * per;
    real* ainv = work + 7 * tot + (size_t)e * RMT_V * RMT_V * N;
    real* coup = work + (7 + RMT_V) * tot + e * per;      // M2 only: per-node upwind coupling
    unsigned* mask = maskbuf + (size_t)e * N;
#if RMT_ROS_SCHEME != 1
    // Kaps-Rentrop / Shampine weights of the solution and of the error estimate (gamma = 1/2)
    const double B1 = 19.0 / 9, B2 = 0.5, B3 = 25.0 / 108, B4 = 125.0 / 108, E1 = 17.0 / 54, E2 = 7.0 / 36,
                 E4 = 125.0 / 108;
#endif
    const double cmax = rmt_ros_coupling_bound(m);
    // step cap: Jacobi contraction factor <= 1/2; the Kaps-Rentrop pair (A- but not L-stable: long steps
    // near steady state damp the stiff modes only slowly) additionally at most RMT_ROS_MAX_FRAC of the interval
#if RMT_ROS_SCHEME == 1
    const double GAM = RMT_RODAS_GAM;          // L-stable: only the Jacobi contraction limits the step
    const double hcap = fmin((RMT_ROS_RHO_MAX / (1.0 - RMT_ROS_RHO_MAX)) / (GAM * cmax), 0.25 * (t1 - t0));
#else
    const double GAM = RMT_ROS_GAM;
    const double hcap = fmin(1.0 / (RMT_ROS_GAM * cmax), RMT_ROS_MAX_FRAC * (t1 - t0));
#endif
    // the sweeps only have to resolve the stage vectors well below the step's error tolerance
    const double logtol = log(fmin(1e-6, fmax(1e-12, RMT_ROS_SOLVE_TOL * rtol)));
    rmt_flags_t flag, trial;
    rmt_flags_clear(flag);
    unsigned lflag = 0u;
    int ph = 0, rp = 0;
    double t = t0, h = fmin(rmt_initial_step(h0, stats, e), hcap);
    long long nacc = 0, nrej = 0;
    while (t < t1 && nacc + nrej < max_steps) {
        bool last = false;
        const double hfull = h;
        if (t + h >= t1) { h = t1 - t; last = true; }
        rmt_flags_clear(trial);
        const real inv_gh = real(1.0 / (GAM * h));
        const double rho = cmax / (1.0 / (GAM * h) + cmax);
        int sweeps = (int)ceil(logtol / log(rho)) + 1;             // rho^sweeps <= 1e-2*rtol
        sweeps = sweeps < 2 ? 2 : (sweeps > RMT_ROS_MAX_SWEEPS ? RMT_ROS_MAX_SWEEPS : sweeps);
#if RMT_ROS_SCHEME == 1
        sweeps += RMT_ROS_XCH - 1;                      // boundary values up to RMT_ROS_XCH - 1 sweeps old
#endif
#ifdef RMT_ROS_FIX_SWEEPS                       // timing experiments only (results are wrong with too few)
        sweeps = RMT_ROS_FIX_SWEEPS;
#endif
        sweeps = (sweeps + RMT_ROS_XCH - 1) / RMT_ROS_XCH * RMT_ROS_XCH;   // whole exchange periods (rmt_rodas_bs)
        real pivmin = real(__builtin_inf());
        const real ih = real(1.0 / h);
#if RMT_ROS_SCHEME == 1
        double errloc = 0.0;
        bool bad = false;
#if RMT_FORCING
        rmt_rodas_blocks(m, sh, s_rc, ph, s_g, ye, YS, N, inv_gh, ih, sweeps, trial, pivmin, rtol, atol, errloc, bad,
                         members + (size_t)e * RMT_NM, t, h);
#else
        rmt_rodas_blocks(m, sh, s_rc, ph, s_g, ye, YS, N, inv_gh, ih, sweeps, trial, pivmin, rtol, atol, errloc, bad);
#endif
#else
        rmt_ros_stage<1>(m, sh, ph, ye, F, G1, G2, G3, G1, ainv, mask, coup, N, inv_gh, ih, sweeps, trial, pivmin);
        rmt_ros_stage<2>(m, sh, ph, ye, F, G1, G2, G3, G2, ainv, mask, coup, N, inv_gh, ih, sweeps, trial, pivmin);
        rmt_ros_stage<3>(m, sh, ph, ye, F, G1, G2, G3, G3, ainv, mask, coup, N, inv_gh, ih, sweeps, trial, pivmin);
        rmt_ros_stage<4>(m, sh, ph, ye, F, G1, G2, G3, G4, ainv, mask, coup, N, inv_gh, ih, sweeps, trial, pivmin);
        // new state (into YS) and error estimate
        double errloc = 0.0;
        bool bad = false;
        for (int base = 0; base < N; base += RMT_BLOCK) {
            const int node = base + (int)threadIdx.x;
            if (node < N) {
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) {
                    const size_t o = (size_t)i * N + node;
                    const double g1 = G1[o], g2 = G2[o], g3 = G3[o], g4 = G4[o], yo = ye[o];
                    const double yn = yo + B1 * g1 + B2 * g2 + B3 * g3 + B4 * g4;
                    const double er = E1 * g1 + E2 * g2 + E4 * g4;
                    YS[o] = real(yn);
                    bad |= !__builtin_isfinite(yn);
                    errloc = fmax(errloc, fabs(er) / (atol + rtol * fmax(fabs(yo), fabs(yn))));
                }
            }
        }
#endif   // RMT_ROS_SCHEME
        bad |= !(pivmin > real(0));
        const double worst = rmt_block_max(sh, rp, (bad || !__builtin_isfinite(errloc)) ? 1.0e300 : errloc);
        rp ^= 1;
        double fac;
        if (worst >= 1.0e300) {
            fac = 0.25;
            ++nrej;
        } else if (worst <= 1.0) {
            t = last ? t1 : t + h;
            ++nacc;
            fac = (worst > 1.89e-4) ? 0.9 * rmt_exp(-0.25 * rmt_log(worst)) : 1.5 * 5.0;     // 4th order: grow <= 7.5x
            fac = fmin(fac, 5.0);
            { real* const tmp = ye; ye = YS; YS = tmp; }          // accepted: the buffers swap roles
            rmt_flags_merge(flag, trial);
        } else {
            ++nrej;
#if RMT_ROS_SCHEME == 1
            fac = fmax(0.2, 0.9 * rmt_exp(-0.25 * rmt_log(worst)));
#else
            fac = fmax(0.2, 0.9 * pow(worst, -1.0 / 3.0));
#endif
        }
        h = fmin(fmax(h * fac, 1e-14), hcap);
        if (last && t >= t1) h = fmin(fmax(h, hfull * fmin(fac, 1.0)), hcap);   // clipped last step: keep h_last
    }
    if (ye != y + e * per) {                                       // odd number of accepted steps: copy back
        real* const yout = y + e * per;
        for (int base = 0; base < N; base += RMT_BLOCK) {
            const int node = base + (int)threadIdx.x;
            if (node < N) {
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) yout[(size_t)i * N + node] = ye[(size_t)i * N + node];
            }
        }
    }
    if (t < t1) lflag |= RMT_FLAG_STEP;
    lflag |= rmt_flags_bits(flag);
    if (threadIdx.x == 0) {
        stats[(size_t)e * 4 + 0] = t;
        stats[(size_t)e * 4 + 1] = h;
        ((long long*)stats)[(size_t)e * 4 + 2] = nacc;
        ((long long*)stats)[(size_t)e * 4 + 3] = nrej;
    }
    if (lflag) atomicOr(&flags[e], lflag);
}

#if RMT_ROS_SCHEME == 1
// ===================================================================== kernel: stiff integrator, ONE reactor over many CUs
// rmt_n2_ros4_mem keeps a reactor on one workgroup: BASELINE's target shape - ONE long reactor - then uses
// one of 256 CUs.  Here reactor e is cut into C chunks of W nodes (W a multiple of RMT_BLOCK), one workgroup
// per chunk, T teams of C workgroups with T*C <= number of CUs (all resident), team t integrating reactors
// t, t+T, ...  Information only travels downstream, so the chunks form a pipeline fed through tagged-word
// links (rmt_link_send): per Rosenbrock stage the {upstream state, pressure} record of the RHS, per Jacobi
// sweep of the stage's linear solve the boundary iterate - synchronous Jacobi across the chunk boundary,
// executed with a time skew of one message latency per chunk - and after stage 6 the running maximum of the
// error norm.  The LAST chunk therefore holds the reactor's error norm; it publishes it in the team's
// decision slot, every chunk reads it and applies the same controller arithmetic, so t, h and the
// accept/reject history stay identical in all chunks without any other synchronisation.
// A step costs 6 stage times + the pipeline skew instead of 6 C stage times.
#if !RMT_FORCING && !RMT_PROFILE       // (a forced or profiled run keeps a reactor on one workgroup: the host selects rmt_n2_ros4_mem)
extern "C" __global__ __launch_bounds__(RMT_BLOCK, RMT_ROS_WAVES) void rmt_n2_ros4_chain(
        real* __restrict__ y, real* __restrict__ work, const double* __restrict__ members, const int N,
        const int E, const int C, const int T, const int W, const double t0, const double t1,
        const double rtol, const double atol, const double h0, const long long max_steps,
        double* __restrict__ stats, unsigned* __restrict__ flags, unsigned long long* __restrict__ rings,
        unsigned long long* __restrict__ decision, unsigned* __restrict__ abort_words) {
    __shared__ RmtShared sh;
    __shared__ real s_g[5][RMT_V][RMT_BLOCK];
    __shared__ RmtRodasCarry s_rc;
    __shared__ double s_dec[2];
    rmt_math_init();
    const int team = blockIdx.x / C, c = blockIdx.x % C;
    const int wave = threadIdx.x >> 6;
    RmtChainCtx ctx;
    ctx.has_in = ctx.has_out = false;
    ctx.sync_in = ctx.sync_out = nullptr;
    ctx.slots_in = nullptr;
    ctx.slots_out = nullptr;
    ctx.q = 0ull;
    ctx.abort = 0;
    ctx.chunk = c;
    const size_t link = (size_t)team * C + c;
    ctx.ring_in = rings + (link - (c > 0 ? 1 : 0)) * RMT_RING * RMT_LINK_WORDS;
    ctx.ring_out = rings + link * RMT_RING * RMT_LINK_WORDS;
    ctx.seq_in = ctx.seq_out = 1u;                       // the host clears the rings: tag 0 never matches
    ctx.abort_word = abort_words + team;
    ctx.dead = 0;
    ctx.bp = false;                                      // the decision rendezvous bounds the producer's lead
    ctx.bp_in = ctx.bp_out = nullptr;
    ctx.known = 0u;
    unsigned long long* const dec = decision + (size_t)team * 2;
    unsigned att = 0u;                                   // step attempts of this team = tag of the decision slot
    const int nlo = c * W, nhi = (nlo + W < N) ? nlo + W : N;
    const size_t per = (size_t)RMT_V * N;
    bool dead = false;
    int e = team;
    for (; e < E && !dead; e += T) {
        RmtMember m;
        rmt_load_member(members + (size_t)e * RMT_NM, m);
        real* ye = y + e * per;
        real* YS = work + e * per;
        const double cmax = rmt_ros_coupling_bound(m);
        const double GAM = RMT_RODAS_GAM;
        const double hcap = fmin((RMT_ROS_RHO_MAX / (1.0 - RMT_ROS_RHO_MAX)) / (GAM * cmax), 0.25 * (t1 - t0));
        const double logtol = log(fmin(1e-6, fmax(1e-12, RMT_ROS_SOLVE_TOL * rtol)));
        rmt_flags_t flag, trial;
        rmt_flags_clear(flag);
        unsigned lflag = 0u;
        int ph = 0, rp = 0;
        double t = t0, h = fmin(rmt_initial_step(h0, stats, e), hcap);
        long long nacc = 0, nrej = 0;
        while (t < t1 && nacc + nrej < max_steps && !dead) {
            bool last = false;
            const double hfull = h;
            if (t + h >= t1) { h = t1 - t; last = true; }
            rmt_flags_clear(trial);
            const real inv_gh = real(1.0 / (GAM * h));
            const double rho = cmax / (1.0 / (GAM * h) + cmax);
            int sweeps = (int)ceil(logtol / log(rho)) + 1;
            sweeps = sweeps < 2 ? 2 : (sweeps > RMT_ROS_MAX_SWEEPS ? RMT_ROS_MAX_SWEEPS : sweeps);
            sweeps += RMT_ROS_XCH - 1;                  // boundary values up to RMT_ROS_XCH - 1 sweeps old
#ifdef RMT_ROS_FIX_SWEEPS
            sweeps = RMT_ROS_FIX_SWEEPS;
#endif
            sweeps = (sweeps + RMT_ROS_XCH - 1) / RMT_ROS_XCH * RMT_ROS_XCH;   // whole exchange periods (rmt_rodas_bs)
            real pivmin = real(__builtin_inf());
            const real ih = real(1.0 / h);
            double errloc = 0.0;
            bool bad = false;
            att = rmt_seq_next(att);
            __syncthreads();                             // the previous attempt's readers of s_rc / s_dec are done
            if (threadIdx.x == 0) {
#pragma unroll
                for (int st = 0; st < 6; ++st) {
                    RmtCarry c0;
                    rmt_carry_inlet(m, c0);              // chunk 0: the inlet; later chunks overwrite P / up from the link
                    s_rc.P[st] = c0.P;
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) { s_rc.up[st][i] = c0.up[i]; s_rc.xc[st][i] = real(0); }
                }
            }
            __syncthreads();
            for (int base = nlo; base < nhi; base += RMT_BLOCK) {
                const int node = base + (int)threadIdx.x;
                const bool valid = node < nhi;
                ctx.has_in = (c > 0) && (base == nlo);
                ctx.has_out = (c < C - 1) && (base + RMT_BLOCK >= nhi);
                real y0[RMT_V], ynew[RMT_V], a[RMT_V][RMT_V], l[RMT_V];
                real nn[RMT_V][RMT_V];
                unsigned mk = 0u;
                rmt_safe_state(m, y0);
                if (valid) {
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) y0[i] = ye[(size_t)i * N + node];
                }
                rmt_rodas_bs<1, 2>(m, sh, s_rc, ph, s_g, y0, valid, node, a, l, mk, ynew, inv_gh, ih, sweeps, trial, pivmin, rtol, atol, errloc, bad, &ctx, nn);
                rmt_rodas_bs<2, 2>(m, sh, s_rc, ph, s_g, y0, valid, node, a, l, mk, ynew, inv_gh, ih, sweeps, trial, pivmin, rtol, atol, errloc, bad, &ctx, nn);
                rmt_rodas_bs<3, 2>(m, sh, s_rc, ph, s_g, y0, valid, node, a, l, mk, ynew, inv_gh, ih, sweeps, trial, pivmin, rtol, atol, errloc, bad, &ctx, nn);
                rmt_rodas_bs<4, 2>(m, sh, s_rc, ph, s_g, y0, valid, node, a, l, mk, ynew, inv_gh, ih, sweeps, trial, pivmin, rtol, atol, errloc, bad, &ctx, nn);
                rmt_rodas_bs<5, 2>(m, sh, s_rc, ph, s_g, y0, valid, node, a, l, mk, ynew, inv_gh, ih, sweeps, trial, pivmin, rtol, atol, errloc, bad, &ctx, nn);
                rmt_rodas_bs<6, 2>(m, sh, s_rc, ph, s_g, y0, valid, node, a, l, mk, ynew, inv_gh, ih, sweeps, trial, pivmin, rtol, atol, errloc, bad, &ctx, nn);
                if (valid) {
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) YS[(size_t)i * N + node] = ynew[i];
                }
            }
            bad |= !(pivmin > real(0));
            double worst = rmt_block_max(sh, rp, (bad || !__builtin_isfinite(errloc)) ? 1.0e300 : errloc);
            rp ^= 1;
            // running maximum down the chain, the last chunk's value (= the reactor's) back to everybody
            if (wave == 0) {
                int st = ctx.dead;
                if (c > 0) {
                    st |= rmt_link_recv(rmt_ring_entry(ctx.ring_in, ctx.seq_in), ctx.seq_in, sh.cin[0], 1, ctx.abort_word, st);
                    worst = fmax(worst, sh.cin[0][0]);
                }
                if ((threadIdx.x & 63) == 0) sh.cst[0][0] = worst;
                if (c < C - 1) {
                    rmt_link_send(rmt_ring_entry(ctx.ring_out, ctx.seq_out), ctx.seq_out, sh.cst[0], 1);
                    st |= rmt_link_recv(dec, att, sh.cin[1], 1, ctx.abort_word, st);
                    worst = sh.cin[1][0];
                } else {
                    rmt_link_send(dec, att, sh.cst[0], 1);
                }
                if ((threadIdx.x & 63) == 0) { s_dec[0] = worst; s_dec[1] = st ? 1.0 : 0.0; }
                ctx.dead |= st;
            }
            if (c > 0) ctx.seq_in = rmt_seq_next(ctx.seq_in);
            if (c < C - 1) ctx.seq_out = rmt_seq_next(ctx.seq_out);
            __syncthreads();
            worst = s_dec[0];
            if (s_dec[1] != 0.0) { dead = true; break; }
            double fac;
            if (worst >= 1.0e300) {
                fac = 0.25;
                ++nrej;
            } else if (worst <= 1.0) {
                t = last ? t1 : t + h;
                ++nacc;
                fac = (worst > 1.89e-4) ? 0.9 * rmt_exp(-0.25 * rmt_log(worst)) : 1.5 * 5.0;
                fac = fmin(fac, 5.0);
                { real* const tmp = ye; ye = YS; YS = tmp; }
                rmt_flags_merge(flag, trial);
            } else {
                ++nrej;
                fac = fmax(0.2, 0.9 * rmt_exp(-0.25 * rmt_log(worst)));
            }
            h = fmin(fmax(h * fac, 1e-14), hcap);
            if (last && t >= t1) h = fmin(fmax(h, hfull * fmin(fac, 1.0)), hcap);
        }
        if (ye != y + e * per) {                             // odd number of accepted steps: copy this chunk back
            real* const yout = y + e * per;
            for (int base = nlo; base < nhi; base += RMT_BLOCK) {
                const int node = base + (int)threadIdx.x;
                if (node < nhi) {
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) yout[(size_t)i * N + node] = ye[(size_t)i * N + node];
                }
            }
        }
        if (t < t1) lflag |= RMT_FLAG_STEP;
        lflag |= rmt_flags_bits(flag);
        if (threadIdx.x == 0 && c == 0) {
            stats[(size_t)e * 4 + 0] = t;
            stats[(size_t)e * 4 + 1] = h;
            ((long long*)stats)[(size_t)e * 4 + 2] = nacc;
            ((long long*)stats)[(size_t)e * 4 + 3] = nrej;
        }
        if (lflag) atomicOr(&flags[e], lflag);
    }
    if (dead && threadIdx.x == 0) {       // a link timed out: the team's remaining reactors were never integrated
        for (int e2 = e; e2 < E; e2 += T) atomicOr(&flags[e2], RMT_FLAG_STEP);
    }
}
#endif   // !RMT_FORCING && !RMT_PROFILE
#endif   // RODAS4
#endif   // !RMT_ROS_QUAD

#endif  // RMT_WITH_ROS4

