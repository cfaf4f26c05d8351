#if RMT_WITH_ROS4 && RMT_ROS_QUAD
// ===================================================================== stiff integrator for WIDE mechanisms: one node on four lanes
// rmt_rodas_bs (60_ros4.inc) keeps a node's V x V inverse - and the two-step product - in the registers of ONE lane:
// 2 x 49 doubles for the 6-species DME mechanism, 2 x 169 for the 12-species one, where the compiler spills 1000-1500
// VGPRs per lane and the sweep loops run out of scratch memory (1.3 ms per step of 64 x 512 nodes,
// profiles/round3_kcache.md; staging the matrix through the workspace did not cure it).  RMT_ROS_QUAD (the host sets it
// for V > 8, model N2) puts ONE NODE ON FOUR LANES instead:
//   * lane q = lane & 3 of the quad owns the matrix rows r = q, q + 4, q + 8, ... (RMT_QR = ceil(V / 4) rows of V
//     doubles: 104 registers for V = 13) - the Gauss-Jordan inversion, p = A^-1 b and every Jacobi sweep cost a quarter
//     of the FMAs per lane, and nothing spills outside the once-per-step Jacobian assembly;
//   * the node function (kinetics, balances) is evaluated REDUNDANTLY by the four lanes - it is a per-node dependent
//     chain that cannot be split across lanes, and 16 nodes per wave instead of 64 is what buys the registers;
//   * the pressure scan runs over the 16 nodes of a wave with the DPP steps row_shr:4, row_shr:8, row_bcast:15,
//     row_bcast:31 (two steps fewer than the 64-node scan); the upstream node is lane - 4: row_shr:4 plus one
//     row_bcast:15 restricted to bank 0 (lanes 0-3 of rows 1-3), the first quad of a wave reads the previous wave's
//     last node from LDS like lane 0 does in the node-per-lane kernels;
//   * the Jacobi iterate crosses the quads through LDS (s_x[node][V]: each lane writes its rows, reads the V entries
//     of node - 1; the same wave executes write and read in order, so no barrier inside a wave), the wave boundary is
//     exchanged with a barrier every second sweep exactly as in rmt_rodas_bs (RMT_ROS_XCH 2), block and chunk
//     boundaries through the same carry / tagged-word links.
// A workgroup of RMT_BLOCK threads covers RMT_QN = RMT_BLOCK / 4 nodes; G_1..G_5 of the block live in LDS
// (5 V RMT_QN doubles).  One Jacobi step per sweep (no two-step product: M alone is register-resident).
// Same controller, tolerances, error norm, hand-overs, stats and flags as rmt_n2_ros4_mem / _chain; the host launches
// these kernels under the same names with nodes-per-block = RMT_QN (plan.ros4_nodes_per_block).
#if RMT_MODEL != 0 || RMT_FP32 || RMT_NPT != 1 || RMT_ROS_SCHEME != 1 || RMT_ROS_JAC_FD
#error "RMT_ROS_QUAD: model N2, fp64, one node per quad (RMT_NPT 1), RODAS4 with the analytic node Jacobian"
#endif
static_assert(RMT_BLOCK % 64 == 0 && RMT_V <= 16, "RMT_ROS_QUAD: whole waves, at most four matrix rows per lane");
#define RMT_QN (RMT_BLOCK / 4)
#define RMT_QR ((RMT_V + 3) / 4)
#define RMT_QNW (RMT_BLOCK / 64)

template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ double rmt_dppm(const double old, const double v) {
    int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, ROW_MASK, BANK_MASK, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, ROW_MASK, BANK_MASK, false);
    return __hiloint2double(hi, lo);
}
// value of lane - 4 (the same matrix-row owner of the upstream node); the first quad of a wave receives 0 (callers
// overwrite it with the value from the previous wave / the carry)
__device__ __forceinline__ double rmt_lane_up4(const double v) {
    const double r = rmt_dpp0<0x114>(v);                 // row_shr:4, zero fill: lanes 4-15 of every row
    return rmt_dppm<0x142, 0xe, 0x1>(r, v);              // row_bcast:15 into bank 0 of rows 1-3: lanes 0-3 <- lane 15 of the row before
}
// value of lane Q of the own quad, for all four lanes
template <int Q>
__device__ __forceinline__ double rmt_quad_bcast(const double v) {
    return rmt_dpp<(Q | (Q << 2) | (Q << 4) | (Q << 6)), 0xf>(v, v);
}

// -d f_r / d y_c of rmt_node_post for the rows this lane owns (r = q + 4 kk), analytic: rmt_node_jac (20_node_n2.inc)
// with the row selection applied where an entry is produced, so that the full V x V block is never assembled.
template <typename FL>
__device__ __forceinline__ void rmt_node_jac_q(const RmtMember& m, const RmtNode& nd, const real* __restrict__ ys,
                                               const preal Pz, const int q, real (&mine)[RMT_QR][RMT_V],
                                               real* __restrict__ rout, FL& flag) {
    const real P = real(Pz);
    real r[RMT_R], drdT[RMT_R], drdx[RMT_R][RMT_S], drdC[RMT_R][RMT_S];
    rmt_kinetics_jac(nd.T, nd.invT, P, nd.x, nd.C, m.user, r, drdT, drdx, drdC, flag);
#pragma unroll
    for (int qq = 0; qq < RMT_R; ++qq) rout[qq] = r[qq];
    real ctot = real(0);
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) ctot += nd.C[i];
    const real ict = rmt_rcp(ctot);
    real act[RMT_S];
#pragma unroll
    for (int j = 0; j < RMT_S; ++j) act[j] = (ys[j] > RMT_EPS) ? m.cmax * ict : real(0);
    real G[RMT_R][RMT_V];                                  // d r_q / d y_c
#pragma unroll
    for (int qq = 0; qq < RMT_R; ++qq) {
        real sx = real(0);
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) sx += nd.x[i] * drdx[qq][i];
#pragma unroll
        for (int j = 0; j < RMT_S; ++j) G[qq][j] = act[j] * (drdC[qq][j] * ctot + (drdx[qq][j] - sx));
#if !RMT_ISO
        G[qq][RMT_S] = m.tf * drdT[qq];
#endif
    }
    const real fm = m.inv_macote;
    const real conv = m.f1 * m.inv_dz;
#if !RMT_ISO
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
    real dcp[RMT_R], ddcp[RMT_R], hq[RMT_R];
    rmt_reaction_dcp(cpbar, dcp);
    rmt_reaction_dcp(dcpb, ddcp);
    real qr = real(0), dqrT = real(0);
#pragma unroll
    for (int qq = 0; qq < RMT_R; ++qq) {
        hq[qq] = dcp[qq] * (T - RMT_TREF) + RMT_DH25[qq];
        qr += r[qq] * hq[qq];
        dqrT += G[qq][RMT_S] * hq[qq] + r[qq] * (m.tf * (dcp[qq] + (T - RMT_TREF) * ddcp[qq]));
    }
    const bool wall = !(m.tm == real(0));
    const real qm = wall ? m.ua * (m.tm - T) : real(0);
    const real dqmT = wall ? -(m.ua * m.tf) : real(0);
    const real icpm = rmt_rcp(cpm);
    const real gain = m.inv_hecote * rmt_rcp(P * nd.MoT) * icpm;
    const real drive = gain * (qm - qr);
    const real iM = rmt_rcp(nd.M);
#endif
    // column by column: the V entries of column c, then the RMT_QR of them this lane owns
#pragma unroll
    for (int c = 0; c < RMT_V; ++c) {
        real col[RMT_R], src[RMT_S], colv[4 * RMT_QR];
#pragma unroll
        for (int qq = 0; qq < RMT_R; ++qq) col[qq] = G[qq][c];
        rmt_species_source(col, src);
#pragma unroll
        for (int i = 0; i < 4 * RMT_QR; ++i) colv[i] = real(0);
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) colv[i] = -(fm * src[i]) + ((i == c) ? conv : real(0));
#if !RMT_ISO
        if (c < RMT_S) {
            const int j = c < RMT_S ? c : 0;
            const real dlg = -act[j] * ((real(1e-3) * RMT_MW[j] - nd.M) * iM + (cpbar[j] - cpm) * icpm);
            real gq = real(0);
#pragma unroll
            for (int qq = 0; qq < RMT_R; ++qq) gq += hq[qq] * G[qq][j];
            colv[RMT_S] = -(dlg * drive - gain * gq);
        } else {
            const real dlgT = m.tf * (nd.invT - dcpm * icpm);
            colv[RMT_S] = m.ft * m.inv_dz - (dlgT * drive + gain * (dqmT - dqrT));
        }
#endif
#pragma unroll
        for (int kk = 0; kk < RMT_QR; ++kk) {
            const real v01 = (q & 1) ? colv[4 * kk + 1] : colv[4 * kk];
            const real v23 = (q & 1) ? colv[4 * kk + 3] : colv[4 * kk + 2];
            mine[kk][c] = (q & 2) ? v23 : v01;
        }
    }
}

// One RHS evaluation of a block of RMT_QN nodes in the quad layout (the N2 rmt_rhs_block of 40_rhs_block.inc with 16
// nodes per wave); every lane of a quad returns the node's full derivative k[V].  One __syncthreads().
// WANT_JAC: also this lane's rows of -d f/d y (analytic); `upm` returns the clamp mask of the upstream node (bit i set =
// the upwind coupling of variable i is active).
template <int CHAIN, bool WANT_JAC, typename FL>
__device__ __forceinline__ void rmt_rhs_block_q(const RmtMember& m, RmtShared& sh, const int buf,
                                                const real (&ys)[RMT_V], const bool valid, const int gnode,
                                                RmtCarry& carry, real (&k)[RMT_V], FL& flag, RmtChainCtx* ctx,
                                                real (&mine)[RMT_QR][RMT_V], unsigned& upm) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int q = lane & 3;
    RmtNode nd;
    RmtAff inc;
    {
        const preal a = rmt_node_pre(m, ys, nd);
        inc.a = valid ? a : preal(1);
        inc.b = valid ? m.beta : preal(0);
    }
    const RmtAff own = inc;
    // inclusive scan of the per-node maps over the 16 nodes of the wave (all four lanes of a quad hold the same map)
#define RMT_QSCAN0(CTRL)                                                        \
    {                                                                           \
        RmtAff prev;                                                            \
        prev.a = rmt_dpp<CTRL, 0xf>(preal(1), inc.a);                           \
        prev.b = rmt_dpp0<CTRL>(inc.b);                                         \
        inc = rmt_then(prev, inc);                                              \
    }
#define RMT_QSCAN(CTRL, MASK)                                                   \
    {                                                                           \
        RmtAff prev;                                                            \
        prev.a = rmt_dpp<CTRL, MASK>(preal(1), inc.a);                          \
        prev.b = rmt_dpp<CTRL, MASK>(preal(0), inc.b);                          \
        inc = rmt_then(prev, inc);                                              \
    }
    RMT_QSCAN0(0x114)             // row_shr:4
    RMT_QSCAN0(0x118)             // row_shr:8
    RMT_QSCAN(0x142, 0xa)         // row_bcast:15 -> rows 1, 3
    RMT_QSCAN(0x143, 0xc)         // row_bcast:31 -> rows 2, 3
#undef RMT_QSCAN0
#undef RMT_QSCAN
    real last[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) last[i] = rmt_max(ys[i], RMT_EPS);               // :4093
#if !RMT_ISO
    last[RMT_S] = ys[RMT_S];                                                          // :4111
#endif
    if (lane == 63) {
        sh.put_total(buf, wave, inc);
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) sh.bnd[buf][wave][i] = last[i];
    }
    // exclusive map = inclusive map of the node before: the scan result minus the node's own map is not available in
    // closed form, so the inclusive values are shifted by one node (four lanes)
    RmtAff exc;
    exc.a = rmt_lane_up4(inc.a);
    exc.b = rmt_lane_up4(inc.b);
    if (lane < 4) { exc.a = preal(1); exc.b = preal(0); }
    real up[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) up[i] = rmt_lane_up4(last[i]);
    if (CHAIN == 2) {
        if (wave == 0) {
            if (ctx->has_in) {                    // stage record {up[V], P} of the upstream chunk's last block
                const int st = rmt_link_recv(rmt_ring_entry(ctx->ring_in, ctx->seq_in), ctx->seq_in, sh.cin[buf], RMT_V + 1,
                                             ctx->abort_word, ctx->dead);
                ctx->dead |= st;
            }
            if (lane == 0) sh.abort[buf] = ctx->dead;
        }
        if (ctx->has_in) ctx->seq_in = rmt_seq_next(ctx->seq_in);
    }
    __syncthreads();
    if (CHAIN == 2) {
        if (ctx->has_in) {
            carry.P = sh.cin[buf][RMT_V];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) carry.up[i] = real(sh.cin[buf][i]);
        }
        ctx->abort = sh.abort[buf];
    }
    const preal pw = rmt_push_before(sh, buf, wave, carry.P);
    if (CHAIN == 2) {
        if (ctx->has_out) {                       // the record for the downstream chunk is complete: send it ahead of the node functions
            if (wave == RMT_QNW - 1 &&
                !(ctx->chunk == RMT_CHAIN_TEST_STALL_CHUNK && ctx->seq_out >= (unsigned)RMT_CHAIN_TEST_STALL_FROM)) {
                const preal pe = sh.through(buf, wave, pw);
                if (lane <= RMT_V)
                    sh.cst[buf][lane] = (lane == RMT_V) ? (double)pe : (double)sh.bnd[buf][RMT_QNW - 1][lane < RMT_V ? lane : 0];
                rmt_link_send(rmt_ring_entry(ctx->ring_out, ctx->seq_out), ctx->seq_out, sh.cst[buf], RMT_V + 1);
            }
            ctx->seq_out = rmt_seq_next(ctx->seq_out);
        }
    }
    if (lane < 4) {                               // first node of the wave: upstream = previous wave's last node / the carry
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) up[i] = carry.up[i];
        } else {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) up[i] = sh.bnd[buf][wave - 1][i];
        }
    }
    const preal P = exc.a * pw + exc.b;
    (void)own;
    if (WANT_JAC) {
        real rj[RMT_R];
        rmt_node_jac_q(m, nd, ys, P, q, mine, rj, flag);
        rmt_node_post<FL, true>(m, nd, ys, up, P, k, flag, rj);
        upm = 0u;
        if (gnode > 0) {                                          // upwind coupling active? (clamp of the upstream value)
#pragma unroll
            for (int i = 0; i < RMT_S; ++i) upm |= (up[i] > RMT_EPS) ? (1u << i) : 0u;
#if !RMT_ISO
            upm |= 1u << RMT_S;
#endif
        }
    } else {
        rmt_node_post(m, nd, ys, up, P, k, flag);
    }
    carry.P = rmt_push_from(sh, buf, wave, pw);
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) carry.up[i] = sh.bnd[buf][RMT_QNW - 1][i];
}

// in-place Gauss-Jordan inverse of the V x V matrix whose rows q, q + 4, ... this lane holds (no pivoting: I/(gamma h) - D
// has a dominant positive diagonal): the pivot row travels through the quad by a DPP broadcast; returns the smallest
// |pivot| among the pivots this lane owns
__device__ __forceinline__ real rmt_invert_q(real (&a)[RMT_QR][RMT_V], const int q) {
    real pmin = real(__builtin_inf());
#pragma unroll
    for (int p = 0; p < RMT_V; ++p) {
        const int qp = p & 3, kp = p >> 2;                        // owner lane of row p and its slot there
        const bool own = (q == qp);
        const real piv = a[kp][p];
        pmin = own ? rmt_min(pmin, rmt_abs(piv)) : pmin;
        const real ip = own ? rmt_rcp(piv) : real(1);
        a[kp][p] = own ? real(1) : piv;
        real prow[RMT_V];
#pragma unroll
        for (int c = 0; c < RMT_V; ++c) {
            a[kp][c] *= ip;
            prow[c] = (qp == 0) ? rmt_quad_bcast<0>(a[kp][c]) : (qp == 1) ? rmt_quad_bcast<1>(a[kp][c])
                    : (qp == 2) ? rmt_quad_bcast<2>(a[kp][c]) : rmt_quad_bcast<3>(a[kp][c]);
        }
#pragma unroll
        for (int kk = 0; kk < RMT_QR; ++kk) {
            const bool isp = own && (kk == kp);                   // the pivot row itself stays as normalised
            const real f = isp ? real(0) : a[kk][p];
            a[kk][p] = isp ? a[kk][p] : real(0);
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) a[kk][c] -= f * prow[c];
        }
    }
    return pmin;
}

// RMT_ROSQ_TWOSTEP 1: two Jacobi steps per sweep, x_z = q_z + N_z x_{z-2} with q = p + M p_up and N_z = M_z M_{z-1}
// (the scheme of rmt_rodas_bs, 60_ros4.inc): every lane writes its rows of M = A^-1 diag(l) to LDS once per step, reads
// the upstream node's M from there and keeps ITS rows of N in registers (another ceil(V/4) V doubles); the block's
// first node has no upstream M and keeps the one-step form through an identity matrix in slot 0.  A sweep then costs
// one quarter-matvec and one barrier per TWO Jacobi steps: 94 instead of 196 instructions per two steps in the sweep
// loops - but N's 2 ceil(V/4) V registers live across the six RHS evaluations of a step push ~400 VGPRs to scratch around
// them, and the 12-species job takes 169 ms instead of 74 (profiles/round3_kcache.md).  Off; kept for mechanisms whose
// node function is small enough to leave the registers.
#ifndef RMT_ROSQ_TWOSTEP
#define RMT_ROSQ_TWOSTEP 0
#endif
struct RmtQuadShared {
    real x[RMT_QN][RMT_V];            // the Jacobi iterate of the block's nodes (rows written by their owner lanes)
#if RMT_ROSQ_TWOSTEP
    real x2[2][RMT_QN + 1][RMT_V];    // two-step sweeps: the iterate by sweep parity; row 0 = the value upstream of the block
    real m[RMT_QN + 1][RMT_V][RMT_V]; // M of every node of the block (slot z + 1; slot 0 = identity), written in stage 1
#endif
};

// one RODAS4 stage of one node block, quad layout (the structure of rmt_rodas_bs)
template <int STAGE, int CH>
__device__ __forceinline__ void rmt_rodas_bs_q(const RmtMember& m, RmtShared& sh, RmtQuadShared& qs, RmtRodasCarry& rc,
                                               int& ph, real (*s_g)[RMT_V][RMT_QN], const real (&y0)[RMT_V],
                                               const bool valid, const int gnode, real (&ainv)[RMT_QR][RMT_V],
                                               unsigned& mk, real (&ynew)[RMT_QR], const real inv_gh, const real ih,
                                               const int sweeps, rmt_flags_t& flag, real& pivmin, const double rtol,
                                               const double atol, double& errloc, bool& bad, RmtChainCtx* ctx,
                                               real (&nn)[RMT_QR][RMT_V]) {
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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane & 3;
    const int nloc = tid >> 2;                                    // node of the block this quad works on
    const bool firstq = lane < 4, lastq = lane >= 60;
    real ys[RMT_V], k[RMT_V], cg[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) {
        real st = y0[i], cc = real(0);
#pragma unroll
        for (int g = 0; g < 5; ++g) {
            if (g < STAGE - 1) {
                const real gv = s_g[g][i][nloc];
                st += A[STAGE - 1][g] * gv;
                cc += Cc[STAGE - 1][g] * gv;
            }
        }
        ys[i] = st;                                               // (quads beyond the end hold the safe inlet state)
        cg[i] = cc * ih;
    }
    RmtCarry carry;                                               // this stage's hand-over from the previous block
    carry.P = rc.P[STAGE - 1];
    real xc[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) { carry.up[i] = rc.up[STAGE - 1][i]; xc[i] = rc.xc[STAGE - 1][i]; }
    rmt_noflags_t nof_stage;
    (void)nof_stage;
    if (STAGE == 1) {
        rmt_rhs_block_q<CH, true>(m, sh, ph, ys, valid, gnode, carry, k, flag, ctx, ainv, mk);
#pragma unroll
        for (int kk = 0; kk < RMT_QR; ++kk)
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) {
                const bool diag = (c == q + 4 * kk);              // A = I/(gamma h) - D on this lane's rows; rows beyond V: identity
                const bool pad = (q + 4 * kk >= RMT_V);
                ainv[kk][c] = pad ? real(0) : (ainv[kk][c] + (diag ? inv_gh : real(0)));
            }
        const real pv = rmt_invert_q(ainv, q);
        if (valid) pivmin = rmt_min(pivmin, pv);
        else {
#pragma unroll
            for (int kk = 0; kk < RMT_QR; ++kk)
#pragma unroll
                for (int c = 0; c < RMT_V; ++c) ainv[kk][c] = real(0);
        }
    } else {
        unsigned dummy = 0u;
        if (RMT_CHECK_ALL_STAGES) rmt_rhs_block_q<CH, false>(m, sh, ph, ys, valid, gnode, carry, k, flag, ctx, ainv, dummy);
        else rmt_rhs_block_q<CH, false>(m, sh, ph, ys, valid, gnode, carry, k, nof_stage, ctx, ainv, dummy);
    }
    ph ^= 1;
    // l = d f_z / d y_{z-1} (diagonal), b = f(Y_i) + sum c_ij G_j / h, p = A^-1 b on this lane's rows
    real l[RMT_V];
    {
        const real cs = m.f1 * m.inv_dz, ct = m.ft * m.inv_dz;
#pragma unroll
        for (int c = 0; c < RMT_V; ++c) l[c] = (((mk >> c) & 1u) && valid) ? ((c < RMT_S) ? cs : ct) : real(0);
    }
    real p[RMT_QR], x[RMT_QR];
#pragma unroll
    for (int kk = 0; kk < RMT_QR; ++kk) {
        real acc = real(0);
#pragma unroll
        for (int c = 0; c < RMT_V; ++c) acc += ainv[kk][c] * (valid ? k[c] + cg[c] : real(0));
        p[kk] = acc;
        x[kk] = acc;
    }
    real u[RMT_V];
#if RMT_ROSQ_TWOSTEP
    (void)firstq;
    if (STAGE == 1) {
        // this lane's rows of M = A^-1 diag(l) into LDS, then its rows of N = M_z M_{z-1} (M_{z-1} = the identity for the
        // block's first node: slot 0, written at kernel start)
#pragma unroll
        for (int kk = 0; kk < RMT_QR; ++kk) {
            if (q + 4 * kk < RMT_V) {
#pragma unroll
                for (int c = 0; c < RMT_V; ++c) qs.m[nloc + 1][q + 4 * kk][c] = ainv[kk][c] * l[c];
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < RMT_QR; ++kk)
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) nn[kk][c] = real(0);
#pragma unroll
        for (int kx = 0; kx < RMT_V; ++kx) {
            real mz[RMT_QR];
#pragma unroll
            for (int kk = 0; kk < RMT_QR; ++kk) mz[kk] = ainv[kk][kx] * l[kx];
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) {
                const real up_ = qs.m[nloc][kx][c];
#pragma unroll
                for (int kk = 0; kk < RMT_QR; ++kk) nn[kk][c] += mz[kk] * up_;
            }
        }
    }
    // q = p + M p_up (p_up = 0 upstream of the block's first node)
#pragma unroll
    for (int kk = 0; kk < RMT_QR; ++kk)
        if (q + 4 * kk < RMT_V) qs.x[nloc][q + 4 * kk] = p[kk];
    if (tid < RMT_V) { qs.x2[0][0][tid] = xc[tid]; qs.x2[1][0][tid] = xc[tid]; }   // the value upstream of the block (mem: exact)
    __syncthreads();
    real qv[RMT_QR];
    {
        const real* src = &qs.x[nloc > 0 ? nloc - 1 : 0][0];
#pragma unroll
        for (int c = 0; c < RMT_V; ++c) u[c] = (nloc > 0) ? src[c] * l[c] : real(0);
#pragma unroll
        for (int kk = 0; kk < RMT_QR; ++kk) {
            real acc = p[kk];
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) acc += ainv[kk][c] * u[c];
            qv[kk] = acc;
        }
    }
    for (int it = 0; it < sweeps; it += 2) {
        const int b2 = (it >> 1) & 1;
#pragma unroll
        for (int kk = 0; kk < RMT_QR; ++kk)
            if (q + 4 * kk < RMT_V) qs.x2[b2][nloc + 1][q + 4 * kk] = x[kk];
        if (CH == 2) {
            if (ctx->has_out) {
                if (wave == RMT_QNW - 1) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // (rows written by other lanes of this wave)
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (lane < RMT_V) sh.cst[b2][lane] = (double)qs.x2[b2][RMT_QN][lane];
                    rmt_link_send(rmt_ring_entry(ctx->ring_out, ctx->seq_out), ctx->seq_out, sh.cst[b2], RMT_V);
                }
                ctx->seq_out = rmt_seq_next(ctx->seq_out);
            }
            if (ctx->has_in) {
                if (wave == 0) {
                    ctx->dead |= rmt_link_recv(rmt_ring_entry(ctx->ring_in, ctx->seq_in), ctx->seq_in, sh.cin[b2], RMT_V,
                                               ctx->abort_word, ctx->dead);
                    if (lane < RMT_V) qs.x2[b2][0][lane] = real(sh.cin[b2][lane]);
                }
                ctx->seq_in = rmt_seq_next(ctx->seq_in);
            }
        }
        __syncthreads();
        {   // x_{z-2} (the boundary value for the block's first two nodes)
            const real* src = &qs.x2[b2][nloc > 0 ? nloc - 1 : 0][0];
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) u[c] = src[c];
        }
#pragma unroll
        for (int kk = 0; kk < RMT_QR; ++kk) {
            real acc = qv[kk];
#pragma unroll
            for (int c = 0; c < RMT_V; ++c) acc += nn[kk][c] * u[c];
            x[kk] = acc;
        }
    }
#else
    (void)nn;
    // Jacobi sweeps x <- p + A^-1 (l .* x_up); the iterate travels through LDS.  Row 0 of sh.xb = the value upstream of
    // the block (carry, or the upstream chunk's boundary iterate), row w + 1 = last node of wave w.
    rmt_sweep_carry(sh, xc);
    for (int it = 0; it < sweeps; it += 2) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int kk = 0; kk < RMT_QR; ++kk)
                if (q + 4 * kk < RMT_V) qs.x[nloc][q + 4 * kk] = x[kk];
            if (half == 0) {                      // boundary values cross the waves (and the chunk link) every second sweep
                if (lastq) {
#pragma unroll
                    for (int kk = 0; kk < RMT_QR; ++kk)
                        if (q + 4 * kk < RMT_V) sh.xb[ph][wave + 1][q + 4 * kk] = x[kk];
                }
                if (CH == 2) {
                    // (the last wave's rows of sh.xb[ph][RMT_QNW] are written by its own lanes just above: same wave, in order)
                    if (ctx->has_out) {
                        if (wave == RMT_QNW - 1) {
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // (rows written by other lanes of this wave)
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                            if (lane < RMT_V) sh.cst[ph][lane] = (double)sh.xb[ph][RMT_QNW][lane];
                            rmt_link_send(rmt_ring_entry(ctx->ring_out, ctx->seq_out), ctx->seq_out, sh.cst[ph], RMT_V);
                        }
                        ctx->seq_out = rmt_seq_next(ctx->seq_out);
                    }
                    if (ctx->has_in) {
                        if (wave == 0) {
                            ctx->dead |= rmt_link_recv(rmt_ring_entry(ctx->ring_in, ctx->seq_in), ctx->seq_in, sh.cin[ph], RMT_V,
                                                       ctx->abort_word, ctx->dead);
                            if (lane < RMT_V) sh.xb[ph][0][lane] = real(sh.cin[ph][lane]);
                        }
                        ctx->seq_in = rmt_seq_next(ctx->seq_in);
                    }
                }
                __syncthreads();
            }
            else {
                // within a wave the LDS write above and the read below execute in order; the fences keep the COMPILER
                // from moving this thread's read (another address) ahead of its write
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            // the upstream node's iterate: node - 1 of the same wave (written above by this wave, in order), or for the
            // first quad of a wave the boundary value of the last exchange
            {
                const real* src = firstq ? &sh.xb[ph][wave][0] : &qs.x[nloc > 0 ? nloc - 1 : 0][0];
#pragma unroll
                for (int c = 0; c < RMT_V; ++c) u[c] = src[c] * l[c];
            }
#pragma unroll
            for (int kk = 0; kk < RMT_QR; ++kk) {
                real acc = p[kk];
#pragma unroll
                for (int c = 0; c < RMT_V; ++c) acc += ainv[kk][c] * u[c];
                x[kk] = acc;
            }
        }
        ph ^= 1;
    }
#endif
    if (STAGE < 6) {              // G_i of the block (read by all four lanes of a quad in the next stage: before the barrier)
#pragma unroll
        for (int kk = 0; kk < RMT_QR; ++kk)
            if (q + 4 * kk < RMT_V) s_g[STAGE - 1][q + 4 * kk][nloc] = x[kk];
    }
    // the boundary value handed to the next node block: the last node's iterate, read by everybody after one barrier
    if (lastq && wave == RMT_QNW - 1) {
#pragma unroll
        for (int kk = 0; kk < RMT_QR; ++kk)
            if (q + 4 * kk < RMT_V) sh.xb[ph][RMT_QNW][q + 4 * kk] = x[kk];
    }
    if (CH == 2 && ctx->has_out) {
        // (nothing to send: the downstream chunk took its last boundary iterate at the final exchange, as in rmt_rodas_bs)
    }
    __syncthreads();
    real cout[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) cout[i] = sh.xb[ph][RMT_QNW][i];
    ph ^= 1;
    if (tid == 0) {
        rc.P[STAGE - 1] = carry.P;
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) { rc.up[STAGE - 1][i] = carry.up[i]; rc.xc[STAGE - 1][i] = cout[i]; }
    }
    if (STAGE == 6) {
#pragma unroll
        for (int kk = 0; kk < RMT_QR; ++kk) {
            const int r = q + 4 * kk;
            // this lane's rows of Y_6 and y_n: a 4-way select over compile-time indices
            real ysr = real(0), y0r = real(0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (4 * kk + j < RMT_V) {
                    ysr = (q == j) ? ys[4 * kk + j] : ysr;
                    y0r = (q == j) ? y0[4 * kk + j] : y0r;
                }
            }
            const double yn = (double)ysr + (double)x[kk];
            ynew[kk] = real(yn);
            if (valid && r < RMT_V) {
                bad |= !__builtin_isfinite(yn);
                errloc = fmax(errloc, fabs((double)x[kk]) / (atol + rtol * fmax(fabs((double)y0r), fabs(yn))));
            }
        }
    }
}

__device__ __forceinline__ void rmt_quad_init(RmtQuadShared& qs) {       // (made visible by the barrier of rmt_math_init)
#if RMT_ROSQ_TWOSTEP
    for (int i = threadIdx.x; i < RMT_V * RMT_V; i += blockDim.x) qs.m[0][i / RMT_V][i % RMT_V] = (i / RMT_V == i % RMT_V) ? real(1) : real(0);
#else
    (void)qs;
#endif
}

// all six stages of one node block (the G_j of the block are complete in LDS before the next stage reads them: every
// stage ends with barriers)
template <int CH>
__device__ __forceinline__ void rmt_rodas_block_q(const RmtMember& m, RmtShared& sh, RmtQuadShared& qs, RmtRodasCarry& rc,
                                                  int& ph, real (*s_g)[RMT_V][RMT_QN], const real* __restrict__ ye,
                                                  real* __restrict__ yout, const int N, const int gnode, const bool valid,
                                                  const real inv_gh, const real ih, const int sweeps, rmt_flags_t& flag,
                                                  real& pivmin, const double rtol, const double atol, double& errloc,
                                                  bool& bad, RmtChainCtx* ctx) {
    const int q = threadIdx.x & 3;
    real y0[RMT_V], ynew[RMT_QR], ainv[RMT_QR][RMT_V], nn[RMT_QR][RMT_V];
    unsigned mk = 0u;
    rmt_safe_state(m, y0);
    if (valid) {
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) y0[i] = ye[(size_t)i * N + gnode];
    }
    rmt_rodas_bs_q<1, CH>(m, sh, qs, rc, ph, s_g, y0, valid, gnode, ainv, mk, ynew, inv_gh, ih, sweeps, flag, pivmin, rtol, atol, errloc, bad, ctx, nn);
    rmt_rodas_bs_q<2, CH>(m, sh, qs, rc, ph, s_g, y0, valid, gnode, ainv, mk, ynew, inv_gh, ih, sweeps, flag, pivmin, rtol, atol, errloc, bad, ctx, nn);
    rmt_rodas_bs_q<3, CH>(m, sh, qs, rc, ph, s_g, y0, valid, gnode, ainv, mk, ynew, inv_gh, ih, sweeps, flag, pivmin, rtol, atol, errloc, bad, ctx, nn);
    rmt_rodas_bs_q<4, CH>(m, sh, qs, rc, ph, s_g, y0, valid, gnode, ainv, mk, ynew, inv_gh, ih, sweeps, flag, pivmin, rtol, atol, errloc, bad, ctx, nn);
    rmt_rodas_bs_q<5, CH>(m, sh, qs, rc, ph, s_g, y0, valid, gnode, ainv, mk, ynew, inv_gh, ih, sweeps, flag, pivmin, rtol, atol, errloc, bad, ctx, nn);
    rmt_rodas_bs_q<6, CH>(m, sh, qs, rc, ph, s_g, y0, valid, gnode, ainv, mk, ynew, inv_gh, ih, sweeps, flag, pivmin, rtol, atol, errloc, bad, ctx, nn);
    if (valid) {
#pragma unroll
        for (int kk = 0; kk < RMT_QR; ++kk)
            if (q + 4 * kk < RMT_V) yout[(size_t)(q + 4 * kk) * N + gnode] = ynew[kk];
    }
}

__device__ __forceinline__ void rmt_rodas_carry_reset(const RmtMember& m, RmtRodasCarry& rc) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int st = 0; st < 6; ++st) {
            RmtCarry c0;
            rmt_carry_inlet(m, c0);
            rc.P[st] = c0.P;
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) { rc.up[st][i] = c0.up[i]; rc.xc[st][i] = real(0); }
        }
    }
}

// ---- kernel: one workgroup per reactor (same arguments, controller and contract as the node-per-lane rmt_n2_ros4_mem)
extern "C" __global__ __launch_bounds__(RMT_BLOCK, RMT_ROS_WAVES) void rmt_n2_ros4_mem(
        real* __restrict__ y, real* __restrict__ work, unsigned* __restrict__ maskbuf,
        const double* __restrict__ members, const int N, const int E, const double t0,
        const double t1, const double rtol, const double atol, const double h0,
        const long long max_steps, double* __restrict__ stats, unsigned* __restrict__ flags) {
    __shared__ RmtShared sh;
    __shared__ RmtQuadShared qs;
    __shared__ real s_g[5][RMT_V][RMT_QN];
    __shared__ RmtRodasCarry s_rc;
    (void)maskbuf;
    rmt_quad_init(qs);
    rmt_math_init();
    const int e = blockIdx.x;
    RmtMember m;
    rmt_load_member(members + (size_t)e * RMT_NM, m);
    const size_t per = (size_t)RMT_V * N, tot = per * E;
    real* ye = y + e * per;
    real* YS = work + 5 * tot + e * per;
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
    while (t < t1 && nacc + nrej < max_steps) {
        bool last = false;
        const double hfull = h;
        if (t + h >= t1) { h = t1 - t; last = true; }
        rmt_flags_clear(trial);
        const real inv_gh = real(1.0 / (GAM * h));
        const double rho = cmax / (1.0 / (GAM * h) + cmax);
        int sweeps = (int)ceil(logtol / log(rho)) + 1;
        sweeps = sweeps < 2 ? 2 : (sweeps > RMT_ROS_MAX_SWEEPS ? RMT_ROS_MAX_SWEEPS : sweeps);
        sweeps += RMT_ROS_XCH - 1;                      // boundary values up to RMT_ROS_XCH - 1 sweeps old
#ifdef RMT_ROS_FIX_SWEEPS
        sweeps = RMT_ROS_FIX_SWEEPS;
#endif
        sweeps = (sweeps + 1) / 2 * 2;                  // whole exchange periods
        real pivmin = real(__builtin_inf());
        const real ih = real(1.0 / h);
        double errloc = 0.0;
        bool bad = false;
        __syncthreads();                                 // the previous step's readers of s_rc are done
        rmt_rodas_carry_reset(m, s_rc);
        __syncthreads();
        for (int base = 0; base < N; base += RMT_QN) {
            const int gnode = base + ((int)threadIdx.x >> 2);
            rmt_rodas_block_q<0>(m, sh, qs, s_rc, ph, s_g, ye, YS, N, gnode, gnode < N, inv_gh, ih, sweeps, trial, pivmin,
                                 rtol, atol, errloc, bad, nullptr);
        }
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

// ---- kernel: one reactor over many CUs (same arguments, links, decision slot and contract as rmt_n2_ros4_chain;
// W = nodes per chunk, a multiple of RMT_QN)
extern "C" __global__ __launch_bounds__(RMT_BLOCK, RMT_ROS_WAVES) void rmt_n2_ros4_chain(
        real* __restrict__ y, real* __restrict__ work, const double* __restrict__ members, const int N,
        const int E, const int C, const int T, const int W, const double t0, const double t1,
        const double rtol, const double atol, const double h0, const long long max_steps,
        double* __restrict__ stats, unsigned* __restrict__ flags, unsigned long long* __restrict__ rings,
        unsigned long long* __restrict__ decision, unsigned* __restrict__ abort_words) {
    __shared__ RmtShared sh;
    __shared__ RmtQuadShared qs;
    __shared__ real s_g[5][RMT_V][RMT_QN];
    __shared__ RmtRodasCarry s_rc;
    __shared__ double s_dec[2];
    rmt_quad_init(qs);
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
    ctx.seq_in = ctx.seq_out = 1u;
    ctx.abort_word = abort_words + team;
    ctx.dead = 0;
    ctx.bp = false;
    ctx.bp_in = ctx.bp_out = nullptr;
    ctx.known = 0u;
    unsigned long long* const dec = decision + (size_t)team * 2;
    unsigned att = 0u;
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
            sweeps += RMT_ROS_XCH - 1;
#ifdef RMT_ROS_FIX_SWEEPS
            sweeps = RMT_ROS_FIX_SWEEPS;
#endif
            sweeps = (sweeps + 1) / 2 * 2;
            real pivmin = real(__builtin_inf());
            const real ih = real(1.0 / h);
            double errloc = 0.0;
            bool bad = false;
            att = rmt_seq_next(att);
            __syncthreads();
            rmt_rodas_carry_reset(m, s_rc);              // chunk 0: the inlet; later chunks overwrite P / up from the link
            __syncthreads();
            for (int base = nlo; base < nhi; base += RMT_QN) {
                const int gnode = base + ((int)threadIdx.x >> 2);
                ctx.has_in = (c > 0) && (base == nlo);
                ctx.has_out = (c < C - 1) && (base + RMT_QN >= nhi);
                rmt_rodas_block_q<2>(m, sh, qs, s_rc, ph, s_g, ye, YS, N, gnode, gnode < nhi, inv_gh, ih, sweeps, trial,
                                     pivmin, rtol, atol, errloc, bad, &ctx);
            }
            bad |= !(pivmin > real(0));
            double worst = rmt_block_max(sh, rp, (bad || !__builtin_isfinite(errloc)) ? 1.0e300 : errloc);
            rp ^= 1;
            if (wave == 0) {                             // running maximum down the chain, the reactor's value back to everybody
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
    if (dead && threadIdx.x == 0) {
        for (int e2 = e; e2 < E; e2 += T) atomicOr(&flags[e2], RMT_FLAG_STEP);
    }
}
#endif   // RMT_WITH_ROS4 && RMT_ROS_QUAD
