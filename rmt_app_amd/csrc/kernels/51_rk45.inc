// ===================================================================== kernel: adaptive RK45, state in memory
// Dormand-Prince 5(4) (the pair behind SciPy's "RK45", which the reference reaches through
// solve_ivp(method=...) at pbHomoReactor.py:3609) with PER-REACTOR step control: every workgroup
// carries its own t, h and accept/reject history.  Controller (restated in oracle/n2_oracle.py
// rk45, which the parity tests compare against):
//   err = max_i |e_i| / (atol + rtol*max(|y_i|, |ynew_i|));  accept iff err <= 1
//   h_new = h * clip(0.9*err^-0.2, 0.2, 5)  (no growth after a rejection);  a stage that produces a
//   non-finite value (Python would raise inside a lambda: SURVEY.md Appendix C) rejects with h/4.
// work = 8 arrays [E][V][N]: K1..K7 and the trial state.  FSAL: K7 of an accepted step is K1 of
// the next.  Each thread only touches its own nodes' entries.
__device__ static const double RMT_DP_A[7][6] = {
    {0, 0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
    {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};
__device__ static const double RMT_DP_E[7] = {      // b5 - b4
    35.0 / 384 - 5179.0 / 57600, 0, 500.0 / 1113 - 7571.0 / 16695, 125.0 / 192 - 393.0 / 640,
    -2187.0 / 6784 + 92097.0 / 339200, 11.0 / 84 - 187.0 / 2100, -1.0 / 40};

// first step of an adaptive launch: h0 > 0 for every reactor, or h0 < 0 = "resume": each reactor starts
// from the h_last its previous launch left in stats (|h0| where that is not a positive finite number)
__device__ __forceinline__ double rmt_initial_step(const double h0, const double* __restrict__ stats, const int e) {
    if (h0 > 0.0) return h0;
    const double hp = stats[(size_t)e * 4 + 1];
    return (hp > 0.0 && __builtin_isfinite(hp)) ? hp : -h0;
}
__device__ __forceinline__ double rmt_block_max(RmtShared& sh, const int buf, double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d));
    if ((threadIdx.x & 63) == 0) sh.red[buf][threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh.red[buf][0];
    for (int w = 1; w < RMT_NW; ++w) r = fmax(r, sh.red[buf][w]);
    return r;
}

// Node blocks are the OUTER loop of a step (see rmt_n2_rk4_mem): a block is read once, taken through
// the seven Dormand-Prince stages on chip - its K_1..K_7 in LDS when they fit (7 V block reals), else in
// the workspace - with one hand-over per stage from the previous block, and y_new / K_7 are written
// once; accepted steps swap the y and K_1 (FSAL) buffers.
#if 7 * RMT_V * RMT_BLOCK * (RMT_FP32 ? 4 : 8) <= 112 * 1024
#define RMT_RK45_KLDS 1
#else
#define RMT_RK45_KLDS 0
#endif
struct RmtStageCarry7 {
    double P[7];
    real up[7][RMT_V];
};
extern "C" __global__ __launch_bounds__(RMT_BLOCK) void rmt_n2_rk45_mem(
        real* __restrict__ y, real* __restrict__ work, const double* __restrict__ members,
        const int N, const int E, const double t0, const double t1, const double rtol,
        const double atol, const double h0, const long long max_steps,
        double* __restrict__ stats /* [E][4]: t_end, h_last, accepted(i64), rejected(i64) */,
        unsigned* __restrict__ flags) {
    __shared__ RmtShared sh;
    __shared__ RmtStageCarry7 s_c;
#if RMT_RK45_KLDS
    __shared__ real s_k[7][RMT_V][RMT_BLOCK];
#define KREF(j, i) s_k[j][i][threadIdx.x]
#else
#define KREF(j, i) wk[(size_t)(j) * tot + (size_t)(i) * N + node]
#endif
    rmt_math_init();
    const int e = blockIdx.x;
    RmtMember m;
    rmt_load_member(members + (size_t)e * RMT_NM, m);
    RMT_PROFILE_BIND(m, e, N)
    const size_t per = (size_t)RMT_V * N, tot = per * E;
    real* ye = y + e * per;
    real* wk = work + e * per;                  // workspace slots j*tot: K_j when they do not fit in LDS
    real* yn = work + 7 * tot + e * per;        // y_new
    real* k1 = work + 8 * tot + e * per;        // K_1 of the current state (FSAL) ...
    real* k7 = work + 9 * tot + e * per;        // ... and K_7 of the trial step
    (void)wk;
    rmt_flags_t flag, trial;
    rmt_flags_clear(flag);
    unsigned lflag = 0u;
    int ph = 0, rp = 0;
    double t = t0, h = rmt_initial_step(h0, stats, e);
    long long nacc = 0, nrej = 0;
    bool have_k1 = false;
    while (t < t1 && nacc + nrej < max_steps) {
        bool last = false;
        const double hfull = h;
        if (t + h >= t1) { h = t1 - t; last = true; }
        rmt_flags_clear(trial);
        double errloc = 0.0;
        bool bad = false;
        __syncthreads();                                 // the previous step's hand-overs have been read
        if (threadIdx.x == 0) {
            RmtCarry c0;
            rmt_carry_inlet(m, c0);
#pragma unroll
            for (int s = 0; s < 7; ++s) {
#if RMT_FORCING
                rmt_forcing_stage(m, c0, members + (size_t)e * RMT_NM, t + rmt_dp_c(s) * h, nullptr);     // each stage: its own inlet
#endif
                s_c.P[s] = c0.P;
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) s_c.up[s][i] = c0.up[i];
            }
        }
        __syncthreads();
        for (int base = 0; base < N; base += RMT_BLOCK) {
            const int node = base + (int)threadIdx.x;
            const bool valid = node < N;
            real y0[RMT_V], ynv[RMT_V];
            rmt_safe_state(m, y0);
            if (valid) {
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) y0[i] = ye[(size_t)i * N + node];
            }
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                real ys[1][RMT_V], k[1][RMT_V];
                // stage input: y + h*sum_j a[s][j] K_j ; s == 6 is the 5th-order solution itself
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        if (j < s && valid) acc += RMT_DP_A[s][j] * (double)KREF(j, i);
                    }
                    ys[0][i] = real((double)y0[i] + h * acc);
                    if (s == 6) ynv[i] = ys[0][i];
                }
                if (s == 0 && have_k1) {                 // FSAL: K_1 = f(y) is the K_7 of the accepted step
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) k[0][i] = valid ? k1[(size_t)i * N + node] : real(0);
                } else {
                    RmtCarry carry;                      // this stage's hand-over from the previous block
                    carry.P = s_c.P[s];
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) carry.up[i] = s_c.up[s][i];
                    RMT_PROFILE_AT(carry, base)
#if RMT_FORCING
                    rmt_forcing_apply3(m, members + (size_t)e * RMT_NM, t + rmt_dp_c(s) * h);    // the wall temperature of this stage (the inlet: s_c)
#endif
                    rmt_rhs_block<1, true>(m, sh, ph, ys, valid ? 1 : 0, carry, k, trial);
                    ph ^= 1;
                    if (threadIdx.x == 0) {
                        s_c.P[s] = carry.P;
#pragma unroll
                        for (int i = 0; i < RMT_V; ++i) s_c.up[s][i] = carry.up[i];
                    }
                }
                if (valid) {
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) {
                        KREF(s, i) = k[0][i];
                        bad |= !__builtin_isfinite(k[0][i]);
                    }
                }
            }
            if (valid) {
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) {
                    const size_t o = (size_t)i * N + node;
                    double ev = 0.0;
#pragma unroll
                    for (int j = 0; j < 7; ++j) ev += RMT_DP_E[j] * (double)KREF(j, i);
                    const double sc = atol + rtol * fmax(fabs((double)y0[i]), fabs((double)ynv[i]));
                    errloc = fmax(errloc, fabs(h * ev) / sc);
                    yn[o] = ynv[i];
                    k7[o] = KREF(6, i);
                    if (!have_k1) k1[o] = KREF(0, i);    // first step: f(y) stays valid if the step is rejected
                }
            }
        }
        const double anybad = rmt_block_max(sh, rp, bad ? 1.0 : 0.0);
        rp ^= 1;
        bad = anybad > 0.0;
        double err = 0.0;
        if (!bad) {
            err = rmt_block_max(sh, rp, __builtin_isfinite(errloc) ? errloc : 1.0e300);
            rp ^= 1;
        }
        have_k1 = true;
        double fac;
        if (bad) {
            fac = 0.25;
            ++nrej;
        } else if (err <= 1.0) {
            t = last ? t1 : t + h;
            ++nacc;
            fac = (err == 0.0) ? 5.0 : fmin(5.0, fmax(0.2, 0.9 * pow(err, -0.2)));
            { real* const tmp = ye; ye = yn; yn = tmp; }              // accept: the buffers swap roles,
            { real* const tmp = k1; k1 = k7; k7 = tmp; }              // K_1 <- K_7 (FSAL)
            rmt_flags_merge(flag, trial);
        } else {
            ++nrej;
            fac = fmax(0.2, 0.9 * pow(err, -0.2));     // K_1 = f(y) stays valid after a rejection
        }
        h = fmax(h * fac, 1e-14);
        if (last && t >= t1) h = fmax(h, hfull * fmin(fac, 1.0));   // a step clipped to the interval end does not shrink h_last
    }
    if (ye != y + e * per) {                                           // odd number of accepted steps
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
#undef KREF
}

// ===================================================================== kernel: adaptive RK45, state on chip
// The same Dormand-Prince 5(4) controller for reactors that fit one workgroup (N <= RMT_BLOCK*RMT_NPT):
// the state is read from HBM once per LAUNCH, every accepted and rejected step runs on chip.  Holding
// y_n and K_1..K_7 (8 V values per node) is more than the CU has, so the step is run in LOW-STORAGE form
// with four long-lived vectors per node (y_n and three slots A, B, C) besides the stage input and the
// current K that every RHS evaluation needs anyway - two more than classic RK4:
//   stages 1-4   A = K_1, B = K_2, C = K_3; the stage inputs are formed from them as usual
//   after K_4    the four derivatives are folded into the accumulators of everything still to come,
//                Z_5 = y + h sum_{j<=4} a_5j K_j (used at once), A = Z_6, B = Z_7, C = E = sum_{j<=4} e_j K_j
//   stage 5, 6   K_s updates the accumulators of the later stages and of the error (B ends as y_new)
//   stage 7      K_7 = f(y_new) completes E;  accepted: y = B, A = K_7 (FSAL)
// K_1 is consumed by the folding, so a REJECTED step recomputes K_1 = f(y_n) (one RHS evaluation on the
// few per cent of steps that are rejected).  RMT_RK45_LDS of the four vectors (order C, B, A, y) live in
// LDS, the others in VGPRs; every thread touches only its own nodes' entries, so they need no barrier.
// Controller, error norm, accept/reject rules and the rtol/atol/h0/stats contract: as rmt_n2_rk45_mem
// (the oracle's rk45).  The Python-exception tests follow the contract of include/rmt_n2.h: K_1 / K_7 - the
// derivatives at visited states - are evaluated by a copy of the RHS with the tests, the trial stages 2-6 by a
// second, test-free copy behind a scalar branch (RMT_RK45_TWO_COPIES 1; with RMT_CHECK_ALL_STAGES one copy
// with the tests serves all stages, as in rmt_n2_rk45_mem).  Two copies measured slower while the machine
// LICM still spilled (5.4 vs 6.1 G node-steps/s) and faster since it is off (7.27 vs 7.03, profiles/round2_rk45.md).
#ifndef RMT_RK45_LDS
#define RMT_RK45_LDS 2
#endif
#define RMT_RK45_SLOT_BYTES (RMT_V * RMT_NODES_WG * (RMT_FP32 ? 4 : 8))
#if RMT_RK45_LDS * RMT_RK45_SLOT_BYTES <= 136 * 1024        // else: code object without the on-chip RK45 (host falls back)
__device__ __forceinline__ double rmt_uniform(const double v) {      // a workgroup-uniform value, told to the compiler
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
// Dormand-Prince a_ij (stages 2..7, non-zero entries in row order) and e_j = b5_j - b4_j (j = 1,3,4,5,6,7).
// Deliberately NOT const: a const table is folded back into literals.
__device__ double rmt_dp_tab[26] = {
    1.0 / 5, 3.0 / 40, 9.0 / 40, 44.0 / 45, -56.0 / 15, 32.0 / 9,
    19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729,
    9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656,
    35.0 / 384, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84,
    35.0 / 384 - 5179.0 / 57600, 500.0 / 1113 - 7571.0 / 16695, 125.0 / 192 - 393.0 / 640,
    -2187.0 / 6784 + 92097.0 / 339200, 11.0 / 84 - 187.0 / 2100, -1.0 / 40};
// workgroup maximum of a non-negative value: wave reduction on the DPP path (no ds_bpermute address
// registers), wave results through LDS, one barrier; every thread returns the same value
__device__ __forceinline__ double rmt_block_max_dpp(RmtShared& sh, double v) {
#if RMT_DPP
#define RMT_MAX_STEP(CTRL, MASK) v = fmax(v, rmt_dpp<CTRL, MASK>(v, v));
    RMT_MAX_STEP(0x111, 0xf)      // row_shr:1
    RMT_MAX_STEP(0x112, 0xf)      // row_shr:2
    RMT_MAX_STEP(0x114, 0xf)      // row_shr:4
    RMT_MAX_STEP(0x118, 0xf)      // row_shr:8  -> lane 15 of each row holds the row maximum
    RMT_MAX_STEP(0x142, 0xa)      // row_bcast:15 -> rows 1, 3
    RMT_MAX_STEP(0x143, 0xc)      // row_bcast:31 -> rows 2, 3: lane 63 holds the wave maximum
#undef RMT_MAX_STEP
    if ((threadIdx.x & 63) == 63) sh.red[0][threadIdx.x >> 6] = v;
#else
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d));
    if ((threadIdx.x & 63) == 0) sh.red[0][threadIdx.x >> 6] = v;
#endif
    __syncthreads();
    double r = sh.red[0][0];
#pragma unroll
    for (int w = 1; w < RMT_NW; ++w) r = fmax(r, sh.red[0][w]);
    return r;
}
// One reactor (CH 0) or one chunk of a chained reactor (CH 2: the RHS evaluations exchange their boundary records
// over the tagged-word links, the error norm runs down the chain and comes back through the team's decision
// slot, see rmt_n2_rk45_chain) from t0 to t1.  `gnode0` = reactor index of this thread's first node.
template <int CH>
__device__ __forceinline__ void rmt_rk45_onchip(
        RmtShared& sh, const double* s_tab, real* __restrict__ y, const double* __restrict__ members, const int N,
        const int e, const int gnode0, const double t0, const double t1, const double rtol, const double atol,
        const double h0, const long long max_steps, double* __restrict__ stats, unsigned* __restrict__ flags,
        RmtChainCtx* ctx, unsigned long long* dec, unsigned& att, bool& dead) {
    const int node0 = (int)threadIdx.x * RMT_NPT;            // index inside the workgroup's slots
#if RMT_RK45_LDS >= 1
    __shared__ real s_c[RMT_V][RMT_NODES_WG];
#define SC(j, i) s_c[i][node0 + (j)]
#else
    real r_c[RMT_NPT][RMT_V];
#define SC(j, i) r_c[j][i]
#endif
#if RMT_RK45_LDS >= 2
    __shared__ real s_b[RMT_V][RMT_NODES_WG];
#define SB(j, i) s_b[i][node0 + (j)]
#else
    real r_b[RMT_NPT][RMT_V];
#define SB(j, i) r_b[j][i]
#endif
#if RMT_RK45_LDS >= 3
    __shared__ real s_a[RMT_V][RMT_NODES_WG];
#define SA(j, i) s_a[i][node0 + (j)]
#else
    real r_a[RMT_NPT][RMT_V];
#define SA(j, i) r_a[j][i]
#endif
#if RMT_RK45_LDS >= 4
    __shared__ real s_y[RMT_V][RMT_NODES_WG];
#define SY(j, i) s_y[i][node0 + (j)]
#else
    real r_y[RMT_NPT][RMT_V];
#define SY(j, i) r_y[j][i]
#endif
    if (CH == 0 && threadIdx.x < RMT_V)      // upstream of node 0 (read by lane 0 of wave 0 after the stage barrier)
        sh.inlet[threadIdx.x] = real(members[(size_t)e * RMT_NM +
                                             (threadIdx.x < RMT_S ? M_CIN + (int)threadIdx.x : M_THETA_IN)]);
    RmtMember m;
    rmt_load_member(members + (size_t)e * RMT_NM, m);
    RMT_PROFILE_BIND(m, e, N)
    RmtCarry carry;
    rmt_carry_inlet(m, carry);
    RMT_PROFILE_AT(carry, gnode0 - node0)
    real* ye = y + (size_t)e * RMT_V * N;
    int nvalid = N - gnode0;
    nvalid = nvalid < 0 ? 0 : (nvalid > RMT_NPT ? RMT_NPT : nvalid);
    real ys[RMT_NPT][RMT_V], k[RMT_NPT][RMT_V];
#pragma unroll
    for (int j = 0; j < RMT_NPT; ++j) {
        rmt_safe_state(m, ys[j]);
        if (j < nvalid) {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) ys[j][i] = ye[(size_t)i * N + gnode0 + j];
        }
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) SY(j, i) = ys[j][i];
    }
    // lanes beyond the reactor's end hold the (valid) inlet state and must KEEP it: their derivative is
    // zeroed, otherwise they integrate a phantom node outside the error control (wave-uniform test)
    const bool ragged = __any(nvalid < RMT_NPT);
#define RMT_RK45_PAD                                                                                    \
    if (ragged) {                                                                                       \
        _Pragma("unroll") for (int j = 0; j < RMT_NPT; ++j)                                             \
            _Pragma("unroll") for (int i = 0; i < RMT_V; ++i) k[j][i] = (j < nvalid) ? k[j][i] : real(0); \
    }
#if RMT_MODEL == 2
    preal pwarm[RMT_NPT];
    int warm = 0;
#pragma unroll
    for (int j = 0; j < RMT_NPT; ++j) pwarm[j] = preal(0);
#define RMT_RK45_EVAL(BUF, FL)                                                                          \
    rmt_rhs_block<RMT_NPT, false, CH>(m, sh, BUF, ys, nvalid, carry, k, FL, ctx, nullptr, pwarm, warm); \
    warm = RMT_M2_WARM;                                                                                 \
    RMT_RK45_PAD
#else
#define RMT_RK45_EVAL(BUF, FL)                                                   \
    rmt_rhs_block<RMT_NPT, false, CH, typename rmt_unref<decltype(FL)>::type, rmt_nocache_t, -1, false>(  \
        m, sh, BUF, ys, nvalid, carry, k, FL, ctx);                                \
    RMT_RK45_PAD
#endif
#ifndef RMT_RK45_TWO_COPIES
#define RMT_RK45_TWO_COPIES 1    // a second, test-free inlined RHS copy for stages 2-6 (see above)
#endif
    // the tests of a tested evaluation as per-call extremes folded into `trial` (rmt_callflags_t, 00_config_math.inc)
#ifndef RMT_RK45_CALL_FLAGS
#define RMT_RK45_CALL_FLAGS 1          // (150 -> 86 lane moves per step loop, 6.54e9 -> 6.78e9 accepted node-steps/s at 256 x 1024)
#endif
#if RMT_RK45_CALL_FLAGS && RMT_FLAGS_MODE == 0
#define RMT_RK45_TESTED(BUF) { rmt_callflags_t cf_; rmt_callflags_clear(cf_); RMT_RK45_EVAL(BUF, cf_) rmt_flags_fold(trial, cf_); }
#else
#define RMT_RK45_TESTED(BUF) RMT_RK45_EVAL(BUF, trial)
#endif
    rmt_noflags_t nof2;
    (void)nof2;
    // Dormand-Prince coefficients: read from rmt_dp_tab (scalar loads) where they are used.  As literals
    // the compiler materialises all of them (and h times each) in VGPRs outside the stage loop and spills.
    // h*a_ij: workgroup-uniform, kept in SGPRs - as plain products the compiler hoists all twenty out of
    // the stage loop into VGPRs that then stay live across every RHS evaluation
#define RMT_HC(i) real(h * s_tab[i])
#define RMT_EC(i) real(s_tab[i])
    rmt_flags_t flag, trial;
    rmt_flags_clear(flag);
    rmt_flags_clear(trial);
    unsigned lflag = 0u;
    double t = t0, h = rmt_uniform(rmt_initial_step(h0, stats, e));
    long long nacc = 0, nrej = 0;
    bool have_k1 = false;
    __shared__ double s_dec[2];                  // CH 2: {the reactor's error norm, chain failed} of this attempt
    while (t < t1 && nacc + nrej < max_steps && !dead) {
        bool last = false;
        const double hfull = h;
        if (t + h >= t1) { h = t1 - t; last = true; }
        bool bad = false;
        double errloc = 0.0;
        // Stage s = 1 runs only when K_1 is not at hand: the first step of the launch and after a rejection.  The stages share ONE copy of the RHS code
        // (seven unrolled copies are 80 KB of instructions, more than the instruction cache); s is
        // wave-uniform, so the stage-specific bookkeeping is behind scalar branches.  LDS exchange buffer =
        // s & 1: consecutive RHS calls alternate, and stage 7 -> stage 1 (both buffer 1) are separated by the
        // barrier of the error reduction.
        int s = 1;
        if (have_k1) {
            s = 2;
            const real c1 = RMT_HC(0);
#pragma unroll
            for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) ys[j][i] = SY(j, i) + c1 * SA(j, i);
        } else {
#pragma unroll
            for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) ys[j][i] = SY(j, i);
        }
#pragma unroll 1
        for (; s <= 7; ++s) {
#if RMT_FORCING
            // the forced boundary values at t + c_s h (K_7 = f(t + h, y_new) is K_1 of the next step: FSAL holds, the forcing
            // is continuous inside a launch)
            rmt_forcing_stage(m, carry, members + (size_t)e * RMT_NM, t + rmt_dp_c(s - 1) * h, CH == 0 ? sh.inlet : nullptr);
#endif
#if RMT_RK45_TWO_COPIES && !RMT_CHECK_ALL_STAGES
            if (s == 7 || s == 1) { RMT_RK45_TESTED(s & 1) }               // K_7 / K_1: derivative of a visited state
            else { RMT_RK45_EVAL(s & 1, nof2) }
#else
            RMT_RK45_TESTED(s & 1)
#endif
            if (CH == 2 && ctx->abort) { dead = true; break; }     // a link timed out (workgroup-uniform)
            if (s == 1) {                          // K_1; input of stage 2
                const real c1 = RMT_HC(0);
#pragma unroll
                for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) {
                        SA(j, i) = k[j][i];
                        ys[j][i] = SY(j, i) + c1 * k[j][i];
                    }
            } else if (s == 2) {                   // K_2; input of stage 3
                const real c1 = RMT_HC(1), c2 = RMT_HC(2);
#pragma unroll
                for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) {
                        SB(j, i) = k[j][i];
                        bad |= (j < nvalid) && !__builtin_isfinite(k[j][i]);   // K_2 has weight 0 in y_new and E
                        ys[j][i] = SY(j, i) + (c1 * SA(j, i) + c2 * k[j][i]);
                    }
            } else if (s == 3) {                   // K_3; input of stage 4
                const real c1 = RMT_HC(3), c2 = RMT_HC(4), c3 = RMT_HC(5);
#pragma unroll
                for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) {
                        SC(j, i) = k[j][i];
                        ys[j][i] = SY(j, i) + (c1 * SA(j, i) + c2 * SB(j, i) + c3 * k[j][i]);
                    }
            } else if (s == 4) {                   // fold K_1..K_4 into the accumulators of stages 5, 6, 7 and of the error
                const real f51 = RMT_HC(6), f52 = RMT_HC(7), f53 = RMT_HC(8), f54 = RMT_HC(9),
                           f61 = RMT_HC(10), f62 = RMT_HC(11), f63 = RMT_HC(12), f64 = RMT_HC(13),
                           f71 = RMT_HC(15), f73 = RMT_HC(16), f74 = RMT_HC(17);
#pragma unroll
                for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) {
                        const real y0 = SY(j, i), k1 = SA(j, i), k2 = SB(j, i), k3 = SC(j, i), k4 = k[j][i];
                        ys[j][i] = y0 + (f51 * k1 + f52 * k2 + f53 * k3 + f54 * k4);      // Z_5
                        SA(j, i) = y0 + (f61 * k1 + f62 * k2 + f63 * k3 + f64 * k4);      // Z_6 so far
                        SB(j, i) = y0 + (f71 * k1 + f73 * k3 + f74 * k4);                 // Z_7 so far
                        SC(j, i) = RMT_EC(20) * k1 + RMT_EC(21) * k3 + RMT_EC(22) * k4;                           // E so far
                    }
            } else if (s == 5) {
                const real f65 = RMT_HC(14), f75 = RMT_HC(18);
#pragma unroll
                for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) {
                        ys[j][i] = SA(j, i) + f65 * k[j][i];                              // Z_6
                        SB(j, i) += f75 * k[j][i];
                        SC(j, i) += RMT_EC(23) * k[j][i];
                    }
            } else if (s == 6) {
                const real f76 = RMT_HC(19);
#pragma unroll
                for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) {
                        ys[j][i] = SB(j, i) + f76 * k[j][i];                              // y_new (5th order)
                        SC(j, i) += RMT_EC(24) * k[j][i];
                    }
            } else {                               // s == 7: k = K_7 = f(y_new); error estimate
#pragma unroll
                for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) {
                        const double ev = (double)(SC(j, i) + RMT_EC(25) * k[j][i]);
                        const double sc = atol + rtol * fmax(fabs((double)SY(j, i)), fabs((double)ys[j][i]));
                        const double q = rmt_div(fabs(h * ev), sc);      // lean division: ~1 ulp, 8 ops instead of ~25
                        if (j < nvalid) {
                            bad |= !__builtin_isfinite(q) || !__builtin_isfinite((double)ys[j][i]);
                            errloc = fmax(errloc, q);
                        }
                    }
            }
        }
        if (CH == 2 && dead) break;
        double worst = rmt_block_max_dpp(sh, bad ? 1.0e300 : errloc);
        if (CH == 2) {
            // running maximum down the chain; the last chunk's value (= the reactor's) comes back to every chunk
            // through the team's decision slot, so t, h and the accept / reject history stay identical in all
            // chunks (as rmt_n2_ros4_chain)
            const int wave = threadIdx.x >> 6;
            att = rmt_seq_next(att);
            if (wave == 0) {
                int st = ctx->dead;
                if (ctx->has_in) {
                    st |= rmt_link_recv(rmt_ring_entry(ctx->ring_in, ctx->seq_in), ctx->seq_in, sh.cin[0], 1, ctx->abort_word, st);
                    worst = fmax(worst, sh.cin[0][0]);
                }
                if ((threadIdx.x & 63) == 0) sh.cst[0][0] = worst;
                if (ctx->has_out) {
                    rmt_link_send(rmt_ring_entry(ctx->ring_out, ctx->seq_out), ctx->seq_out, sh.cst[0], 1);
                    st |= rmt_link_recv(dec, att, sh.cin[1], 1, ctx->abort_word, st);
                    worst = sh.cin[1][0];
                } else {
                    rmt_link_send(dec, att, sh.cst[0], 1);
                }
                if ((threadIdx.x & 63) == 0) { s_dec[0] = worst; s_dec[1] = st ? 1.0 : 0.0; }
                ctx->dead |= st;
            }
            if (ctx->has_in) ctx->seq_in = rmt_seq_next(ctx->seq_in);
            if (ctx->has_out) ctx->seq_out = rmt_seq_next(ctx->seq_out);
            __syncthreads();
            worst = s_dec[0];
            if (s_dec[1] != 0.0) { dead = true; break; }
        }
        const double err = rmt_uniform(worst);
        // 0.9 err^-1/5 through the lean exp/log of the kinetics (their literals are in registers anyway; the
        // library pow brings ~25 more fp64 literals that the compiler parks in VGPRs across the whole step)
        const double grow = (err > 0.0 && err < 1.0e300) ? 0.9 * rmt_exp(-0.2 * rmt_log(err)) : 5.0;
        double fac;
        if (err >= 1.0e300) {                     // a stage produced a non-finite value: Python would have raised
            fac = 0.25;
            ++nrej;
            have_k1 = false;
            rmt_flags_clear(trial);
        } else if (err <= 1.0) {
            t = last ? t1 : t + h;
            ++nacc;
            fac = fmin(5.0, fmax(0.2, grow));
#pragma unroll
            for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) {
                    SY(j, i) = ys[j][i];
                    SA(j, i) = k[j][i];                                               // FSAL
                }
            have_k1 = true;
            rmt_flags_merge(flag, trial);
            rmt_flags_clear(trial);
        } else {
            ++nrej;
            fac = fmax(0.2, grow);
            have_k1 = false;
            rmt_flags_clear(trial);
        }
        h = fmax(h * fac, 1e-14);
        if (last && t >= t1) h = fmax(h, hfull * fmin(fac, 1.0));   // a step clipped to the interval end does not shrink h_last
    }
#pragma unroll
    for (int j = 0; j < RMT_NPT; ++j) {
        if (j < nvalid) {
            real v[RMT_V];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) {
                v[i] = SY(j, i);
                ye[(size_t)i * N + gnode0 + j] = v[i];
            }
            lflag |= rmt_finite_flag(v);
        }
    }
    if (t < t1) lflag |= RMT_FLAG_STEP;
    lflag |= rmt_flags_bits(flag);
    if (threadIdx.x == 0 && (CH == 0 || ctx->chunk == 0)) {
        stats[(size_t)e * 4 + 0] = t;
        stats[(size_t)e * 4 + 1] = h;
        ((long long*)stats)[(size_t)e * 4 + 2] = nacc;
        ((long long*)stats)[(size_t)e * 4 + 3] = nrej;
    }
    if (lflag) atomicOr(&flags[e], lflag);
#undef SA
#undef SB
#undef SC
#undef SY
#undef RMT_RK45_EVAL
#undef RMT_RK45_TESTED
#undef RMT_RK45_PAD
#undef RMT_HC
#undef RMT_EC
}

extern "C" __global__ __launch_bounds__(RMT_BLOCK) void rmt_n2_rk45_reg(
        real* __restrict__ y, const double* __restrict__ members, const int N, const double t0,
        const double t1, const double rtol, const double atol, const double h0, const long long max_steps,
        double* __restrict__ stats, unsigned* __restrict__ flags) {
    __shared__ RmtShared sh;
    __shared__ double s_tab[26];                 // the coefficient table, staged once (visible after the barrier below)
    if (threadIdx.x < 26) s_tab[threadIdx.x] = rmt_dp_tab[threadIdx.x];
    rmt_math_init();
    unsigned att = 0u;
    bool dead = false;
    rmt_rk45_onchip<0>(sh, s_tab, y, members, N, (int)blockIdx.x, (int)threadIdx.x * RMT_NPT, t0, t1, rtol, atol, h0,
                       max_steps, stats, flags, nullptr, nullptr, att, dead);
}

// ===================================================================== kernel: adaptive RK45 on chip, chained workgroups
// The same stepper for reactors of more than RMT_BLOCK*RMT_NPT nodes (and to give a few long reactors more than one
// CU each): reactor e is cut into C chunks of RMT_NODES_WG nodes, one workgroup per chunk with the chunk's state on
// chip, T teams of C resident workgroups (T*C <= number of CUs), team t integrating reactors t, t+T, ...  Every
// RHS evaluation hands its boundary record {clamped state of the last node, pressure after it} to the next chunk
// over a tagged-word link (rmt_rhs_block<.., 2>), so the seven stages of a step pipeline down the chain with a skew
// of one message latency per chunk; after stage 7 the running maximum of the error norm travels the same way and
// the last chunk publishes the reactor's norm in the team's decision slot.  A step costs 7 stage times + the
// skew + one decision round trip instead of the memory-resident stepper's walk over all node blocks on ONE CU.
#if !RMT_PROFILE      // (a profiled run keeps a reactor on one workgroup: the chained form does not carry the profile)
extern "C" __global__ __launch_bounds__(RMT_BLOCK) void rmt_n2_rk45_chain(
        real* __restrict__ y, const double* __restrict__ members, const int N, const int E, const int C,
        const int T, const double t0, const double t1, const double rtol, const double atol, const double h0,
        const long long max_steps, double* __restrict__ stats, unsigned* __restrict__ flags,
        unsigned long long* __restrict__ rings, unsigned long long* __restrict__ decision,
        unsigned* __restrict__ abort_words) {
    __shared__ RmtShared sh;
    __shared__ double s_tab[26];
    if (threadIdx.x < 26) s_tab[threadIdx.x] = rmt_dp_tab[threadIdx.x];
    rmt_math_init();
    const int team = blockIdx.x / C, c = blockIdx.x % C;
    RmtChainCtx ctx;
    ctx.has_in = c > 0;
    ctx.has_out = c < C - 1;
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
    ctx.bp = false;                                      // the decision rendezvous bounds the producer's lead (8 messages)
    ctx.bp_in = ctx.bp_out = nullptr;
    ctx.known = 0u;
    unsigned long long* const dec = decision + (size_t)team * 2;
    unsigned att = 0u;                                   // step attempts of this team = tag of the decision slot
    bool dead = false;
    int e = team;
    for (; e < E && !dead; e += T) {
        rmt_rk45_onchip<2>(sh, s_tab, y, members, N, e, c * RMT_NODES_WG + (int)threadIdx.x * RMT_NPT, t0, t1, rtol,
                           atol, h0, max_steps, stats, flags, &ctx, dec, att, dead);
        __syncthreads();                                 // the next reactor reuses the workgroup's slots
    }
    if (dead && threadIdx.x == 0) {       // a link timed out: let the rest of the chain drain; the team's reactors
        __hip_atomic_store(ctx.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // from this one on are not advanced
        for (int e2 = e; e2 < E; e2 += T) atomicOr(&flags[e2], RMT_FLAG_STEP);    // (the one in flight has it: t < t1)
    }
}
#endif   // !RMT_PROFILE
#endif   // on-chip RK45 fits

