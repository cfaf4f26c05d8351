#if RMT_WITH_N1
#ifndef RMT_ROS_GAM
#define RMT_ROS_GAM 0.5
#endif
// ===================================================================== kernel: steady-state model N1 (batched)
// (node functions rmt_n1_init / rmt_n1_rhs / rmt_n1_rhs_jac of the steady model RMT_SS_MODEL and its member-row layout:
// see the node-physics section above; the V1 x V1 inverse rmt_invert_n: 00_config_math.inc)
#ifndef RMT_N1_SCHEME
#define RMT_N1_SCHEME 1          // 1: RODAS4, 0: Kaps-Rentrop/Shampine
#endif
extern "C" __global__ __launch_bounds__(64) void rmt_n1_ros4(
        const double* __restrict__ members1, double* __restrict__ out /* [E][nout][V1] */,
        const int E, const int nout, const double rtol, const double atol, const double h0,
        const long long max_steps, double* __restrict__ stats, unsigned* __restrict__ flags) {
    rmt_math_init();
    const int e = blockIdx.x * 64 + (int)threadIdx.x;
    const bool live = e < E;
    const double* mr = members1 + (size_t)(live ? e : 0) * RMT_NM1;
    const double A21 = 2.0, A31 = 48.0 / 25, A32 = 6.0 / 25, C21 = -8.0, C31 = 372.0 / 25, C32 = 12.0 / 5,
                 C41 = -112.0 / 125, C42 = -54.0 / 125, C43 = -2.0 / 5, B1 = 19.0 / 9, B2 = 0.5,
                 B3 = 25.0 / 108, B4 = 125.0 / 108, E1 = 17.0 / 54, E2 = 7.0 / 36, E4 = 125.0 / 108;
    real u[RMT_V1];
    rmt_n1_init(mr, u);                                  // the model's state at z* = 0 (22_node_n1.inc, 23_node_steady.inc)
    rmt_flags_t flag, trial;
    rmt_flags_clear(flag);
    double z = 0.0, h = h0;
    long long nacc = 0, nrej = 0;
    int kout = 0;
    if (live) {
#pragma unroll
        for (int i = 0; i < RMT_V1; ++i) out[((size_t)e * nout + 0) * RMT_V1 + i] = (double)u[i];
    }
    kout = 1;
    bool active = live;
    // every lane runs its own step sequence; the loop ends when no lane of the wave is active
    while (__any(active)) {
        if (active) {
            const double zt = (double)kout / (double)(nout - 1);
            bool hit = false;
            double hs = h;
            if (z + hs >= zt) { hs = zt - z; hit = true; }
            rmt_flags_clear(trial);
            real f1[RMT_V1], a[RMT_V1][RMT_V1];
#if !RMT_N1_JAC_FD
            rmt_n1_rhs_jac(mr, u, f1, a, trial);
#else
            rmt_n1_rhs(mr, u, f1, trial);
#pragma unroll
            for (int c = 0; c < RMT_V1; ++c) {
                real up[RMT_V1], fp[RMT_V1];
#pragma unroll
                for (int i = 0; i < RMT_V1; ++i) up[i] = u[i];
                const real d = real(RMT_FP32 ? 3e-4 : 1.5e-8) * rmt_max(rmt_abs(u[c]), real(1e-3));
                up[c] += d;
                const real id = rmt_rcp(up[c] - u[c]);
                rmt_noflags_t sf;
                rmt_n1_rhs(mr, up, fp, sf);
#pragma unroll
                for (int r = 0; r < RMT_V1; ++r) a[r][c] = -(fp[r] - f1[r]) * id;
            }
#endif
            const real inv_gh = real(1.0 / ((RMT_N1_SCHEME == 1 ? 0.25 : RMT_ROS_GAM) * hs)), ih = real(1.0 / hs);
#pragma unroll
            for (int i = 0; i < RMT_V1; ++i) a[i][i] += inv_gh;
            const real pv = rmt_invert_n<RMT_V1>(a);
#if RMT_N1_SCHEME == 1
            // RODAS4 (see rmt_rodas_bs): Y_i = u + sum a_ij G_j, A G_i = f(Y_i) + sum c_ij G_j / h,
            // Y_6 = Y_5 + G_5, u_new = Y_6 + G_6, error = G_6
            const real RA[6][5] = {{0, 0, 0, 0, 0}, {real(1.544), 0, 0, 0, 0},
                {real(0.9466785280815826), real(0.2557011698983284), 0, 0, 0},
                {real(3.314825187068521), real(2.896124015972201), real(0.9986419139977817), 0, 0},
                {real(1.221224509226641), real(6.019134481288629), real(12.53708332932087), real(-0.6878860361058950), 0},
                {real(1.221224509226641), real(6.019134481288629), real(12.53708332932087), real(-0.6878860361058950), real(1)}};
            const real RC[6][5] = {{0, 0, 0, 0, 0}, {real(-5.6688), 0, 0, 0, 0},
                {real(-2.430093356833875), real(-0.2063599157091915), 0, 0, 0},
                {real(-0.1073529058151375), real(-9.594562251023355), real(-20.47028614809616), 0, 0},
                {real(7.496443313967647), real(-10.24680431464352), real(-33.99990352819905), real(11.70890893206160), 0},
                {real(8.083246795921522), real(-7.981132988064893), real(-31.52159432874371), real(16.31930543123136),
                 real(-6.058818238834054)}};
            real g[6][RMT_V1], us[RMT_V1], un[RMT_V1];
#pragma unroll
            for (int st = 0; st < 6; ++st) {
                real fs[RMT_V1], b[RMT_V1];
#pragma unroll
                for (int i = 0; i < RMT_V1; ++i) {
                    real acc = u[i], cc = real(0);
#pragma unroll
                    for (int q = 0; q < 5; ++q) {
                        if (q < st) { acc += RA[st][q] * g[q][i]; cc += RC[st][q] * g[q][i]; }
                    }
                    us[i] = acc;
                    b[i] = cc * ih;
                }
                if (st == 0) {
#pragma unroll
                    for (int i = 0; i < RMT_V1; ++i) fs[i] = f1[i];
                } else {
                    rmt_n1_rhs(mr, us, fs, trial);
                }
#pragma unroll
                for (int r = 0; r < RMT_V1; ++r) {
                    real acc = real(0);
#pragma unroll
                    for (int c = 0; c < RMT_V1; ++c) acc += a[r][c] * (fs[c] + b[c]);
                    g[st][r] = acc;
                }
            }
            double worst = 0.0;
            bool bad = !(pv > real(0));
#pragma unroll
            for (int i = 0; i < RMT_V1; ++i) {
                const double yn = (double)us[i] + (double)g[5][i];
                un[i] = real(yn);
                bad |= !__builtin_isfinite(yn);
                worst = fmax(worst, fabs((double)g[5][i]) / (atol + rtol * fmax(fabs((double)u[i]), fabs(yn))));
            }
#else
            real g1[RMT_V1], g2[RMT_V1], g3[RMT_V1], g4[RMT_V1], b[RMT_V1], us[RMT_V1], f3[RMT_V1];
#define RMT_MATVEC(dst, src)                                                        \
            _Pragma("unroll") for (int r_ = 0; r_ < RMT_V1; ++r_) {                 \
                real acc_ = real(0);                                                \
                _Pragma("unroll") for (int c_ = 0; c_ < RMT_V1; ++c_) acc_ += a[r_][c_] * src[c_]; \
                dst[r_] = acc_;                                                     \
            }
            RMT_MATVEC(g1, f1)
#pragma unroll
            for (int i = 0; i < RMT_V1; ++i) us[i] = u[i] + real(A21) * g1[i];
            rmt_n1_rhs(mr, us, f3, trial);
#pragma unroll
            for (int i = 0; i < RMT_V1; ++i) b[i] = f3[i] + real(C21) * g1[i] * ih;
            RMT_MATVEC(g2, b)
#pragma unroll
            for (int i = 0; i < RMT_V1; ++i) us[i] = u[i] + real(A31) * g1[i] + real(A32) * g2[i];
            rmt_n1_rhs(mr, us, f3, trial);
#pragma unroll
            for (int i = 0; i < RMT_V1; ++i) b[i] = f3[i] + (real(C31) * g1[i] + real(C32) * g2[i]) * ih;
            RMT_MATVEC(g3, b)
#pragma unroll
            for (int i = 0; i < RMT_V1; ++i)
                b[i] = f3[i] + (real(C41) * g1[i] + real(C42) * g2[i] + real(C43) * g3[i]) * ih;
            RMT_MATVEC(g4, b)
#undef RMT_MATVEC
            double worst = 0.0;
            bool bad = !(pv > real(0));
            real un[RMT_V1];
#pragma unroll
            for (int i = 0; i < RMT_V1; ++i) {
                const double yn = (double)u[i] + B1 * (double)g1[i] + B2 * (double)g2[i] + B3 * (double)g3[i] + B4 * (double)g4[i];
                const double er = E1 * (double)g1[i] + E2 * (double)g2[i] + E4 * (double)g4[i];
                un[i] = real(yn);
                bad |= !__builtin_isfinite(yn);
                worst = fmax(worst, fabs(er) / (atol + rtol * fmax(fabs((double)u[i]), fabs(yn))));
            }
#endif
            if (bad || !__builtin_isfinite(worst)) {
                h = fmax(hs * 0.25, 1e-14);
                ++nrej;
            } else if (worst <= 1.0) {
                z = hit ? zt : z + hs;
                ++nacc;
#pragma unroll
                for (int i = 0; i < RMT_V1; ++i) u[i] = un[i];
                rmt_flags_merge(flag, trial);
                const double fac = fmin((worst > 1.89e-4) ? 0.9 * rmt_exp(-0.25 * rmt_log(worst)) : 7.5, 5.0);
                h = (hit ? h : hs) * fac;                       // a clipped step does not shrink h
                if (hit) {
#pragma unroll
                    for (int i = 0; i < RMT_V1; ++i) out[((size_t)e * nout + kout) * RMT_V1 + i] = (double)u[i];
                    ++kout;
                }
            } else {
                ++nrej;
                h = fmax(hs * fmax(0.2, 0.9 * pow(worst, RMT_N1_SCHEME == 1 ? -0.25 : -1.0 / 3.0)), 1e-14);
            }
            if (kout >= nout || nacc + nrej >= max_steps) active = false;
        }
    }
    if (live) {
        unsigned lf = rmt_flags_bits(flag);
        if (kout < nout) lf |= RMT_FLAG_STEP;
        stats[(size_t)e * 4 + 0] = z;
        stats[(size_t)e * 4 + 1] = h;
        ((long long*)stats)[(size_t)e * 4 + 2] = nacc;
        ((long long*)stats)[(size_t)e * 4 + 3] = nrej;
        if (lf) atomicOr(&flags[e], lf);
    }
}
#endif  // RMT_WITH_N1
#endif  // RMT_HOST_EMULATION
