// Sampled PI controller of the dynamic model N2 (solver-config "control", rmt_app_amd/control.py): measure, evaluate the
// control law and write the manipulated value into the member's device row - between two launches of a stepper, without
// the host.  Mechanism-independent and a translation unit of its own (NOT part of the stepper template kernels/*.inc):
// compiled once with hipRTC (rmt_n2_control_source -> rmt_n2_compile, WITH -ffp-contract=off: every operation of the law
// is one correctly rounded fp64 operation, so numpy reproduces it bit for bit) and loaded by rmt_n2_control_create.
//
// One wave per member, members walked grid-stride.  Per member e:
//   * measurement from y[e] ([V][N] doubles): the outlet values are single loads, the peak temperature a strided read of
//     the temperature row and a wave reduction - the access pattern of rmt_mon_row (monitor_kernels.inc): 16-byte loads
//     from the first aligned address, a scalar head and tail; comparisons are plain >, so a NaN never wins;
//   * lane 0 evaluates the law from the member's parameter block and the setpoint of this sample:
//         e = r - pv;   I' = I + ki*e   (I' = I when ki == 0)
//         v = u0 + kp*e + I';  u = min(max(v, lo), hi);   I = I' only if v == u
//   * lane 0 writes the controller state {I, u, count}, slice k of the log {pv, r, u, saturated} and the manipulated field
//     of the member row in the row's own scaling (the mapping of plan.forced_fields, restated in rmt_ctl_store_field), the
//     matching slope in the row's tail set to 0;
//   * hold != 0: only the held u (state[1]) is written into the row again - the host's refresh uploads whole rows - and
//     nothing else changes; a member that has not been sampled yet (count == 0) keeps the row it has.
// No atomics, no LDS, no scratch; every store is an ordinary vector store.
#define RMT_CTL_BLOCK 256
#define RMT_CTL_PARAMS 8          // doubles per member: kp, ki = kp*Ts/Ti, u0, lo, hi, selector, species index, reserved
#define RMT_CTL_STATE 3           // I, u, number of samples taken
#define RMT_CTL_LOG 4             // pv, r, u, saturated (0.0 / 1.0)
// selector: what is measured
#define RMT_CTL_OUTLET_T 0
#define RMT_CTL_PEAK_T 1
#define RMT_CTL_OUTLET_X 2
// member row (kernels/00_config_math.inc): the fields a controller may move, and the scale of the temperatures
#define RMT_CTL_M_TF 1
#define RMT_CTL_M_P0 2
#define RMT_CTL_M_THETA_IN 3
#define RMT_CTL_M_TM 14

typedef double rmt_ctl_vec __attribute__((ext_vector_type(2)));

// largest element of p[0..N) for the 64 lanes of one wave (every lane returns it); -inf when no element compares greater
__device__ __forceinline__ double rmt_ctl_row_max(const double* __restrict__ p, int N, int lane) {
    double vmax = -__builtin_huge_val();
    // head: up to the first 16-byte boundary (an address is always a multiple of 8)
    int head = (int)(((16u - (unsigned)((size_t)p & 15u)) & 15u)/sizeof(double));
    if (head > N) head = N;
    const int nvec = (N - head)/2;
    const int tail0 = head + nvec*2;
    if (lane < head) { const double x = p[lane]; if (x > vmax) vmax = x; }
    const rmt_ctl_vec* __restrict__ pv = (const rmt_ctl_vec*)(p + head);
    int j = lane;
    for (; j + 3*64 < nvec; j += 4*64) {          // four independent 16-byte loads in flight per lane
        const rmt_ctl_vec v0 = pv[j], v1 = pv[j + 64], v2 = pv[j + 128], v3 = pv[j + 192];
        if (v0[0] > vmax) vmax = v0[0];
        if (v0[1] > vmax) vmax = v0[1];
        if (v1[0] > vmax) vmax = v1[0];
        if (v1[1] > vmax) vmax = v1[1];
        if (v2[0] > vmax) vmax = v2[0];
        if (v2[1] > vmax) vmax = v2[1];
        if (v3[0] > vmax) vmax = v3[0];
        if (v3[1] > vmax) vmax = v3[1];
    }
    for (; j < nvec; j += 64) {
        const rmt_ctl_vec v = pv[j];
        if (v[0] > vmax) vmax = v[0];
        if (v[1] > vmax) vmax = v[1];
    }
    if (tail0 + lane < N) { const double x = p[tail0 + lane]; if (x > vmax) vmax = x; }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double o = __shfl_xor(vmax, m, 64);
        if (o > vmax) vmax = o;
    }
    return vmax;
}

// the manipulated value u in the member row: THETA_IN = (T_in - Tf)/Tf, P0 = P_in, TM = MeTe; its slope in the tail
// {t_ref, d THETA_IN/dt, d P0/dt, d TM/dt} (kernels/11_forcing.inc) becomes 0: u holds until the next sample
__device__ __forceinline__ void rmt_ctl_store_field(double* __restrict__ row, int tail_at, int field, double u) {
    if (field == 0) {
        const double tf = row[RMT_CTL_M_TF];
        row[RMT_CTL_M_THETA_IN] = (u - tf)/tf;
    } else if (field == 1) {
        row[RMT_CTL_M_P0] = u;
    } else {
        row[RMT_CTL_M_TM] = u;
    }
    row[tail_at + 1 + field] = 0.0;
}

// y [E][V][N]; rows [E][width] (the device rows of a forced code object, tail at tail_at); params [E][RMT_CTL_PARAMS];
// setpoint [E] (this sample's); state [E][RMT_CTL_STATE]; log [E][RMT_CTL_LOG] (this sample's slice); field 0 / 1 / 2 =
// inlet temperature / inlet pressure / medium temperature.  y, setpoint and log are not touched when hold != 0.
extern "C" __global__ __launch_bounds__(RMT_CTL_BLOCK) void rmt_n2_control_update_f64(
    const double* __restrict__ y, double* __restrict__ rows, const double* __restrict__ params,
    const double* __restrict__ setpoint, double* __restrict__ state, double* __restrict__ log, int E, int S, int V, int N,
    int width, int tail_at, int field, int hold) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, waves = (int)blockDim.x >> 6;
    for (long long e = (long long)blockIdx.x*waves + wave; e < E; e += (long long)gridDim.x*waves) {
        double* __restrict__ row = rows + (size_t)e*(size_t)width;
        double* __restrict__ st = state + (size_t)e*RMT_CTL_STATE;
        if (hold) {
            if (lane == 0 && st[2] > 0.0) rmt_ctl_store_field(row, tail_at, field, st[1]);
            continue;
        }
        const double* __restrict__ prm = params + (size_t)e*RMT_CTL_PARAMS;
        const double* __restrict__ ye = y + (size_t)e*(size_t)V*(size_t)N;
        const int sel = (int)prm[5];                       // the same in every lane of the wave
        double theta = 0.0;
        if (sel == RMT_CTL_PEAK_T) theta = rmt_ctl_row_max(ye + (size_t)(V - 1)*(size_t)N, N, lane);
        if (lane == 0) {
            double pv;
            if (sel == RMT_CTL_OUTLET_X) {
                const int s = (int)prm[6];
                double sum = 0.0;
                for (int i = 0; i < S; ++i) sum += ye[(size_t)i*(size_t)N + (size_t)(N - 1)];
                pv = s >= 0 && s < S ? ye[(size_t)s*(size_t)N + (size_t)(N - 1)]/sum : __builtin_nan("");
            } else {
                if (sel != RMT_CTL_PEAK_T) theta = ye[(size_t)(V - 1)*(size_t)N + (size_t)(N - 1)];
                const double tf = row[RMT_CTL_M_TF];
                pv = theta*tf + tf;
            }
            const double kp = prm[0], ki = prm[1], u0 = prm[2], lo = prm[3], hi = prm[4];
            const double r = setpoint[e];
            const double I = st[0];
            const double err = r - pv;
            const double Ip = ki != 0.0 ? I + ki*err : I;
            const double v = (u0 + kp*err) + Ip;
            double u = v < lo ? lo : v;
            u = u > hi ? hi : u;
            const bool free = v == u;
            st[0] = free ? Ip : I;
            st[1] = u;
            st[2] = st[2] + 1.0;
            double* __restrict__ lg = log + (size_t)e*RMT_CTL_LOG;
            lg[0] = pv;
            lg[1] = r;
            lg[2] = u;
            lg[3] = free ? 0.0 : 1.0;
            rmt_ctl_store_field(row, tail_at, field, u);
        }
    }
}
