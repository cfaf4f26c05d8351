// Monitor of the dynamic models (solver-config "monitor", rmt_app_amd/monitor.py): per state row y[e][v][0..N) the five
// numbers a time series needs,
//     out[e][v][0..5) = { y[N-1], max_n y, argmax_n y (as double), min_n y, max_n |dydt| (0.0 when dydt is null) }.
// Mechanism-independent and a translation unit of its own (NOT part of the stepper template kernels/*.inc): compiled
// once with hipRTC (rmt_n2_monitor_source -> rmt_n2_compile) and loaded by rmt_n2_monitor_create.
//
// Semantics, the same for every grid shape:
//   * comparisons are plain > and <, so a NaN entry never wins;
//   * ties resolve to the lowest node index (a flat profile: argmax 0); a row without any winner (all NaN or -inf)
//     reports max = -inf, argmax 0, min = +inf;
//   * no floating-point arithmetic beyond fabs (fp32 states are widened to double, which is exact).
// A pure read stream of E*V*N reals.  rows_per_block != 1: one wave per row (thousands of 20-node rows, or enough rows
// to fill the device with waves), 1: one workgroup per row, its waves combined through LDS (a few long rows).  The
// workgroup size is the launch's (a multiple of 64, at most RMT_MON_MAX_BLOCK; the library launches 256).  Rows are walked grid-stride.  Loads are
// 16 bytes per lane from the first 16-byte boundary of the row on, scalar before it and behind the last full vector.
// No atomics, no scratch, 448 bytes of LDS.
#define RMT_MON_MAX_BLOCK 1024
#define RMT_MON_MAX_WAVES (RMT_MON_MAX_BLOCK/64)
#define RMT_MON_NOIDX 0x7fffffff

template <typename real> struct rmt_mon_vec;
template <> struct rmt_mon_vec<double> { typedef double type __attribute__((ext_vector_type(2))); enum { W = 2 }; };
template <> struct rmt_mon_vec<float> { typedef float type __attribute__((ext_vector_type(4))); enum { W = 4 }; };

struct rmt_mon_acc {
    double vmax, vmin, amax;
    int imax;
};

__device__ __forceinline__ void rmt_mon_take(rmt_mon_acc& a, double x, int i) {
    if (x > a.vmax) { a.vmax = x; a.imax = i; }
    if (x < a.vmin) a.vmin = x;
}

// (value, index) pairs of different lanes / waves: the larger value, on a tie the lower index
__device__ __forceinline__ void rmt_mon_merge(rmt_mon_acc& a, double vmax, int imax, double vmin, double amax) {
    if (vmax > a.vmax || (vmax == a.vmax && imax < a.imax)) { a.vmax = vmax; a.imax = imax; }
    if (vmin < a.vmin) a.vmin = vmin;
    if (amax > a.amax) a.amax = amax;
}

// elements of one row for one of `nt` cooperating lanes (t = 0..nt-1); every lane sees its indices in increasing order
template <typename real, bool ABS>
__device__ __forceinline__ void rmt_mon_row(const real* __restrict__ p, int N, int t, int nt, rmt_mon_acc& a) {
    typedef typename rmt_mon_vec<real>::type vec;
    const int W = rmt_mon_vec<real>::W;
    // head: up to the first 16-byte boundary (an address is always a multiple of sizeof(real))
    int head = (int)(((16u - (unsigned)((size_t)p & 15u)) & 15u)/sizeof(real));
    if (head > N) head = N;
    const int nvec = (N - head)/W;
    const int tail0 = head + nvec*W;
    if (t < head) {
        const double x = (double)p[t];
        if (ABS) { const double f = __builtin_fabs(x); if (f > a.amax) a.amax = f; }
        else rmt_mon_take(a, x, t);
    }
    const vec* __restrict__ pv = (const vec*)(p + head);
    int j = t;
    for (; j + 3*nt < nvec; j += 4*nt) {          // four independent 16-byte loads in flight per lane
        const vec v0 = pv[j], v1 = pv[j + nt], v2 = pv[j + 2*nt], v3 = pv[j + 3*nt];
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (ABS) { const double f = __builtin_fabs((double)v0[c]); if (f > a.amax) a.amax = f; }
            else rmt_mon_take(a, (double)v0[c], head + j*W + c);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (ABS) { const double f = __builtin_fabs((double)v1[c]); if (f > a.amax) a.amax = f; }
            else rmt_mon_take(a, (double)v1[c], head + (j + nt)*W + c);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (ABS) { const double f = __builtin_fabs((double)v2[c]); if (f > a.amax) a.amax = f; }
            else rmt_mon_take(a, (double)v2[c], head + (j + 2*nt)*W + c);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (ABS) { const double f = __builtin_fabs((double)v3[c]); if (f > a.amax) a.amax = f; }
            else rmt_mon_take(a, (double)v3[c], head + (j + 3*nt)*W + c);
        }
    }
    for (; j < nvec; j += nt) {
        const vec v = pv[j];
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (ABS) { const double f = __builtin_fabs((double)v[c]); if (f > a.amax) a.amax = f; }
            else rmt_mon_take(a, (double)v[c], head + j*W + c);
        }
    }
    if (tail0 + t < N) {                           // fewer than W elements behind the last full vector
        const double x = (double)p[tail0 + t];
        if (ABS) { const double f = __builtin_fabs(x); if (f > a.amax) a.amax = f; }
        else rmt_mon_take(a, x, tail0 + t);
    }
}

template <typename real>
__device__ __forceinline__ void rmt_n2_monitor_rows(const real* __restrict__ y, const real* __restrict__ dydt,
                                                    double* __restrict__ out, long long rows, int N, int rows_per_block) {
    __shared__ double s_max[RMT_MON_MAX_WAVES], s_min[RMT_MON_MAX_WAVES], s_abs[RMT_MON_MAX_WAVES];
    __shared__ int s_idx[RMT_MON_MAX_WAVES];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, waves = (int)blockDim.x >> 6;
    const bool per_wave = rows_per_block != 1;            // the same in every lane of the grid
    const int t = per_wave ? lane : (int)threadIdx.x, nt = per_wave ? 64 : (int)blockDim.x;
    const long long step = (long long)gridDim.x*(per_wave ? waves : 1);
    const long long first = per_wave ? (long long)blockIdx.x*waves + wave : (long long)blockIdx.x;
    // (one workgroup per row: every wave of the block walks the same rows, so the barriers below are uniform)
    for (long long row = first; row < rows; row += step) {
        const real* __restrict__ p = y + (size_t)row*(size_t)N;
        rmt_mon_acc a = {-__builtin_huge_val(), __builtin_huge_val(), 0.0, RMT_MON_NOIDX};
        rmt_mon_row<real, false>(p, N, t, nt, a);
        if (dydt) rmt_mon_row<real, true>(dydt + (size_t)row*(size_t)N, N, t, nt, a);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
            rmt_mon_merge(a, __shfl_xor(a.vmax, m, 64), __shfl_xor(a.imax, m, 64), __shfl_xor(a.vmin, m, 64),
                          __shfl_xor(a.amax, m, 64));
        if (!per_wave) {
            if (lane == 0) { s_max[wave] = a.vmax; s_idx[wave] = a.imax; s_min[wave] = a.vmin; s_abs[wave] = a.amax; }
            __syncthreads();
            if (threadIdx.x == 0)
                for (int w = 1; w < waves; ++w) rmt_mon_merge(a, s_max[w], s_idx[w], s_min[w], s_abs[w]);
            __syncthreads();                              // (the next row's partial results overwrite s_*)
        }
        if (per_wave ? lane == 0 : threadIdx.x == 0) {
            double* __restrict__ o = out + (size_t)row*5u;
            o[0] = (double)p[N - 1];
            o[1] = a.vmax;
            o[2] = (double)(a.imax == RMT_MON_NOIDX ? 0 : a.imax);
            o[3] = a.vmin;
            o[4] = a.amax;
        }
    }
}

extern "C" __global__ __launch_bounds__(RMT_MON_MAX_BLOCK) void rmt_n2_monitor_rows_f64(
    const double* y, const double* dydt, double* out, long long rows, int N, int rows_per_block) {
    rmt_n2_monitor_rows<double>(y, dydt, out, rows, N, rows_per_block);
}

extern "C" __global__ __launch_bounds__(RMT_MON_MAX_BLOCK) void rmt_n2_monitor_rows_f32(
    const float* y, const float* dydt, double* out, long long rows, int N, int rows_per_block) {
    rmt_n2_monitor_rows<float>(y, dydt, out, rows, N, rows_per_block);
}
