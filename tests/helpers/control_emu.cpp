// TEST INFRASTRUCTURE: the controller's kernel (rmt_app_amd/csrc/control_kernels.inc) built for the host, so that the kernel's
// indexing, its law and the host walk around it can be checked without a GPU (tests/test_control_emulated_cpu.py).
// Every thread of a workgroup runs the kernel on its own, twice: in the first pass each lane records the partial maximum
// it brings to the wave reduction, in the second pass the reduction returns the maximum over the wave's recorded values
// (the side effects of the first pass are undone in between).  Compiled with clang++ -ffp-contract=off.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
struct d3 { unsigned x, y, z; };
static d3 threadIdx, blockIdx, blockDim, gridDim;
static int g_pass = 1;
static std::vector<double> g_part[1024];     // per thread of the block: partial maxima, one per reduction
static int g_calls[1024];
static double __shfl_xor(double v, int m, int) {
    const unsigned t = threadIdx.x;
    const int group = g_calls[t] / 6;
    g_calls[t]++;
    if (g_pass == 1) { if (m == 32) g_part[t].push_back(v); return v; }
    if (m != 32) return v;
    double best = v;
    const unsigned w0 = t & ~63u;
    for (unsigned l = w0; l < w0 + 64; ++l) { const double o = g_part[l][group]; if (o > best) best = o; }
    return best;
}
#include "control_kernels.inc"

extern "C" void emu_update(const double* y, double* rows, const double* params, const double* setpoint, double* state,
                           double* log, int E, int S, int V, int N, int width, int tail_at, int field, int hold, int grid) {
    blockDim = {256, 1, 1}; gridDim = {(unsigned)grid, 1, 1};
    std::vector<double> rows0(rows, rows + (size_t)E*width), state0(state, state + (size_t)E*3);
    for (unsigned b = 0; b < (unsigned)grid; ++b) {
        blockIdx = {b, 0, 0};
        for (int t = 0; t < 256; ++t) { g_part[t].clear(); }
        for (g_pass = 1; g_pass <= 2; ++g_pass) {
            if (g_pass == 2) {      // undo the side effects of the first pass for the members of this block
                memcpy(rows, rows0.data(), rows0.size()*8); memcpy(state, state0.data(), state0.size()*8);
            }
            for (unsigned t = 0; t < 256; ++t) {
                threadIdx = {t, 0, 0}; g_calls[t] = 0;
                rmt_n2_control_update_f64(y, rows, params, setpoint, state, log, E, S, V, N, width, tail_at, field, hold);
            }
        }
        rows0.assign(rows, rows + (size_t)E*width); state0.assign(state, state + (size_t)E*3);
    }
}
