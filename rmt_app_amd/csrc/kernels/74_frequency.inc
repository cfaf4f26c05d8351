//>>> RMT_FREQ  (plan.Mechanism.source generates every unit but the frequency unit, codeplan.freq_plan, WITHOUT the lines
// from this mark to the closing one; the block lies inside the marks of RMT_SENS, whose closing mark is the last line of
// this file: a unit without RMT_SENS has neither text, the sensitivity unit is what it is without this file)
#if RMT_FREQ
// ===================================================================== frequency response of the N2 operating point
// solver-config "frequency-response" (host: rmt_app_amd/frequency.py).  A small harmonic disturbance of an input,
// p(t) = p0 + Re(dp e^{iwt}), moves the linearised dynamic model dy/dt = f (pressure algebraic) along y* + Re(s e^{iwt}):
//     (a_z + i w I) s_z = U D_{z-1} s_{z-1} + (df/dP) pi_z + df/dp,          pi_{z+1} = az_z pi_z + P_z (d az/dy . s_z)
// - the tangent march of 73_sensitivity.inc with the shift i w I and complex s, pi; everything else is what rmt_sens_eval
// forms (real).  One (member, frequency) pair per lane; w = 0 is the sensitivity.  The shifted node matrix is not
// inverted: the lane eliminates [a + i w I | the NP right-hand sides] in the order of rmt_invert_n (Gauss-Jordan, no
// pivoting), in real / imaginary pairs.  w is in the time unit of the right-hand side (the unit of `period`).
#if RMT_FREQ != 1
#error "RMT_FREQ: 1 (the frequency sweep behind the steady-state march) or undefined"
#endif
#if !RMT_SENS
#error "RMT_FREQ: needs RMT_SENS (the frequency unit is the march unit plus RMT_SENS plus RMT_FREQ and RMT_FREQ_NP)"
#endif
#ifndef RMT_FREQ_NP
#error "RMT_FREQ: RMT_FREQ_NP (the number of inputs, 1..4) must be defined"
#endif
#if RMT_FREQ_NP < 1 || RMT_FREQ_NP > 4
#error "RMT_FREQ_NP: 1..4"
#endif

// All inputs at one node: s = (a + i w I)^-1 (U sd + fP pi + df/dp) with sn as rmt_sens_eval left it (sn.ainv holds a, NOT
// inverted); then sd <- D s and pi <- az pi + P (d az/dy . s) for the node behind.  (sr, si): the node's rows.  False when
// a pivot is zero or anything is not finite.
__device__ __forceinline__ bool rmt_freq_node(const RmtMember& m, const RmtSensNode& sn, const real* __restrict__ ys,
                                              const preal Pz, const real w, const RmtSensDesc& desc,
                                              real (&sdr)[RMT_FREQ_NP][RMT_V], real (&sdi)[RMT_FREQ_NP][RMT_V],
                                              preal (&pir)[RMT_FREQ_NP], preal (&pii)[RMT_FREQ_NP],
                                              real (&sr)[RMT_FREQ_NP][RMT_V], real (&si)[RMT_FREQ_NP][RMT_V]) {
    real ar[RMT_V][RMT_V], ai[RMT_V][RMT_V];
#pragma unroll
    for (int r = 0; r < RMT_V; ++r)
#pragma unroll
        for (int c = 0; c < RMT_V; ++c) {
            ar[r][c] = sn.ainv[r][c];
            ai[r][c] = (r == c) ? w : real(0);
        }
    const real conv = m.f1 * m.inv_dz;
#pragma unroll
    for (int p = 0; p < RMT_FREQ_NP; ++p) {
        const real pr = real(pir[p]), pim = real(pii[p]);
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) {
            sr[p][i] = conv * sdr[p][i] + sn.fP[i] * pr;
            si[p][i] = conv * sdi[p][i] + sn.fP[i] * pim;
        }
#if !RMT_ISO
        sr[p][RMT_S] = (m.ft * m.inv_dz) * sdr[p][RMT_S] + sn.fP[RMT_S] * pr + (desc.kind[p] == RMT_SENS_TM ? sn.ftm : real(0));
        si[p][RMT_S] = (m.ft * m.inv_dz) * sdi[p][RMT_S] + sn.fP[RMT_S] * pim;
#endif
    }
    real pmin = real(__builtin_inf());
#pragma unroll
    for (int p = 0; p < RMT_V; ++p) {
        const real qr = ar[p][p], qi = ai[p][p];
        pmin = rmt_min(pmin, rmt_abs(qr) + rmt_abs(qi));
        const real iq = rmt_rcp(qr * qr + qi * qi);
        const real ipr = qr * iq, ipi = -(qi * iq);                  // 1 / pivot
#pragma unroll
        for (int c = p + 1; c < RMT_V; ++c) {
            const real xr = ar[p][c], xi = ai[p][c];
            ar[p][c] = xr * ipr - xi * ipi;
            ai[p][c] = xr * ipi + xi * ipr;
        }
#pragma unroll
        for (int k = 0; k < RMT_FREQ_NP; ++k) {
            const real xr = sr[k][p], xi = si[k][p];
            sr[k][p] = xr * ipr - xi * ipi;
            si[k][p] = xr * ipi + xi * ipr;
        }
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) {
            if (r != p) {
                const real fr = ar[r][p], fi = ai[r][p];
#pragma unroll
                for (int c = p + 1; c < RMT_V; ++c) {
                    ar[r][c] -= fr * ar[p][c] - fi * ai[p][c];
                    ai[r][c] -= fr * ai[p][c] + fi * ar[p][c];
                }
#pragma unroll
                for (int k = 0; k < RMT_FREQ_NP; ++k) {
                    sr[k][r] -= fr * sr[k][p] - fi * si[k][p];
                    si[k][r] -= fr * si[k][p] + fi * sr[k][p];
                }
            }
        }
    }
    bool ok = pmin > real(0) && __builtin_isfinite((double)pmin);
#pragma unroll
    for (int k = 0; k < RMT_FREQ_NP; ++k) {
        preal dr = preal(0), di = preal(0);
#pragma unroll
        for (int r = 0; r < RMT_V; ++r) {
            ok = ok && __builtin_isfinite((double)sr[k][r]) && __builtin_isfinite((double)si[k][r]);
            dr += preal(sn.daz[r]) * preal(sr[k][r]);
            di += preal(sn.daz[r]) * preal(si[k][r]);
        }
#pragma unroll
        for (int i = 0; i < RMT_S; ++i) {
            const bool on = ys[i] > RMT_EPS;
            sdr[k][i] = on ? sr[k][i] : real(0);
            sdi[k][i] = on ? si[k][i] : real(0);
        }
#if !RMT_ISO
        sdr[k][RMT_S] = sr[k][RMT_S];
        sdi[k][RMT_S] = si[k][RMT_S];
#endif
        pir[k] = sn.az * pir[k] + Pz * dr;
        pii[k] = sn.az * pii[k] + Pz * di;
        ok = ok && __builtin_isfinite((double)pir[k]) && __builtin_isfinite((double)pii[k]);
    }
    return ok;
}

#ifndef RMT_HOST_EMULATION
// kernel: lane g = e F + f (frequency fastest: the lanes of a member read the same y and member row); the lane walks
// z = 0..N-1 over the converged state y[e][v][z] as rmt_n2_steady_sens does and carries D s [NP][V] and pi [NP] (complex)
// and the real P recurrence in registers.  np must be RMT_FREQ_NP.  All outputs are (re, im) pairs of doubles in the
// scaled units of the state per unit of the member-row value; row V is pi_z:
//   out  [E][F][NP][2][V+1][2]   the rows of the outlet node (slot 0) and of node peak[e] (slot 1; a node outside
//                                0..N-1 leaves the slot as it is)
//   tab  [E][F][NP][V+1][N][2]   every node, only with profile != 0 (else not touched, may be null)
//   failed [E][F]                the node at which the lane stopped, -1: none
// A lane with a singular node (or a non-finite result) sets RMT_FLAG_NONFINITE on its member, writes NaN into its columns
// of `tab` at that node and into both slots of `out`, and stops there.
extern "C" __global__ __launch_bounds__(64) void rmt_n2_steady_freq(
        const real* __restrict__ y /* [E][V][N] */, const double* __restrict__ members, const int N, const int E, const int F,
        const int np, const RmtSensDesc desc, const double* __restrict__ omegas /* [F] */, const int* __restrict__ peak /* [E] */,
        const int profile, double* __restrict__ out, double* __restrict__ tab, double* __restrict__ failed,
        unsigned* __restrict__ flags) {
    rmt_math_init();
    const long long g = (long long)blockIdx.x * 64 + (long long)threadIdx.x;
    const bool live = F > 0 && g < (long long)E * (long long)F;
    const int e = live ? (int)(g / F) : 0, f = live ? (int)(g % F) : 0;       // dead lanes read member 0 and write nothing
    if (np != RMT_FREQ_NP) {          // the caller sized the buffers for another unit: write nothing but the flag
        if (live) atomicOr(&flags[e], RMT_FLAG_NONFINITE);
        return;
    }
    RmtMember m;
    rmt_load_member(members + (size_t)e * RMT_NM, m);
    RMT_PROFILE_BIND(m, e, N)
    const real w = live ? real(omegas[f]) : real(0);
    const int zp = peak[e];
    real sdr[RMT_FREQ_NP][RMT_V], sdi[RMT_FREQ_NP][RMT_V];
    preal pir[RMT_FREQ_NP], pii[RMT_FREQ_NP];
#pragma unroll
    for (int p = 0; p < RMT_FREQ_NP; ++p) {
        rmt_sens_seed(m, desc.kind[p], desc.index[p], sdr[p], pir[p]);
        pii[p] = preal(0);
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) sdi[p][i] = real(0);
    }
    preal P = m.p0;
    rmt_flags_t flag;
    rmt_flags_clear(flag);
    const real* ye = y + (size_t)e * RMT_V * N;
    const size_t lane = (size_t)e * (size_t)F + (size_t)f;
    double* oe = out + lane * RMT_FREQ_NP * 2 * (RMT_V + 1) * 2;
    double* te = profile ? tab + lane * RMT_FREQ_NP * (RMT_V + 1) * (size_t)N * 2 : nullptr;
    int z = 0, stopped = -1;
    bool active = live && N > 0;
    while (__any(active)) {
        if (active) {
            real yz[RMT_V];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) yz[i] = ye[(size_t)i * N + z];
#if RMT_PROFILE
            m.act = real(m.prof[z]);                      // (active: z < N)
            m.dtm = real(m.prof[N + z]);
#endif
            RmtSensNode sn;
            rmt_sens_eval(m, yz, P, sn, flag);
            preal pzr[RMT_FREQ_NP], pzi[RMT_FREQ_NP];
#pragma unroll
            for (int p = 0; p < RMT_FREQ_NP; ++p) {
                pzr[p] = pir[p];
                pzi[p] = pii[p];
            }
            real sr[RMT_FREQ_NP][RMT_V], si[RMT_FREQ_NP][RMT_V];
            const bool ok = rmt_freq_node(m, sn, yz, P, w, desc, sdr, sdi, pir, pii, sr, si);
            const double nan = __builtin_nan("");
            const bool last = z == N - 1, at_peak = z == zp;
#pragma unroll
            for (int p = 0; p < RMT_FREQ_NP; ++p) {
#pragma unroll
                for (int i = 0; i <= RMT_V; ++i) {
                    const double vr = !ok ? nan : (i < RMT_V ? (double)sr[p][i < RMT_V ? i : 0] : (double)pzr[p]);
                    const double vi = !ok ? nan : (i < RMT_V ? (double)si[p][i < RMT_V ? i : 0] : (double)pzi[p]);
                    if (profile) {
                        double* t = te + (((size_t)p * (RMT_V + 1) + i) * (size_t)N + z) * 2;
                        t[0] = vr;
                        t[1] = vi;
                    }
                    if (last || !ok) {
                        double* o = oe + (((size_t)p * 2 + 0) * (RMT_V + 1) + i) * 2;
                        o[0] = vr;
                        o[1] = vi;
                    }
                    if (at_peak || !ok) {
                        double* o = oe + (((size_t)p * 2 + 1) * (RMT_V + 1) + i) * 2;
                        o[0] = vr;
                        o[1] = vi;
                    }
                }
            }
            if (!ok) {
                stopped = z;
                active = false;
            } else {
                P = rmt_pressure_next(m, sn.az, P);
                if (++z >= N) active = false;
            }
        }
    }
    if (live) {
        failed[lane] = (double)stopped;
        if (stopped >= 0) atomicOr(&flags[e], RMT_FLAG_NONFINITE);
    }
}
#endif  // RMT_HOST_EMULATION
#endif  // RMT_FREQ
//<<< RMT_FREQ
//<<< RMT_SENS
