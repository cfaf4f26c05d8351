// ===================================================================== kernel: one RHS evaluation
// dydt[e] = f(y[e]) for every reactor e = blockIdx.x; any N (blocks of RMT_BLOCK nodes, carry
// handed from block to block).  Replaces one call of modelEquationN2 (pbHomoReactor.py:3706).
#ifndef RMT_RHS_WAVES
#define RMT_RHS_WAVES 1          // min waves per SIMD asked from the register allocator (streaming kernel)
#endif
extern "C" __global__ __launch_bounds__(RMT_BLOCK, RMT_RHS_WAVES) void rmt_n2_rhs(
        const real* __restrict__ y, real* __restrict__ dydt, const double* __restrict__ members,
        const int N, const int E, unsigned* __restrict__ flags) {
    __shared__ RmtShared sh;
    rmt_math_init();
    // Workgroups are PERSISTENT over the reactors (the host launches at most a few per CU): building the 16 KiB exp
    // table and starting a workgroup costs as much as evaluating a few node blocks, and a 1024-node reactor is only four
    // of them - with one workgroup per reactor the streaming case (16384 x 1024 nodes) ran at half the per-RHS rate of
    // the on-chip RK4 kernel.
    int ph = 0;
    for (int e = blockIdx.x; e < E; e += gridDim.x) {
#if RMT_MEMBER_LDS
        __shared__ RmtMember m;      // read back with broadcast ds_reads: frees ~2*(15+S) SGPRs
        __syncthreads();
        if (threadIdx.x == 0) rmt_load_member(members + (size_t)e * RMT_NM, m);
        __syncthreads();
#else
        RmtMember m;
        rmt_load_member(members + (size_t)e * RMT_NM, m);
        RMT_PROFILE_BIND(m, e, N)
#endif
        RmtCarry carry;
        rmt_carry_inlet(m, carry);
        const real* ye = y + (size_t)e * RMT_V * N;
        real* de = dydt + (size_t)e * RMT_V * N;
        rmt_flags_t flag;
        rmt_flags_clear(flag);
        unsigned lflag = 0u;
        for (int base = 0; base < N; base += RMT_BLOCK, ph ^= 1) {
            const int node = base + (int)threadIdx.x;
            const bool valid = node < N;
            real ys[1][RMT_V], k[1][RMT_V];
            rmt_safe_state(m, ys[0]);
            if (valid) {
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) ys[0][i] = ye[(size_t)i * N + node];
            }
            RMT_PROFILE_AT(carry, base)
            rmt_rhs_block<1, true>(m, sh, ph, ys, valid ? 1 : 0, carry, k, flag);
            if (valid) {
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) de[(size_t)i * N + node] = k[0][i];
                lflag |= rmt_finite_flag(k[0]);
            }
        }
        lflag |= rmt_flags_bits(flag);
        if (lflag) atomicOr(&flags[e], lflag);
    }
}

// ===================================================================== kernel: RK4, state on chip
// nsteps classic RK4 steps of size h (tableau and update order of odeSolver.py:17-40) for reactor
// e = blockIdx.x with N <= RMT_BLOCK*RMT_NPT nodes.  The state is read from HBM once, kept on
// chip for all steps and written once: HBM traffic is 2*V*sizeof(real) per node per LAUNCH.
// RMT_LDS_STATE selects where the two long-lived RK4 vectors live (only the stage input and the
// current K are always in VGPRs):  2 = y_n and the K accumulator in LDS,  1 = y_n in LDS,
// 0 = both in VGPRs.  Each thread only touches its own nodes' LDS slots, so no barrier is needed.
#ifndef RMT_LDS_STATE
#define RMT_LDS_STATE 0
#endif
#define RMT_NODES_WG (RMT_BLOCK * RMT_NPT)

// RMT_KCACHE 1 (host: n2.device_source, when the cache fits in LDS beside everything else): the temperature-only rate
// constants of the mechanism (lowering.Lowered.kcache_plan) are evaluated in full at stage 1 of every step - the step's
// own state y_n is the reference point, stored per node in LDS - and taken from there by a short Taylor step at stages
// 2-4, whose temperatures differ from T(y_n) by h dT/dt.  There is no second code path in the step loop (the kernel sits at
// the 256 VGPRs two waves per SIMD allow; a fallback branch costs 25-60 spilled registers, profiles/round3_kcache.md):
// a lane whose stage temperature leaves the range the Taylor step serves (|d| <= 2^-9 in every exponent) only sets a
// sticky bit; a workgroup that saw one stores NOTHING - the state in memory is still the launch's input - and flags its
// reactor with RMT_FLAG_REDO, which the kernel rmt_n2_rk4_reg_redo (launched right behind, the same arguments)
// picks up: it integrates those reactors with the plain evaluation and clears the bit.  CACHED = false is that plain
// stepper, and the only one when RMT_KCACHE is 0.
#ifndef RMT_KCACHE
#define RMT_KCACHE 0
#endif
#if RMT_KCACHE && RMT_KC_SLOTS > 0 && (RMT_MODEL == 0 || RMT_MODEL == 2)
#define RMT_RK4_KC 1
#else
#define RMT_RK4_KC 0
#endif
// RMT_CALL_FLAGS 1: the exception tests of a tested stage of the CACHED stepper as per-call extremes (rmt_callflags_t):
// 168 -> 56 SGPR-spill lane moves per step, 1.76e10 -> 1.81e10 node-steps/s on the bench shape.  (The plain 512 x 2 stepper
// has no registers for them: it keeps the compare masks.)
#ifndef RMT_CALL_FLAGS
#define RMT_CALL_FLAGS (RMT_FLAGS_MODE == 0)
#endif
template <typename T> struct rmt_unref { typedef T type; };
template <typename T> struct rmt_unref<T&> { typedef T type; };
// RMT_KC_REFRESH: most steps between two moves of the cache's reference point.  1 = stage 1 of every step evaluates in
// full; K > 1 = only every K-th step at most does, in between stage 1 takes the cached path as well (its exception tests
// still run on everything that is not a function of the temperature alone).  The kernel shortens the period so that no
// reference point gets older than RMT_KC_MAX_AGE of model time (6 steps at dt = 2 us): the range the Taylor steps serve
// has to hold the temperature's drift over that age, +-0.065 K at 520 K for the DME constants, i.e. |dT/dt| up to
// ~5000 K/s - the start-up of the bench sweep peaks at 440 K/s (launch averages) for its coldest block of members and at
// 2900 K/s for its hottest one (tools/kcache_transient.py, no fallback) - beyond that a reactor is integrated again by the
// plain stepper.  Measured on the bench shape, period 1 / 4 / 8 / 16: 1.804 / 1.867 / 1.879 / 1.884e10.
#ifndef RMT_KC_REFRESH
#define RMT_KC_REFRESH 1
#endif
#ifndef RMT_KC_MAX_AGE
#define RMT_KC_MAX_AGE 1.3e-5      // [s] oldest reference point: 6 steps of 2 us (n2.KC_MAX_AGE)
#endif
#ifndef RMT_KC_NODE_MAJOR
#define RMT_KC_NODE_MAJOR 0
#endif
#define RMT_KC_ROW ((RMT_KC_SLOTS + 1) & ~1)        // doubles per node of a node-major cache (128-bit aligned rows)
#define RMT_FLAG_REDO 0x80000000u     // internal: never visible to the host (set and cleared within one rmt_n2_rk4 call)

template <bool CACHED>
__device__ __forceinline__ void rmt_rk4_reg_body(
        real* __restrict__ y, const double* __restrict__ members, const int N, const double h_,
        const long long nsteps, unsigned* __restrict__ flags) {
    __shared__ RmtShared sh;
    if constexpr (CACHED) rmt_math_init6();            // (the 64-entry exp table under RMT_KC_SMALL_EXP, else the usual one)
    else rmt_math_init();
#if RMT_LDS_STATE >= 1
    __shared__ real s_y0[RMT_V][RMT_NODES_WG];
#endif
#if RMT_LDS_STATE >= 2
    __shared__ real s_acc[RMT_V][RMT_NODES_WG];
#endif
    const int e = blockIdx.x;
    if (threadIdx.x < RMT_V)      // upstream of node 0 (read by lane 0 of wave 0 after the stage barrier)
        sh.inlet[threadIdx.x] = real(members[(size_t)e * RMT_NM +
                                             (threadIdx.x < RMT_S ? M_CIN + (int)threadIdx.x : M_THETA_IN)]);
    // RMT_UP_LDS 1: neighbour states through LDS (two exchange buffers of V (BLOCK+1) reals) instead of DPP moves.
    // Measured slower on MI355X (1.53 vs 1.57e10 node-steps/s: the LDS address arithmetic and the extra
    // SGPR pressure cost more VALU instructions than the 14 DPP moves per stage they replace) - off.
#ifndef RMT_UP_LDS
#define RMT_UP_LDS 0
#endif
#if RMT_UP_LDS
    __shared__ real s_upl[2][RMT_V][RMT_BLOCK + 1];
    if (threadIdx.x < RMT_V) {    // slot 0 of both buffers: the inlet values (the upstream of node 0 never changes)
        const real v = real(members[(size_t)e * RMT_NM + (threadIdx.x < RMT_S ? M_CIN + (int)threadIdx.x : M_THETA_IN)]);
        s_upl[0][threadIdx.x][0] = v;
        s_upl[1][threadIdx.x][0] = v;
    }
#define RMT_UPL , nullptr, nullptr, nullptr, 0, nullptr, s_upl
#else
#define RMT_UPL
#endif
#if RMT_MEMBER_LDS
    __shared__ RmtMember m;      // read back with broadcast ds_reads: frees ~2*(15+S) SGPRs
    if (threadIdx.x == 0) rmt_load_member(members + (size_t)e * RMT_NM, m);
    __syncthreads();
#else
    RmtMember m;
    rmt_load_member(members + (size_t)e * RMT_NM, m);
    RMT_PROFILE_BIND(m, e, N)                 // (the reactor is one block: carry.node0 stays 0)
#endif
    RmtCarry carry;
    rmt_carry_inlet(m, carry);
    real* ye = y + (size_t)e * RMT_V * N;
    const int node0 = (int)threadIdx.x * RMT_NPT;
    int nvalid = N - node0;
    nvalid = nvalid < 0 ? 0 : (nvalid > RMT_NPT ? RMT_NPT : nvalid);
    real ys[RMT_NPT][RMT_V], k[RMT_NPT][RMT_V];
#if RMT_RK4_KC
#if RMT_KC_NODE_MAJOR       // a node's slots side by side: ONE address register per node, every slot an immediate offset.
    // RMT_KC_PAD 1: 16 bytes of padding after every 8 nodes, so that the 16 lanes of a 128-bit LDS access hit 16 different
    // bank groups (rows of 12 doubles = 96 B repeat theirs every 8 lanes) - measured 0.5 % SLOWER than the plain rows
    // (1.940e10 against 1.950e10: three more spills outweigh the conflicts), off
#ifndef RMT_KC_PAD
#define RMT_KC_PAD 0
#endif
    __shared__ __attribute__((aligned(16))) real s_kc[CACHED ? RMT_NODES_WG * RMT_KC_ROW + RMT_NODES_WG / 4 : 2];
#else
    __shared__ real s_kc[CACHED ? RMT_KC_SLOTS : 1][CACHED ? RMT_NODES_WG : 1];
#endif
    RmtKC kcs[RMT_NPT];
#pragma unroll
    for (int j = 0; j < RMT_NPT; ++j) {
#if RMT_KC_NODE_MAJOR
        {
            const int node_ = j * RMT_BLOCK + (int)threadIdx.x;
            kcs[j].base = &s_kc[CACHED ? node_ * RMT_KC_ROW + (RMT_KC_PAD ? (node_ >> 3) * 2 : 0) : 0];
            kcs[j].stride = 1;
        }
#else
        kcs[j].base = &s_kc[0][CACHED ? j * RMT_BLOCK + (int)threadIdx.x : 0];
        kcs[j].stride = RMT_NODES_WG;
#endif
        kcs[j].valid = true;             // sticky: false once a stage temperature left the cache's range
    }
#endif
#if RMT_LDS_STATE < 1
    real y0[RMT_NPT][RMT_V];
#define Y0(j, i) y0[j][i]
#else
#define Y0(j, i) s_y0[i][node0 + (j)]
#endif
#if RMT_LDS_STATE < 2
    real acc[RMT_NPT][RMT_V];
#define ACC(j, i) acc[j][i]
#else
#define ACC(j, i) s_acc[i][node0 + (j)]
#endif
#pragma unroll
    for (int j = 0; j < RMT_NPT; ++j) {
        rmt_safe_state(m, ys[j]);
        if (j < nvalid) {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) ys[j][i] = ye[(size_t)i * N + node0 + j];
        }
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) Y0(j, i) = ys[j][i];
    }
    const real h = real(h_), hh = real(0.5 * h_), h6 = real(h_ / 6.0);
    rmt_flags_t flag;
    rmt_flags_clear(flag);
#if RMT_MODEL == 2
#ifndef RMT_M2_WARM
#define RMT_M2_WARM 1            // 1: warm-started pressure sweeps after the first RHS of the launch
#endif
    preal pwarm[RMT_NPT];
    int warm = 0;
#pragma unroll
    for (int j = 0; j < RMT_NPT; ++j) pwarm[j] = preal(0);
#endif
    rmt_noflags_t nof;
    unsigned lflag = 0u;
#if RMT_KC_REFRESH > 1
    // steps between two moves of the reference point: at most RMT_KC_REFRESH, and no reference point older than
    // RMT_KC_MAX_AGE of model time - what the Taylor range has to hold is the temperature's drift over that age, whatever
    // the step size (|dT/dt| up to ~4000 K/s at the default)
    int kc_period = (h_ > 0.0) ? (int)fmin((double)RMT_KC_REFRESH, fmax(1.0, RMT_KC_MAX_AGE / h_)) : 1;
    int kc_age = 0;
    (void)kc_period; (void)kc_age;
#endif
    for (long long step = 0; step < nsteps; ++step) {
        // One copy of the RHS code serves the four stages (a fully unrolled step is ~64 KB of
        // instructions - the size of the instruction cache); s is wave-uniform.
#if RMT_STAGE_UNROLL
#pragma unroll
#else
#pragma unroll 1
#endif
        for (int s = 0; s < 4; ++s) {
#if RMT_FORCING
            // the forced boundary values at this stage's time t, t + h/2, t + h/2, t + h (the launch starts at t_ref)
            rmt_forcing_stage(m, carry, members + (size_t)e * RMT_NM,
                              members[(size_t)e * RMT_NM + M_FORCE] + ((double)step + rmt_rk4_c(s)) * h_, sh.inlet);
#endif
            // Python-exception tests only on K1 = f(y_n); a failure inside the trial stages still
            // ends in a non-finite state (RMT_FLAG_NONFINITE)
#if RMT_MODEL == 2
            auto stage2 = [&](auto& fl, auto ks_tag) {      // model M2: the same choice of versions, its own RHS block
                typedef typename rmt_unref<decltype(fl)>::type FLT;
#if RMT_RK4_KC
                if constexpr (CACHED)
                    rmt_rhs_block<RMT_NPT, false, 0, FLT, RmtKC, decltype(ks_tag)::value>(
                        m, sh, s & 1, ys, nvalid, carry, k, fl, nullptr, nullptr, pwarm, warm, nullptr, nullptr, kcs);
                else
#endif
                rmt_rhs_block<RMT_NPT, false, 0, FLT>(m, sh, s & 1, ys, nvalid, carry, k, fl, nullptr, nullptr, pwarm, warm);
            };
            if (s == 0) {
#if RMT_KC_REFRESH > 1
                if (kc_age == 0) stage2(flag, rmt_int_t<0>{});
                else stage2(flag, rmt_int_t<2>{});
                kc_age = (kc_age + 1 >= kc_period) ? 0 : kc_age + 1;
#else
                stage2(flag, rmt_int_t<0>{});
#endif
            } else if (RMT_CHECK_ALL_STAGES) stage2(flag, rmt_int_t<2>{});
            else stage2(nof, rmt_int_t<2>{});
            warm = RMT_M2_WARM;
#else
            // (the stage loop is unrolled: one version of the node functions per stage, no run-time choice.  KS: how a
            // cached stepper treats the rate constants - 0 in full, moving the reference point; 2 from the cache)
            auto stage = [&](auto& fl, auto ks_tag) {
                typedef typename rmt_unref<decltype(fl)>::type FLT;
#if RMT_RK4_KC
                if constexpr (CACHED)
                    rmt_rhs_block<RMT_NPT, false, 0, FLT, RmtKC, decltype(ks_tag)::value>(
                        m, sh, s & 1, ys, nvalid, carry, k, fl, nullptr, nullptr, nullptr, 0, nullptr, nullptr, kcs);
                else
#endif
                rmt_rhs_block<RMT_NPT, false, 0, FLT>(m, sh, s & 1, ys, nvalid, carry, k, fl RMT_UPL);
            };
            auto tested_stage = [&](auto ks_tag) {
#if RMT_CALL_FLAGS
                if constexpr (CACHED) {           // the tests of this evaluation as running extremes, see rmt_callflags_t
                    rmt_callflags_t cf;
                    rmt_callflags_clear(cf);
                    stage(cf, ks_tag);
                    rmt_flags_fold(flag, cf);
                } else
#endif
                stage(flag, ks_tag);
            };
            if (s == 0) {
#if RMT_TIMING_KC_NEVER               // instruction counting only (bench.py): stage 1 from the cache in EVERY step
                tested_stage(rmt_int_t<2>{});
#elif RMT_KC_REFRESH > 1
                // the reference point moves every kc_period steps only; in between stage 1 takes the cached path too
                if (kc_age == 0) tested_stage(rmt_int_t<0>{});
                else tested_stage(rmt_int_t<2>{});
                kc_age = (kc_age + 1 >= kc_period) ? 0 : kc_age + 1;
#else
                tested_stage(rmt_int_t<0>{});
#endif
            } else if (RMT_CHECK_ALL_STAGES) tested_stage(rmt_int_t<2>{});
            else stage(nof, rmt_int_t<2>{});
#endif
            if (s < 3) {
                const real cn = (s == 2) ? h : hh;                // stage inputs y+K1 h/2, y+K2 h/2, y+K3 h
                const real wk = (s == 0) ? real(1) : real(2);     // weights 1,2,2,(1)
#pragma unroll
                for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) {
                        ACC(j, i) = (s == 0) ? k[j][i] : ACC(j, i) + wk * k[j][i];
                        ys[j][i] = Y0(j, i) + k[j][i] * cn;
                    }
            } else {
#pragma unroll
                for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) {             // y + h(K1+2K2+2K3+K4)/6
                        const real yn = Y0(j, i) + h6 * (ACC(j, i) + k[j][i]);
                        Y0(j, i) = yn;
                        ys[j][i] = yn;
                    }
            }
        }
    }
#if RMT_RK4_KC
    if constexpr (CACHED) {
        bool left = false;
#pragma unroll
        for (int j = 0; j < RMT_NPT; ++j) left = left || !kcs[j].valid;
        if (__syncthreads_or(left ? 1 : 0)) {         // void: nothing stored, the reactor is integrated again in full
            if (threadIdx.x == 0) atomicOr(&flags[e], RMT_FLAG_REDO);
            return;
        }
    }
#endif
#pragma unroll
    for (int j = 0; j < RMT_NPT; ++j) {
        if (j < nvalid) {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) ye[(size_t)i * N + node0 + j] = ys[j][i];
            lflag |= rmt_finite_flag(ys[j]);
        }
    }
    lflag |= rmt_flags_bits(flag);
    if (lflag) atomicOr(&flags[e], lflag);
#undef Y0
#undef ACC
#undef RMT_UPL
}

extern "C" __global__ __launch_bounds__(RMT_BLOCK) void rmt_n2_rk4_reg(
        real* __restrict__ y, const double* __restrict__ members, const int N, const double h_,
        const long long nsteps, unsigned* __restrict__ flags) {
    rmt_rk4_reg_body<RMT_RK4_KC != 0>(y, members, N, h_, nsteps, flags);
}
#if RMT_RK4_KC
extern "C" __global__ __launch_bounds__(RMT_BLOCK) void rmt_n2_rk4_reg_redo(
        real* __restrict__ y, const double* __restrict__ members, const int N, const double h_,
        const long long nsteps, unsigned* __restrict__ flags) {
    const bool redo = (__hip_atomic_load(&flags[blockIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & RMT_FLAG_REDO) != 0u;
    // flags[E + 1] != 0: the host runs this kernel ALONE for a while (a cached launch lost half of its reactors)
    const bool all = __hip_atomic_load(&flags[gridDim.x + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
    if (!redo && !all) return;                         // (workgroup-uniform)
    __syncthreads();                                   // every thread has read the bit before it is cleared
    if (redo && threadIdx.x == 0) {
        atomicAnd(&flags[blockIdx.x], ~RMT_FLAG_REDO);
        atomicAdd(&flags[gridDim.x], 1u);              // the word behind the E status words: rmt_n2_fallbacks
    }
    rmt_rk4_reg_body<false>(y, members, N, h_, nsteps, flags);
}
#endif

// ===================================================================== kernel: RK4 on chip, chained workgroups
// Same on-chip stepper for N > RMT_BLOCK*RMT_NPT (or to spread one reactor over several CUs):
// reactor e is cut into C chunks of RMT_NODES_WG nodes; the grid is T teams of C workgroups
// (T*C <= number of CUs, so every workgroup is resident), team t integrates reactors
// t, t+T, t+2T, ...  The hand-over between consecutive chunks is described at RmtChainCtx.
#ifndef RMT_LDS_STATE_CHAIN
#define RMT_LDS_STATE_CHAIN RMT_LDS_STATE
#endif
// Hand-over protocol of the chained RK4 stepper: the tagged-word links of the stiff stepper (no publisher drain: the
// s_waitcnt of the flag protocol held the last wave of every chunk ~1 us per RK stage, a quarter of the stage), with a
// consumed counter as back-pressure since no per-step rendezvous bounds the producer's lead.  Model M2 (whose chunks need
// the upstream pressure BEFORE their Newton sweeps: received ahead of them, sent right after) used the flag protocol
// until the end of round 2: 1.25e10 -> 1.37e10 node-steps/s for 64 x 4096 nodes, 3.7e8 -> 4.8e8 for one 4096-node
// reactor.  RMT_CHAIN_TAGGED 0 selects the flag protocol.
#ifndef RMT_CHAIN_TAGGED
#define RMT_CHAIN_TAGGED 1
#endif
#ifndef RMT_CHAIN_UNROLL
#define RMT_CHAIN_UNROLL 1     // stages unrolled, Python-exception checks on stage 1 only (12.0 vs 10.5 G node-steps/s)
#endif
// RMT_KCACHE_CHAIN 1 (host: n2.kcache_choice): the chunks cache the temperature-only rate constants exactly like
// rmt_rk4_reg_body<true> - stage 1 in full, stages 2-4 from the cache, no second code path.  What differs is the way out
// when a stage temperature leaves the cache's range, because a chunk cannot know what the other chunks of its reactor
// saw: every chunk saves the launch's input of its nodes to `backup` before the first step and stores its result as
// usual; a chunk that left the range sets redo[e]; status bits go to falt[e] instead of flags[e].  The kernel
// rmt_n2_rk4_chain_redo, launched right behind on the same grid, walks the same reactors: redo[e] clear -> falt[e] is
// merged into flags[e]; set -> the plain chained stepper integrates the reactor again FROM `backup`.  (redo / falt are
// cleared by the host before every launch; without the cache both pointers are null and unused.)
#ifndef RMT_KCACHE_CHAIN
#define RMT_KCACHE_CHAIN 0
#endif
#ifndef RMT_KC_REFRESH_CHAIN
#define RMT_KC_REFRESH_CHAIN 1
#endif
#if RMT_KCACHE_CHAIN && RMT_KC_SLOTS > 0 && RMT_MODEL == 0 && RMT_CHAIN_TAGGED && RMT_CHAIN_UNROLL
#define RMT_RK4C_KC 1
#else
#define RMT_RK4C_KC 0
#endif

#if !RMT_PROFILE      // (a profiled run keeps a reactor on one workgroup: the chained form does not carry the profile)
template <bool CACHED, bool REDO>
__device__ __forceinline__ void rmt_rk4_chain_body(
        real* __restrict__ y, const double* __restrict__ members, const int N, const int E,
        const int C, const int T, const double h_, const long long nsteps,
        unsigned long long* __restrict__ sync, double* __restrict__ slots,
        unsigned* __restrict__ flags, unsigned long long* __restrict__ rings,
        unsigned* __restrict__ abort_words, real* __restrict__ backup, unsigned* __restrict__ redo,
        unsigned* __restrict__ falt) {
#if RMT_CHAIN_TAGGED
#define RMT_CH 2
#else
#define RMT_CH 1
#endif
    __shared__ RmtShared sh;
    if constexpr (CACHED) rmt_math_init6();
    else rmt_math_init();
#if RMT_LDS_STATE_CHAIN >= 1
    __shared__ real s_y0[RMT_V][RMT_NODES_WG];
#endif
#if RMT_LDS_STATE_CHAIN >= 2
    __shared__ real s_acc[RMT_V][RMT_NODES_WG];
#endif
#if RMT_RK4C_KC
#if RMT_KC_NODE_MAJOR
    __shared__ __attribute__((aligned(16))) real s_kcc[CACHED ? RMT_NODES_WG * RMT_KC_ROW : 2];
#else
    __shared__ real s_kcc[CACHED ? RMT_KC_SLOTS : 1][CACHED ? RMT_NODES_WG : 1];
#endif
    RmtKC kcs[RMT_NPT];
#pragma unroll
    for (int j = 0; j < RMT_NPT; ++j) {
#if RMT_KC_NODE_MAJOR
        kcs[j].base = &s_kcc[CACHED ? (j * RMT_BLOCK + (int)threadIdx.x) * RMT_KC_ROW : 0];
        kcs[j].stride = 1;
#else
        kcs[j].base = &s_kcc[0][CACHED ? j * RMT_BLOCK + (int)threadIdx.x : 0];
        kcs[j].stride = RMT_NODES_WG;
#endif
        kcs[j].valid = true;
    }
#endif
    const int team = blockIdx.x / C, c = blockIdx.x % C;
    RmtChainCtx ctx;
    ctx.has_in = c > 0;
    ctx.has_out = c < C - 1;
    const size_t link = (size_t)team * C + c;
    ctx.sync_in = sync + (link - (c > 0 ? 1 : 0)) * RMT_SYNC_STRIDE;
    ctx.sync_out = sync + link * RMT_SYNC_STRIDE;
    ctx.slots_in = slots + (link - (c > 0 ? 1 : 0)) * RMT_CHAIN_DEPTH * (RMT_V + 1);
    ctx.slots_out = slots + link * RMT_CHAIN_DEPTH * (RMT_V + 1);
    ctx.q = 0ull;
    ctx.abort = 0;
    ctx.chunk = c;
    ctx.ring_in = rings + (link - (c > 0 ? 1 : 0)) * RMT_RING * RMT_LINK_WORDS;
    ctx.ring_out = rings + link * RMT_RING * RMT_LINK_WORDS;
    ctx.seq_in = ctx.seq_out = 1u;                       // the host clears the rings: tag 0 never matches
    ctx.abort_word = abort_words + team;
    ctx.dead = 0;
    ctx.bp = true;
    ctx.bp_in = ctx.sync_in + 16;
    ctx.bp_out = ctx.sync_out + 16;
    ctx.known = 0u;
    const int node0 = c * RMT_NODES_WG + (int)threadIdx.x * RMT_NPT;
    int nvalid = N - node0;
    nvalid = nvalid < 0 ? 0 : (nvalid > RMT_NPT ? RMT_NPT : nvalid);
    const int lnode0 = (int)threadIdx.x * RMT_NPT;
    const real h = real(h_), hh = real(0.5 * h_), h6 = real(h_ / 6.0);
    bool dead = false;
    int e = team;
    for (; e < E && !dead; e += T) {
        if constexpr (REDO) {
            // (redo[e] / falt[e] were written by the kernel before this one: every chunk of the team reads the same)
            if (__hip_atomic_load(&redo[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
                if (c == 0 && threadIdx.x == 0) {
                    const unsigned fa = __hip_atomic_load(&falt[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (fa) atomicOr(&flags[e], fa);
                }
                continue;
            }
            // (2 in every byte: the host runs this kernel alone for a while - not a fallback of THIS launch)
            if (c == 0 && threadIdx.x == 0 &&
                __hip_atomic_load(&redo[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1u)
                atomicAdd(&flags[E], 1u);      // rmt_n2_fallbacks
        }
        unsigned* const flags_out = CACHED ? falt : flags;
        RmtMember m;
        rmt_load_member(members + (size_t)e * RMT_NM, m);
        RmtCarry carry;
        rmt_carry_inlet(m, carry);
        real* ye = y + (size_t)e * RMT_V * N;
        const real* yin = REDO ? backup + (size_t)e * RMT_V * N : ye;
        real ys[RMT_NPT][RMT_V], k[RMT_NPT][RMT_V];
#if RMT_LDS_STATE_CHAIN < 1
        real y0[RMT_NPT][RMT_V];
#define Y0(j, i) y0[j][i]
#else
#define Y0(j, i) s_y0[i][lnode0 + (j)]
#endif
#if RMT_LDS_STATE_CHAIN < 2
        real acc[RMT_NPT][RMT_V];
#define ACC(j, i) acc[j][i]
#else
#define ACC(j, i) s_acc[i][lnode0 + (j)]
#endif
#pragma unroll
        for (int j = 0; j < RMT_NPT; ++j) {
            rmt_safe_state(m, ys[j]);
            if (j < nvalid) {
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) ys[j][i] = yin[(size_t)i * N + node0 + j];
                if constexpr (CACHED) {           // the launch's input, for rmt_n2_rk4_chain_redo
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) backup[((size_t)e * RMT_V + i) * N + node0 + j] = ys[j][i];
                }
            }
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) Y0(j, i) = ys[j][i];
        }
        rmt_flags_t flag;
        rmt_flags_clear(flag);
        unsigned lflag = 0u;
#if RMT_RK4C_KC
#pragma unroll
        for (int j = 0; j < RMT_NPT; ++j) kcs[j].valid = true;        // a new reactor: nothing has left the range yet
#endif
#if RMT_MODEL == 2
        preal pwarm[RMT_NPT];            // warm start of the pressure sweeps (see rmt_n2_rk4_reg)
        int warm = 0;
#pragma unroll
        for (int j = 0; j < RMT_NPT; ++j) pwarm[j] = preal(0);
#endif
        for (long long step = 0; step < nsteps && !dead; ++step) {
#if RMT_CHAIN_UNROLL
            rmt_noflags_t nof;
#pragma unroll
#else
#pragma unroll 1
#endif
            for (int s = 0; s < 4; ++s) {
                ctx.q += 1ull;
#if RMT_CHAIN_UNROLL && RMT_MODEL == 2
                if (s == 0 || RMT_CHECK_ALL_STAGES) rmt_rhs_block<RMT_NPT, false, RMT_CH>(m, sh, s & 1, ys, nvalid, carry, k, flag, &ctx, nullptr, pwarm, warm);
                else rmt_rhs_block<RMT_NPT, false, RMT_CH>(m, sh, s & 1, ys, nvalid, carry, k, nof, &ctx, nullptr, pwarm, warm);
                warm = 1;
#elif RMT_CHAIN_UNROLL
                auto stage = [&](auto& fl, auto ks_tag) {
                    typedef typename rmt_unref<decltype(fl)>::type FLT;
#if RMT_RK4C_KC
                    if constexpr (CACHED)
                        rmt_rhs_block<RMT_NPT, false, RMT_CH, FLT, RmtKC, decltype(ks_tag)::value>(
                            m, sh, s & 1, ys, nvalid, carry, k, fl, &ctx, nullptr, nullptr, 0, nullptr, nullptr, kcs);
                    else
#endif
                    rmt_rhs_block<RMT_NPT, false, RMT_CH, FLT>(m, sh, s & 1, ys, nvalid, carry, k, fl, &ctx);
                };
                auto tested_stage = [&](auto ks_tag) {
#if RMT_CALL_FLAGS
                    if constexpr (CACHED) {
                        rmt_callflags_t cf;
                        rmt_callflags_clear(cf);
                        stage(cf, ks_tag);
                        rmt_flags_fold(flag, cf);
                    } else
#endif
                    stage(flag, ks_tag);
                };
                // (RMT_KC_REFRESH_CHAIN: as RMT_KC_REFRESH of the one-workgroup stepper.  1 at 512 x 2, where the second version of
                // stage 1 costs this kernel 105 scratch accesses per step; the small chunks of ONE long reactor have the registers)
                if (s == 0) {
#if RMT_KC_REFRESH_CHAIN > 1
                    if (step % RMT_KC_REFRESH_CHAIN == 0) tested_stage(rmt_int_t<0>{});
                    else tested_stage(rmt_int_t<2>{});
#else
                    tested_stage(rmt_int_t<0>{});
#endif
                } else if (RMT_CHECK_ALL_STAGES) tested_stage(rmt_int_t<2>{});
                else stage(nof, rmt_int_t<2>{});
#else
                rmt_rhs_block<RMT_NPT, false, RMT_CH>(m, sh, s & 1, ys, nvalid, carry, k, flag, &ctx);
#endif
                if (ctx.abort) { dead = true; break; }
                if (s < 3) {
                    const real cn = (s == 2) ? h : hh;
                    const real wk = (s == 0) ? real(1) : real(2);
#pragma unroll
                    for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                        for (int i = 0; i < RMT_V; ++i) {
                            ACC(j, i) = (s == 0) ? k[j][i] : ACC(j, i) + wk * k[j][i];
                            ys[j][i] = Y0(j, i) + k[j][i] * cn;
                        }
                } else {
#pragma unroll
                    for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                        for (int i = 0; i < RMT_V; ++i) {
                            const real yn = Y0(j, i) + h6 * (ACC(j, i) + k[j][i]);
                            Y0(j, i) = yn;
                            ys[j][i] = yn;
                        }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < RMT_NPT; ++j) {
            if (j < nvalid) {
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) ye[(size_t)i * N + node0 + j] = ys[j][i];
                lflag |= rmt_finite_flag(ys[j]);
            }
        }
        lflag |= rmt_flags_bits(flag);
        if (dead) lflag |= RMT_FLAG_STEP;
        if (lflag) atomicOr(&flags_out[e], lflag);
#if RMT_RK4C_KC
        if constexpr (CACHED) {
            bool left = false;
#pragma unroll
            for (int j = 0; j < RMT_NPT; ++j) left = left || !kcs[j].valid;
            if (__any(left) && (threadIdx.x & 63) == 0) atomicOr(&redo[e], 1u);
        }
#endif
#undef Y0
#undef ACC
    }
    unsigned* const flags_tail = CACHED ? falt : flags;
    if (dead && threadIdx.x == 0) {       // let the rest of the chain drain
#if RMT_CH == 2
        __hip_atomic_store(ctx.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
        __hip_atomic_store(ctx.sync_out, RMT_CHAIN_POISON, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c > 0)
            __hip_atomic_store(ctx.sync_in + 16, RMT_CHAIN_POISON, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
        // the team's remaining reactors were never integrated: they must not read as "advanced"
        for (int e2 = e; e2 < E; e2 += T)
            if (!REDO || __hip_atomic_load(&redo[e2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)
                atomicOr(&flags_tail[e2], RMT_FLAG_STEP);
    }
#undef RMT_CH
}

extern "C" __global__ __launch_bounds__(RMT_BLOCK) void rmt_n2_rk4_chain(
        real* __restrict__ y, const double* __restrict__ members, const int N, const int E,
        const int C, const int T, const double h_, const long long nsteps,
        unsigned long long* __restrict__ sync, double* __restrict__ slots,
        unsigned* __restrict__ flags, unsigned long long* __restrict__ rings,
        unsigned* __restrict__ abort_words, real* __restrict__ backup, unsigned* __restrict__ redo,
        unsigned* __restrict__ falt) {
    rmt_rk4_chain_body<RMT_RK4C_KC != 0, false>(y, members, N, E, C, T, h_, nsteps, sync, slots, flags, rings, abort_words,
                                                 backup, redo, falt);
}
#if RMT_RK4C_KC
extern "C" __global__ __launch_bounds__(RMT_BLOCK) void rmt_n2_rk4_chain_redo(
        real* __restrict__ y, const double* __restrict__ members, const int N, const int E,
        const int C, const int T, const double h_, const long long nsteps,
        unsigned long long* __restrict__ sync, double* __restrict__ slots,
        unsigned* __restrict__ flags, unsigned long long* __restrict__ rings,
        unsigned* __restrict__ abort_words, real* __restrict__ backup, unsigned* __restrict__ redo,
        unsigned* __restrict__ falt) {
    rmt_rk4_chain_body<false, true>(y, members, N, E, C, T, h_, nsteps, sync, slots, flags, rings, abort_words,
                                    backup, redo, falt);
}
#endif
#endif   // !RMT_PROFILE

// ===================================================================== kernel: RK4, state in memory
// Same integrator for any N with ONE workgroup per reactor.  Information only travels downstream and
// RK stage s of a node block needs nothing but stage s of the block before it, so the node blocks are
// the OUTER loop of a time step: a block of RMT_BLOCK*RMT_NPT nodes is read once, taken through all
// four stages on chip - each stage with its own hand-over {pressure, clamped upstream state} from the
// previous block, kept in LDS - and written once.  112 B of memory traffic per node-step instead of
// the ~1 KB of a stage-by-stage walk (which this kernel used to do: 4.6e9 node-steps/s).
struct RmtStageCarry {
    double P[4];
    real up[4][RMT_V];
};
extern "C" __global__ __launch_bounds__(RMT_BLOCK) void rmt_n2_rk4_mem(
        real* __restrict__ y, real* __restrict__ work, const double* __restrict__ members,
        const int N, const int E, const double h_, const long long nsteps,
        unsigned* __restrict__ flags) {
    __shared__ RmtShared sh;
    __shared__ RmtStageCarry s_c;
#if RMT_LDS_STATE_CHAIN >= 1                             // the block's y_n / K accumulator in LDS, as in the chained kernel
    __shared__ real s_y0[RMT_V][RMT_NODES_WG];
#define Y0M(j, i) s_y0[i][lnode0 + (j)]
#else
#define Y0M(j, i) y0[j][i]
#endif
#if RMT_LDS_STATE_CHAIN >= 2
    __shared__ real s_acc[RMT_V][RMT_NODES_WG];
#define ACCM(j, i) s_acc[i][lnode0 + (j)]
#else
#define ACCM(j, i) acc[j][i]
#endif
    const int lnode0 = (int)threadIdx.x * RMT_NPT;
    rmt_math_init();
    (void)work;
    (void)E;
    const int e = blockIdx.x;
    RmtMember m;
    rmt_load_member(members + (size_t)e * RMT_NM, m);
    RMT_PROFILE_BIND(m, e, N)
    real* ye = y + (size_t)e * RMT_V * N;
    const real h = real(h_), hh = real(0.5 * h_), h6 = real(h_ / 6.0);
    rmt_flags_t flag;
    rmt_flags_clear(flag);
    rmt_noflags_t nof;
    unsigned lflag = 0u;
    int ph = 0;
    for (long long step = 0; step < nsteps; ++step) {
#if RMT_FORCING
        const double tstep = members[(size_t)e * RMT_NM + M_FORCE] + (double)step * h_;     // the launch starts at t_ref
#endif
        __syncthreads();                                 // the previous step's hand-overs have been read
        if (threadIdx.x == 0) {
            RmtCarry c0;
            rmt_carry_inlet(m, c0);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#if RMT_FORCING
                rmt_forcing_stage(m, c0, members + (size_t)e * RMT_NM, tstep + rmt_rk4_c(s) * h_, nullptr);   // each stage: its own inlet
#endif
                s_c.P[s] = c0.P;
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) s_c.up[s][i] = c0.up[i];
            }
        }
        __syncthreads();
        for (int base = 0; base < N; base += RMT_BLOCK * RMT_NPT) {
            const int node0 = base + (int)threadIdx.x * RMT_NPT;
            const int nvalid = (N - node0) < 0 ? 0 : ((N - node0) > RMT_NPT ? RMT_NPT : (N - node0));
            real ys[RMT_NPT][RMT_V], k[RMT_NPT][RMT_V];
#if RMT_LDS_STATE_CHAIN < 1
            real y0[RMT_NPT][RMT_V];
#endif
#if RMT_LDS_STATE_CHAIN < 2
            real acc[RMT_NPT][RMT_V];
#endif
#pragma unroll
            for (int j = 0; j < RMT_NPT; ++j) {
                rmt_safe_state(m, ys[j]);
                if (j < nvalid) {
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) ys[j][i] = ye[(size_t)i * N + node0 + j];
                }
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) Y0M(j, i) = ys[j][i];
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                RmtCarry carry;                          // this stage's hand-over from the previous block
                carry.P = s_c.P[s];
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) carry.up[i] = s_c.up[s][i];
                RMT_PROFILE_AT(carry, base)
#if RMT_FORCING
                rmt_forcing_apply3(m, members + (size_t)e * RMT_NM, tstep + rmt_rk4_c(s) * h_);    // the wall temperature of this stage (the inlet: s_c)
#endif
                if (s == 0 || RMT_CHECK_ALL_STAGES) rmt_rhs_block<RMT_NPT, true>(m, sh, ph, ys, nvalid, carry, k, flag);
                else rmt_rhs_block<RMT_NPT, true>(m, sh, ph, ys, nvalid, carry, k, nof);
                ph ^= 1;
                if (threadIdx.x == 0) {                  // (every reader of slot s is past the barrier inside)
                    s_c.P[s] = carry.P;
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) s_c.up[s][i] = carry.up[i];
                }
                if (s < 3) {
                    const real cn = (s == 2) ? h : hh;
                    const real wk = (s == 0) ? real(1) : real(2);
#pragma unroll
                    for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                        for (int i = 0; i < RMT_V; ++i) {
                            ACCM(j, i) = (s == 0) ? k[j][i] : ACCM(j, i) + wk * k[j][i];
                            ys[j][i] = Y0M(j, i) + k[j][i] * cn;
                        }
                } else {
#pragma unroll
                    for (int j = 0; j < RMT_NPT; ++j)
#pragma unroll
                        for (int i = 0; i < RMT_V; ++i) ys[j][i] = Y0M(j, i) + h6 * (ACCM(j, i) + k[j][i]);
                }
            }
#pragma unroll
            for (int j = 0; j < RMT_NPT; ++j) {
                if (j < nvalid) {
#pragma unroll
                    for (int i = 0; i < RMT_V; ++i) ye[(size_t)i * N + node0 + j] = ys[j][i];
                    lflag |= rmt_finite_flag(ys[j]);
                }
            }
        }
    }
    lflag |= rmt_flags_bits(flag);
    if (lflag) atomicOr(&flags[e], lflag);
#undef Y0M
#undef ACCM
}

