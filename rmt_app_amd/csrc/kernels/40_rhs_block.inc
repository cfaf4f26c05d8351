#if RMT_MODEL == 0
// RHS for the NPT consecutive nodes owned by this thread (nodes base+tid*NPT ...).
// `nvalid` = how many of them exist (< NPT only at the reactor's end).  One __syncthreads().
// buf = LDS ping-pong index; callers alternate it between consecutive calls.
// CHAIN: 0 = the reactor lives in this workgroup, 1 = chained workgroups with the flag protocol (explicit
// steppers), 2 = chained workgroups with tagged-word links (stiff stepper)
template <int NPT, bool CARRY_OUT, int CHAIN = 0, typename FL = rmt_flags_t, typename KC = rmt_nocache_t, int KSTATIC = -1,
          bool WAVE_SGPR = true>
__device__ __forceinline__ void rmt_rhs_block(const RmtMember& m, RmtShared& sh, const int buf,
                                              const real (&ys)[NPT][RMT_V], const int nvalid,
                                              RmtCarry& carry, real (&k)[NPT][RMT_V],
                                              FL& flag, RmtChainCtx* ctx = nullptr,
                                              RmtLocal* loc_out = nullptr, preal* = nullptr, const int = 0,
                                              real (*jac)[RMT_V] = nullptr,
                                              real (*upl)[RMT_V][RMT_BLOCK + 1] = nullptr, KC* kcs = nullptr) {
    // jac (NPT == 1 only): also return -d f_z/d y_z of the node, analytic, sharing the rate evaluation
    // kcs (KC = RmtKC): the NPT nodes' caches of the temperature-only rate constants (on-chip steppers)
    // upl (single-block reactors only): the clamped last-node states travel to the downstream lane through LDS
    //   (slot tid + 1 written, slot tid read after the barrier; slot 0 = the inlet, written once by the kernel)
    //   instead of 2 V DPP moves + the lane-0 special case - LDS instructions do not occupy the VALU
    const int lane = threadIdx.x & 63;
    // the wave index is wave-uniform by construction: as a scalar, the LDS addresses derived from it need no long-lived
    // VGPRs (they had been spilled to scratch in the RK4 steppers).  WAVE_SGPR false keeps the vector form for callers
    // that are short of SGPRs instead (the RK45 stepper: 10 scratch accesses per step against 23)
    const int wave = WAVE_SGPR ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);
    RmtNode nd[NPT];
    RmtAff loc[NPT];
    RmtAff mine = {preal(1), preal(0)};
    // RMT_NODE_PAIR_RCP (the caching steppers at two nodes per lane): the two nodes' 1/(sum(state) T) from ONE reciprocal
    // of the product, 3 multiplications instead of the second v_rcp_f64 and its Newton steps.  A lane beyond the
    // reactor's end carries the inlet state: every factor is positive and O(1)..O(1e3)
    real pair_ct[NPT], pair_inv[NPT];
    constexpr bool PAIR = (NPT == 2) && KC::enabled && (RMT_NODE_PAIR_RCP != 0) && (RMT_NODE_RCP_MERGE != 0);
    if constexpr (PAIR) {
        const real d0 = rmt_node_pre_sum(m, ys[0], nd[0], pair_ct[0]);
        const real d1 = rmt_node_pre_sum(m, ys[NPT - 1], nd[NPT - 1], pair_ct[NPT - 1]);
        const real t = rmt_rcp(d0 * d1);
        pair_inv[0] = t * d1;
        pair_inv[NPT - 1] = t * d0;
    }
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        preal a;
        if constexpr (PAIR) a = rmt_node_pre_fin(m, nd[j], pair_ct[j], pair_inv[j]);
        else a = rmt_node_pre(m, ys[j], nd[j]);
#if RMT_PROFILE
        static_assert(CHAIN == 0, "RMT_PROFILE: the chained forms do not carry the profile");
        RMT_PROFILE_NODE(m, nd[j], carry.node0 + (int)threadIdx.x * NPT + j)     // issued ahead of the scan and the barrier
#endif
        loc[j].a = (j < nvalid) ? a : preal(1);
        loc[j].b = (j < nvalid) ? m.beta : preal(0);
        mine = rmt_then(mine, loc[j]);
    }
    // inclusive scan of the per-lane maps over the wave
    RmtAff inc = mine;
#if RMT_DPP
    {   // lanes whose source is out of range / masked receive the identity map (a = 1, b = 0)
#define RMT_SCAN_STEP(CTRL, MASK)                                               \
        {                                                                       \
            RmtAff prev;                                                        \
            prev.a = rmt_dpp<CTRL, MASK>(preal(1), inc.a);                      \
            prev.b = rmt_dpp<CTRL, MASK>(preal(0), inc.b);                      \
            inc = rmt_then(prev, inc);                                          \
        }
#define RMT_SCAN_STEP0(CTRL)           /* all rows enabled: the identity b = 0 is the zero fill */ \
        {                                                                       \
            RmtAff prev;                                                        \
            prev.a = rmt_dpp<CTRL, 0xf>(preal(1), inc.a);                       \
            prev.b = rmt_dpp0<CTRL>(inc.b);                                     \
            inc = rmt_then(prev, inc);                                          \
        }
        RMT_SCAN_STEP0(0x111)          // row_shr:1
        RMT_SCAN_STEP0(0x112)          // row_shr:2
        RMT_SCAN_STEP0(0x114)          // row_shr:4
        RMT_SCAN_STEP0(0x118)          // row_shr:8
        RMT_SCAN_STEP(0x142, 0xa)      // row_bcast:15 -> rows 1, 3
        RMT_SCAN_STEP(0x143, 0xc)      // row_bcast:31 -> rows 2, 3
#undef RMT_SCAN_STEP
#undef RMT_SCAN_STEP0
    }
#else
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        RmtAff prev;
        prev.a = __shfl_up(inc.a, d);
        prev.b = __shfl_up(inc.b, d);
        if (lane >= d) inc = rmt_then(prev, inc);
    }
#endif
    // clamped state of my last node, for my downstream neighbour
    real last[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) last[i] = rmt_max(ys[NPT - 1][i], RMT_EPS);      // :4093
#if !RMT_ISO
    last[RMT_S] = ys[NPT - 1][RMT_S];                                                // :4111
#endif
    if (lane == 63) {
        sh.put_total(buf, wave, inc);
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) sh.bnd[buf][wave][i] = last[i];
    }
    RmtAff exc;
    exc.a = rmt_lane_up1(inc.a);
    exc.b = rmt_lane_up1(inc.b);
    if (lane == 0) { exc.a = preal(1); exc.b = preal(0); }
    real up[RMT_V];
    if (upl) {
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) upl[buf][i][threadIdx.x + 1] = last[i];
    } else {
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) up[i] = rmt_lane_up1(last[i]);
    }
    if (CHAIN == 2) {
        if (wave == 0) {
            if (ctx->has_in) {                    // stage record {up[V], P} of the upstream chunk's last block
                const int st = rmt_link_recv(rmt_ring_entry(ctx->ring_in, ctx->seq_in), ctx->seq_in, sh.cin[buf], RMT_V + 1,
                                             ctx->abort_word, ctx->dead);
                ctx->dead |= st;
                if (ctx->bp && lane == 0)         // taken: the producer may reuse the ring entry
                    __hip_atomic_store(ctx->bp_in, (unsigned long long)ctx->seq_in, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (lane == 0) sh.abort[buf] = ctx->dead;
        }
        if (ctx->has_in) ctx->seq_in = rmt_seq_next(ctx->seq_in);
    }
    if (CHAIN == 1) {
        if (wave == 0) {                          // all waiting is done by one wave, before the barrier
            int st = 0;
            double rec = 0.0;
            if (ctx->has_in) {
                if (lane == 0) st = rmt_chain_wait(ctx->sync_in, ctx->q);
                st = __shfl(st, 0);
                if (lane <= RMT_V) {              // sc1 load (bypasses this CU's L1): no acquire fence needed
                    rec = __longlong_as_double((long long)__hip_atomic_load(
                        (const unsigned long long*)ctx->slots_in +
                            (size_t)(ctx->q % RMT_CHAIN_DEPTH) * (RMT_V + 1) + lane,
                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                    sh.cin[buf][lane] = rec;
                }
            }
            if (ctx->has_out && lane == 0 && ctx->q > RMT_CHAIN_DEPTH)      // slot free again?
                st |= rmt_chain_wait(ctx->sync_out + 16, ctx->q - RMT_CHAIN_DEPTH);
            if (lane == 0) sh.abort[buf] = st;
        }
    }
#ifndef RMT_TIMING_NO_BARRIER             // timing experiments only: results are wrong without it
    __syncthreads();
#endif
    if (CHAIN == 2) {
        if (ctx->has_in) {
            carry.P = sh.cin[buf][RMT_V];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) carry.up[i] = real(sh.cin[buf][i]);
        }
        ctx->abort = sh.abort[buf];               // workgroup-uniform view of wave 0's sticky failure
    }
    if (CHAIN == 1) {
        if (ctx->has_in) {                        // chunk 0 keeps the inlet carry it was given
            carry.P = sh.cin[buf][RMT_V];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) carry.up[i] = real(sh.cin[buf][i]);
        }
        ctx->abort = sh.abort[buf];
        if (ctx->has_in && threadIdx.x == 0)      // record consumed (it sits in LDS now)
            __hip_atomic_store(ctx->sync_in + 16, ctx->q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // pressure entering this wave = carry.P pushed through the totals of the waves before it
    const preal pw = rmt_push_before(sh, buf, wave, carry.P);
    if (CHAIN == 2) {
        // The stage record for the downstream chunk {clamped state of the last node, pressure after it} is complete
        // HERE, before the node functions (kinetics: three quarters of the evaluation) run: sending it now
        // lets the next chunk start its own evaluation of this stage a quarter of a stage time after this one
        // instead of a whole one - the skew a stepper with a per-step rendezvous pays on every step.
        if (ctx->has_out) {
            if (wave == RMT_NW - 1 &&             // (staged in LDS by the sending wave itself; test hook: a stuck producer)
                !(ctx->chunk == RMT_CHAIN_TEST_STALL_CHUNK && ctx->seq_out >= (unsigned)RMT_CHAIN_TEST_STALL_FROM)) {
                if (ctx->bp && ctx->seq_out - ctx->known >= (unsigned)(RMT_RING - 8)) {
                    // about to lap the ring: wait until the consumer has taken message seq_out - RMT_RING + 8
                    unsigned got = ctx->known;
                    if (lane == 0) {
                        unsigned spins = 0;
                        for (;;) {
                            got = (unsigned)__hip_atomic_load(ctx->bp_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (ctx->seq_out - got < (unsigned)(RMT_RING - 8)) break;
                            if (++spins > RMT_CHAIN_SPINS ||
                                __hip_atomic_load(ctx->abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                                __hip_atomic_store(ctx->abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                break;
                            }
                            __builtin_amdgcn_s_sleep(2);
                        }
                    }
                    ctx->known = (unsigned)__shfl((int)got, 0);
                }
                const preal pe = sh.through(buf, wave, pw);
                if (lane <= RMT_V)
                    sh.cst[buf][lane] = (lane == RMT_V) ? (double)pe : (double)sh.bnd[buf][RMT_NW - 1][lane < RMT_V ? lane : 0];
                rmt_link_send(rmt_ring_entry(ctx->ring_out, ctx->seq_out), ctx->seq_out, sh.cst[buf], RMT_V + 1);
            }
            ctx->seq_out = rmt_seq_next(ctx->seq_out);
        }
    }
    if (upl) {
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) up[i] = upl[buf][i][threadIdx.x];
    } else if (lane == 0) {
        if (!CARRY_OUT && CHAIN == 0) {
            // the reactor is one block: the upstream of node 0 never changes; reading it from LDS
            // (written once at kernel start) instead of the member's SGPRs saves ~25 VALU lane
            // moves per stage that only reloaded spilled scalars
            const real* src = (wave == 0) ? sh.inlet : sh.bnd[buf][wave == 0 ? 0 : wave - 1];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) up[i] = src[i];
        } else if (wave == 0) {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) up[i] = carry.up[i];
        } else {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) up[i] = sh.bnd[buf][wave - 1][i];
        }
    }
    preal P = exc.a * pw + exc.b;
    // The node functions in the version the caller asks for when it passes caches of the temperature-only rate
    // constants (KC = RmtKC): KSTATIC 0 evaluates in full and moves every node's reference point to this state,
    // KSTATIC 2 takes the constants from the cache - without a second code path: a node that leaves the cache's range
    // only clears its `valid`, for good (inside rmt_kinetics), and the caller voids the step (rmt_rk4_reg_body).
    auto node_loop = [&](auto kmode_tag_) {
        constexpr int KMODE_ = decltype(kmode_tag_)::value;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            // lanes beyond the reactor's end carry the (valid) inlet state, so their checks are not masked
#if RMT_WITH_ROS4 && !RMT_ROS_JAC_FD
            if (jac) {
                real rj[RMT_R];
                rmt_node_jac(m, nd[j], ys[j], P, *reinterpret_cast<real (*)[RMT_V][RMT_V]>(jac), rj, flag);
                rmt_node_post<FL, true>(m, nd[j], ys[j], up, P, k[j], flag, rj);
            } else
#endif
            rmt_node_post<FL, false, KC, KMODE_>(m, nd[j], ys[j], up, P, k[j], flag, nullptr, KC::enabled ? &kcs[j] : nullptr);
            if (loc_out) {                                   // frozen neighbourhood of node j (Jacobian)
                loc_out[j].P = P;
#pragma unroll
                for (int i = 0; i < RMT_V; ++i) loc_out[j].up[i] = up[i];
            }
            P = loc[j].a * P + loc[j].b;
            if (j + 1 < NPT) {
#pragma unroll
                for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(ys[j][i], RMT_EPS);
#if !RMT_ISO
                up[RMT_S] = ys[j][RMT_S];
#endif
            }
        }
    };
    static_assert(!KC::enabled || KSTATIC == 0 || KSTATIC == 2, "callers with a cache fix the version per call");
    node_loop(rmt_int_t<(KC::enabled ? KSTATIC : 0)>{});
    if (CARRY_OUT) {
        carry.P = rmt_push_from(sh, buf, wave, pw);
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) carry.up[i] = sh.bnd[buf][RMT_NW - 1][i];
    }
    if (CHAIN == 1) {
        if (wave == RMT_NW - 1 && rmt_chain_publishes(ctx)) {        // publish this stage's record
            const preal pe = sh.through(buf, wave, pw);
            if (lane <= RMT_V) {                  // sc1 (write-through) stores, drained before the flag
                const double v = (lane == RMT_V) ? (double)pe : (double)sh.bnd[buf][RMT_NW - 1][lane < RMT_V ? lane : 0];
                __hip_atomic_store((unsigned long long*)ctx->slots_out +
                                       (size_t)(ctx->q % RMT_CHAIN_DEPTH) * (RMT_V + 1) + lane,
                                   (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0)
                __hip_atomic_store(ctx->sync_out, ctx->q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

#else
// Model M2: same contract as the N2 version above, but the pressure recurrence
// P[z+1] = phi_z(P[z]) = P[z] - u_z/P[z] - w_z/P[z]^2 is nonlinear (EOS velocity).  Newton's method
// on the whole march: linearise every phi_z at the current iterate, P[z+1] = a_z P[z] + b_z with
// a_z = phi_z'(P_z) = 1 + u/P^2 + 2w/P^3 and b_z = phi_z(P_z) - a_z P_z = -2u/P - 3w/P^2, solve that
// affine recurrence with the scan, repeat.  The error contracts quadratically; with the bed's
// pressure drop up to ~15 % of P, 3 sweeps reach rounding level, 2 up to ~0.5 % (the host picks
// RMT_M2_NEWTON from the feed-state drop, plan.m2_newton_sweeps; the size of the last update is
// checked: RMT_FLAG_PRESSURE).  One __syncthreads() per sweep plus one between sweeps.
__device__ __forceinline__ RmtAff rmt_wave_scan(RmtAff inc) {
#if RMT_DPP
#define RMT_SCAN_STEP(CTRL, MASK)                                               \
    {                                                                           \
        RmtAff prev;                                                            \
        prev.a = rmt_dpp<CTRL, MASK>(preal(1), inc.a);                          \
        prev.b = rmt_dpp<CTRL, MASK>(preal(0), inc.b);                          \
        inc = rmt_then(prev, inc);                                              \
    }
    RMT_SCAN_STEP(0x111, 0xf)      // row_shr:1
    RMT_SCAN_STEP(0x112, 0xf)      // row_shr:2
    RMT_SCAN_STEP(0x114, 0xf)      // row_shr:4
    RMT_SCAN_STEP(0x118, 0xf)      // row_shr:8
    RMT_SCAN_STEP(0x142, 0xa)      // row_bcast:15 -> rows 1, 3
    RMT_SCAN_STEP(0x143, 0xc)      // row_bcast:31 -> rows 2, 3
#undef RMT_SCAN_STEP
#else
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        RmtAff prev;
        prev.a = __shfl_up(inc.a, d);
        prev.b = __shfl_up(inc.b, d);
        if (lane >= d) inc = rmt_then(prev, inc);
    }
#endif
    return inc;
}

template <int NPT, bool CARRY_OUT, int CHAIN = 0, typename FL = rmt_flags_t, typename KC = rmt_nocache_t, int KSTATIC = -1,
          bool WAVE_SGPR = true>
__device__ __forceinline__ void rmt_rhs_block(const RmtMember& m, RmtShared& sh, const int buf,
                                              const real (&ys)[NPT][RMT_V], const int nvalid,
                                              RmtCarry& carry, real (&k)[NPT][RMT_V],
                                              FL& flag, RmtChainCtx* ctx = nullptr,
                                              RmtLocal* loc_out = nullptr, preal* pwarm = nullptr,
                                              const int warm = 0, real (*jac)[RMT_V] = nullptr,
                                              real (*)[RMT_V][RMT_BLOCK + 1] = nullptr, KC* kcs = nullptr) {
    static_assert(!KC::enabled || KSTATIC == 0 || KSTATIC == 2, "callers with a cache fix the version per call");
    // kcs (KC = RmtKC): the NPT nodes' caches of the temperature-only rate constants, as in the N2 block above
    // jac (NPT == 1, with loc_out): also return -d f_z/d y_z of the node and the coupling d f_z/d up (loc_out[].lco)
    // pwarm/warm: the caller's pressures of the previous RHS evaluation as the starting iterate - between
    // two RK stages P moves by ~1e-9 relative, so ONE sweep is converged (the check below still applies)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    RmtNode nd[NPT];
    RmtPc pc[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        pc[j] = rmt_node_pre(m, ys[j], nd[j]);
        if (j >= nvalid) { pc[j].u = preal(0); pc[j].w = preal(0); }
    }
    real last[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) last[i] = rmt_max(ys[NPT - 1][i], RMT_EPS);      // :1138
    last[RMT_S] = ys[NPT - 1][RMT_S];                                                // :1154
    if (lane == 63) {
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) sh.bnd[buf][wave][i] = last[i];
    }
    real up[RMT_V];
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) up[i] = rmt_lane_up1(last[i]);
    if (CHAIN == 2) {
        // tagged-word links (see the N2 version); as with the flag protocol below the record must be here BEFORE
        // the sweeps, so it is awaited now and handed to all waves by one extra barrier
        if (wave == 0) {
            if (ctx->has_in) {
                const int st = rmt_link_recv(rmt_ring_entry(ctx->ring_in, ctx->seq_in), ctx->seq_in, sh.cin[buf], RMT_V + 1,
                                             ctx->abort_word, ctx->dead);
                ctx->dead |= st;
                if (ctx->bp && lane == 0)
                    __hip_atomic_store(ctx->bp_in, (unsigned long long)ctx->seq_in, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (lane == 0) sh.abort[buf] = ctx->dead;
        }
        if (ctx->has_in) ctx->seq_in = rmt_seq_next(ctx->seq_in);
        __syncthreads();
        if (ctx->has_in) {
            carry.P = sh.cin[buf][RMT_V];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) carry.up[i] = real(sh.cin[buf][i]);
        }
        ctx->abort = sh.abort[buf];
    }
    if (CHAIN == 1) {
        // chained workgroups (see the N2 version): the upstream chunk's record {clamped state of its last
        // node, pressure after it} must be here BEFORE the sweeps (it is their starting pressure), so it
        // is awaited by wave 0 now and handed to all waves by one extra barrier
        if (wave == 0) {
            int st = 0;
            if (ctx->has_in) {
                if (lane == 0) st = rmt_chain_wait(ctx->sync_in, ctx->q);
                st = __shfl(st, 0);
                if (lane <= RMT_V)
                    sh.cin[buf][lane] = __longlong_as_double((long long)__hip_atomic_load(
                        (const unsigned long long*)ctx->slots_in +
                            (size_t)(ctx->q % RMT_CHAIN_DEPTH) * (RMT_V + 1) + lane,
                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
            if (ctx->has_out && lane == 0 && ctx->q > RMT_CHAIN_DEPTH)      // slot free again?
                st |= rmt_chain_wait(ctx->sync_out + 16, ctx->q - RMT_CHAIN_DEPTH);
            if (lane == 0) sh.abort[buf] = st;
        }
        __syncthreads();
        if (ctx->has_in) {                        // chunk 0 keeps the inlet carry it was given
            carry.P = sh.cin[buf][RMT_V];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) carry.up[i] = real(sh.cin[buf][i]);
        }
        ctx->abort = sh.abort[buf];
        if (ctx->has_in && threadIdx.x == 0)      // record consumed (it sits in LDS now)
            __hip_atomic_store(ctx->sync_in + 16, ctx->q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    preal Pj[NPT], dlast = preal(0), pw = carry.P;
    const bool usewarm = (pwarm != nullptr) && (warm != 0);          // workgroup-uniform
#pragma unroll
    for (int j = 0; j < NPT; ++j) Pj[j] = usewarm ? pwarm[j] : carry.P;
    const int nsweeps = usewarm ? 1 : RMT_M2_NEWTON;
#pragma unroll
    for (int it = 0; it < RMT_M2_NEWTON; ++it) {
        if (it >= nsweeps) break;
        RmtAff loc[NPT];
        RmtAff mine = {preal(1), preal(0)};
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const preal ip = rmt_rcp(Pj[j]);
            const preal a1 = pc[j].u * ip, a2 = pc[j].w * ip * ip;
            loc[j].a = preal(1) + (a1 + preal(2) * a2) * ip;
            loc[j].b = -(preal(2) * a1 + preal(3) * a2);
            mine = rmt_then(mine, loc[j]);
        }
        const RmtAff inc = rmt_wave_scan(mine);
        if (it > 0) __syncthreads();              // the previous sweep's totals have been read
        if (lane == 63) {
            sh.put_total(buf, wave, inc);
        }
        RmtAff exc;
        exc.a = rmt_lane_up1(inc.a);
        exc.b = rmt_lane_up1(inc.b);
        if (lane == 0) { exc.a = preal(1); exc.b = preal(0); }
        __syncthreads();
        pw = rmt_push_before(sh, buf, wave, carry.P);
        preal P = exc.a * pw + exc.b;
        dlast = preal(0);
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            dlast = rmt_max(dlast, rmt_abs(P - Pj[j]));
            Pj[j] = P;
            P = loc[j].a * P + loc[j].b;
        }
    }
    // quadratic contraction e' <= 0.05 e^2 (measured up to a 27 % drop): a last update below
    // 3e-7 P leaves an error below 1e-14 P
    RMT_CHECK(flag, !(dlast <= preal(3e-7) * rmt_abs(Pj[0])), RMT_FLAG_PRESSURE);
    if (pwarm) {
#pragma unroll
        for (int j = 0; j < NPT; ++j) pwarm[j] = Pj[j];
    }
    if (CHAIN == 2) {
        // the record for the downstream chunk is complete once the pressure sweeps are: sent before the node
        // functions run (see the N2 version)
        if (ctx->has_out) {
            if (wave == RMT_NW - 1 &&
                !(ctx->chunk == RMT_CHAIN_TEST_STALL_CHUNK && ctx->seq_out >= (unsigned)RMT_CHAIN_TEST_STALL_FROM)) {
                if (ctx->bp && ctx->seq_out - ctx->known >= (unsigned)(RMT_RING - 8)) {
                    unsigned got = ctx->known;
                    if (lane == 0) {
                        unsigned spins = 0;
                        for (;;) {
                            got = (unsigned)__hip_atomic_load(ctx->bp_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (ctx->seq_out - got < (unsigned)(RMT_RING - 8)) break;
                            if (++spins > RMT_CHAIN_SPINS ||
                                __hip_atomic_load(ctx->abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                                __hip_atomic_store(ctx->abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                break;
                            }
                            __builtin_amdgcn_s_sleep(2);
                        }
                    }
                    ctx->known = (unsigned)__shfl((int)got, 0);
                }
                const preal pe = sh.through(buf, wave, pw);
                if (lane <= RMT_V)
                    sh.cst[buf][lane] = (lane == RMT_V) ? (double)pe : (double)sh.bnd[buf][RMT_NW - 1][lane < RMT_V ? lane : 0];
                rmt_link_send(rmt_ring_entry(ctx->ring_out, ctx->seq_out), ctx->seq_out, sh.cst[buf], RMT_V + 1);
            }
            ctx->seq_out = rmt_seq_next(ctx->seq_out);
        }
    }
    if (lane == 0) {
        if (!CARRY_OUT && !CHAIN) {
            // the reactor is one block: the upstream of node 0 never changes; reading it from LDS
            // (written once at kernel start) instead of the member's SGPRs saves ~25 VALU lane
            // moves per stage that only reloaded spilled scalars
            const real* src = (wave == 0) ? sh.inlet : sh.bnd[buf][wave == 0 ? 0 : wave - 1];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) up[i] = src[i];
        } else if (wave == 0) {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) up[i] = carry.up[i];
        } else {
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) up[i] = sh.bnd[buf][wave - 1][i];
        }
    }
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
#if RMT_WITH_ROS4 && !RMT_ROS_JAC_FD
        if (jac && loc_out) {
            real rj[RMT_R];
            rmt_node_jac(m, nd[j], ys[j], up, Pj[j], *reinterpret_cast<real (*)[RMT_V][RMT_V]>(jac), rj,
                         loc_out[j].lco, flag);
            rmt_node_post<FL, true>(m, nd[j], ys[j], up, Pj[j], k[j], flag, rj);
        } else
#endif
        rmt_node_post<FL, false, KC, (KC::enabled ? KSTATIC : 0)>(m, nd[j], ys[j], up, Pj[j], k[j], flag, nullptr,
                                                                    KC::enabled ? &kcs[j] : nullptr);
        if (loc_out) {
            loc_out[j].P = Pj[j];
#pragma unroll
            for (int i = 0; i < RMT_V; ++i) loc_out[j].up[i] = up[i];
        }
        if (j + 1 < NPT) {
#pragma unroll
            for (int i = 0; i < RMT_S; ++i) up[i] = rmt_max(ys[j][i], RMT_EPS);
            up[RMT_S] = ys[j][RMT_S];
        }
    }
    if (CARRY_OUT) {
        carry.P = rmt_push_from(sh, buf, wave, pw);
#pragma unroll
        for (int i = 0; i < RMT_V; ++i) carry.up[i] = sh.bnd[buf][RMT_NW - 1][i];
    }
    if (CHAIN == 1) {
        if (wave == RMT_NW - 1 && rmt_chain_publishes(ctx)) {        // publish this stage's record
            const preal pe = sh.through(buf, wave, pw);
            if (lane <= RMT_V) {                  // sc1 (write-through) stores, drained before the flag
                const double v = (lane == RMT_V) ? (double)pe : (double)sh.bnd[buf][RMT_NW - 1][lane < RMT_V ? lane : 0];
                __hip_atomic_store((unsigned long long*)ctx->slots_out +
                                       (size_t)(ctx->q % RMT_CHAIN_DEPTH) * (RMT_V + 1) + lane,
                                   (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0)
                __hip_atomic_store(ctx->sync_out, ctx->q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

#endif  // RMT_MODEL

// ------------------------------------------------------------------ helpers for the kernels
__device__ __forceinline__ void rmt_safe_state(const RmtMember& m, real* __restrict__ v) {
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) v[i] = m.cin[i];
#if !RMT_ISO
    v[RMT_S] = m.theta_in;
#endif
}

__device__ __forceinline__ unsigned rmt_finite_flag(const real* __restrict__ v) {
    unsigned f = 0u;
#pragma unroll
    for (int i = 0; i < RMT_V; ++i) f |= __builtin_isfinite(v[i]) ? 0u : RMT_FLAG_NONFINITE;
    return f;
}

