#ifndef RMT_HOST_EMULATION
// ---- cross-lane moves on the DPP path (no LDS crossbar round trip) ----------------------------
// RMT_DPP 1: v_mov_b32 ... row_shr / row_bcast / wave_shr (gfx9 DPP controls) for the 64-lane
// scan and the lane-1 neighbour fetch; RMT_DPP 0: __shfl_up (ds_bpermute_b32).
#ifndef RMT_DPP
#define RMT_DPP 1
#endif
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double rmt_dpp(const double old, const double v) {
    int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float rmt_dpp(const float old, const float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
// zero-filling form (bound_ctrl, all rows / banks enabled): lanes without a source lane receive 0 and the
// destination needs no initialisation - the two-operand form above costs a v_mov per dword to seed `old`
template <int CTRL>
__device__ __forceinline__ double rmt_dpp0(const double v) {
    int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ float rmt_dpp0(const float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// value of lane-1; lane 0 receives 0 (every caller overwrites lane 0 with the value from the previous wave /
// the carry), unlike __shfl_up(v, 1) which leaves lane 0 its own value
template <typename T>
__device__ __forceinline__ T rmt_lane_up1(const T v) {
#if RMT_DPP
    return rmt_dpp0<0x138>(v);                        // wave_shr:1
#else
    return __shfl_up(v, 1);
#endif
}
// value of lane-1; lane 0 KEEPS `old` (DPP without bound_ctrl leaves a destination lane that has no source lane
// untouched: no select, and no move either when `old` is the previous value of the destination)
template <typename T>
__device__ __forceinline__ T rmt_lane_up1_keep(const T old, const T v) {
#if RMT_DPP
    return rmt_dpp<0x138, 0xf>(old, v);               // wave_shr:1
#else
    const T u = __shfl_up(v, 1);
    return (threadIdx.x & 63) == 0 ? old : u;
#endif
}

// ---- per-node cache of the temperature-only rate / equilibrium constants (lowering.Lowered.kcache_plan) ----------
// RMT_KC_SLOTS doubles per mesh node in LDS - slot-major ([slot][node of the workgroup], stride = nodes per workgroup)
// or node-major (RMT_KC_NODE_MAJOR: a node's slots side by side, stride 1); each thread only touches its own nodes'
// entries, so no barrier.  `valid` is per lane and sticky: it turns false when a stage temperature leaves the range the
// Taylor steps serve (inside rmt_kinetics, MODE 2), and the CALLER then discards what it computed (rmt_rk4_reg_body).
struct RmtKC {
    static constexpr bool enabled = true;
    real* base;          // the node's slot 0
    int stride;          // doubles between two slots of the node
    bool valid;
    __device__ __forceinline__ real get(const int s) const { return base[s * stride]; }
    __device__ __forceinline__ void put(const int s, const real v) const { base[s * stride] = v; }
    __device__ __forceinline__ void leave(const bool out) { valid = valid && !out; }     // (sticky, see rmt_rk4_reg_body)
};

struct RmtShared {
#if RMT_NW > 1
    alignas(16) RmtAff tot[2][RMT_NW];   // a wave's total {a, b}: one 16-byte record (25_prefix.inc)
#else
    preal tot_a[2][RMT_NW];              // one wave: there is no cross-wave prefix, and the unit's layout stays what it was
    preal tot_b[2][RMT_NW];
#endif
    real bnd[2][RMT_NW][RMT_V];
    real red[2][RMT_NW];
    double cin[2][RMT_V + 1];     // chained workgroups: upstream record (up[V], P) of this stage
    double cst[2][RMT_V + 1];     // tagged-word links: staging of the message the last wave sends
    real xb[2][RMT_NW + 1][RMT_V];   // Jacobi sweeps of the stiff stepper: row 0 = the value upstream of the block
                                     // (carry or the upstream chunk's iterate), row w + 1 = last lane of wave w
    real inlet[RMT_V];            // single-workgroup stepper: the inlet values seen by node 0 (written once)
    int abort[2];
    // wave `wave` leaves its total / p pushed through the total of wave `wave`
    __device__ __forceinline__ void put_total(const int buf, const int wave, const RmtAff& t) {
#if RMT_NW > 1
        tot[buf][wave] = t;
#else
        tot_a[buf][wave] = t.a;
        tot_b[buf][wave] = t.b;
#endif
    }
    __device__ __forceinline__ preal through(const int buf, const int wave, const preal p) const {
#if RMT_NW > 1
        return tot[buf][wave].a * p + tot[buf][wave].b;
#else
        return tot_a[buf][wave] * p + tot_b[buf][wave];
#endif
    }
};

// pressure entering wave `wave` = p pushed through the totals of the waves before it, and the pressure leaving the
// block from the one entering wave `wave` (25_prefix.inc)
__device__ __forceinline__ preal rmt_push_before(const RmtShared& sh, const int buf, const int wave, preal p) {
#ifdef RMT_TIMING_NO_PUSH                  // timing experiments only: results are wrong with it
    return p;
#elif RMT_NW > 1
    return rmt_prefix_before<RMT_PREFIX_MODE>(sh.tot[buf], wave, p);
#else                                     // one wave: the unit's code stays what it was (the scalar loop of mode 2)
    const int wu = __builtin_amdgcn_readfirstlane(wave);
    for (int w = 0; w < wu; ++w) p = sh.through(buf, w, p);
    return p;
#endif
}
__device__ __forceinline__ preal rmt_push_from(const RmtShared& sh, const int buf, const int wave, preal p) {
#if RMT_NW > 1
    return rmt_prefix_from<RMT_PREFIX_MODE>(sh.tot[buf], wave, p);
#else
    const int wu = __builtin_amdgcn_readfirstlane(wave);
    for (int w = wu; w < RMT_NW; ++w) p = sh.through(buf, w, p);
    return p;
#endif
}

// ---- chained workgroups (one reactor spread over C workgroups) --------------------------------
// Information only flows downstream (upwind stencil, pressure march from the inlet), so the
// workgroups of a reactor form a producer->consumer chain with NO grid barrier: per RHS stage,
// chunk c hands chunk c+1 one record {clamped state of its last node, pressure after its last
// node} through a ring of RMT_CHAIN_DEPTH slots in global memory.  Protocol = the fence-free
// form of the CDNA guide (MI355X_MICROARCH "Valid forms", table row 1): every payload byte is
// stored sc1 (agent-scope relaxed atomic store = write-through) by ONE wave, that wave drains
// vmcnt, then ONE lane stores the sequence flag sc1; the consumer's polling wave reads the flag
// and then the payload with sc1 loads (agent-scope relaxed atomic loads, L1-bypassing).  A
// consumed-counter gives back-pressure.  (The release/acquire-fence form measured ~3 us more per
// stage.)  Every spin is bounded; a timeout poisons both counters so that the whole
// chain drains and the launch ends with RMT_FLAG_STEP instead of hanging.
#ifndef RMT_CHAIN_DEPTH
#define RMT_CHAIN_DEPTH 8
#endif
#define RMT_CHAIN_POISON (~0ull)
#ifndef RMT_CHAIN_SPINS
#define RMT_CHAIN_SPINS (1u << 22)
#endif
// test hook (tests/test_gpu_chain.py): chunk RMT_CHAIN_TEST_STALL_CHUNK stops publishing its records from
// sequence number RMT_CHAIN_TEST_STALL_FROM on - a stuck producer; the launch must end with RMT_FLAG_STEP
#ifndef RMT_CHAIN_TEST_STALL_CHUNK
#define RMT_CHAIN_TEST_STALL_CHUNK (-1)
#endif
#ifndef RMT_CHAIN_TEST_STALL_FROM
#define RMT_CHAIN_TEST_STALL_FROM 0
#endif
#define RMT_SYNC_STRIDE 32        // u64 words per link: [0] published seq, [16] consumed seq (own 128-B lines)

struct RmtChainCtx {
    bool has_in, has_out;
    unsigned long long* sync_in;      // link c-1 -> c
    unsigned long long* sync_out;     // link c -> c+1
    const double* slots_in;
    double* slots_out;
    unsigned long long q;             // sequence number of the current stage (1, 2, ...)
    int abort;                        // workgroup-uniform, valid after the stage's barrier
    int chunk;                        // position of this workgroup in its chain
    // tagged-word links (the chained stiff stepper, see rmt_link_send): ring of the link into / out of this
    // chunk, running exchange numbers (both ends count alike), the team's abort word, sticky failure
    unsigned long long* ring_in;
    unsigned long long* ring_out;
    unsigned seq_in, seq_out;
    unsigned* abort_word;
    int dead;
    // back-pressure of a tagged-word link whose producer is not held back by a per-step rendezvous (explicit
    // steppers): the consumer publishes the number of the last message it took, the producer looks at it only
    // when it is about to lap the ring
    bool bp;
    unsigned long long* bp_in;        // written by this chunk as consumer of link c-1 -> c
    unsigned long long* bp_out;       // read by this chunk as producer of link c -> c+1
    unsigned known;                   // last consumed number seen (sending wave only)
};
__device__ __forceinline__ bool rmt_chain_publishes(const RmtChainCtx* ctx) {
    return ctx->has_out && !ctx->abort &&
           !(ctx->chunk == RMT_CHAIN_TEST_STALL_CHUNK && ctx->q >= (unsigned long long)RMT_CHAIN_TEST_STALL_FROM);
}

__device__ __forceinline__ int rmt_chain_wait(unsigned long long* word, const unsigned long long need) {
    unsigned spins = 0;
    for (;;) {
        const unsigned long long v = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v == RMT_CHAIN_POISON) return 1;
        if (v >= need) return 0;
        if (++spins > RMT_CHAIN_SPINS) return 1;
        __builtin_amdgcn_s_sleep(2);
    }
}

// ---- tagged-word links (chained STIFF stepper) --------------------------------------------------
// The stiff stepper hands its downstream neighbour far more than one record per stage: per stage the
// {upstream state, pressure} record AND one boundary vector per Jacobi sweep of the linear solve, ~170
// messages per step.  The flag protocol above costs the publisher a drain (s_waitcnt vmcnt(0), ~1 us) per
// message; here every 8-byte word is SELF-VALIDATING instead: a double travels as two words
// {payload half (32 bit) << 32 | tag (32 bit)}, tag = the running exchange number.  An aligned 8-byte store
// is indivisible, so the consumer accepts a word exactly when its tag matches - no flag, no ordering between
// the words of a message, no drain; the publisher fires 2(V+1) lane-parallel stores and goes on.  Messages
// sit in a ring of RMT_RING entries indexed by the exchange number; the producer is never more than one
// step attempt (< RMT_RING exchanges) ahead of its consumer, because every chunk waits for the last chunk's
// accept/reject decision before the next attempt - so the ring needs no back-pressure either.  The host
// clears the rings before each launch.  Waits are bounded; a timeout raises the team's abort word, which
// every later wait sees: the launch then runs out quickly and ends with RMT_FLAG_STEP.
#ifndef RMT_RING
#define RMT_RING 512
#endif
#define RMT_LINK_WORDS (2 * (RMT_V + 1))
// the host sizes every ring with RMT_N2_RING (include/rmt_n2.h, ensure_rings in rmt_n2.cpp): a code object built with
// another depth would index past the allocation; one message is sent / polled by ONE wave, a word per lane
static_assert(RMT_RING == 512, "RMT_RING must equal RMT_N2_RING = 512, the ring depth the host library allocates");
static_assert(RMT_LINK_WORDS <= 64, "a link message is 2 (V + 1) words handled by one wave: V <= 31");
// exchange numbers run 1, 2, ... and skip 0 when they wrap: a cleared ring word carries tag 0
__device__ __forceinline__ unsigned rmt_seq_next(const unsigned s) { return (s + 1u == 0u) ? 1u : s + 1u; }
__device__ __forceinline__ unsigned long long* rmt_ring_entry(unsigned long long* ring, const unsigned seq) {
    return ring + (size_t)(seq % RMT_RING) * RMT_LINK_WORDS;
}
// one wave: lanes l < 2n send word l of the message tagged `seq` to `entry`; vals = n doubles in LDS
__device__ __forceinline__ void rmt_link_send(unsigned long long* entry, const unsigned seq,
                                              const double* vals, const int n) {
    const int l = threadIdx.x & 63;
    if (l < 2 * n) {
        const double v = vals[l >> 1];
        const unsigned half = (l & 1) ? (unsigned)__double2hiint(v) : (unsigned)__double2loint(v);
        const unsigned long long w = ((unsigned long long)half << 32) | (unsigned long long)seq;
        __hip_atomic_store(entry + l, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// one wave: lanes l < 2n poll word l of message `seq`, the doubles land in out[0..n) (LDS); returns != 0
// when the wait timed out or the team is aborting (then out[] is not meaningful)
__device__ __forceinline__ int rmt_link_recv(unsigned long long* entry, const unsigned seq, double* out,
                                             const int n, unsigned* abort_word, const int dead) {
    const int l = threadIdx.x & 63;
    int st = dead;
    unsigned half = 0u;
    if (l < 2 * n && !dead) {
        unsigned long long* word = entry + l;
        unsigned spins = 0;
        for (;;) {
            const unsigned long long w = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned)w == seq) { half = (unsigned)(w >> 32); break; }
            ++spins;
            if ((spins & 255u) == 0u &&
                __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { st = 1; break; }
            if (spins > RMT_CHAIN_SPINS) {
                __hip_atomic_store(abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                st = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    st = __any(st) ? 1 : 0;
    const unsigned hi = __shfl_down(half, 1);
    if (l < 2 * n && !(l & 1)) out[l >> 1] = __hiloint2double((int)hi, (int)half);
    return st;
}

struct RmtLocal {       // what a node's balances see of the rest of the reactor
    preal P;            // pressure at the node
    real up[RMT_V];     // clamped state of the upstream node (inlet values for node 0)
#if RMT_MODEL != 0
    real lco[RMT_V];    // d f_r / d up_r at the node (model M2: state dependent; written with the analytic Jacobian)
#endif
};

struct RmtCarry {       // workgroup-uniform hand-over between consecutive node blocks
    preal P;            // pressure at the first node of the block
    real up[RMT_V];     // clamped state of the node just upstream of the block (inlet for block 0)
#if RMT_PROFILE
    int node0;          // global index of the block's first node (12_profile.inc; callers that walk node blocks set it)
#endif
};

__device__ __forceinline__ void rmt_carry_inlet(const RmtMember& m, RmtCarry& c) {
    c.P = m.p0;
#pragma unroll
    for (int i = 0; i < RMT_S; ++i) c.up[i] = m.cin[i];                 // :4090
#if !RMT_ISO
    c.up[RMT_S] = m.theta_in;                                           // :4108
#endif
    RMT_PROFILE_AT(c, 0)
}

