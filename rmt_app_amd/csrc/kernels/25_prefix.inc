// ------------------------------------------------------------------ affine maps P -> a*P + b
struct RmtAff { preal a, b; };
__device__ __forceinline__ RmtAff rmt_then(const RmtAff first, const RmtAff second) {
    RmtAff o;
    o.a = second.a * first.a;
    o.b = second.a * first.b + second.b;
    return o;
}

// ---- the cross-wave part of the pressure scan ----------------------------------------------------
// Behind the barrier of an RHS evaluation tot[w] holds the total map {a, b} of wave w (16-byte records, RmtShared).
// The pressure entering wave `wave` is p pushed through the totals of the waves before it, p = a_w p + b_w for
// w = 0 .. wave-1 in this order; every mode performs these operations and no others, so all return the same bits.
// Plain C++ without a lane or LDS intrinsic (the host compiles this file too: tests/helpers/prefix_chain_emu.cpp).
//   RMT_PREFIX_MODE 0  the plain loop over the per-lane wave index (an exec-mask loop on the device)
//                   2  the trip count made wave-uniform: a scalar loop, one LDS round trip PER RECORD before the wave
//                      may use its pressure - wave 7 of 8 waits seven times (profiles/prefix_chain.md)
//                   4  records fetched RMT_PREFIX_BATCH at a time by independent reads (one round trip per batch: at
//                      most two for 8 waves), then the dependent fmas behind wave-uniform branches.  A batch reads
//                      records its wave does not need, too: they lie inside tot[] and cost no wait of their own.
// Default: 2.  n2.code_plan writes RMT_PREFIX_MODE 4 into the defines of the one unit it was timed in, the caching
// one-workgroup RK4 stepper at 512 x 2 built without RK45 or an optional kernel family (the bench unit).
#ifndef RMT_PREFIX_MODE
#define RMT_PREFIX_MODE 2
#endif
#ifndef RMT_PREFIX_BATCH
#define RMT_PREFIX_BATCH 4
#endif
#ifdef RMT_HOST_EMULATION
#define RMT_WAVE_UNIFORM(x) (x)
#define RMT_PREFIX_TAKEN()
inline void rmt_prefix_pin(RmtAff (&)[RMT_PREFIX_BATCH], const int) {}
#else
#define RMT_WAVE_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
// keeps a wave-uniform branch a branch (if-converted, every record costs two selects on the VALU)
#define RMT_PREFIX_TAKEN() asm volatile("")
// the first n records of the batch are complete HERE, ahead of the branches, behind ONE wait: without it the compiler
// sinks each read into the branch that uses it (a round trip per record again); n is a constant of the unrolled caller
__device__ __forceinline__ void rmt_prefix_pin(RmtAff (&r)[RMT_PREFIX_BATCH], const int n) {
    static_assert(RMT_PREFIX_BATCH == 4, "written for batches of four records");
    if (n == 1) asm volatile("" :: "v"(r[0].a), "v"(r[0].b));
    if (n == 2) asm volatile("" :: "v"(r[0].a), "v"(r[0].b), "v"(r[1].a), "v"(r[1].b));
    if (n == 3) asm volatile("" :: "v"(r[0].a), "v"(r[0].b), "v"(r[1].a), "v"(r[1].b), "v"(r[2].a), "v"(r[2].b));
    if (n == 4) asm volatile("" :: "v"(r[0].a), "v"(r[0].b), "v"(r[1].a), "v"(r[1].b), "v"(r[2].a), "v"(r[2].b),
                                            "v"(r[3].a), "v"(r[3].b));
}
#endif
#define RMT_PREFIX_MIN(a, b) ((a) < (b) ? (a) : (b))

template <int MODE>
__device__ __forceinline__ preal rmt_prefix_before(const RmtAff* tot, const int wave, preal p) {
    if constexpr (MODE == 4) {
        const int wu = RMT_WAVE_UNIFORM(wave);
#pragma unroll
        for (int w0 = 0; w0 < RMT_NW - 1; w0 += RMT_PREFIX_BATCH) {
            if (wu <= w0) break;
            RmtAff r[RMT_PREFIX_BATCH];
#pragma unroll
            for (int j = 0; j < RMT_PREFIX_BATCH; ++j)
                if (w0 + j < RMT_NW - 1) r[j] = tot[w0 + j];
            rmt_prefix_pin(r, RMT_PREFIX_MIN(RMT_PREFIX_BATCH, RMT_NW - 1 - w0));
#pragma unroll
            for (int j = 0; j < RMT_PREFIX_BATCH; ++j) {
                if (w0 + j < RMT_NW - 1 && w0 + j < wu) {
                    RMT_PREFIX_TAKEN();
                    p = r[j].a * p + r[j].b;
                }
            }
        }
    } else if constexpr (MODE == 2) {
        const int wu = RMT_WAVE_UNIFORM(wave);
        for (int w = 0; w < wu; ++w) p = tot[w].a * p + tot[w].b;
    } else {
        for (int w = 0; w < wave; ++w) p = tot[w].a * p + tot[w].b;
    }
    return p;
}
// the pressure leaving the block: p, the one entering wave `wave`, pushed through the totals of waves wave .. RMT_NW-1
template <int MODE>
__device__ __forceinline__ preal rmt_prefix_from(const RmtAff* tot, const int wave, preal p) {
    if constexpr (MODE == 4) {
        const int wu = RMT_WAVE_UNIFORM(wave);
#pragma unroll
        for (int w0 = 0; w0 < RMT_NW; w0 += RMT_PREFIX_BATCH) {
            if (wu >= w0 + RMT_PREFIX_BATCH) continue;
            RmtAff r[RMT_PREFIX_BATCH];
#pragma unroll
            for (int j = 0; j < RMT_PREFIX_BATCH; ++j)
                if (w0 + j < RMT_NW) r[j] = tot[w0 + j];
            rmt_prefix_pin(r, RMT_PREFIX_MIN(RMT_PREFIX_BATCH, RMT_NW - w0));
#pragma unroll
            for (int j = 0; j < RMT_PREFIX_BATCH; ++j) {
                if (w0 + j < RMT_NW && w0 + j >= wu) {
                    RMT_PREFIX_TAKEN();
                    p = r[j].a * p + r[j].b;
                }
            }
        }
    } else if constexpr (MODE == 2) {
        const int wu = RMT_WAVE_UNIFORM(wave);
        for (int w = wu; w < RMT_NW; ++w) p = tot[w].a * p + tot[w].b;
    } else {
        for (int w = wave; w < RMT_NW; ++w) p = tot[w].a * p + tot[w].b;
    }
    return p;
}
