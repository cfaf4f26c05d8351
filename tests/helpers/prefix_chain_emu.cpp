// TEST HELPER: the cross-wave part of the pressure scan (csrc/kernels/25_prefix.inc) compiled for the host, for one
// RMT_NW (-DRMT_NW=...).  Random wave totals {a, b}; for every wave index the batched form (RMT_PREFIX_MODE 4) of
// rmt_prefix_before / rmt_prefix_from against the scalar loop (mode 2) and the plain loop (mode 0): the bits must agree.
// The totals live in a heap block of exactly RMT_NW records, so a batch that read past the last record would be an
// out-of-bounds read for AddressSanitizer.  Prints "ok <comparisons>" and returns 0, or the first difference and 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#define RMT_HOST_EMULATION 1
#define __device__
#define __forceinline__ inline
typedef double preal;
#ifndef RMT_NW
#error "compile with -DRMT_NW=<waves per workgroup>"
#endif
#include RMT_PREFIX_SOURCE

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {                       // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545f4914f6cdd1dull;
}
static double uni() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }

static bool same(const double x, const double y) { return std::memcmp(&x, &y, sizeof x) == 0; }

int main() {
    long n = 0;
    for (int trial = 0; trial < 2000; ++trial) {
        std::vector<RmtAff> heap(RMT_NW);
        RmtAff* tot = heap.data();
        // the maps of a packed bed: a just below 1, b a small pressure loss; every fourth trial of any size and sign
        const bool wide = (trial % 4) == 3;
        for (int w = 0; w < RMT_NW; ++w) {
            tot[w].a = wide ? (uni() - 0.5) * 4.0 : 1.0 - 1e-3 * uni();
            tot[w].b = wide ? (uni() - 0.5) * 1e3 : -1e-2 * uni();
        }
        const double p = wide ? (uni() - 0.5) * 1e2 : 1.0 + 49.0 * uni();
        for (int wave = 0; wave < RMT_NW; ++wave) {
            const double b4 = rmt_prefix_before<4>(tot, wave, p), b2 = rmt_prefix_before<2>(tot, wave, p),
                         b0 = rmt_prefix_before<0>(tot, wave, p);
            const double f4 = rmt_prefix_from<4>(tot, wave, p), f2 = rmt_prefix_from<2>(tot, wave, p),
                         f0 = rmt_prefix_from<0>(tot, wave, p);
            if (!same(b4, b2) || !same(b4, b0) || !same(f4, f2) || !same(f4, f0)) {
                std::printf("differs: RMT_NW %d trial %d wave %d before %a %a %a from %a %a %a\n", RMT_NW, trial, wave,
                            b4, b2, b0, f4, f2, f0);
                return 1;
            }
            // the chain itself: entering the block at p, leaving wave `wave` and going on from there is the whole block
            if (wave + 1 < RMT_NW) {
                const double whole = rmt_prefix_from<4>(tot, 0, p);
                const double split = rmt_prefix_from<4>(tot, wave + 1, rmt_prefix_before<4>(tot, wave + 1, p));
                if (!same(whole, split)) {
                    std::printf("split differs: RMT_NW %d trial %d wave %d %a %a\n", RMT_NW, trial, wave, whole, split);
                    return 1;
                }
            }
            n += 4;
        }
    }
    std::printf("ok %ld\n", n);
    return 0;
}
