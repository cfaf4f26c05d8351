// ------------------------------------------------------------------ axial profiles: catalyst activity, coolant zones
// solver-config "axial-profile" (host: rmt_app_amd/profile.py): per member and mesh node z_n = n/(N-1) the device holds the
// catalyst activity a_n and the coolant offset delta_n = Tm(z_n) - MeTe of the member, as a table [E][2][N] of doubles
// beside the member rows (rmt_n2_set_profile; 16 KB per 1024-node reactor: it stays in L2).  A code object generated with
// RMT_PROFILE 1 evaluates, in the node function (20_node_n2.inc),
//     r_q <- a_n r_q  for every reaction q (species sources AND the heat of reaction),
//     wall term  UA (tm + delta_n - T),  tm = the member field as it is at that stage (a forced coolant moves the common
//     level, the zones keep their offsets); the adiabatic switch stays tm == 0.
// RmtNode carries the two values (act, dtm); rmt_node_pre sets the identity (1, 0), a caller that knows its node overwrites
// them: rmt_rhs_block from the table - two vector loads per node at the top of every call, nothing lives across the
// stages - at the global node index carry.node0 + threadIdx.x * NPT + j, CLAMPED to [0, N-1] (lanes and nodes beyond the
// reactor's end run the node function on the inlet state); the per-lane march through the member (m.act, m.dtm).
// The upwind stencil, the Ergun recurrence and the scaling are untouched.  The chained kernels, the multistep kernel and
// the stiff stepper's four-lane layout do not carry the profile: a profiled unit does not contain them.
// A build without the define contains none of this.
#if RMT_PROFILE
#if RMT_PROFILE != 1
#error "RMT_PROFILE: 1 (catalyst activity and coolant offset per mesh node) or undefined"
#endif
#if RMT_MODEL != 0 || RMT_FP32 || RMT_MEMBER_LDS
#error "RMT_PROFILE: model N2 in fp64 with the member in registers only"
#endif
#if RMT_ROS_QUAD
#error "RMT_PROFILE: the stiff stepper carries the profile in its one-node-per-lane form only"
#endif
#if defined(RMT_UP_LDS) && RMT_UP_LDS
#error "RMT_PROFILE: not built for the LDS neighbour exchange"
#endif
#ifndef RMT_HOST_EMULATION
__device__ const double* rmt_profile_tab = nullptr;      // [E][2][N], set by the host before the first launch
__device__ __forceinline__ void rmt_profile_bind(RmtMember& m, const int e, const int N) {
    m.prof = rmt_profile_tab + (size_t)e * 2 * (size_t)N;
    m.prof_n = N;
}
#endif
// the two values of global node `node` (clamped) into its RmtNode
#define RMT_PROFILE_NODE(m, nd, node)                                                        \
    {                                                                                        \
        int pn_ = (node) < (m).prof_n - 1 ? (node) : (m).prof_n - 1;                         \
        pn_ = pn_ < 0 ? 0 : pn_;                                                             \
        (nd).act = real((m).prof[pn_]);                                                      \
        (nd).dtm = real((m).prof[(m).prof_n + pn_]);                                         \
    }
#define RMT_PROFILE_BIND(m, e, N) rmt_profile_bind(m, e, N);
#define RMT_PROFILE_AT(carry, base) (carry).node0 = (base);
#else
#define RMT_PROFILE_NODE(m, nd, node)
#define RMT_PROFILE_BIND(m, e, N)
#define RMT_PROFILE_AT(carry, base)
#endif   // RMT_PROFILE

