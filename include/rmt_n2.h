/*
 * rmt_n2.h - C ABI of the MI355X-native integrator for PyREMOT's dynamic packed-bed model "N2".
 *
 * The reference (sinagilassi/rmt-app, pure Python) has no FFI; its boundary for this path is the
 * Python-level contract listed in SURVEY.md section 8(b).  Each entry point below names the
 * reference interface it replaces (paths relative to the reference repo):
 *
 *   rmt_n2_compile      - (new) lowers nothing itself: turns the host-generated kernel source
 *                         (lowered `reaction-rates` lambdas + mechanism tables) into a gfx950 code
 *                         object.  Replaces the per-call Python evaluation of the lambdas in
 *                         reactionRateExe, PyREMOT/docs/rmtReaction.py:11-61.
 *   rmt_n2_create       - the setup half of PackedBedHomoReactorClass.runN2,
 *                         PyREMOT/docs/pbHomoReactor.py:3334-3580 (paramsSet construction): takes
 *                         the packed per-reactor constants instead of nested dicts.
 *   rmt_n2_rhs          - PackedBedHomoReactorClass.modelEquationN2(t, y, paramsSet),
 *                         PyREMOT/docs/pbHomoReactor.py:3706-4134 (one RHS evaluation).
 *   rmt_n2_rk4          - RK4(t0, tn, n, y0, f, params), PyREMOT/solvers/odeSolver.py:17-40, as used
 *                         from the `ivp == "AM"` plug point pbHomoReactor.py:3598-3607 (only the
 *                         last column - the end state - is produced, which is all runN2 keeps,
 *                         :3630, :3685).
 *   rmt_n2_multistep    - AdBash3 / PreCorr3, PyREMOT/solvers/odeSolver.py:43-102; PreCorr3 is what
 *                         runN2 calls for ivp == "AM" (pbHomoReactor.py:3598-3601).
 *   rmt_n2_rk45         - scipy.integrate.solve_ivp(funSet, t, IV, method=..., args=(paramsSet,))
 *                         at pbHomoReactor.py:3609-3610, restricted to an explicit embedded pair
 *                         (Dormand-Prince 5(4)) with per-reactor step control.
 *   rmt_n2_ros4         - the same solve_ivp call site with a STIFF method (the reference's default is
 *                         LSODA, pbHomoReactor.py:3576): linearly-implicit Rosenbrock method RODAS4
 *                         (6 stages, order 4(3), L-stable; Hairer & Wanner) with per-reactor step
 *                         control; SURVEY.md section 8(f) rank 2.  Also integrates model M2
 *                         (pbReactor.py:719) when the code object was generated for it.
 *   rmt_n1_profile      - PackedBedHomoReactorClass.runN1 / modelEquationN1 (pbHomoReactor.py:2694-3314):
 *                         the steady-state model N1, integrated along z* for E reactors at once
 *                         (one per lane) with the same Rosenbrock scheme; SURVEY.md 8(f) rank 1.
 *                         Models M7 / M1 (PackedBedReactorClass.runM3 / runM1, pbReactor.py:1170-1575, 141-547)
 *                         use it too, with code objects generated for them (RMT_SS_MODEL).
 *   (model M2)          - PackedBedReactorClass.runM2 / modelEquationM2 (pbReactor.py:552-1165) uses the
 *                         SAME entry points: the generated prelude selects its node functions
 *                         (RMT_MODEL 2), state rows are kmol/m^3 and K; SURVEY.md 8(f) rank 3.
 *   rmt_n2_status       - the exceptions Python raises inside the user lambdas / `raise` at
 *                         pbHomoReactor.py:3614-3626, as per-reactor flag words.
 *
 * Conventions: every function returns 0 on success, non-zero on error (rmt_n2_last_error() gives
 * a thread-local message).  `y`, `dydt` and `flags` are DEVICE pointers owned by the caller;
 * plan contents are HOST memory, copied during rmt_n2_create.  Work is enqueued on the stream set
 * with rmt_n2_set_stream (default: the null stream) and is NOT synchronised by these calls.
 * State layout: y[E][V][N] = the reference's row-major flattening of the (V, N) matrix
 * (pbHomoReactor.py:3483-3497, 3873) for each of E independent reactors; V = S (+1 unless
 * iso-thermal); real = double, or float when the code object was generated with fp32.
 * A handle is bound to the device that was current at create time; handles are not thread-safe,
 * distinct handles are independent.  No global state besides the last-error string.
 */
#ifndef RMT_N2_H
#define RMT_N2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMT_N2_ABI_VERSION 2

/* status bits written by the kernels (OR-ed per reactor) */
#define RMT_N2_FLAG_DOMAIN 1u    /* Python: ValueError("math domain error")          */
#define RMT_N2_FLAG_DIV0 2u      /* Python: ZeroDivisionError                         */
#define RMT_N2_FLAG_OVERFLOW 4u  /* Python: OverflowError("math range error")         */
#define RMT_N2_FLAG_NONFINITE 8u /* a state/derivative became NaN or Inf              */
#define RMT_N2_FLAG_STEP 16u     /* rk45: step size underflow / max steps exceeded    */
#define RMT_N2_FLAG_PRESSURE 32u /* model M2: Newton sweeps of the pressure march did not converge */
/* Contract of the three Python-exception bits: the explicit steppers test the conditions on which the
 * reference's lambdas would raise on the FIRST stage of every step (f(y_n)); an exception that exists
 * only at a trial-stage state surfaces as RMT_N2_FLAG_NONFINITE when it poisons the state (the lean
 * fp64 division and exp of the kernels turn an intermediate inf into NaN - 1/(1+inf) is NaN, not 0 - so
 * the usual ways of mapping an overflow back to a finite rate do poison it).  Code objects
 * generated with RMT_CHECK_ALL_STAGES=1 (solver-config "strict-flags") test every stage.
 * Dynamic range of the generated rate laws (fp64 code objects without a node Jacobian): divisions whose
 * denominators do not depend on each other share ONE reciprocal, of the product of up to four denominators
 * (rmt_app_amd/lowering.py div_groups).  That product can overflow or underflow where each quotient alone
 * would not (four denominators near 1e-80, say).  The device reciprocal refines v_rcp_f64 by Newton steps,
 * which turn the reciprocal of an overflowed (inf) or underflowed (0) product into NaN: the rates are then
 * non-finite and the reactor ends in RMT_N2_FLAG_NONFINITE instead of carrying a wrong number; the
 * division-by-zero test still runs on every denominator itself.  This holds for that reciprocal only: a plain
 * 1.0/b gives 0 for an overflowed product, so the rates can come out finite and wrong without a flag - the
 * case of the host emulation of the generated source (oracle/hostemu.py), which mirrors the default emission.
 * Code objects built with RMT_FAST_MATH=0 and fp32 code objects (v_rcp_f32, no Newton step, range 1e+-38)
 * never share reciprocals.  The generator switch RMT_DIV_BATCH=0 (a define handed to
 * plan.Mechanism.source; the kernel source does not read it) keeps one reciprocal per division everywhere.
 * Product species clamped at 1e-30, the start of a reactor fed without products, give a product near 1e-52:
 * far inside the fp64 range.
 * Every entry point taking a handle runs on the device that was current at rmt_n2_create and
 * restores the caller's current device before returning. */

/* chained steppers (rmt_n2_ros4 / rmt_n2_rk45 / rmt_n2_rk4 with one reactor over several CUs): ring depth of a tagged-word link
 * (= RMT_RING of csrc/kernels/30_lanes_links.inc) and the largest number of chunks one reactor is cut into */
#define RMT_N2_RING 512
#define RMT_N2_MAX_CHUNKS 64

/* member row layout: doubles per reactor = 16 + S + NU (see rmt_app_amd/csrc/kernels/00_config_math.inc M_*):
 * 16 fixed operating-point scalars, S inlet values, then the NU = plan.n_user_params scalar constants of the
 * user's reaction-rates.VARS that differ between the reactors of the ensemble (the reference copies VARS into
 * the rate lambdas' namespace on every call, PyREMOT/docs/rmtReaction.py:44-51; the generated kinetics read
 * them as U[k]) */
#define RMT_N2_MEMBER_FIXED 16

typedef struct rmt_n2_plan {
    int32_t abi_version;     /* RMT_N2_ABI_VERSION */
    int32_t n_species;       /* S */
    int32_t n_reactions;     /* R (informational) */
    int32_t n_vars;          /* V = S or S+1 */
    int32_t n_nodes;         /* N (zNo) */
    int32_t n_members;       /* E */
    int32_t fp32;            /* 1: real = float */
    int32_t block;           /* RMT_BLOCK the code object was generated with */
    int32_t nodes_per_thread;/* RMT_NPT the code object was generated with */
    int32_t n_user_params;   /* NU (RMT_NU of the code object; 0 = every VARS constant is a literal of the kernel) */
    int32_t ros4_nodes_per_block; /* mesh nodes one workgroup of the stiff stepper covers: 0 = `block` (one node per lane);
                              * block / 4 for code objects generated with RMT_ROS_QUAD (one node on four lanes, the
                              * layout for mechanisms wider than 8 variables, kernels/61_ros4_quad.inc) */
    int32_t profiled;        /* 1: the code object was generated with RMT_PROFILE (solver-config "axial-profile": catalyst
                              * activity and coolant offset per mesh node, kernels/12_profile.inc) and every launch needs
                              * the table of rmt_n2_set_profile; 0: none (the field was `reserved`, always 0) */
    const void* code_object; /* gfx950 code object from rmt_n2_compile (host memory) */
    size_t code_size;
    const double* members;   /* host [E][16+S+NU] packed constants */
} rmt_n2_plan;

typedef struct rmt_n2_handle rmt_n2_handle;

typedef struct rmt_n2_stats {   /* per reactor, written by rmt_n2_rk45 (device memory) */
    double t_end;
    double h_last;
    int64_t accepted;
    int64_t rejected;
} rmt_n2_stats;

/* hipRTC: source text -> code object for `arch` (e.g. "gfx950"); works without a GPU.
 * *code is malloc'ed (free with rmt_n2_free); *log (may be NULL) receives the compiler log. */
int rmt_n2_compile(const char* source, const char* arch, const char* extra_opts, void** code,
                   size_t* code_size, char** log);
void rmt_n2_free(void* p);
/* the device template that rmt_n2_compile expects to follow the generated prelude */
const char* rmt_n2_kernel_template(void);
/* path of the hipRTC library this process compiles with (a process that loaded PyTorch first uses the one
 * PyTorch bundles, otherwise /opt/rocm's; both report version 9.0 but generate different code): part of the key
 * of any code-object cache */
const char* rmt_n2_hiprtc_path(void);
/* the options rmt_n2_compile adds to every compilation besides --offload-arch and `extra_opts` (an `extra_opts`
 * that sets -mllvm ...machine-licm... itself replaces the default of that switch): the other part of a cache key */
const char* rmt_n2_compile_options(void);

int rmt_n2_create(const rmt_n2_plan* plan, rmt_n2_handle** out);
void rmt_n2_destroy(rmt_n2_handle* h);
int rmt_n2_set_stream(rmt_n2_handle* h, void* hip_stream);
/* replace the per-member constants (same E) without recompiling; fields that the code object's
 * prelude baked in as literals (#define RMT_MC_<FIELD>) are not affected */
int rmt_n2_set_members(rmt_n2_handle* h, const double* members);
/* the same, stream-ordered and without waiting: the copy is queued on the handle's stream between the launches around
 * it, `members` must be page-locked host memory that stays untouched until the stream has passed the copy.  Forced code
 * objects (prelude #define RMT_FORCING 1, solver-config "schedule") have their rows refreshed this way before every
 * launch: such a row is 16 + S + NU + 4 doubles - the plan's n_user_params counts the four extra ones - the ordinary
 * fields P0, THETA_IN and TM hold the values at the start of the launch and the tail {t_ref, d THETA_IN/dt, d P0/dt,
 * d TM/dt} the time of that start and the slopes over the launch (kernels/11_forcing.inc). */
int rmt_n2_set_members_async(rmt_n2_handle* h, const double* members_pinned);

/* Axial profiles (handles created with plan.profiled = 1 only; on any other handle this is an error): `table_host` is
 * [E][2][N] doubles, per member first the N catalyst activities a_n >= 0, then the N coolant offsets delta_n [K], for the
 * mesh nodes z_n = n/(N-1).  The node function of such a code object multiplies every reaction rate of node n by a_n and
 * uses the coolant temperature Tm = tm + delta_n in its wall term, where tm is the member field M_TM as it is at that
 * stage (a forced coolant moves the common level, the zones keep their offsets; tm == 0 stays the adiabatic switch).
 * ONE synchronous upload into a buffer the handle owns (freed by rmt_n2_destroy), to be made before the first launch; it
 * is not on the launch path.  Until it has been made every launch entry point of a profiled handle returns an error
 * instead of launching.  A profiled code object has no chained kernels and no multistep kernel. */
int rmt_n2_set_profile(rmt_n2_handle* h, const double* table_host);

int rmt_n2_rhs(rmt_n2_handle* h, double t, const void* y, void* dydt);
int rmt_n2_rk4(rmt_n2_handle* h, void* y_inout, double t0, double dt, int64_t nsteps);
/* method: 0 = AdBash3, 1 = PreCorr3 (needs nsteps >= 3, like the reference) */
int rmt_n2_multistep(rmt_n2_handle* h, void* y_inout, double t0, double dt, int64_t nsteps, int method);
/* h0 > 0: first step of every reactor.  h0 < 0: "resume" - every reactor starts from the h_last
 * its previous launch left in stats_out[e] (|h0| where that is not a positive finite number);
 * h_last is the controller's proposal for the step AFTER t1 (a last step clipped to t1 does not
 * shrink it), so consecutive output intervals chain without a restart transient. */
int rmt_n2_rk45(rmt_n2_handle* h, void* y_inout, double t0, double t1, double rtol, double atol,
                double h0, int64_t max_steps, rmt_n2_stats* stats_out);
int rmt_n2_ros4(rmt_n2_handle* h, void* y_inout, double t0, double t1, double rtol, double atol,
                double h0, int64_t max_steps, rmt_n2_stats* stats_out);
/* (tuning experiments: the environment variable RMT_N2_ROS4_CHUNKS=c overrides the number of chunks rmt_n2_ros4 cuts a
 * reactor into, 1 = one workgroup per reactor; unset = the library's estimate) */
/* members1: HOST [E][16+S+NU] rows (layout M1_* in csrc/kernels/22_node_n1.inc); out: DEVICE double [E][nout][S+2]
 * (S+1 when iso-thermal) = the state at z* = k/(nout-1); stats: DEVICE [E].
 * The same entry point drives any steady module: a code object generated with RMT_SS_MODEL 7 (model M7, runM3) or 1
 * (model M1, runM1) reads rows of the same width in its own layout (csrc/kernels/23_node_steady.inc) and writes
 * [E][nout][V1] scaled states, V1 = S+2 (M7) or S+3 (M1). */
int rmt_n1_profile(rmt_n2_handle* h, const double* members1, void* out, int nout, double rtol,
                   double atol, double h0, int64_t max_steps, rmt_n2_stats* stats_out);
/* Steady state of model N2 (solver-config "initial": "steady"): y_out DEVICE double [E][V][N] receives, per member, the
 * state with f(y) = 0 for the member's rows as they are on the device (a forced row: its values at the row's reference
 * time).  The discrete steady state is block lower-bidiagonal (first-order upwind, downstream Ergun recurrence), so one
 * lane marches one reactor from the inlet and solves a V x V system per node by pseudo-transient continuation with the
 * analytic node Jacobian (csrc/kernels/71_steady_march.inc).  A node is converged when its scaled residual
 * max_i |f_i| / (F1 (N-1) max(|y_i|, 1e-6)) is at most `tol` and so is its last relative update (or three updates in a
 * row are, at steps no shorter than the cell's residence time: the residual is at the noise of its evaluation); `max_iter`
 * bounds the pseudo-time steps per node.  Enqueues ONE kernel on the handle's stream and does not synchronise; needs a code object
 * generated with RMT_WITH_MARCH (fp64, model N2), else it returns an error.  stats_out DEVICE [E]: t_end = the worst
 * node's scaled residual, h_last = the node that failed (-1: none), accepted = the largest per-node step count,
 * rejected = the number of nodes that needed a rejected step.  A member whose march fails (a node at max_iter, a
 * non-finite state, a zero pivot) gets RMT_N2_FLAG_STEP / RMT_N2_FLAG_NONFINITE and keeps the input downstream of it. */
int rmt_n2_steady_march(rmt_n2_handle* h, void* y_out, double tol, int64_t max_iter, rmt_n2_stats* stats_out);
/* Parametric sensitivities of that steady state (solver-config "sensitivity", csrc/kernels/73_sensitivity.inc): y DEVICE
 * double [E][V][N] is the converged state rmt_n2_steady_march left, out DEVICE double [E][n_params][V+1][N] receives per
 * member and parameter the rows d y_v,z / dp (v < V, in the scaled units of the state) and d P_z / dp (row V).  The
 * parameters are values of the member's device row: kinds[p] = 0 TM, 1 THETA_IN, 2 P0 (indices[p] = 0), 3 CIN[indices[p]],
 * 4 the user column indices[p]; kinds and indices are HOST arrays of n_params ints, 1 <= n_params <= 8.  All derivatives
 * are analytic (the tangent system of the block lower-bidiagonal steady state is a downstream march as well: one V x V
 * inverse per node, applied to every right-hand side).  Needs a code object generated with RMT_SENS 1 and
 * RMT_SENS_NP == n_params beside RMT_WITH_MARCH, else it returns an error (a mismatch of n_params that only the kernel
 * can see flags every member).  Enqueues ONE kernel on the handle's stream and does not synchronise.  A member with a
 * singular node gets RMT_N2_FLAG_NONFINITE and NaN in its rows at that node; the nodes behind it are not written. */
int rmt_n2_steady_sens(rmt_n2_handle* h, const void* y, int n_params, const int* kinds, const int* indices, double* out);
/* Frequency response of that steady state (solver-config "frequency-response", csrc/kernels/74_frequency.inc): for a
 * harmonic disturbance exp(i w t) of a value of the member's device row the linearised dynamic model answers with
 * s exp(i w t), (a_z + i w I) s_z = U D s_(z-1) + (df/dP) pi_z + df/dp - the tangent march of rmt_n2_steady_sens with a
 * complex shift, one (member, frequency) pair per lane; w = 0 gives the sensitivities.  y DEVICE double [E][V][N] (the
 * converged state); kinds / indices HOST arrays of n_inputs ints as for rmt_n2_steady_sens, kinds 0..3 only,
 * 1 <= n_inputs <= 4; omegas_host HOST [n_freq] doubles >= 0 in radians per unit of the right-hand side's time,
 * 1 <= n_freq <= 4096; peak_nodes_host HOST [E] ints: the node whose rows are returned beside the outlet's (a node outside
 * 0..N-1: none).  out_host HOST doubles, complex numbers as (re, im) pairs, in the scaled units of the state per unit of
 * the row value, row V = d P_z:
 *   [E][n_freq][n_inputs][2][V+1][2]      the rows of the outlet node (slot 0) and of the member's peak node (slot 1)
 *   [E][n_freq][n_inputs][V+1][N][2]      every node - only with profile != 0, else this part is absent
 *   [E][n_freq]                           the node at which the lane stopped (-1: none), as a double
 * Needs a code object generated with RMT_FREQ 1 and RMT_FREQ_NP == n_inputs beside RMT_SENS and RMT_WITH_MARCH, else it
 * returns an error.  Uploads, enqueues ONE kernel on the handle's stream, copies back and synchronises.  A lane with a
 * singular or non-finite node sets RMT_N2_FLAG_NONFINITE on its member, writes NaN at that node (and into both slots) and
 * stops there. */
int rmt_n2_steady_freq(rmt_n2_handle* h, const void* y, int n_inputs, const int* kinds, const int* indices, int n_freq,
                       const double* omegas_host, const int* peak_nodes_host, int profile, double* out_host);
/* Time-on-stream campaigns (solver-config "deactivation", csrc/kernels/72_campaign.inc): the bed is quasi-steady, its
 * catalyst activity a_n follows da_n/dt = -k_d(T_n) (a_n - a_inf)^m, k_d(T) = k_ref exp(-(Ed/R)(1/T - 1/Tref)), T_n the
 * node's temperature in kelvin (the member's inlet temperature in an iso-thermal run).  The three calls need a handle whose
 * code object holds rmt_n2_campaign_step (generated with RMT_CAMPAIGN, RMT_WITH_MARCH and RMT_PROFILE; plan.profiled = 1)
 * and whose profile table has been set (rmt_n2_set_profile: the fresh bed's activities and the coolant offsets); the
 * second and third also a law.  Otherwise they return an error and rmt_n2_last_error names the function.
 *  rmt_n2_set_campaign_law   law_host HOST [E][5] doubles {k_ref [1/s] > 0, Ed [J/mol] >= 0, Tref [K] > 0, m >= 1,
 *                            0 <= a_inf < 1} per member; one blocking upload.
 *  rmt_n2_campaign_step      ONE march of every member with the activities as they are in the handle's table (the kernel
 *                            shape and the node solver of rmt_n2_steady_march, every node started from its converged
 *                            upstream state), and at every converged node a_n <- the law's exact solution over `dt`
 *                            seconds at that node's temperature, in place in the table.  dt = 0 changes no a_n (bit for bit).
 *                            y DEVICE double [E][V][N] receives the marched state; log_row DEVICE [E][V+6] doubles = {the
 *                            outlet state [V], peak theta, its node, mean and minimum of the activities the march read,
 *                            worst scaled node residual, largest per-node step count}; stats as rmt_n2_steady_march, and so
 *                            are a failed member's flags - it keeps its activities from the failed node on.  Enqueues ONE
 *                            kernel on the handle's stream and synchronises nothing.
 *  rmt_n2_get_profile        the handle's table as it is now into HOST [E][2][N] doubles; synchronises the stream. */
int rmt_n2_set_campaign_law(rmt_n2_handle* h, const double* law_host);
int rmt_n2_campaign_step(rmt_n2_handle* h, void* y, double dt, double tol, int64_t max_iter, double* log_row,
                         rmt_n2_stats* stats_out);
int rmt_n2_get_profile(rmt_n2_handle* h, double* table_host);
/* Constant-yield operation of a campaign (solver-config "deactivation" "policy", csrc/kernels/72_campaign.inc under
 * RMT_CAMPAIGN_POLICY): per member and step the common coolant level T [K] (the member field TM; the zones of the profile
 * table keep their offsets) is moved within [lo, hi] so that the outlet mole fraction of one component equals a target -
 * a bracketing root-find (the limits, the carried level, Illinois regula falsi) in which every function value is a whole
 * march, all inside ONE kernel, one reactor per lane.  The three calls need what the campaign's calls need - the table and
 * the law - and a code object that also holds rmt_n2_campaign_policy_step (generated with RMT_CAMPAIGN_POLICY beside
 * RMT_CAMPAIGN); the second and third also the policy.  Otherwise they return an error naming the function.
 *  rmt_n2_set_campaign_policy   rows_host HOST [E][4] doubles {target in (0, 1), lo, hi [K] with 0 < lo <= hi, tolerance > 0
 *                               (absolute, on the mole fraction)}, `component` the index of the held species, levels_host
 *                               HOST [E] the levels step 0 carries in (within the member's limits); one blocking upload.
 *  rmt_n2_campaign_policy_step  as rmt_n2_campaign_step, with the root-find around the march: y, log_row and stats
 *                               describe the march at the accepted level, which is always the last one marched, and the
 *                               activities move over `dt` at the temperatures of that state.  policy_row DEVICE [E][4]
 *                               doubles = {accepted level [K], held mole fraction, marches of this step, saturated: -1 at
 *                               lo, 0 inside, +1 at hi}.  No sign change between the limits: the limit with the smaller
 *                               |r| is accepted (a tie: lo).  A member whose bracket falls below 1e-9 K with |r| above
 *                               the tolerance (the outlet jumps there: a node changed branch) gets
 *                               RMT_N2_FLAG_POLICY_BRACKET and policy_row[3] = 2, one that reaches `max_evaluations`
 *                               (>= 4) marches RMT_N2_FLAG_POLICY_EVALS and 3; like a member whose node solve fails in
 *                               any march they keep their activities and their carried level.  ONE kernel, nothing is
 *                               synchronised.
 *  rmt_n2_get_campaign_level    the carried levels as they are now into HOST [E] doubles; synchronises the stream. */
#define RMT_N2_FLAG_POLICY_BRACKET 64u
#define RMT_N2_FLAG_POLICY_EVALS 128u
int rmt_n2_set_campaign_policy(rmt_n2_handle* h, const double* rows_host, int component, const double* levels_host);
int rmt_n2_campaign_policy_step(rmt_n2_handle* h, void* y, double dt, double tol, int64_t max_iter, int max_evaluations,
                                double* log_row, double* policy_row, rmt_n2_stats* stats_out);
int rmt_n2_get_campaign_level(rmt_n2_handle* h, double* levels_host);
/* copies the E flag words to host memory (synchronises the stream) and clears them on device */
int rmt_n2_status(rmt_n2_handle* h, uint32_t* flags_host);
/* which stepper rmt_n2_rk4 / rk45 / ros4 use: 0 = auto (on-chip if N fits one workgroup, else chained
 * workgroups - rk45: code objects that hold the on-chip stepper, at most RMT_N2_MAX_CHUNKS chunks of
 * block*nodes_per_thread nodes - else memory; ros4: one workgroup per reactor unless cutting the reactors
 * into chunks on several CUs, the teams working through the ensemble in rounds, is estimated to be faster),
 * 1 = on-chip single workgroup, 2 = one workgroup per reactor with the state in memory, 3 = chained workgroups */
int rmt_n2_set_mode(rmt_n2_handle* h, int mode);
/* how the last rk4 / rk45 / ros4 launch was laid out: workgroups (chunks) per reactor - 1 = one workgroup per reactor -
 * and the number of teams that worked through the ensemble (= E when every reactor had its own workgroup) */
int rmt_n2_last_geometry(rmt_n2_handle* h, int* chunks, int* teams);
/* Code objects whose on-chip RK4 steppers cache the temperature-only rate constants between the stages of a step
 * (kernels/50_rk4.inc) integrate a reactor whose temperature moved out of the cache's range during a launch again with
 * the plain stepper, inside the same rmt_n2_rk4 call (results are those of the plain stepper; the cost is that launch
 * twice).  How many reactor-launches that has happened to since rmt_n2_create (0 for every other code object);
 * synchronises the handle's stream. */
int rmt_n2_fallbacks(rmt_n2_handle* h, uint64_t* count);
/* timing of the last rk4/rk45/rhs launch in ms (HIP events on the handle's stream; synchronises) */
int rmt_n2_last_kernel_ms(rmt_n2_handle* h, float* ms);

/* Monitor (solver-config "monitor"): per state row y[e][v][0..N) the numbers a time series needs, reduced on the device,
 *   out[e][v][0..5) = { y[N-1], max_n y, argmax_n y (as double), min_n y, max_n |dydt| (0.0 when dydt is NULL) }.
 * Comparisons are plain > and <: a NaN entry never wins, ties resolve to the lowest node index.  The kernels are a
 * translation unit of their own (csrc/monitor_kernels.inc), independent of any mechanism: compile
 * rmt_n2_monitor_source() with rmt_n2_compile, load it with rmt_n2_monitor_create on the current device.  The object is
 * independent of rmt_n2_handle.  rmt_n2_monitor_reduce enqueues ONE kernel on `hip_stream` and does not synchronise;
 * y / dydt are DEVICE [E][V][N] reals (float when fp32), out DEVICE [E][V][5] doubles. */
const char* rmt_n2_monitor_source(void);
typedef struct rmt_n2_monitor rmt_n2_monitor;
int rmt_n2_monitor_create(const void* code, size_t size, rmt_n2_monitor** out);
void rmt_n2_monitor_destroy(rmt_n2_monitor* m);
int rmt_n2_monitor_reduce(rmt_n2_monitor* m, void* hip_stream, const void* y, const void* dydt_or_null,
                          int E, int V, int N, int fp32, double* out);
/* how the last reduce was laid out: rows per workgroup - 4 = one wave per row (short rows, or rows enough to fill the
 * device with waves), 1 = one workgroup per row (a few long rows); 0 before any */
int rmt_n2_monitor_last_rows_per_block(const rmt_n2_monitor* m);

/* Controller (solver-config "control"): a sampled PI controller per member, evaluated on the device between two launches
 * of a stepper (csrc/control_kernels.inc, a translation unit of its own, independent of any mechanism: compile
 * rmt_n2_control_source() with rmt_n2_compile and the option -ffp-contract=off - the law is then reproducible bit for bit
 * on the host - and load it with rmt_n2_control_create on the current device).
 * rmt_n2_control_update enqueues ONE kernel (rmt_n2_control_update_f64, one wave per member) on the stream of `h`, behind
 * whatever refreshed the member rows and ahead of the next stepper launch, and does not synchronise.  `h` is the N2 handle
 * whose DEVICE member rows are written - it must come from a forced code object (RMT_FORCING 1 or 2, fp64) whose rows
 * carry their tail {t_ref, three slopes, ...} at index `tail_at` (16 + S + the mechanism's own parameters).
 *   y        DEVICE [E][V][N] doubles, the state at the sample time (E = the handle's members; V and N are arguments: the
 *            kernel only reads y)
 *   params   DEVICE [E][8] doubles {Kp, Kp*Ts/Ti (0: P only), u0, lo, hi, selector, species index, 0}; selector 0 = outlet
 *            temperature, 1 = peak temperature, 2 = outlet mole fraction of the species
 *   setpoint DEVICE [E] doubles, r(t_k) of this sample
 *   state    DEVICE [E][3] doubles {I, u, samples taken}, zero before the first sample
 *   log      DEVICE [E][4] doubles {pv, r, u, saturated (0.0 / 1.0)}: this sample's slice of the caller's log
 *   field    0 / 1 / 2 = inlet temperature (THETA_IN = (u - Tf)/Tf) / inlet pressure (P0 = u) / medium temperature (TM = u);
 *            the slope of that field in the row's tail becomes 0
 *   hold     non-zero: only the held u (state[1]) is written into the rows again (behind a refresh that uploaded whole
 *            rows); y, setpoint and log may be NULL and nothing else changes; members not sampled yet keep their rows
 * Law: e = r - pv; I' = I + (Kp*Ts/Ti)*e; v = u0 + Kp*e + I'; u = min(max(v, lo), hi); I = I' only if v == u. */
const char* rmt_n2_control_source(void);
typedef struct rmt_n2_control rmt_n2_control;
int rmt_n2_control_create(const void* code, size_t size, rmt_n2_control** out);
void rmt_n2_control_destroy(rmt_n2_control* c);
/* the DEVICE member rows of `h` as they are now ([E][16 + S + n_user_params] doubles into host memory; synchronises the
 * handle's stream): what the last rmt_n2_set_members* uploaded and rmt_n2_control_update wrote since */
int rmt_n2_get_members(rmt_n2_handle* h, double* members);
int rmt_n2_control_update(rmt_n2_control* c, rmt_n2_handle* h, const double* y, int V, int N, const double* params,
                          const double* setpoint, double* state, double* log, int tail_at, int field, int hold);

/* Fit (solver-config "fit"): kinetic parameter estimation from steady-state data - the reduction over the experiments and
 * one Levenberg-Marquardt step on the device, between rmt_n2_steady_sens of one iteration and rmt_n2_steady_march of the
 * next (csrc/fit_kernels.inc, a translation unit of its own, independent of any mechanism: compile rmt_n2_fit_source()
 * with rmt_n2_compile and the option -ffp-contract=off - both kernels are then reproducible on the host - and load it with
 * rmt_n2_fit_create on the current device).
 * rmt_n2_fit_step enqueues TWO kernels on the stream of `h` and does not synchronise.  `h` is an N2 handle of the
 * sensitivity unit (rmt_n2_steady_march and rmt_n2_steady_sens in one code object, fp64) whose members are the experiments
 * and whose per-reactor inputs hold the fitted constants; S, V, N must be the handle's.
 *   y         DEVICE [E][V][N] doubles, the marched state
 *   sens      DEVICE [E][n_params][V+1][N] doubles as rmt_n2_steady_sens wrote it for the fitted columns (kind 4)
 *   stats     DEVICE [E] the march's statistics: a member with h_last >= 0 (a failed node) counts as failed
 *   columns   HOST n_params ints, 1 <= n_params <= 8: the user column of each fitted constant
 *   meas      DEVICE [E][MQ][3] doubles {code, value, weight = 1/sigma}; code = a species index (outlet mole fraction), S
 *             (outlet temperature, K), S+1 (peak temperature, K); entries with weight 0 are padding; 1 <= MQ <= 64
 *   pred      DEVICE [E][MQ] doubles, receives the predictions (0 at a padded entry)
 *   contrib   DEVICE [E][46] doubles, receives per experiment {C = 1/2 sum r^2, g = J^T r [8], the upper triangle of J^T J
 *             row by row [36], failed (1.0: the march failed or a number is not finite)}, r = (pred - value) weight
 *   state     DEVICE [80] doubles, zero before the first call: {started, C_cur, lambda, nu, converged, passes, status,
 *             predicted reduction, p_cur[8], p_trial[8], g_cur[8], H_cur[36], delta[8], reserved[4]}
 *   log_slice DEVICE [68] doubles, this call's slice of the caller's log: {C_trial, C_cur, lambda, nu, accepted, converged,
 *             failed experiments, status, p_trial[8] (what the rows now hold), p_cur[8], g[8], H[36] (this pass's sums)}
 * The kernel rmt_n2_fit_residuals_f64, one wave per experiment, writes pred and contrib; rmt_n2_fit_update_f64, one workgroup, sums
 * the 46 columns over the experiments in index order - no atomics, the sums do not depend on the launch geometry - and
 * evaluates the law: the first call sets the current point from the columns of member 0 (status 1 when an experiment
 * failed there); a trial is accepted when its cost is finite, no experiment failed and it is below C_cur; on accept
 * lambda <- lambda max(1/3, 1 - (2 rho - 1)^3), nu = 2 with rho = (C_cur - C_trial) / (1/2 delta^T (lambda D delta - g)), on
 * reject lambda <- lambda nu, nu <- 2 nu; (H + lambda D) delta = -g by Cholesky, D = diag(H) floored at 1e-300, on a pivot
 * that is not positive lambda <- 10 lambda at most 8 times, then status 2; converged when max_j |delta_j| / max(|p_j|, 1e-300)
 * <= tolerance or C_cur == 0.  The trial values p_cur + delta are written into the columns 16 + S + columns[j] of EVERY
 * member's device row.  Converged (or with a status): p_trial = p_cur and later calls change nothing but pred, contrib and
 * their log slice. */
const char* rmt_n2_fit_source(void);
typedef struct rmt_n2_fit rmt_n2_fit;
int rmt_n2_fit_create(const void* code, size_t size, rmt_n2_fit** out);
void rmt_n2_fit_destroy(rmt_n2_fit* f);
int rmt_n2_fit_step(rmt_n2_fit* f, rmt_n2_handle* h, const double* y, const double* sens, const rmt_n2_stats* stats, int S,
                    int V, int N, int n_params, const int* columns, const double* meas, int MQ, double* contrib,
                    double* pred, double* state, double* log_slice, double tolerance, double damping0);
/* rmt_n2_fit_step with log-scaled and bounded parameters and measurements along the bed: the sibling kernels
 * rmt_n2_fit_residuals_ex_f64 and rmt_n2_fit_update_ex_f64 of the same translation unit (rmt_n2_fit_create loads all four).
 * Every argument of rmt_n2_fit_step with the same meaning and the same checks, except
 *   meas      two more codes: S+2 the temperature (K), S+3+i the mole fraction of species i, at the entry's position
 *   log_slice DEVICE [70] doubles: the 68 of rmt_n2_fit_step, then the parameters of the current point that sit on their
 *             lower / on their upper bound with the gradient pushing outwards, one bit each (also state words 76, 77)
 * and three more:
 *   pos       DEVICE [E][MQ][2] doubles {n0, f} per entry of meas (read for the two new codes only): the prediction is
 *             (1-f) q(n0) + f q(n0+1) with q the node temperature or the node mole fraction of the clamped node state, the
 *             Jacobian row the same combination; 0 <= n0 <= N-2 (a record outside fails the experiment)
 *   log_scale HOST n_params ints: 1 = the law works in theta = ln p for this parameter (J's column is multiplied by the
 *             member's own value of the constant), 0 = in p
 *   box       HOST [4][8] doubles {lo in p, hi in p, lo in theta, hi in theta}, -HUGE_VAL / HUGE_VAL where open; lo < hi
 * The law, in order: the active set A = {j: p_j <= lo_j and g_j > 0, or p_j >= hi_j and g_j < 0} - rows and columns of
 * H + lambda D become the unit vector, g_j = 0, and all parameters in A is converged -; the step, with theta + delta clamped
 * into the box; the predicted reduction - without a clamped component that of rmt_n2_fit_step, else the model's own
 * -(g^T d + 1/2 d^T H d), which must be > 0 or lambda grows as after a failed pivot -; converged when max |d_j| / s_j <=
 * tolerance, s_j = 1 for a log parameter; the trial p + d, p exp(d) for a log parameter, the bound itself where the step was
 * clamped, kept inside the box in p.  Without flags, bounds and new codes it computes what rmt_n2_fit_step computes. */
int rmt_n2_fit_step_ex(rmt_n2_fit* f, rmt_n2_handle* h, const double* y, const double* sens, const rmt_n2_stats* stats,
                       int S, int V, int N, int n_params, const int* columns, const double* meas, int MQ, double* contrib,
                       double* pred, double* state, double* log_slice, double tolerance, double damping0,
                       const double* pos, const int* log_scale, const double* box);

const char* rmt_n2_last_error(void);
int rmt_n2_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RMT_N2_H */
