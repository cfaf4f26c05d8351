"""WHICH code object a run of the device models loads: geometry tables, the RK4 rate-constant cache, the CodePlan record
with its translation unit, cache key and hipRTC options, and the compile entry points.  Host logic only: needs no GPU."""
import os
from collections import namedtuple

import numpy as np

from . import campaign, frequency, hipbind, plan, profile, schedule, sensitivity

FEATURE_DEFINES = {"ros4": "RMT_WITH_ROS4", "n1": "RMT_WITH_N1", "march": "RMT_WITH_MARCH"}
MARCH_BLOCK = 64         # csrc/kernels/71_steady_march.inc: one reactor per lane, one wave per workgroup


N_CUS = 256          # MI355X; the C library clamps the team count to the device's real CU count


def choose_geometry(N, V, fp32=False, E=None):
    """(block, nodes_per_thread) of the generated kernels for E reactors of N nodes.
    The on-chip stepper holds block*npt nodes per workgroup; longer reactors are chained over
    several workgroups (rmt_n2_rk4_chain).  The table is what measured fastest on MI355X
    (profiles/round1_chain.md, round2_shapes.md):
      * big ensembles: 512 threads x 2 nodes (1024-node chunks, 2 waves/SIMD);
      * ensembles that would leave at least half of the 256 CUs idle with one workgroup per 1024 nodes:
        the reactors are cut into 128-, 256- or 512-node chunks (the smallest that keeps E x chunks <= 256
        workgroups, all resident), e.g. ONE 4096-node reactor over 32 CUs (10.7 us/step vs 217 us on one CU),
        64 x 1024 nodes as 4 chunks each (1.55x the one-CU-per-reactor rate)."""
    if N > 256 and E is not None and 2*E*(-(-N//1024)) <= N_CUS:
        for block, npt in ((128, 1), (256, 1), (256, 2)):
            if E*(-(-N//(block*npt))) <= N_CUS:
                return block, npt
    for block in (64, 128, 256, 512):
        if N <= block:
            return block, 1
    return (512, 2) if V <= 8 else (512, 1)


def ros4_quad(mech, fp32=False):
    """True when the stiff stepper runs in its one-node-on-four-lanes layout (kernels/61_ros4_quad.inc): mechanisms
    wider than 8 variables, whose V x V node inverse does not fit one lane's registers (model N2, fp64)."""
    return mech.V > 8 and getattr(mech, "model", "N2") == "N2" and not fp32


def ros4_block(V, N, fp32=False, quad=None):
    """Workgroup size for the stiff stepper: at most 256 threads (one V x V block inverse per lane),
    and the block's five stage vectors G_1..G_5 must fit in LDS next to the 16 KiB exp table and the
    hand-over buffers (5*V*block*sizeof(real) <= 140 KiB).  (Quad layout, V > 8 in fp64: 256 threads = 64 nodes.)"""
    if quad is None:
        quad = V > 8 and not fp32
    if quad:
        return 256 if N > 32 else 64*((4*N + 63)//64)
    block = min(256, 64*((N + 63)//64))
    while block > 64 and 5*V*block*(4 if fp32 else 8) > 140*1024:
        block //= 2
    return block


def rk45_block(V, N, fp32=False):
    """Workgroup size for the adaptive explicit stepper: the largest (<= 256) whose seven stage
    derivatives of a node block fit in LDS (7*V*block*sizeof(real) <= 112 KiB, csrc RMT_RK45_KLDS)."""
    block = min(256, 64*((N + 63)//64))
    while block > 64 and 7*V*block*(4 if fp32 else 8) > 112*1024:
        block //= 2
    return block


MAX_CHUNKS = 64          # include/rmt_n2.h RMT_N2_MAX_CHUNKS


def rk45_geometry(V, N, fp32=False, chain=True, E=None):
    """(block, nodes_per_thread, defines) for the adaptive explicit stepper.  The on-chip kernels keep 4
    long-lived vectors per node, RMT_RK45_LDS of them in LDS (V*block*npt reals each, at most 136 KiB
    together), the rest in VGPRs - measured on MI355X (profiles/round2_rk45.md): 512 x 2 with 2 vectors in LDS
    for V <= 8, 256 x 2 for the 12-species mechanism.  A reactor that fits one such workgroup runs
    rmt_n2_rk45_reg; a longer one is cut into chunks of that size on as many CUs (rmt_n2_rk45_chain; `chain`),
    up to MAX_CHUNKS; beyond that the memory-resident kernel (rk45_block).
    `E` (reactors on this GPU, when the caller knows it): an ensemble that leaves CUs idle with those chunks is cut
    finer - ONE node per lane, chunks of 512 / 256 nodes (256 / 128 for V > 8) - as long as all chunks of all
    reactors stay co-resident: a step is latency-bound per lane, so half the work per lane on twice the CUs is
    30-70 % faster (profiles/round2_rk45_chain.md)."""
    size = 4 if fp32 else 8
    big = V <= 8
    if big and N <= 1024:
        block, npt = choose_geometry(N, V, fp32)
    elif N <= 512:
        block, npt = (256, 2) if N > 256 else (64*((N + 63)//64), 1)
    elif chain and -(-N//(1024 if big else 512)) <= min(MAX_CHUNKS, N_CUS):
        block, npt = (512, 2) if big else (256, 2)
    else:
        return rk45_block(V, N, fp32), 1, {}
    if chain and E is not None and N > 256:
        for blk in ((256, 512) if big else (128, 256)):          # finest first
            C = -(-N//blk)
            if C >= 2 and blk < block*npt and E*C <= N_CUS and C <= MAX_CHUNKS:
                block, npt = blk, 1
                break
    slots = 2
    while slots > 0 and slots*V*block*npt*size > 136*1024:
        slots -= 1
    if slots == 0:
        return rk45_block(V, N, fp32), 1, {}
    return block, npt, {"RMT_RK45_LDS": str(slots)}


KC_REFRESH = 8          # csrc/kernels/50_rk4.inc RMT_KC_REFRESH: the cache's reference point moves every 8th step ...
KC_MAX_AGE = 1.3e-5     # ... RMT_KC_MAX_AGE: or sooner, so that no reference point is older than this much model time [s]


def is_forced(defines):
    """True for the prelude defines of a code object that evaluates a schedule (csrc/kernels/11_forcing.inc): its member
    rows carry schedule.TAIL more doubles ("1") or schedule.TAIL + S more ("2": the schedule also moves the feed
    composition) and none of the forced fields is baked into the kernel."""
    return forcing_level(defines) in ("1", "2")


def forcing_level(defines):
    """The RMT_FORCING value of the prelude defines as a string: "0" (none), "1" or "2"."""
    return str((defines or {}).get("RMT_FORCING", "0"))


def forced_tail(defines, S):
    """doubles a member row of that code object carries behind the ordinary 16 + S + NU"""
    level = forcing_level(defines)
    return schedule.TAIL + int(S) if level == "2" else schedule.TAIL if level == "1" else 0


def is_profiled(defines):
    """True for the prelude defines of a code object that reads an axial profile (csrc/kernels/12_profile.inc): its handle
    needs the table of rmt_n2_set_profile, and it holds no chained kernel."""
    return str((defines or {}).get(profile.DEFINE, "0")) == "1"


def forced_literals(member_defines, level="1"):
    """The sweep-invariant member fields a FORCED code object may take as literals: all but the ones the schedule moves -
    three for RMT_FORCING 1, the inlet composition as well for RMT_FORCING 2 (``level``) - no RMT_MC_* literal may freeze a
    forced field; the others never change between the launches of a run."""
    moved = ("RMT_MC_THETA_IN", "RMT_MC_P0", "RMT_MC_TM") + (("RMT_MC_CIN",) if str(level) == "2" else ())
    return {k: v for k, v in member_defines.items() if k not in moved}


def forced_mode(ivp, N, block, npt, want=None, key="schedule", what="forcing"):
    """The kernel form of a forced launch, set by the HOST (rmt_n2_set_mode): the chained forms do not carry the forcing,
    so the library's auto mode must not pick them.  The same rule serves profiled runs (``key`` "axial-profile", ``what``
    "profile"), forced or not.  "reg" (the on-chip steppers) when the reactor fits one workgroup,
    else "mem"; the stiff stepper always runs rmt_n2_ros4_mem (any N on one workgroup).  `want`: solver-config
    "device-mode"."""
    if want not in (None, "auto", "reg", "mem"):
        raise ValueError("solver-config 'device-mode' must be 'reg' or 'mem' together with '%s' (got %r): the "
                         "chained kernels do not carry the %s" % (key, want, what))
    if ivp == "hip-ros4":
        return "mem"
    fits = int(N) <= int(block)*int(npt)
    if want == "reg" and not fits:
        raise ValueError("solver-config 'device-mode': 'reg' holds at most %d nodes per reactor (zNo = %d)"
                         % (int(block)*int(npt), int(N)))
    return want if want in ("reg", "mem") else ("reg" if fits else "mem")


def kc_period(defines, dt):
    """steps between two moves of the reference point of a caching one-workgroup RK4 stepper at step size dt (the kernel's
    own rule, csrc/kernels/50_rk4.inc rmt_rk4_reg_body)."""
    K = int(defines.get("RMT_KC_REFRESH", 1))
    age = float(defines.get("RMT_KC_MAX_AGE", KC_MAX_AGE))
    return 1 if K <= 1 or not dt > 0 else int(min(float(K), max(1.0, age/dt)))


def kcache_choice(mech, N, fp32, block, npt, lds_state, defines):
    """(defines, lds_state) with the RK4 steppers' cache of the temperature-only rate constants switched on where it has
    been measured to pay (csrc/kernels/50_rk4.inc rmt_rk4_reg_body / rmt_rk4_chain_body; profiles/round3_kcache.md), model
    N2 in fp64 (the list is for at most 8 variables per node; wider mechanisms: see the table in the body):

    * one workgroup per reactor at 512 x 2 (RMT_KCACHE; the bench shape, 1.62e10 -> 1.95e10 node-steps/s) and at the
      small geometries of short reactors (2048 x 20 nodes at 64 x 1: 3.2e9 -> 5.0e9, 2048 x 128 at 128 x 1: 1.21e10 ->
      1.53e10, 1024 x 256 at 256 x 1: 1.47e10 -> 1.58e10; profiles/round3_kcache.md): 1/T_ref,
      log T_ref, T_ref, the Arrhenius constants AND the equilibrium constants (RMT_KCACHE_GEN 2: one slot each, the
      exponent's change from the differences of its basis functions T^n, log T) when the mechanism's exponents decompose
      that way and every table-driven exp is then a cached constant (the kernel keeps the 64-entry exp table, which makes
      the room in LDS); else without the equilibrium constants (RMT_KCACHE_GEN 0).  y_n moves to LDS (lds_state 1) to make
      room in the register file; the reference point moves every 8th step;
    * chained workgroups, every geometry (RMT_KCACHE_CHAIN, RMT_KCACHE_GEN 0): 256 x 4096 nodes at 512 x 2 +10 %, 128 x
      1024 at 256 x 2 +8 %, 64 x 1024 at 256 x 1 +5 %, ONE 4096-node reactor at 128 x 1 +7.5 %.

    An explicit "RMT_KCACHE" / "RMT_KCACHE_CHAIN" in `defines` (0 or 1) is left alone, and so is an lds_state that does
    not leave the room."""
    defs = dict(defines or {})
    chained = int(N) > int(block)*int(npt)
    if is_forced(defs) and (chained or os.environ.get("RMT_N2_FORCED_PLAIN")):
        return defs, lds_state       # (a forced reactor beyond one workgroup runs the memory-resident form, never the chain)
    if is_profiled(defs) and (chained or os.environ.get("RMT_N2_PROFILED_PLAIN")):
        return defs, lds_state       # (the same for a profiled one: a profiled unit has no chained kernel)
    key = "RMT_KCACHE_CHAIN" if chained else "RMT_KCACHE"
    geo = (int(block), int(npt))
    model = getattr(mech, "model", "N2")
    if key in defs or fp32 or model not in ("N2", "M2"):
        return defs, lds_state
    if model == "M2":
        # the dimensional model: its one-workgroup stepper at 512 x 2 (which keeps y_n in LDS anyway), Arrhenius constants
        # only - with the equilibrium constants its step loop spills (28 scratch accesses)
        if chained or geo != (512, 2) or lds_state not in (None, 1) or mech.V > 8 \
                or not mech.kcache_fits(fp32, block, npt, 1, gen=False):
            return defs, lds_state
        defs.update({key: "1", "RMT_KCACHE_GEN": "0"})
        defs.setdefault("RMT_KC_REFRESH", str(KC_REFRESH))
        return defs, 1
    # where the cache measured faster (profiles/round3_kcache.md) -> the lds_state it needs (None: the geometry's default).
    # At most 8 variables per node (DME): every chained geometry; one workgroup per reactor at 512 x 2, at 64 / 128 / 256
    # threads and at 512 x 1 with y_n in LDS (1.52e10 -> 1.72e10; with the geometry's own lds_state it is SLOWER).  Wider mechanisms (12 species, V = 13): 64 x 1 (8.7e9 ->
    # 1.21e10), 512 x 1 (1.07e10 -> 1.16e10) and the chained 512 x 1 (9.9e9 -> 1.04e10), with y_n in LDS; 128 x 1 is
    # SLOWER there (8.8e9 -> 7.1e9).
    if mech.V <= 8:
        good = {geo: (1 if geo == (512, 2) else lds_state)} if chained and geo[1] <= 2 else \
            {(512, 2): 1, (64, 1): lds_state, (128, 1): lds_state, (256, 1): lds_state, (512, 1): 1}
    else:
        good = {(512, 1): 1} if chained else {(64, 1): lds_state, (512, 1): 1}
    if geo not in good or (good[geo] == 1 and lds_state not in (None, 1)):
        return defs, lds_state
    want = good[geo]
    if chained:
        if not mech.kcache_fits_chain(fp32, block, npt, want, gen=False):
            return defs, lds_state
        defs.update({key: "1", "RMT_KCACHE_GEN": "0"})
        return defs, want
    # equilibrium constants too where that measured faster: everywhere but at 128 x 1 (1.53e10 with the Arrhenius
    # constants alone against 1.39e10 - the wider kernel loses a wave of occupancy there) and 512 x 1 (1.72e10 against 1.52e10)
    if geo not in ((128, 1), (512, 1)) and mech.kcache_small_exp("basis") and mech.kcache_slots("basis") > mech.kcache_slots(False) \
            and mech.kcache_fits(fp32, block, npt, want, gen="basis", small_exp=True, node_major=True):
        # (a node's slots side by side in LDS: one address register per node; with slot-major rows of 8 KiB the far slots
        # need registers of their own and the 512 x 2 step loop spills - 1.86e10 against 1.95e10 node-steps/s)
        defs.update({key: "1", "RMT_KCACHE_GEN": "2", "RMT_KC_SMALL_EXP": "1", "RMT_KC_NODE_MAJOR": "1"})
    elif mech.kcache_fits(fp32, block, npt, want, gen=False):
        defs.update({key: "1", "RMT_KCACHE_GEN": "0"})
    else:
        return defs, lds_state
    defs.setdefault("RMT_KC_REFRESH", str(KC_REFRESH))
    return defs, want


CodePlan = namedtuple("CodePlan", "block npt lds_state defines features")


def code_plan(mech, N, fp32=False, E=None, block=None, npt=None, lds_state=None, defines=None, features=(),
              rows=None, specialize=None, literals=None, newton=True):
    """WHICH code object a run loads - the one place that decides it: geometry (the caller's, else choose_geometry for E
    members per GPU), the RK4 rate-constant cache (kcache_choice), the optional kernel families, the stiff stepper's
    layout, model M2's Newton sweeps and the sweep-invariant member fields as literals.  The single-process route passes
    its member ``rows`` (E and, with ``specialize``, the literals come from them; a single reactor is NOT specialised by
    default - every new operating point would cost a 2-3 s JIT); a multi-rank job passes the members per GPU and the
    defines its ranks agreed on (``literals``).  A forced code object takes no literal for a field its schedule moves.
    The translation unit and its cache key (plan_unit) and the hipRTC options (compile_options) follow from the record;
    needs no GPU."""
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        rows = rows.reshape(1, -1) if rows.ndim == 1 else rows
        E = rows.shape[0] if E is None else E
        specialize = E >= 2 if specialize is None else specialize
    b, n = choose_geometry(int(N), mech.V, fp32, E)
    block, npt = int(block or b), int(npt or n)
    defs, lds_state = kcache_choice(mech, N, fp32, block, npt, lds_state, defines)
    # optional kernel families: "ros4" (stiff stepper), "n1" (steady-state model); their
    # unrolled VxV linear algebra is most of the JIT time, so they are compiled on demand
    for f in features:
        defs[FEATURE_DEFINES[f]] = "1"
    # the cross-wave part of the pressure scan (csrc/kernels/25_prefix.inc): the batched form where it was timed - the unit
    # of the caching one-workgroup RK4 stepper of model N2 at 512 x 2, built for nothing else (the bench unit; the same
    # condition as compile_options' register-pressure trackers).  The RK45 unit of that geometry, units with an optional
    # kernel family and every other geometry keep the template's default, the scalar loop (profiles/prefix_chain.md)
    if "RMT_PREFIX_MODE" not in defs and str(defs.get("RMT_KCACHE", "0")) == "1" and (block, npt) == (512, 2) \
            and not features and "RMT_RK45_LDS" not in defs and not fp32 and getattr(mech, "model", "N2") == "N2":
        defs["RMT_PREFIX_MODE"] = "4"
    if "ros4" in features and "RMT_ROS_QUAD" not in defs and ros4_quad(mech, fp32) and npt == 1:
        defs["RMT_ROS_QUAD"] = "1"            # wide mechanism: one node on four lanes (N2Device tells the C library)
    if getattr(mech, "model", "N2") == "M2" and "RMT_M2_NEWTON" not in defs and rows is not None and newton:
        # (a multi-rank job passes the maximum over its ranks as a define)
        defs["RMT_M2_NEWTON"] = str(plan.m2_newton_sweeps(rows, mech, int(N)))
    if specialize:                            # sweep-invariant member fields become literals (frees SGPRs)
        literals = plan.uniform_member_defines(rows[:, :mech.row_width], mech.S)
    if literals:
        defs.update(forced_literals(literals, forcing_level(defs)) if is_forced(defs) else literals)
    # "RMT_KCACHE": "1" (kcache_choice above, or the caller's own): the on-chip RK4 stepper caches the temperature-only
    # rate constants per node in LDS - that has to fit
    gen = plan.KCACHE_GEN[str(defs.get("RMT_KCACHE_GEN", "1"))]
    small = str(defs.get("RMT_KC_SMALL_EXP", "0")) == "1"
    if small and not mech.kcache_small_exp(gen):
        raise ValueError("RMT_KC_SMALL_EXP=1: the mechanism has table-driven exp evaluations that are not cached constants")
    if str(defs.get("RMT_KCACHE_CHAIN", "0")) == "1" and not mech.kcache_fits_chain(
            fp32, block, npt, lds_state, gen, small, str(defs.get("RMT_KC_NODE_MAJOR", "0")) == "1"):
        raise ValueError("RMT_KCACHE_CHAIN=1: the cache of the temperature-only rate constants (%d doubles per node) does "
                         "not fit beside the chunk's RK4 vectors (model N2, fp64)" % mech.kcache_slots(gen))
    if str(defs.get("RMT_KCACHE", "0")) == "1" and not (
            int(N) <= block*npt and mech.kcache_fits(fp32, block, npt, lds_state, gen, small,
                                                     str(defs.get("RMT_KC_NODE_MAJOR", "0")) == "1")):
        raise ValueError("RMT_KCACHE=1: the cache of the temperature-only rate constants (%d doubles per node) does not "
                         "fit this geometry (needs the on-chip RK4 stepper with its vectors in registers, model N2, fp64)"
                         % mech.kcache_slots())
    return CodePlan(block, npt, lds_state, defs, tuple(features))


def march_plan(mech, N, defines=None, rows=None):
    """The code object of the steady-state march (solver-config "initial", csrc/kernels/71_steady_march.inc): a unit of
    its own - the stepper's code object and its cache key are those of a run without the key.  block = 64 (one reactor per
    lane), the family "march" (RMT_WITH_MARCH: the analytic node Jacobian without the stiff stepper's kernels), no
    rate-constant cache, fp64.  Of the run's ``defines`` only the row layout travels (RMT_FORCING: the rows are the
    stepper's); the member fields stay run-time values, so one object serves every operating point of a mechanism."""
    defs = {"RMT_KCACHE": "0", "RMT_KCACHE_CHAIN": "0"}
    if is_forced(defines):
        defs["RMT_FORCING"] = forcing_level(defines)
    if is_profiled(defines):          # (the march reads the table for the node it is solving)
        defs[profile.DEFINE] = "1"
    return code_plan(mech, N, False, None, MARCH_BLOCK, 1, None, defs, ("march",), rows, specialize=False)


def is_campaign(defines):
    """True for the prelude defines of the campaign unit (csrc/kernels/72_campaign.inc): the one unit generated from the
    whole template text (plan.Mechanism.source cuts that file's text out of every other unit)."""
    return str((defines or {}).get(campaign.DEFINE, "0")) == "1"


def campaign_plan(mech, N, rows=None):
    """The code object of a time-on-stream run (solver-config "deactivation", csrc/kernels/72_campaign.inc): the profiled
    march unit (march_plan) plus RMT_CAMPAIGN - rmt_n2_campaign_step beside rmt_n2_steady_march.  The only unit such a run
    loads; one object serves every operating point, law and mesh of a mechanism."""
    cp = march_plan(mech, N, {profile.DEFINE: "1"}, rows)
    return CodePlan(cp.block, cp.npt, cp.lds_state, {**cp.defines, campaign.DEFINE: "1"}, cp.features)


def campaign_policy_plan(mech, N, rows=None):
    """The code object of a time-on-stream run with a "policy" (campaign.POLICY_DEFINE): the campaign unit plus
    RMT_CAMPAIGN_POLICY - rmt_n2_campaign_policy_step beside rmt_n2_campaign_step.  A campaign without the key keeps loading
    the unit of campaign_plan."""
    cp = campaign_plan(mech, N, rows)
    return CodePlan(cp.block, cp.npt, cp.lds_state, {**cp.defines, campaign.POLICY_DEFINE: "1"}, cp.features)


def sens_plan(mech, N, n_params, defines=None, rows=None):
    """The code object of a run with solver-config "sensitivity" (csrc/kernels/73_sensitivity.inc): whatever march_plan
    gives for the run (forced or profiled rows) plus RMT_SENS and RMT_SENS_NP - rmt_n2_steady_sens beside
    rmt_n2_steady_march.  ``mech``: the mechanism of the sensitivity unit (the "rate-constant" parameters among its
    per-reactor inputs).  It takes the place of the march unit on the march handle (N2Device.attach_march: where its
    mechanism is the run's own; else it gets a handle of its own beside the plain march unit); every other unit of the
    run is what it is without the key."""
    cp = march_plan(mech, N, defines, rows)
    return CodePlan(cp.block, cp.npt, cp.lds_state,
                    {**cp.defines, sensitivity.DEFINE: "1", sensitivity.DEFINE_NP: str(int(n_params))}, cp.features)


def freq_plan(mech, N, n_inputs, defines=None, rows=None):
    """The code object of solver-config "frequency-response" (csrc/kernels/74_frequency.inc): the sensitivity unit of the
    run's own mechanism (sens_plan with RMT_SENS_NP = n_inputs) plus RMT_FREQ and RMT_FREQ_NP - rmt_n2_steady_freq beside
    rmt_n2_steady_sens and rmt_n2_steady_march.  It always lives on a handle of its own (N2Device.attach_frequency): every
    other unit of the run, the march and the sensitivity unit included, is what it is without the key."""
    cp = sens_plan(mech, N, n_inputs, defines, rows)
    return CodePlan(cp.block, cp.npt, cp.lds_state,
                    {**cp.defines, frequency.DEFINE: "1", frequency.DEFINE_NP: str(int(n_inputs))}, cp.features)


def code_plans(mech, N, fp32=False, E=None, block=None, npt=None, lds_state=None, defines=None, features=(),
               rows=None, specialize=None, literals=None, newton=True):
    """EVERY code object a run loads, as CodePlans: the stepper's (code_plan with the same arguments, the feature "march"
    taken out) and, with the feature "march", the unit of the steady-state march behind it (march_plan)."""
    step = tuple(f for f in features if f != "march")
    plans = [code_plan(mech, N, fp32, E, block, npt, lds_state, defines, step, rows, specialize, literals, newton)]
    if "march" in features:
        plans.append(march_plan(mech, N, defines, rows))
    return plans


def plan_unit(mech, fp32, cp):
    """(translation unit, cache key) of a CodePlan"""
    tpl = hipbind.kernel_template()
    # (the user's lds_state, possibly None, is what selects the per-kernel defaults)
    return (mech.source(tpl, fp32, cp.block, cp.npt, cp.lds_state, cp.defines),
            mech.digest(tpl, fp32, cp.block, cp.npt, cp.lds_state, cp.defines))


def compile_plan(mech, fp32, cp, arch="gfx950", extra_opts=""):
    """The code object of a CodePlan, from the in-tree cache or hipRTC (no GPU needed)."""
    src, key = plan_unit(mech, fp32, cp)
    return hipbind.compile_cached(src, key, arch, compile_options(cp.block, cp.npt, cp.features, extra_opts, cp.defines))


def device_source(mech, members, N, fp32=False, block=None, npt=None, lds_state=None, defines=None,
                  specialize=None, features=()):
    """What N2Device compiles for (mechanism, member rows, mesh): (block, npt, prelude #defines, translation unit, cache
    key)."""
    cp = code_plan(mech, N, fp32, None, block, npt, lds_state, defines, features, members, specialize)
    return (cp.block, cp.npt, cp.defines) + plan_unit(mech, fp32, cp)


def compile_options(block, npt, features=(), extra_opts="", defines=None):
    """hipRTC options beyond the library's own (csrc/rmt_n2.cpp rmt_n2_compile) for a code object of this geometry.  The
    RK4 steppers at 512 x 2 - two waves per SIMD at the register limit - are scheduled with LLVM's AMDGPU register
    pressure trackers (`-amdgpu-use-amdgpu-trackers=1`): bench 2.018e10 -> 2.045e10 node-steps/s, chained 256 x 4096
    nodes 1.53e10 -> 1.58e10; the stiff stepper (-1.5 %) and the small chunks of ONE long reactor (-1.9 %) are SLOWER
    with it, and so is the on-chip RK45 stepper on the bench sweep (6.90e9 -> 6.71e9; tools/microbench/exp_r3ae.sh,
    rk45_ab.py): code objects with optional kernel families or built for RK45 (rk45_geometry's "RMT_RK45_LDS") keep the
    default."""
    auto = "-mllvm -amdgpu-use-amdgpu-trackers=1" if ((int(block), int(npt)) == (512, 2) and not features
                                                       and "RMT_RK45_LDS" not in (defines or {})) else ""
    if os.environ.get("RMT_N2_NO_TRACKERS"):          # (A/B measurements)
        auto = ""
    if not auto or "amdgpu-use-amdgpu-trackers" in (extra_opts or ""):
        return extra_opts or ""
    return ("%s %s" % (extra_opts, auto)).strip()


def precompile(mech, members, N, arch="gfx950", extra_opts="", **kw):
    """Cross-compile (hipRTC, no GPU needed) the code object N2Device(mech, members, N, **kw) will load and
    leave it in the in-tree cache; returns its cache key."""
    cp = code_plan(mech, N, rows=members, **kw)
    compile_plan(mech, kw.get("fp32", False), cp, arch, extra_opts)
    return plan_unit(mech, kw.get("fp32", False), cp)[1]


def compile_mechanism(mech, N, fp32=False, block=None, npt=None, lds_state=None, defines=None,
                      arch="gfx950", E=None, extra_opts="", features=()):
    """Code object for (mechanism, mesh size, members per rank) - what ensemble rank 0 compiles
    and broadcasts; pass the same E/block/npt/lds_state/defines/features to N2Device(code=...)."""
    return compile_plan(mech, fp32, code_plan(mech, N, fp32, E, block, npt, lds_state, defines, features), arch, extra_opts)


def device_arch(device=None):
    """Architecture the JIT targets: that of ``device``; without one the current GPU's, gfx950 when none is visible
    (cross-compile)."""
    if device is not None:
        import torch
        return torch.cuda.get_device_properties(device).gcnArchName.split(":")[0]
    try:
        import torch
        if torch.cuda.is_available():
            return device_arch(torch.cuda.current_device())
    except Exception:
        pass
    return "gfx950"
