"""Device-side driver of model N2: the replacement for the time loop of
PackedBedHomoReactorClass.runN2 (PyREMOT/docs/pbHomoReactor.py:3556-3704).

The reference calls scipy's solve_ivp once per output interval with a Python RHS
(:3589-3610); here each interval is ONE launch of a device-resident explicit stepper
(fixed-step RK4 or adaptive Dormand-Prince RK45) over all mesh nodes of all ensemble members.
torch is used only as the owner of device memory and streams.
"""
import ctypes as C
from collections import namedtuple
from timeit import default_timer as timer

import os

import numpy as np

from . import campaign, control, hipbind, initial, launches, monitor, plan, profile, schedule, sensitivity
from .ensemble import DistributedEnsemble, active_ranks, guarded
from .lowering import FLAG_DIV0, FLAG_DOMAIN, FLAG_NONFINITE, FLAG_OVERFLOW, FLAG_STEP
from .settings import DEVICE_DEFAULTS, ROUND_FUN_ACCURACY, solverSetting

FLAG_PRESSURE = 32
DEVICE_IVPS = ("hip-rk4", "hip-rk45", "hip-ros4", "hip-auto", "AM", "hip-ab3")
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


def flag_error(flags):
    """Device status words (one per reactor) -> the exception the reference's Python path raises inside the user lambdas
    (SURVEY.md section 5 'Failure detection') for the first reactor that has one set; None when all are clear."""
    bad = np.nonzero(flags)[0]
    if len(bad) == 0:
        return None
    f = int(flags[bad[0]])
    where = "reactor %d of %d (flags=0x%x)" % (bad[0], len(flags), f)
    if f & FLAG_DOMAIN:
        return ValueError("math domain error in " + where)
    if f & FLAG_DIV0:
        return ZeroDivisionError("float division by zero in " + where)
    if f & FLAG_OVERFLOW:
        return OverflowError("math range error in " + where)
    if f & FLAG_STEP:
        return RuntimeError("adaptive step control failed (step underflow / max steps) in " + where)
    if f & FLAG_NONFINITE:
        return FloatingPointError("state became NaN/Inf in " + where + " - step size too large?")
    if f & FLAG_PRESSURE:
        return RuntimeError("model M2: the Newton sweeps of the pressure march did not converge in "
                            + where + " - pass defines={'RMT_M2_NEWTON': 4} (pressure drop > 15 % of P)")
    if f & (campaign.FLAG_POLICY_BRACKET | campaign.FLAG_POLICY_EVALS):
        return RuntimeError("the coolant policy of a time-on-stream step gave up (%s) in %s"
                            % ("its bracket collapsed: the outlet jumps there" if f & campaign.FLAG_POLICY_BRACKET
                               else "evaluation limit reached", where))
    return RuntimeError("device error in " + where)


def stepper_args(cfg, stepper, first, auto=False):
    """(rtol, atol, h0, max_steps) of N2Device.rk45 / .ros4 ("rk45" / "ros4") from the solver-config.  The first launch
    of a stepper starts every reactor at h0; later ones RESUME (h0 < 0): each reactor starts from the step its own
    controller proposed at the end of the previous launch (stats.h_last).  ``auto``: the explicit pair under "hip-auto"
    has tolerances of its own."""
    tol = "auto-rk45" if auto and stepper == "rk45" else stepper
    h0 = float(cfg.get('h0', DEVICE_DEFAULTS[stepper + '-h0']))
    return (float(cfg.get('rtol', DEVICE_DEFAULTS[tol + '-rtol'])), float(cfg.get('atol', DEVICE_DEFAULTS[tol + '-atol'])),
            h0 if first else -h0, int(cfg.get('max-steps', DEVICE_DEFAULTS['rk45-max-steps'])))


def step_counts(raw):
    """(accepted, rejected) per reactor from the adaptive steppers' counters [E][4] = {t_end, h_last, accepted, rejected}
    (the two counts travel as the bit patterns of int64)"""
    return raw[:, 2].copy().view(np.int64), raw[:, 3].copy().view(np.int64)


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise hipbind.RmtN2Error("no HIP device visible: the N2 integrator has no CPU fallback")
    return torch


class N2Device:
    """One compiled mechanism + E packed member rows on one GPU."""
    # launches, row updates (set_members_async) and copies of the counters tensor (_stats) are queued on one stream, and
    # nothing between two launches needs the host: integrate_intervals may queue several launches at once
    stream_ordered = True

    def __init__(self, mech, members, N, fp32=False, block=None, npt=None, device=None,
                 extra_opts="", lds_state=None, defines=None, code=None, specialize=None,
                 features=(), profile=None):
        """``profile``: the table [E][2][N] of an axial profile (profile.Profile.table: per member the catalyst activities,
        then the coolant offsets).  The code object is generated with RMT_PROFILE and the table uploaded before anything
        is launched.  (``defines={"RMT_PROFILE": "1"}`` alone creates the profiled device without a table: set_profile.)"""
        torch = _torch()
        if profile is not None:
            defines = {**(defines or {}), "RMT_PROFILE": "1"}
        self.torch = torch
        self.mech, self.N, self.fp32 = mech, int(N), bool(fp32)
        members = np.ascontiguousarray(members, dtype=np.float64)
        if members.ndim == 1:
            members = members.reshape(1, -1)
        self.forced = is_forced(defines)
        self.row_width = mech.row_width + forced_tail(defines, mech.S)
        assert members.shape[1] == self.row_width, \
            "member rows must hold 16 + S + NU doubles (+ 4 when forced, + 4 + S with a forced composition)"
        self.E = members.shape[0]
        self.members = members
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        cp = code_plan(mech, self.N, self.fp32, None, block, npt, lds_state, defines, features, members, specialize,
                       newton=code is None)
        self.block, self.npt, self.defines, self.features = cp.block, cp.npt, cp.defines, cp.features
        self.lds_state = mech.lds_state(self.fp32, self.block, self.npt, cp.lds_state)
        if code is None:      # an ensemble rank may receive rank 0's code object instead
            code = compile_plan(mech, self.fp32, cp, device_arch(self.device), extra_opts)
        self._code = C.create_string_buffer(code, len(code))
        p = hipbind.Plan()
        p.abi_version = hipbind.ABI_VERSION
        p.n_species, p.n_reactions, p.n_vars = mech.S, mech.R, mech.V
        p.n_nodes, p.n_members, p.fp32 = self.N, self.E, int(self.fp32)
        p.block, p.nodes_per_thread = self.block, self.npt
        p.n_user_params = self.row_width - plan.MEMBER_FIXED - mech.S       # (a forced row's tail travels as 4 or 4 + S more)
        self.ros_quad = str(self.defines.get("RMT_ROS_QUAD", "0")) == "1"
        p.ros4_nodes_per_block = self.block//4 if self.ros_quad else 0
        self.profiled = is_profiled(self.defines)
        p.profiled = int(self.profiled)
        p.code_object = C.cast(self._code, C.c_void_p)
        p.code_size = len(code)
        p.members = members.ctypes.data_as(C.POINTER(C.c_double))
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            hipbind.check(hipbind.lib().rmt_n2_create(C.byref(p), C.byref(h)))
        self.h = h
        # node-function evaluations one Jacobian of the stiff stepper costs: the analytic Jacobian comes with the
        # stage-1 evaluation (rates and their partials in ONE fused pass, rmt_node_jac) and is charged as one more;
        # the forward-difference form (RMT_ROS_JAC_FD 1) costs V columns, +1 in model M2 for the upwind coupling
        fd = str(self.defines.get("RMT_ROS_JAC_FD", "0")) == "1"
        self.jacobian_evals = (mech.V + (1 if getattr(mech, "model", "N2") == "M2" else 0)) if fd else 1
        self.dtype = torch.float32 if self.fp32 else torch.float64
        self._stats = torch.zeros((self.E, 4), dtype=torch.float64, device=self.device)
        self.march = None       # a second device of the same rows with the steady-state march (attach_march)
        self.sens = None        # ... and a third with the sensitivity unit, where that needs a mechanism of its own
        self.use_current_stream()
        self.profile = None
        if profile is not None:
            try:
                self.set_profile(profile)
            except Exception:
                self.close()
                raise

    # -- plumbing
    def use_current_stream(self):
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        hipbind.check(hipbind.lib().rmt_n2_set_stream(self.h, C.c_void_p(s)))
        self._stream = s

    def set_members(self, members):
        """Replace the per-reactor constant rows (same E) without recompiling - e.g. the next
        point of a sweep.  Not available when member fields were baked into the kernel as literals
        (``specialize``): those fields would silently keep their old values."""
        if any(k.startswith("RMT_MC_") for k in self.defines) and not self.forced:
            # (a forced device only ever has its forced fields and the tail refreshed - those are never literals)
            raise hipbind.RmtN2Error("this kernel was specialised on its member rows "
                                     "(N2Device(..., specialize=False) keeps them run-time)")
        members = np.ascontiguousarray(members, dtype=np.float64).reshape(self.E, -1)
        assert members.shape[1] == self.row_width
        self.members = members
        hipbind.check(hipbind.lib().rmt_n2_set_members(self.h, members.ctypes.data_as(C.POINTER(C.c_double))))

    def set_members_async(self, members):
        """set_members queued on the current stream without waiting for it (between two queued launches: the rows of a
        forced run are refreshed before every launch).  Returns the page-locked staging tensor, which the caller keeps
        alive until the stream has passed the copy."""
        members = np.ascontiguousarray(members, dtype=np.float64).reshape(self.E, self.row_width)
        pinned = self.torch.empty(members.shape, dtype=self.torch.float64, pin_memory=True)
        pinned.copy_(self.torch.from_numpy(members))
        self.members = members
        hipbind.check(hipbind.lib().rmt_n2_set_members_async(self.h, C.c_void_p(pinned.data_ptr())))
        return pinned

    def set_profile(self, table):
        """Upload the axial profile [E][2][N] (rmt_n2_set_profile: one synchronous copy, before the first launch).  Only
        for a device whose code object was generated with RMT_PROFILE."""
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.shape != (self.E, 2, self.N):
            raise hipbind.RmtN2Error("the profile table must be [E][2][N] = %r doubles (got %r)"
                                     % ((self.E, 2, self.N), table.shape))
        hipbind.check(hipbind.lib().rmt_n2_set_profile(self.h, table.ctypes.data_as(C.POINTER(C.c_double))))
        self.profile = table
        if self.march is not None:
            self.march.set_profile(table)
        if self.sens is not None:
            self.sens.set_profile(table)

    def get_members(self):
        """The device rows as they are now [E][row_width] (synchronises the stream): what the last refresh uploaded and
        the controller's kernel wrote since."""
        out = np.zeros((self.E, self.row_width))
        hipbind.check(hipbind.lib().rmt_n2_get_members(self.h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def set_mode(self, mode):
        hipbind.check(hipbind.lib().rmt_n2_set_mode(self.h, {"auto": 0, "reg": 1, "mem": 2, "chain": 3}[mode]))

    def close(self):
        if getattr(self, "_mon", None) is not None:
            self._mon.close()
            self._mon = None
        if getattr(self, "march", None) is not None:
            self.march.close()
            self.march = None
        if getattr(self, "sens", None) is not None:
            self.sens.close()
            self.sens = None
        if getattr(self, "h", None):
            hipbind.lib().rmt_n2_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def monitor(self, y, out, residual=False):
        """Queue the row reductions of the state y on the device's stream: out (device double [E][V][5]) = per member
        and variable {y[N-1], max, argmax, min, max|dy/dt|} - the last one only with ``residual`` (rmt_n2_rhs at y is
        queued first), else 0.  Nothing is copied or synchronised.  The monitor object (mechanism-independent kernels,
        csrc/monitor_kernels.inc) is created on first use."""
        self._chk_state(y)
        assert out.is_cuda and out.dtype == self.torch.float64 and out.is_contiguous()
        assert out.numel() == self.E*self.mech.V*monitor.SLOTS, "monitor output must be [E][V][5] doubles"
        if getattr(self, "_mon", None) is None:
            with self.torch.cuda.device(self.device):
                self._mon = hipbind.Monitor(device_arch(self.device))
        dydt = self.rhs(y) if residual else None       # (stays allocated until the stream is past the reduce: torch's
        #                                                 caching allocator hands memory out in stream order)
        self._mon.reduce(self._stream, y.data_ptr(), dydt.data_ptr() if residual else 0, self.E, self.mech.V, self.N,
                         self.fp32, out.data_ptr())

    def control(self, y, loop, k=None):
        """Queue the controller's kernel on the device's stream, behind the refresh of the member rows and ahead of the
        next stepper launch (csrc/control_kernels.inc): sample ``k`` of the ControlLoop - measure on the state y, evaluate
        the law, write slice k of the log and the manipulated field of this device's rows - or, with k = None, only
        write the held value into the rows again.  Nothing is copied or synchronised."""
        if not self.forced or self.fp32:
            raise hipbind.RmtN2Error("the controller writes the rows of a forced fp64 code object (RMT_FORCING 1 or 2)")
        if k is not None:
            self._chk_state(y)
        assert loop.E == self.E
        loop.kernel.update(self.h, y.data_ptr() if k is not None else 0, self.mech.V, self.N, loop.params.data_ptr(),
                           loop.setpoints[k].data_ptr() if k is not None else 0, loop.state.data_ptr(),
                           loop.log[k].data_ptr() if k is not None else 0, self.mech.row_width, loop.field, k is None)

    def to_device(self, y):
        t = self.torch.as_tensor(np.ascontiguousarray(y), dtype=self.dtype)
        return t.reshape(self.E, self.mech.V*self.N).contiguous().to(self.device)

    def _chk_state(self, y):
        assert y.is_cuda and y.dtype == self.dtype and y.is_contiguous()
        assert y.numel() == self.E*self.mech.V*self.N, "state must be [E][V][N]"

    # -- hot path entry points
    def rhs(self, y, t=0.0):
        self._chk_state(y)
        out = self.torch.empty_like(y)
        hipbind.check(hipbind.lib().rmt_n2_rhs(self.h, float(t), C.c_void_p(y.data_ptr()),
                                               C.c_void_p(out.data_ptr())))
        return out

    def rk4(self, y, dt, nsteps, t0=0.0):
        """In place: nsteps RK4 steps of size dt."""
        self._chk_state(y)
        hipbind.check(hipbind.lib().rmt_n2_rk4(self.h, C.c_void_p(y.data_ptr()), float(t0), float(dt),
                                               int(nsteps)))

    def multistep(self, y, dt, nsteps, method="PreCorr3", t0=0.0):
        """In place: the reference's AdBash3 / PreCorr3 (odeSolver.py:43-102), nsteps >= 3."""
        self._chk_state(y)
        hipbind.check(hipbind.lib().rmt_n2_multistep(
            self.h, C.c_void_p(y.data_ptr()), float(t0), float(dt), int(nsteps),
            {"AdBash3": 0, "PreCorr3": 1}[method]))

    def rk45(self, y, t0, t1, rtol, atol, h0, max_steps):
        self._chk_state(y)
        hipbind.check(hipbind.lib().rmt_n2_rk45(self.h, C.c_void_p(y.data_ptr()), float(t0), float(t1),
                                                float(rtol), float(atol), float(h0), int(max_steps),
                                                C.c_void_p(self._stats.data_ptr())))

    def ros4(self, y, t0, t1, rtol, atol, h0, max_steps):
        """In place: stiff integration (RODAS4, order 4(3)) from t0 to t1 with per-reactor step control
        (needs a code object generated with features=("ros4",) and block <= 512; 256 is fastest)."""
        self._chk_state(y)
        if "ros4" not in self.features:
            raise hipbind.RmtN2Error("create the device with features=('ros4',) to use the stiff stepper")
        hipbind.check(hipbind.lib().rmt_n2_ros4(self.h, C.c_void_p(y.data_ptr()), float(t0), float(t1),
                                                float(rtol), float(atol), float(h0), int(max_steps),
                                                C.c_void_p(self._stats.data_ptr())))

    def attach_march(self, sens=None):
        """A second handle on the same member rows whose code object holds the steady-state march (march_plan): the
        stepper's own code object stays what it is without it.  steady_march / march_result then go through it.
        ``sens`` = (n_params, mechanism, rows) (solver-config "sensitivity"): with the run's own mechanism the handle's code
        object is the sensitivity unit (sens_plan) - the march kernel in it is the march unit's text - and steady_sens goes
        through it as well.  With another mechanism (a "rate-constant" the run keeps a literal is a per-reactor input
        there, the rows are widened by it) the march stays on the plain march unit, so that the started state is the one
        of the run without the key, and a third handle holds the sensitivity unit for steady_sens alone."""
        if "march" not in self.features and self.march is None:
            if self.fp32 or getattr(self.mech, "model", "N2") != "N2":
                raise hipbind.RmtN2Error("the steady-state march is for model N2 in fp64")
            if sens is None or sens[1] is not self.mech:
                mech, rows, cp = self.mech, self.members, march_plan(self.mech, self.N, self.defines, self.members)
            else:
                n_params, mech, rows = sens
                cp = sens_plan(mech, self.N, n_params, self.defines, rows)
            self.march = N2Device(mech, rows, self.N, block=cp.block, npt=cp.npt, device=self.device.index,
                                  defines=cp.defines, specialize=False, features=cp.features, profile=self.profile)
            if sens is not None and sens[1] is not self.mech:
                n_params, mech, rows = sens
                cp = sens_plan(mech, self.N, n_params, self.defines, rows)
                self.sens = N2Device(mech, rows, self.N, block=cp.block, npt=cp.npt, device=self.device.index,
                                     defines=cp.defines, specialize=False, features=cp.features, profile=self.profile)
        return self

    def steady_sens(self, y, kinds, indices):
        """Parametric sensitivities of the steady state y (rmt_n2_steady_sens, behind steady_march on the same handle):
        returns the device tensor [E][NP][V+1][N] - per member and parameter d(scaled state)/d(row value) and, in row V,
        dP/d(row value).  ``kinds`` / ``indices``: sensitivity.Sensitivity.descriptors.  Queued on the stream, nothing is
        synchronised; status() reads the flags.  Needs a code object of sens_plan with RMT_SENS_NP = len(kinds)."""
        if self.sens is not None:
            return self.sens.steady_sens(y, kinds, indices)
        if "march" not in self.features and self.march is not None:
            return self.march.steady_sens(y, kinds, indices)
        self._chk_state(y)
        if str(self.defines.get(sensitivity.DEFINE, "0")) != "1" or int(self.defines[sensitivity.DEFINE_NP]) != len(kinds):
            raise hipbind.RmtN2Error("steady_sens needs the sensitivity unit (sens_plan) with RMT_SENS_NP = %d" % len(kinds))
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        assert kinds.shape == indices.shape and kinds.ndim == 1
        out = self.torch.zeros((self.E, len(kinds), self.mech.V + 1, self.N), dtype=self.torch.float64, device=self.device)
        hipbind.check(hipbind.lib().rmt_n2_steady_sens(self.h, C.c_void_p(y.data_ptr()), len(kinds),
                                                       kinds.ctypes.data_as(C.POINTER(C.c_int)),
                                                       indices.ctypes.data_as(C.POINTER(C.c_int)),
                                                       C.c_void_p(out.data_ptr())))
        return out

    def sens_status(self):
        """The status words of the handle steady_sens ran on, read and cleared (synchronises)."""
        if self.sens is not None:
            return self.sens.status()
        if "march" not in self.features and self.march is not None:
            return self.march.status()
        return self.status()

    def steady_march(self, y, tol=initial.DEFAULTS["tolerance"], max_iter=initial.DEFAULTS["max-iterations"]):
        """In place: every member's state becomes the discrete steady state f(y) = 0 of its device rows (a forced row: its
        values at the row's reference time), found by marching from the inlet with one V x V solve per node
        (rmt_n2_steady_march).  Queued on the stream, nothing is synchronised; march_result reads what came of it.
        Needs features=("march",), or attach_march()."""
        self._chk_state(y)
        if "march" not in self.features:
            if self.march is None:
                raise hipbind.RmtN2Error("create the device with features=('march',) or call attach_march() to use the "
                                         "steady-state march")
            return self.march.steady_march(y, tol, max_iter)
        hipbind.check(hipbind.lib().rmt_n2_steady_march(self.h, C.c_void_p(y.data_ptr()), float(tol), int(max_iter),
                                                        C.c_void_p(self._stats.data_ptr())))

    def march_result(self):
        """(stats, flags) of the last steady_march (synchronises): per member the worst node's scaled residual, the node
        that failed (-1: none), the largest per-node step count and the number of nodes that needed a rejected step; the
        status words, read and cleared."""
        if "march" not in self.features and self.march is not None:
            return self.march.march_result()
        raw = self._stats.cpu().numpy()
        its, damped = step_counts(raw)
        return ({"scaled-residual": raw[:, 0].copy(), "failed-node": raw[:, 1].astype(np.int64), "iterations": its,
                 "nodes-damped": damped}, self.status())

    def set_campaign_law(self, law):
        """Upload the deactivation law [E][5] = {k_ref, Ed, Tref, m, a_inf} (rmt_n2_set_campaign_law: one blocking copy).
        Needs the campaign unit (campaign_plan) and a profile table."""
        law = np.ascontiguousarray(law, dtype=np.float64)
        if law.shape != (self.E, len(campaign.LAW_KEYS)):
            raise hipbind.RmtN2Error("the law must be [E][5] = %r doubles (got %r)" % ((self.E, 5), law.shape))
        hipbind.check(hipbind.lib().rmt_n2_set_campaign_law(self.h, law.ctypes.data_as(C.POINTER(C.c_double))))
        self.law = law

    def campaign_step(self, y, dt, log_row, stats=None, tol=initial.DEFAULTS["tolerance"],
                      max_iter=initial.DEFAULTS["max-iterations"]):
        """One step of a campaign (rmt_n2_campaign_step): y becomes every member's steady state for the activities in the
        handle's table, which then move over ``dt`` seconds at the node temperatures of that state.  ``log_row``: device
        doubles [E][V+6]; ``stats``: device doubles [E][4] (default: the device's own, march_result reads them).  Queued on
        the stream, nothing is synchronised."""
        self._chk_state(y)
        stats = self._stats if stats is None else stats
        for t, n in ((log_row, self.E*(self.mech.V + campaign.LOG_EXTRA)), (stats, self.E*4)):
            assert t.is_cuda and t.dtype == self.torch.float64 and t.is_contiguous() and t.numel() == n, \
                "campaign_step: the log row is [E][V+6], the stats [E][4] device doubles"
        hipbind.check(hipbind.lib().rmt_n2_campaign_step(self.h, C.c_void_p(y.data_ptr()), float(dt), float(tol),
                                                         int(max_iter), C.c_void_p(log_row.data_ptr()),
                                                         C.c_void_p(stats.data_ptr())))

    def set_campaign_policy(self, rows, component, levels):
        """Upload the policy rows [E][4] = {target, lo, hi, tolerance}, the index of the held component and the levels
        [E] step 0 carries in (rmt_n2_set_campaign_policy: one blocking copy).  Needs the policy unit
        (campaign_policy_plan), a profile table and a law."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        levels = np.ascontiguousarray(levels, dtype=np.float64)
        if rows.shape != (self.E, campaign.POLICY_ROW) or levels.shape != (self.E,):
            raise hipbind.RmtN2Error("the policy rows must be [E][4] = %r doubles and the levels [E] (got %r and %r)"
                                     % ((self.E, 4), rows.shape, levels.shape))
        hipbind.check(hipbind.lib().rmt_n2_set_campaign_policy(self.h, rows.ctypes.data_as(C.POINTER(C.c_double)),
                                                               int(component), levels.ctypes.data_as(C.POINTER(C.c_double))))

    def campaign_policy_step(self, y, dt, log_row, policy_row, stats=None, tol=initial.DEFAULTS["tolerance"],
                             max_iter=initial.DEFAULTS["max-iterations"],
                             max_evaluations=campaign.POLICY_DEFAULTS["max-evaluations"]):
        """campaign_step with the coolant policy (rmt_n2_campaign_policy_step): y becomes every member's steady state at the
        coolant level that holds the target (or at the better limit), the activities then move over ``dt`` seconds.
        ``policy_row``: device doubles [E][4] = {level, held, marches, saturated}.  Queued on the stream, nothing is
        synchronised."""
        self._chk_state(y)
        stats = self._stats if stats is None else stats
        for t, n in ((log_row, self.E*(self.mech.V + campaign.LOG_EXTRA)), (policy_row, self.E*campaign.POLICY_LOG),
                     (stats, self.E*4)):
            assert t.is_cuda and t.dtype == self.torch.float64 and t.is_contiguous() and t.numel() == n, \
                "campaign_policy_step: the log row is [E][V+6], the policy row [E][4], the stats [E][4] device doubles"
        hipbind.check(hipbind.lib().rmt_n2_campaign_policy_step(
            self.h, C.c_void_p(y.data_ptr()), float(dt), float(tol), int(max_iter), int(max_evaluations),
            C.c_void_p(log_row.data_ptr()), C.c_void_p(policy_row.data_ptr()), C.c_void_p(stats.data_ptr())))

    def get_campaign_level(self):
        """The carried coolant levels [E] as they are now (rmt_n2_get_campaign_level; synchronises the stream)."""
        out = np.zeros(self.E)
        hipbind.check(hipbind.lib().rmt_n2_get_campaign_level(self.h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def get_profile(self):
        """The handle's table [E][2][N] as it is now (rmt_n2_get_profile; synchronises the stream): the activities the
        campaign steps have written, and the coolant offsets."""
        out = np.zeros((self.E, 2, self.N))
        hipbind.check(hipbind.lib().rmt_n2_get_profile(self.h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def n1_profile(self, rows1, nout, rtol, atol, h0, max_steps, V1=None):
        """Steady-state model N1 (needs features=("n1",)): one profile per member row of ``rows1`` (layout M1_*),
        sampled at z* = k/(nout-1); returns the host array [E][nout][S+2] (S+1 when iso-thermal).  A module generated
        for another steady model (RMT_SS_MODEL, steady.py) passes its own number of unknowns V1."""
        torch = self.torch
        rows1 = np.ascontiguousarray(rows1, dtype=np.float64).reshape(self.E, self.mech.row_width)
        if V1 is None:
            V1 = self.mech.S + (1 if self.mech.iso else 2)
        out = torch.zeros((self.E, int(nout), V1), dtype=torch.float64, device=self.device)
        hipbind.check(hipbind.lib().rmt_n1_profile(
            self.h, rows1.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(out.data_ptr()), int(nout),
            float(rtol), float(atol), float(h0), int(max_steps), C.c_void_p(self._stats.data_ptr())))
        return out.cpu().numpy()

    def rk45_stats(self):
        raw = self._stats.cpu().numpy()
        acc, rej = step_counts(raw)
        return {"t_end": raw[:, 0].copy(), "h_last": raw[:, 1].copy(), "accepted": acc, "rejected": rej}

    def status(self):
        flags = np.zeros(self.E, dtype=np.uint32)
        hipbind.check(hipbind.lib().rmt_n2_status(self.h, flags.ctypes.data_as(C.POINTER(C.c_uint32))))
        return flags

    def last_geometry(self):
        """(workgroups per reactor, teams) of the last rk4 / rk45 / ros4 launch - what the library's auto mode chose."""
        c, t = C.c_int(), C.c_int()
        hipbind.check(hipbind.lib().rmt_n2_last_geometry(self.h, C.byref(c), C.byref(t)))
        return c.value, t.value

    def fallbacks(self):
        """Reactor-launches the cached RK4 steppers handed to their plain twins so far (rmt_n2_fallbacks): a reactor whose
        temperature left the range of its cached rate constants during a launch is integrated again in full."""
        n = C.c_uint64()
        hipbind.check(hipbind.lib().rmt_n2_fallbacks(self.h, C.byref(n)))
        return int(n.value)

    def last_kernel_ms(self):
        ms = C.c_float()
        hipbind.check(hipbind.lib().rmt_n2_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def raise_on_flags(self):
        err = flag_error(self.status())
        if err is not None:
            raise err


class AutoStepper:
    """ivp "hip-auto": the device counterpart of LSODA's automatic method switching (what the reference's default
    `solve_ivp(..., method="LSODA")` does, pbHomoReactor.py:3576, 3609), decided per output interval and for the
    whole ensemble at once:

      * the first interval starts with a PROBE: at most `auto-probe-steps` Dormand-Prince steps.  If they reach
        the end of the interval the problem is not stiff at this scale and the explicit pair carries on.
      * otherwise the step size the controller settled on tells how many explicit steps the interval would cost
        ((t1 - t0) / min h_last: the explicit pair sits at its stability limit ~3.3/|lambda| on a stiff problem).
        Up to `auto-max-explicit-steps` the interval is redone with the explicit pair, beyond that the
        Rosenbrock stepper takes over - for good (chemistry gets stiffer as the bed heats up, not milder).
      * an explicit interval that exhausts its step budget is redone with the stiff stepper as well, and one that
        needed more than `auto-max-explicit-steps` steps is the last explicit one.

    Two devices (the on-chip RK45 geometry and the Rosenbrock kernel family) share the state tensor."""
    stream_ordered = False                  # the host decides between two launches

    def __init__(self, dev_rk45, dev_ros4):
        """dev_ros4: the stiff device, or a zero-argument factory for it (single-process runs build - and JIT-
        compile - the Rosenbrock kernel family only when the problem turns out to be stiff)."""
        self.d45, self._dr = dev_rk45, dev_ros4
        self.mode = None                    # None: undecided, "rk45", "ros4"
        self.last = dev_rk45
        self.rhs_evals = 0
        self.choices = []
        self.jacobian_evals = dev_rk45.jacobian_evals
        self.prev_steps = 0
        self._started = {"rk45": False, "ros4": False}

    @property
    def dr(self):
        if callable(self._dr):
            self._dr = self._dr()
            if getattr(self, "_rows", None) is not None:
                self._dr.set_members(self._rows)
            if getattr(self, "_loop", None) is not None:      # (its rows came from the host: the held value again)
                self._dr.control(None, self._loop)
        return self._dr

    def set_members(self, rows):
        """the member rows of the next launch, for both devices (a forced run refreshes them before every launch)"""
        self._rows = rows
        self.d45.set_members(rows)
        if not callable(self._dr):
            self._dr.set_members(rows)

    def to_device(self, y):
        return self.d45.to_device(y)

    def close(self):
        self.d45.close()
        if not callable(self._dr):
            self._dr.close()

    def rk45_stats(self):
        return self.last.rk45_stats()

    def attach_march(self, sens=None):
        self.d45.attach_march(sens)
        return self

    def steady_sens(self, y, kinds, indices):
        return self.d45.steady_sens(y, kinds, indices)

    def sens_status(self):
        return self.d45.sens_status()

    def steady_march(self, y, tol=initial.DEFAULTS["tolerance"], max_iter=initial.DEFAULTS["max-iterations"]):
        """the steady-state march on the rows of the explicit device (both devices hold the same rows)"""
        self.d45.steady_march(y, tol, max_iter)

    def march_result(self):
        return self.d45.march_result()

    def monitor(self, y, out, residual=False):
        self.last.monitor(y, out, residual)

    def control(self, y, loop, k=None):
        """the controller's kernel for both devices: the explicit one takes the sample, the stiff one - once it exists -
        has the held value written into its own rows"""
        self._loop = loop
        self.d45.control(y, loop, k)
        if not callable(self._dr):
            self._dr.control(y, loop, None)

    def raise_on_flags(self):
        self.last.raise_on_flags()

    def last_geometry(self):
        return self.last.last_geometry()

    @property
    def _stats(self):
        return self.last._stats

    def _run(self, which, y, t0, t1, cfg, max_steps):
        dev = self.d45 if which == "rk45" else self.dr
        rtol, atol, h0, _ = stepper_args(cfg, which, not self._started[which], auto=True)
        self._started[which] = True
        getattr(dev, which)(y, t0, t1, rtol, atol, h0, int(max_steps))
        self.last = dev
        return dev

    def _explicit(self, y, t0, t1, cfg, budget):
        """One explicit attempt; True when every reactor reached t1 (other failures are left for raise_on_flags)."""
        dev = self._run("rk45", y, t0, t1, cfg, budget)
        st = dev.rk45_stats()
        tried = st["accepted"] + st["rejected"]
        self.rhs_evals += int(np.sum(6*tried) + dev.E)
        done = bool(np.all(st["t_end"] >= t1))
        if not done:
            err = flag_error(dev.status() & ~np.uint32(FLAG_STEP))       # read and clear: only the step budget may be set
            if err is not None:             # a genuine failure
                raise err
        return done, st

    def advance(self, y, t0, t1, cfg):
        hard_max = stepper_args(cfg, "ros4", False)[3]
        if self.mode != "ros4":
            backup = y.clone()
            if self.mode is None:
                done, st = self._explicit(y, t0, t1, cfg, min(hard_max, DEVICE_DEFAULTS['auto-probe-steps']))
                if done:
                    self.mode = "rk45"
                else:
                    hmin = float(np.min(st["h_last"]))
                    est = (t1 - t0)/max(hmin, 1e-300)
                    y.copy_(backup)
                    self._started["rk45"] = False
                    self.mode = "rk45" if est <= DEVICE_DEFAULTS['auto-max-explicit-steps'] else "ros4"
                    if self.mode == "rk45":
                        done, st = self._explicit(y, t0, t1, cfg, min(hard_max, int(4*est) + 200))
                        if not done:
                            y.copy_(backup)
                            self.mode = "ros4"
            else:
                done, st = self._explicit(y, t0, t1, cfg, min(hard_max, 4*self.prev_steps + 200))
                if not done:
                    y.copy_(backup)
                    self.mode = "ros4"
            if self.mode == "rk45":
                self.prev_steps = int(np.max(st["accepted"] + st["rejected"]))
                self.choices.append("rk45")
                if self.prev_steps > DEVICE_DEFAULTS['auto-max-explicit-steps']:
                    self.mode = "ros4"          # the interval just taken was too expensive explicitly: hand over
                return
        dev = self._run("ros4", y, t0, t1, cfg, hard_max)
        st = dev.rk45_stats()
        self.rhs_evals += int(np.sum((6 + dev.jacobian_evals)*(st["accepted"] + st["rejected"])))
        self.choices.append("ros4")


# --------------------------------------------------------------------------- result packing
def pack_interval(Y, named, mech, zNo, t_end, modelId):
    """One dataPack entry (pbHomoReactor.py:3630-3678; sortResult5, solResultAnalysis.py:252-301)."""
    S = mech.S
    Y = np.reshape(np.asarray(Y, dtype=np.float64), (mech.V, zNo))
    conc_dl = Y[:-1] if not mech.iso else Y[:]
    # dataYCons1 is dataYs_Reshaped[:-1] for BOTH process types in the reference (:3636): with V = S
    # (iso-thermal) that silently drops the last species; the schema is the spec, so it is mirrored
    cons1 = Y[:-1]
    temp_dl = Y[-1] if not mech.iso else np.repeat(0, zNo).reshape(zNo)
    conc = conc_dl*named["Cmax"]
    T_dl_row = Y[-1, :].reshape((1, zNo)) if not mech.iso else np.repeat(0, zNo).reshape((1, zNo))
    Treal = T_dl_row*named["Tf"] + named["Tf"]
    mofr = conc/np.sum(conc, axis=0)
    labelList = list(mech.compList) + ["Temperature"]
    return {
        "modelId": modelId, "processType": mech.processType, "successStatus": True,
        "dataShape": np.array(t_end).shape, "labelList": labelList, "indexList": [S, S + 1, S],
        "dataTime": t_end, "dataXs": np.linspace(0, 1, zNo),
        "dataYCons1": cons1, "dataYCons2": conc, "dataYTemp1": temp_dl, "dataYTemp2": Treal,
        "dataYs": np.concatenate((mofr, Treal), axis=0),
    }


def pack_intervals(Yg, named, mech, zNo, t_end, modelId):
    """pack_interval for EVERY member of an ensemble at once (Yg: [E][V*zNo]) - the arithmetic of sortResult5 as
    array operations over the member axis; entry e equals pack_interval(Yg[e], named[e], ...) bit for bit (same
    elementwise operations, the species sum taken in the same order).  A 2048-member sweep packs in ~10 ms per output
    time instead of 2048 Python-level passes (27 us each: several times the 50 ms the device needs for the sweep)."""
    S, E = mech.S, len(named)
    Y = np.reshape(np.asarray(Yg, dtype=np.float64), (E, mech.V, zNo))
    cmax = np.array([nm["Cmax"] for nm in named], dtype=np.float64).reshape(E, 1, 1)
    tf = np.array([nm["Tf"] for nm in named], dtype=np.float64).reshape(E, 1, 1)
    conc_dl = Y[:, :-1] if not mech.iso else Y
    conc = conc_dl*cmax
    if mech.iso:
        T_dl = np.zeros((E, 1, zNo), dtype=np.int64)          # np.repeat(0, zNo) of the reference: integer zeros
    else:
        T_dl = Y[:, -1:, :]
    Treal = T_dl*tf + tf
    mofr = conc/np.sum(conc, axis=1, keepdims=True)
    dataYs = np.concatenate((mofr, Treal), axis=1)
    labelList = list(mech.compList) + ["Temperature"]
    xs = np.linspace(0, 1, zNo) if zNo > 1 else np.array([1.0])
    shape = np.array(t_end).shape
    return [{
        "modelId": modelId, "processType": mech.processType, "successStatus": True,
        "dataShape": shape, "labelList": list(labelList), "indexList": [S, S + 1, S],
        "dataTime": t_end, "dataXs": xs,
        "dataYCons1": Y[e, :-1], "dataYCons2": conc[e], "dataYTemp1": T_dl[e, 0], "dataYTemp2": Treal[e],
        "dataYs": dataYs[e],
    } for e in range(E)]


def _progress(i, total, quiet):
    if quiet:
        return
    pct = ("{0:.1f}").format(100*(i/float(total)))
    filled = int(50*i//total)
    print('\rProgress: |%s| %s%% Complete' % ('█'*filled + '-'*(50 - filled), pct),
          end="\r" if i < total else "\n")


def compile_mechanism(mech, N, fp32=False, block=None, npt=None, lds_state=None, defines=None,
                      arch="gfx950", E=None, extra_opts="", features=()):
    """Code object for (mechanism, mesh size, members per rank) - what ensemble rank 0 compiles
    and broadcasts; pass the same E/block/npt/lds_state/defines/features to N2Device(code=...)."""
    return compile_plan(mech, fp32, code_plan(mech, N, fp32, E, block, npt, lds_state, defines, features), arch, extra_opts)


def resolve_ivp(ivp):
    """the reference's "default" is SciPy's LSODA (pbHomoReactor.py:3576) - Adams / BDF with AUTOMATIC
    stiffness detection: it maps to "hip-auto" (AutoStepper below: explicit Dormand-Prince while the problem is
    not stiff, the Rosenbrock stepper when it is); SciPy's always-implicit choices BDF / Radau map to the
    device's stiff Rosenbrock stepper, the explicit pairs to the device Dormand-Prince stepper."""
    ivp = {"default": "hip-auto", "LSODA": "hip-auto", "BDF": "hip-ros4", "Radau": "hip-ros4",
           "RK45": "hip-rk45", "RK23": "hip-rk45", "DOP853": "hip-rk45"}.get(ivp, ivp)
    if ivp not in DEVICE_IVPS:
        raise ValueError("`ivp` must be one of %s, 'default' or a SciPy method name (got %r)"
                         % (DEVICE_IVPS, ivp))
    return ivp


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


def device_cls():
    """The device class the ensemble path instantiates (looked up at call time: the gloo CPU tests put a
    host-emulation stand-in here, tests/emu_device.py)."""
    return N2Device


def mechanism_for(modelInput, inputs, cfg):
    """The ONE compiled mechanism of a launch: the base input's, with every scalar VARS constant that differs
    between the members (ensemble.member_parameters - which also refuses members that differ in anything the
    member row cannot express) or that solver-config "vars-as-parameters" names kept as a per-reactor parameter."""
    params = list(cfg.get('vars-as-parameters', ()))
    if len(inputs) > 1 or inputs[0] is not modelInput:
        from .ensemble import member_parameters
        varying = member_parameters(modelInput, inputs)
        VARS = modelInput['reaction-rates']['VARS']
        params = [k for k in VARS if k in params or k in varying] + [k for k in params if k not in VARS]
    return plan.Mechanism(modelInput, params=params)


def open_members(mech, inputs, zNo, pack, init, sync=None, fp32=False, block=None, npt=None, defines=None,
                 features=(), forcing=None, march=False, prof=None, sens=None):
    """Device + initial state for the members THIS process integrates.

    Single process: all of ``inputs``.  As one rank of a torch.distributed job (``sync``, see
    ensemble.RankSync): the rank's contiguous block; rank 0 compiles, every rank loads the broadcast
    code object, sweep-invariant member fields agreed over all ranks become kernel literals.
    Returns (device, named constants of the local members, local initial states [E_local][V*N]).
    ``forcing`` (a Forcing, solver-config "schedule"): the code object is generated with RMT_FORCING (2 when the schedule
    moves the feed composition, else 1), the rows get their tail, and the host fixes the kernel form (forced_mode).
    ``march`` (solver-config "initial", single process): a second handle on the same rows holds the steady-state march
    (N2Device.attach_march); with ``sens`` (a sensitivity.Sensitivity, solver-config "sensitivity") that handle's code
    object is the sensitivity unit (sens_plan) and ``sens.mech`` / ``sens.rows`` receive its mechanism and rows.
    ``prof`` (a profile.Profile, solver-config "axial-profile", single process): the code object is generated with
    RMT_PROFILE, the table is uploaded before anything is launched, and the host fixes the kernel form by the rule of the
    forced runs (no chained form carries the profile)."""
    if prof is not None and sync is not None:
        raise NotImplementedError("solver-config 'axial-profile' is not available in a multi-rank run")
    if march and sync is not None:
        raise NotImplementedError("solver-config 'initial' is not available in a multi-rank run")
    if forcing is not None:
        defines = {**(defines or {}), "RMT_FORCING": forcing.sched.forcing_level}
    if sync is None:
        pairs = [pack(mi, mech, zNo) for mi in inputs]
        rows = np.array([r for _, r in pairs])
        IV = plan.initial_states([nm for nm, _ in pairs], mech, zNo, init)
        if forcing is not None:
            rows = forcing.attach(rows, [nm for nm, _ in pairs])
        extra = {} if prof is None else {"profile": prof.table()}
        dev = device_cls()(mech, rows, zNo, fp32=fp32, block=block, npt=npt, defines=defines, features=features, **extra)
        if forcing is not None:
            forcing.fix_mode(dev, "hip-ros4" if "ros4" in features else "explicit")
        elif prof is not None:
            prof.modes["ros4" if "ros4" in features else "explicit"] = mode = forced_mode(
                "hip-ros4" if "ros4" in features else "explicit", zNo, dev.block, dev.npt, prof.want_mode,
                "axial-profile", "profile")
            dev.set_mode(mode)
        if march:
            try:
                if sens is not None:
                    sens.mech = mech if sens.unit_params(mech.params) == tuple(mech.params) \
                        else plan.Mechanism(inputs[0], params=sens.unit_params(mech.params))
                    sens.rows = sens.widen(rows, mech, sens.mech, inputs)
                dev.attach_march(None if sens is None else (sens.NP, sens.mech, sens.rows))
            except Exception:
                dev.close()
                raise
        return dev, [nm for nm, _ in pairs], IV
    # Multi-rank: every rank-LOCAL phase (packing, the rank-0 compile inside DistributedEnsemble, loading the
    # module and allocating on the device) runs under ensemble.guarded / agree: a failure on one rank is raised
    # on every rank instead of leaving the others in the next collective until the backend's timeout.
    defs = dict(defines or {})
    if getattr(mech, "model", "N2") == "M2" and "RMT_M2_NEWTON" not in defs:
        sweeps = guarded(sync, lambda: plan.m2_newton_sweeps(
            np.array([pack(mi, mech, zNo)[1] for mi in inputs[sync.lo:sync.hi]]), mech, zNo))
        defs["RMT_M2_NEWTON"] = str(sync.max_int(sweeps))
    arch = device_arch()

    def planned(mdef):      # one geometry for all ranks (block sizes differ by <= 1 member); the literals they agreed on
        return code_plan(mech, zNo, fp32, max(sync.counts), block, npt, None, defs, features, literals=mdef)
    ens = DistributedEnsemble(mech, inputs, zNo, group=sync.group, device=sync.device,
                              compile_fn=lambda mdef: compile_plan(mech, fp32, planned(mdef), arch))
    rows = ens.rows if forcing is None else guarded(sync, forcing.attach, ens.rows, ens.named)
    # (the device re-derives the same record from its fields: code_plan leaves its own decisions alone)
    cp = planned(ens.member_defines)
    dev = guarded(sync, device_cls(), mech, rows, zNo, fp32=fp32, block=cp.block, npt=cp.npt, lds_state=cp.lds_state,
                  defines=cp.defines, specialize=False, code=ens.code, features=features)
    if forcing is not None:
        guarded(sync, forcing.fix_mode, dev, "hip-ros4" if "ros4" in features else "explicit")
    return dev, ens.named, ens.IV


def open_auto(mech, inputs, zNo, pack, init, sync, fp32, defines, block=None, npt=None, forcing=None, march=False,
              prof=None, sens=None):
    """The two devices of ivp "hip-auto" (explicit pair in its on-chip geometry, Rosenbrock family) behind one
    AutoStepper; an explicit `block` / `nodes-per-thread` of the solver-config applies to the explicit device."""
    if block is None and (forcing is not None or prof is not None):       # (no chained chunks: they carry neither)
        b45, n45, d45 = rk45_geometry(mech.V, zNo, fp32, chain=False)
    elif block is None:
        b45, n45, d45 = rk45_geometry(mech.V, zNo, fp32, E=len(inputs) if sync is None else max(sync.counts))
    else:
        b45, n45, d45 = block, npt, {}
    dev45, named_local, IV = open_members(mech, inputs, zNo, pack, init, sync, fp32=fp32, block=b45, npt=n45,
                                          defines={**(defines or {}), **d45}, forcing=forcing, march=march, prof=prof,
                                          sens=sens)
    def make_ros4():
        return open_members(mech, inputs, zNo, pack, init, sync, fp32=fp32, block=ros4_block(mech.V, zNo, fp32),
                            npt=1, defines=defines, features=("ros4",), forcing=forcing, prof=prof)[0]
    if sync is None:
        return AutoStepper(dev45, make_ros4), named_local, IV       # built only if the problem turns out stiff
    try:        # multi-rank: creation involves collectives and the ranks may decide differently -> build it now
        devr = make_ros4()
    except Exception:
        dev45.close()
        raise
    return AutoStepper(dev45, devr), named_local, IV


def finish_stats(stats, ivp, n_members, tNo, zNo, jacobian_evals):
    """Totals of the device-stats record from the per-member step counts."""
    if stats.get("accepted") is not None:
        # adaptive steppers: "steps" is the sum over the members; per attempted step the Dormand-Prince
        # pair costs 6 RHS evaluations (FSAL; +1 for the first step of a launch), RODAS4 6 stage
        # evaluations + the node Jacobian (jacobian_evals node-function evaluations)
        tried = stats["accepted"] + stats["rejected"]
        stats["steps"] = int(np.sum(stats["accepted"]))
        if ivp == "hip-rk45":
            stats["rhs_evals"] = int(np.sum(6*tried) + n_members*tNo)
        else:
            stats["rhs_evals"] = int(np.sum((6 + jacobian_evals)*tried))
        stats["node_steps"] = stats["steps"]*zNo
    else:
        stats["node_steps"] = stats["steps"]*zNo*n_members
    return stats


def gather_stats(stats, sync, ivp, tNo, zNo, jacobian_evals):
    """Rank 0: the record for the WHOLE ensemble (per-member step counts gathered); other ranks keep theirs."""
    if stats.get("accepted") is not None:
        acc, rej = sync.gather(stats["accepted"]), sync.gather(stats["rejected"])
        if acc is not None:
            stats["accepted"], stats["rejected"] = acc, rej
    n = sync.n_total if sync.rank == 0 else sync.hi - sync.lo
    stats["ranks"] = sync.world
    return finish_stats(stats, ivp, n, tNo, zNo, jacobian_evals)


def outlet_only(cfg):
    """solver-config "ensemble-output": "outlet" - only the outlet node of every member leaves the device (and, in a
    multi-rank job, travels to rank 0) per output time: E x V doubles instead of the E x V x zNo state (117 MB per
    output time for 2048 x 1024 nodes).  The dataPack entries keep their schema with ONE axial column (dataXs = [1])."""
    out = cfg.get('ensemble-output', 'profile')
    if out not in ('profile', 'outlet'):
        raise ValueError("solver-config 'ensemble-output' must be 'profile' or 'outlet' (got %r)" % (out,))
    return out == 'outlet'


class Forcing:
    """A parsed schedule bound to one run: the local members' ordinary rows and the refresh of the device rows ahead of
    every launch of the run's list (schedule.Schedule.forced_rows)."""

    def __init__(self, sched, walk, N, want_mode=None):
        self.sched, self.N, self.want_mode = sched, int(N), want_mode
        self.first = walk[0].t0, walk[0].t1
        self.rows = self.named = None
        self.modes = {}

    def attach(self, rows, named):
        """the local members' rows -> the forced rows of the first launch (called where the device is created)"""
        if self.rows is None:
            if self.sched.E != len(named):          # one rank's block of the ensemble
                raise ValueError("solver-config 'schedule': %d member rows for a schedule of %d members"
                                 % (len(named), self.sched.E))
            self.rows, self.named = np.array(rows, dtype=np.float64), list(named)
        return self.sched.forced_rows(self.rows, self.named, *self.first)

    def fix_mode(self, dev, ivp):
        mode = forced_mode(ivp, self.N, dev.block, dev.npt, self.want_mode)
        dev.set_mode(mode)
        self.modes["ros4" if ivp == "hip-ros4" else "explicit"] = mode

    def refresh(self, dev, t0, t1, queued=False):
        """the rows of the launch (t0, t1) onto the device; ``queued`` (a stream-ordered device): between the queued
        launches, returns what has to stay alive until the stream got there"""
        rows = self.sched.forced_rows(self.rows, self.named, t0, t1)
        if queued:
            return dev.set_members_async(rows)
        dev.set_members(rows)
        return None


class ControlLoop:
    """The device side of one run's controllers (control.Control): the kernel's module and its buffers - parameter blocks
    [E][8], setpoints [K][E], controller state [E][3] and the log [K][E][4], which comes back once, at the end."""

    def __init__(self, ctl, dev):
        d = getattr(dev, "d45", dev)                  # ("hip-auto": both devices live on the same GPU)
        torch = d.torch
        self.ctl, self.E, self.field = ctl, ctl.E, ctl.field
        with torch.cuda.device(d.device):
            self.kernel = hipbind.Control(device_arch(d.device))
        self.params = torch.from_numpy(ctl.params()).to(d.device)
        self.setpoints = torch.from_numpy(np.ascontiguousarray(ctl.setpoints)).to(d.device)
        self.state = torch.zeros((ctl.E, control.STATE), dtype=torch.float64, device=d.device)
        self.log = torch.zeros((ctl.K, ctl.E, control.LOG), dtype=torch.float64, device=d.device)
        self.taken = 0

    def close(self):
        self.kernel.close()


PIPELINE_BYTES = 1 << 30       # pinned host memory one batch of queued output intervals may hold (integrate_intervals)


def integrate_intervals(dev, y, cfg, ivp, walk, n_members, zNo, quiet, on_interval, sync=None, outlet=False,
                        forcing=None, mon=None, ctl=None):
    """The reference's time loop (pbHomoReactor.py:3589-3690, pbReactor.py:711-762): one device launch per entry of
    ``walk`` (the list of launches.merge: without "schedule", "monitor" and "control" one per output interval);
    ``on_interval(i, t1, Y_host)`` packs the end state ([E][V*zNo], or [E][V] = the outlet node with ``outlet``) of a launch
    that ends at an output time.  With ``sync`` (multi-rank ensemble) a failure on any rank is raised on every rank before
    the next gather.  Returns (stats, raw): the statistics record and the one-off device buffers
    {"monitor": [K][E_local][V][5] or None, "control": [K][E_local][4] or None}.
    ``forcing`` (solver-config "schedule"): the device rows are refreshed before each launch is queued.
    ``mon`` (a monitor.Monitor, solver-config "monitor"): behind a launch that ends at sample k the row reductions of the
    state are queued into slice k of ONE device buffer [K][E][V][5] (sample 0 before the first launch; with "residual"
    behind rmt_n2_rhs at that state).  Nothing is copied or synchronised per sample: the buffer comes back once, at the
    end.  A run that raises on flags returns no monitor.
    ``ctl`` (a control.Control, solver-config "control"; needs ``forcing``): the order in the stream for every launch is:
    refresh of the rows, the controller's kernel, the stepper - the update when the launch starts at a sample time, else
    (once a sample has been taken) the rewrite of the held value, because the refresh uploads whole rows.  The log comes
    back once, at the end."""
    import torch
    nL = len(walk)
    loop = ControlLoop(ctl, dev) if ctl is not None else None
    mbuf = None
    if mon is not None:
        mbuf = torch.zeros((mon.K, y.shape[0], y.shape[1]//zNo, monitor.SLOTS), dtype=torch.float64, device=y.device)

    def sample(k):
        if mbuf is not None and k is not None:
            dev.monitor(y, mbuf[k], mon.residual)
    stats = {"steps": 0, "rhs_evals": 0, "node_steps": 0, "accepted": None, "rejected": None}
    if mon is not None or ctl is not None:
        stats["launches"] = nL
    adaptive = ivp in ("hip-rk45", "hip-ros4", "hip-auto")

    def step(i, t0, t1):
        if ivp == "hip-rk4":
            dt_req = float(cfg.get('dt', DEVICE_DEFAULTS['rk4-dt']))
            n = max(1, int(round((t1 - t0)/dt_req)))
            dev.rk4(y, (t1 - t0)/n, n, t0)
            stats["steps"] += n
            stats["rhs_evals"] += 4*n
        elif ivp in ("AM", "hip-ab3"):
            # the reference's plug point: PreCorr3 with n fixed steps per output interval,
            # n from solverSetting['T1']['ode-solver']['PreCorr3']['n'] (pbHomoReactor.py:3572,3601)
            n = int(cfg.get('n', solverSetting['T1']['ode-solver']['PreCorr3']['n']))
            dev.multistep(y, abs(t1 - t0)/n, n, "PreCorr3" if ivp == "AM" else "AdBash3", t0)
            stats["steps"] += n
            stats["rhs_evals"] += (2*n + 6) if ivp == "AM" else (n + 8)
        elif ivp == "hip-auto":
            dev.advance(y, t0, t1, cfg)
        else:
            stepper = ivp[4:]                                    # "rk45" / "ros4"
            getattr(dev, stepper)(y, t0, t1, *stepper_args(cfg, stepper, i == 0))

    # One process, a stepper that needs no host decision between the intervals (a stream-ordered device): the launches of
    # SEVERAL output intervals are queued back to back, each followed in the stream by the copy of its end state into
    # pinned host memory (and of its step counters), and the host packs while the device integrates.  With a
    # synchronisation per interval the device idled - and clocked down - while the host packed: 0.18 s for the bench's
    # 256-member sweep against 0.04 s of kernel time.  The status words are sticky, so one look at the end of a batch
    # raises what any of its launches flagged.  Batches are bounded by PIPELINE_BYTES of pinned memory.
    # Every other run (multi-rank, "hip-auto", the host-emulation stand-in) is the same walk with batches of ONE launch
    # and blocking copies; with ``sync`` the flags are read - and agreed on - inside the rank-local phase, ahead of the
    # gather in on_interval.  (A device class that does not declare ``stream_ordered`` - a stand-in written before the
    # attribute existed - is not: the synchronous walk asks nothing of it beyond the stepper and raise_on_flags.)
    queued = sync is None and getattr(dev, "stream_ordered", False)
    E_loc = y.shape[0]
    per = E_loc*(y.shape[1]//zNo if outlet else y.shape[1])*y.element_size()
    batch = int(max(1, min(nL, PIPELINE_BYTES//max(per, 1)))) if queued else 1

    def to_host(src):
        if not queued:
            return src.cpu()
        host = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
        host.copy_(src, non_blocking=True)                       # stream-ordered: reads src before the next launch writes it
        return host

    def queue(lo, hi):
        staged = []
        for i in range(lo, hi):
            launch = walk[i]
            _progress(i + 1, nL + 1, quiet)
            # (the page-locked rows of a queued refresh stay alive until the batch has landed)
            rows = forcing.refresh(dev, launch.t0, launch.t1, queued) if forcing is not None else None
            if loop is not None and (launch.control is not None or loop.taken):
                dev.control(y, loop, launch.control)             # behind the refresh, ahead of the stepper
                loop.taken += launch.control is not None
            step(i, launch.t0, launch.t1)
            sample(launch.sample)                                # queued right behind its launch, into its slice
            state = counters = landed = None
            if launch.out is not None:
                state = to_host(y.reshape(E_loc, -1, zNo)[:, :, zNo - 1] if outlet else y)
            if adaptive:
                counters = to_host(dev._stats)
            if queued:
                landed = torch.cuda.Event()
                landed.record()
            staged.append((launch, state, counters, landed, rows))
        if sync is not None:
            dev.raise_on_flags()
        return staged

    _progress(0, nL + 1, quiet)
    guarded(sync, sample, 0)
    raw = {"monitor": None, "control": None}
    try:
        for lo in range(0, nL, batch):
            for launch, state, counters, landed, _ in guarded(sync, queue, lo, min(nL, lo + batch)):
                if landed is not None:                                # packing launch i while the device is at i+1, i+2, ...
                    landed.synchronize()
                if counters is not None:
                    acc, rej = step_counts(counters.numpy())
                    stats["accepted"] = acc if stats["accepted"] is None else stats["accepted"] + acc
                    stats["rejected"] = rej if stats["rejected"] is None else stats["rejected"] + rej
                if launch.out is not None:                            # (None: a breakpoint or a sample time - nothing to pack)
                    on_interval(launch.out - 1, launch.t1, state.numpy().astype(np.float64))
            if sync is None:
                dev.raise_on_flags()                                  # (sticky status words: whatever a launch of the batch flagged)
        if ivp == "hip-auto":
            stats["method-per-interval"] = list(dev.choices)
        if mbuf is not None:
            raw["monitor"] = mbuf.cpu().numpy()                       # the ONE copy of the monitor buffer
        if loop is not None:
            raw["control"] = loop.log.cpu().numpy()                   # the ONE copy of the controllers' log
    finally:
        if loop is not None:
            loop.close()
    if sync is not None:
        stats = gather_stats(stats, sync, ivp, nL, zNo, dev.jacobian_evals)
    else:
        stats = finish_stats(stats, ivp, n_members, nL, zNo, dev.jacobian_evals)
    if ivp == "hip-auto":
        stats["rhs_evals"] = dev.rhs_evals          # includes the probe and any abandoned explicit attempt
    return stats, raw


def attach_monitor(raw, sync, convert):
    """The monitor entries of every member, on the process that returns the results: the raw buffer integrate_intervals
    returned ([K][E_local][V][5]), gathered to rank 0 ONCE in a multi-rank job, each member converted by
    ``convert(e, raw [K][V][5])``.  None without a monitor and on the other ranks."""
    if raw is None:
        return None
    raw = np.ascontiguousarray(np.swapaxes(raw, 0, 1))            # [E_local][K][V][5]
    if sync is not None:
        raw = sync.gather(raw)
        if raw is None:
            return None
    return [convert(e, raw[e]) for e in range(raw.shape[0])]


def steady_profiles(modelInput, members_inputs, pack, nout, defines=None, extra=None, handle_rows=None):
    """What the steady-state models (n1.run_n1, steady.run_steady) share: pack the members' rows (``pack(mi, mech)`` ->
    (named, row)), open an N2 handle of the module with the steady kernel family, ONE guarded launch of n1_profile, and
    the gather of the profiles and step counts.  As one rank of a torch.distributed job a process integrates its
    contiguous block of profiles; every rank-local phase (packing, device creation, the launch + status read) runs under
    ensemble.guarded: a failure on one rank is raised on every rank before the next collective.
    ``extra``: the model has S + extra unknowns (default: model N1's own count, N2Device.n1_profile);
    ``handle_rows(inputs, mech)``: the handle's own N2 member rows where the steady rows do not serve (model N1).
    Returns (mech, named of every member, U [E][nout][V1], {"accepted", "rejected"}) on the process that returns the
    results (rank 0, or the only one), None on the other ranks."""
    cfg = modelInput['solver-config']
    all_inputs = list(members_inputs) if members_inputs else [modelInput]
    mech = mechanism_for(modelInput, all_inputs, cfg)
    sync = active_ranks(len(all_inputs)) if members_inputs else None
    inputs = all_inputs if sync is None else all_inputs[sync.lo:sync.hi]

    def pack_and_open():
        pairs = [pack(mi, mech) for mi in inputs]
        rows1 = np.ascontiguousarray(np.array([r for _, r in pairs]))
        # the handle is an N2 handle of the same generated module; only its steady kernel is used
        return pairs, rows1, device_cls()(mech, rows1 if handle_rows is None else handle_rows(inputs, mech), 64, block=64,
                                          npt=1, specialize=False, features=("n1",), defines=defines)
    pairs, rows1, dev = guarded(sync, pack_and_open)
    try:
        def launch():
            out = dev.n1_profile(rows1, nout, float(cfg.get('rtol', DEVICE_DEFAULTS['n1-rtol'])),
                                 float(cfg.get('atol', DEVICE_DEFAULTS['n1-atol'])), float(cfg.get('h0', 1e-6)),
                                 int(cfg.get('max-steps', 10**7)), V1=None if extra is None else mech.S + extra)
            dev.raise_on_flags()
            return dev.rk45_stats(), out
        stats, U = guarded(sync, launch)
    finally:
        dev.close()
    if sync is not None:                    # rank 0 returns every member's profile, the other ranks None
        U = sync.gather(U)
        stats = {k: sync.gather(stats[k]) for k in ("accepted", "rejected")}
        if U is None:
            return None
        pairs = [pack(mi, mech) for mi in all_inputs]
    return mech, [nm for nm, _ in pairs], U, stats


def start_steady(dev, y, ini, mech):
    """solver-config "initial": "steady" - the state y becomes every member's steady state (N2Device.steady_march on the
    device rows as they are), then rmt_n2_rhs and ONE monitor reduction measure max_n |dy/dt| of what the run starts from.
    Raises through flag_error when a member's march failed - the message names the member and the node; there is no
    fallback to the cold start.  Returns the members' result entries."""
    dev.steady_march(y, ini.tolerance, ini.max_iterations)
    st, flags = dev.march_result()
    err = flag_error(flags)
    if err is not None:
        e = int(np.nonzero(flags)[0][0])
        raise type(err)("solver-config 'initial': the steady-state march failed at node %d of member %d (%d pseudo-time "
                        "steps, 'max-iterations' = %d): %s"
                        % (int(st["failed-node"][e]), e, int(st["iterations"][e]), ini.max_iterations, err))
    E = y.shape[0]
    import torch
    out = torch.zeros((E, mech.V, monitor.SLOTS), dtype=torch.float64, device=y.device)
    dev.monitor(y, out, residual=True)
    res = out.cpu().numpy()[:, :, monitor.RESIDUAL].max(axis=1)
    dev.raise_on_flags()
    return [ini.result_entry(res[e], st["iterations"][e], st["nodes-damped"][e]) for e in range(E)]


def start_sensitivity(dev, y, sens, named):
    """solver-config "sensitivity": ONE launch of rmt_n2_steady_sens on the march handle behind the march that made y, the
    buffer [E][NP][V+1][N] comes back once.  Raises FloatingPointError naming the member and the node when a node of the
    tangent march is singular.  Returns the members' result entries."""
    kinds, indices = sens.descriptors(sens.mech)
    raw = dev.steady_sens(y, kinds, indices).cpu().numpy()
    flags = dev.sens_status()
    if np.any(flags):
        e = int(np.nonzero(flags)[0][0])
        raise FloatingPointError("solver-config 'sensitivity': the node Jacobian is singular (or a sensitivity is not "
                                 "finite) at node %d of member %d (flags=0x%x)"
                                 % (sensitivity.failed_node(raw[e]), e, int(flags[e])))
    Yh = y.cpu().numpy()
    return [sensitivity.result_entry(sens, raw[e], Yh[e], sens.rows[e], named[e], sens.mech) for e in range(raw.shape[0])]


def policy_error(cam, e, first, plog):
    """The exception for member ``e`` whose policy step gave up: ``plog`` [n][4] are its policy log rows from step ``first``
    on; the first row with `saturated` 2 (bracket collapsed) or 3 (evaluation limit) is the step that failed."""
    codes = plog[:, campaign.SATURATED].astype(np.int64)
    bad = np.nonzero(codes >= campaign.BRACKET_COLLAPSED)[0]
    j = int(bad[0]) if len(bad) else len(plog) - 1
    k, row, pol = first + j, plog[j], cam.policy
    where = ("member %d in step %d (time on stream %g s), after %d marches, at %.9g K with %s = %.12g against the target %.12g"
             % (e, k, cam.times[k], int(row[campaign.EVALUATIONS]), row[campaign.LEVEL], pol.component,
                row[campaign.HELD], pol.rows[e, 0]))
    if codes[j] == campaign.BRACKET_COLLAPSED:
        return RuntimeError("solver-config 'deactivation' 'policy': the bracket of the coolant level fell below %g K with the "
                            "held value outside its 'tolerance' = %g: %s - the outlet jumps there, a node changed its branch "
                            "of steady states" % (campaign.MIN_BRACKET, pol.tolerance, where))
    return RuntimeError("solver-config 'deactivation' 'policy': 'max-evaluations' = %d reached with the held value outside "
                        "its 'tolerance' = %g: %s" % (pol.max_evaluations, pol.tolerance, where))


def run_campaign(modelInput, members_inputs, cam, pack_all, result):
    """solver-config "deactivation" (campaign.py): the time-on-stream run of a quasi-steady bed.  Opens the members' rows
    with the campaign unit only (campaign_plan), uploads the fresh bed's table and the law, and queues one launch of
    rmt_n2_campaign_step per step (K + 1 launches; the log [K+1][E][V+6] and the march statistics [K+1][E][4] stay on the
    device and come back once).  At every output step the activities a(t_k) (before the launch), the state and the status
    words come to the host: a member whose march failed raises there through flag_error - the message names the member, the
    node, the step and its time on stream - and not behind launches queued after the failed one."""
    start = timer()
    cfg = modelInput['solver-config']
    zNo = int(cfg.get('zNo', solverSetting['N2']['zNo']))
    inputs = list(members_inputs) if members_inputs else [modelInput]
    mech = mechanism_for(modelInput, inputs, cfg)
    cam.check_budget(mech.V, PIPELINE_BYTES)
    prof = profile.parse(modelInput, members_inputs, None, False)
    pairs = [plan.member_constants(mi, mech, zNo) for mi in inputs]
    named, rows = [nm for nm, _ in pairs], np.array([r for _, r in pairs])
    E = len(inputs)
    table = prof.table() if prof is not None else np.stack([np.ones((E, zNo)), np.zeros((E, zNo))], axis=1)
    IV = plan.initial_states(named, mech, zNo, plan.initial_state)
    pol = cam.policy
    cp = campaign_plan(mech, zNo, rows) if pol is None else campaign_policy_plan(mech, zNo, rows)
    dev = device_cls()(mech, rows, zNo, block=cp.block, npt=cp.npt, defines=cp.defines, specialize=False,
                       features=cp.features, profile=table)
    try:
        import torch
        dev.set_campaign_law(cam.law)
        y = dev.to_device(IV)
        if pol is not None:                # the policy unit: the rows, and ONE more device buffer beside the log
            dev.set_campaign_policy(pol.rows, pol.index, pol.levels)
            plog = torch.zeros((cam.K + 1, E, campaign.POLICY_LOG), dtype=torch.float64, device=y.device)
        log = torch.zeros((cam.K + 1, E, mech.V + campaign.LOG_EXTRA), dtype=torch.float64, device=y.device)
        stats = torch.zeros((cam.K + 1, E, 4), dtype=torch.float64, device=y.device)
        marks = {int(k): i for i, k in enumerate(cam.output_steps)}
        acts, packs, checked = [table[:, 0].copy()], [[] for _ in named], 0
        for k, dt in enumerate(cam.dts()):
            if k in marks:
                acts.append(dev.get_profile()[:, 0] if k else table[:, 0].copy())       # a(t_k): launch k moves it on
            if pol is None:
                dev.campaign_step(y, dt, log[k], stats[k], cam.tolerance, cam.max_iterations)
            else:
                dev.campaign_policy_step(y, dt, log[k], plog[k], stats[k], cam.tolerance, cam.max_iterations,
                                         pol.max_evaluations)
            if k not in marks:
                continue
            Yh = y.cpu().numpy()
            flags = dev.status()
            err = flag_error(flags)
            if err is not None:
                e = int(np.nonzero(flags)[0][0])
                if int(flags[e]) & (campaign.FLAG_POLICY_BRACKET | campaign.FLAG_POLICY_EVALS):
                    raise policy_error(cam, e, checked, plog[checked:k + 1, e].cpu().numpy())
                st = stats[checked:k + 1, e].cpu().numpy()
                bad = np.nonzero(st[:, 1] >= 0)[0]
                j = int(bad[0]) if len(bad) else len(st) - 1
                raise type(err)("solver-config 'deactivation': the march failed at node %d of member %d in step %d (time "
                                "on stream %g s; %d pseudo-time steps, 'max-iterations' = %d): %s"
                                % (int(st[j, 1]), e, checked + j, cam.times[checked + j],
                                   int(step_counts(st[j:j + 1])[0][0]), cam.max_iterations, err))
            checked = k + 1
            for e, pk in enumerate(pack_all(Yh, named, mech, zNo, float(cam.times[k]))):
                packs[e].append(pk)
        logs = log.cpu().numpy()
        plogs = plog.cpu().numpy() if pol is not None else None
        raw = stats.cpu().numpy()
        dstats = {"launches": cam.K + 1, "steps": cam.K, "march-iterations": int(step_counts(raw.reshape(-1, 4))[0].max()),
                  "nodes-damped": int(step_counts(raw.reshape(-1, 4))[1].sum())}
    finally:
        dev.close()
    acts = np.array(acts)                                                   # [n_out+1][E][N]
    entries = [campaign.result_entry(cam, e, logs[:, e], acts[:, e], mech, zNo, named[e]) for e in range(E)]
    if pol is not None:
        for e, entry in enumerate(entries):
            entry[campaign.POLICY] = campaign.policy_entry(cam, e, plogs[:, e])
    res = result(packs[0], modelInput, zNo, cam.outputs)
    res["computation-time"] = np.round(timer() - start, ROUND_FUN_ACCURACY)
    res["device-stats"] = dstats
    if members_inputs:
        res["ensemble"] = [result(p, mi, zNo, cam.outputs) for p, mi in zip(packs, inputs)]
    res[campaign.KEY] = entries[0]
    if prof is not None:
        res["axial-profile"] = profile.result_entry(prof, 0)
    if members_inputs:
        for e, entry in enumerate(res["ensemble"]):
            entry[campaign.KEY] = entries[e]
            if prof is not None:
                entry["axial-profile"] = profile.result_entry(prof, e)
    return res


def run_dynamic(modelInput, members_inputs, model, pack, init, pack_all, result, fp32=False, defines=None,
                with_schedule=False, outlet=False, display=False):
    """What run_n2 and m2.run_m2 share: the ranks of a torchrun job, the geometry of the `ivp`, the device(s), the walk
    over the output intervals with the gather of every member's state on the process that returns the results, the
    monitor, and the result with its "ensemble" / "ensemble-shard" entries.  The models hand in what differs:
    ``pack`` / ``init`` (member constants and initial state), ``pack_all(Yg, named, mech, zNo, t1)`` (the dataPack entries
    of all members at one output time; zNo = 1 with ``outlet``), ``result(dataPack, member input, zNo, opTSpan)`` (one
    member's result dict), and whether fp32, "schedule", "ensemble-output" and "display-result" apply."""
    start = timer()
    cfg = modelInput['solver-config']
    ivp = resolve_ivp(cfg['ivp'])
    setting = solverSetting['N2' if model == "N2" else 'S2']        # (runM2 reads S2: pbReactor.py:625, :694)
    zNo, tNo = int(cfg.get('zNo', setting['zNo'])), int(cfg.get('tNo', setting['tNo']))
    quiet = bool(cfg.get('quiet', False))
    opT = modelInput['operating-conditions']['period']
    opTSpan = np.linspace(0, opT, tNo + 1)
    inputs = list(members_inputs) if members_inputs else [modelInput]
    mech = mechanism_for(modelInput, inputs, cfg)
    sync = active_ranks(len(inputs)) if members_inputs else None       # one rank of a torchrun job?
    E_gpu = len(inputs) if sync is None else max(sync.counts)
    block, npt = cfg.get('block'), cfg.get('nodes-per-thread')
    # "schedule": time-varying inlet / coolant conditions (schedule.py); absent = None = exactly the run without it
    sched = schedule.parse(modelInput, members_inputs, ivp) if with_schedule else None
    # "control": a sampled PI controller per member on the device (control.py); absent = None = exactly the run without it.
    # A controlled run is a forced run: without a "schedule" it gets a constant one of every member's own values.
    control.check_model(modelInput)
    ctl, forced_by = control.parse(modelInput, members_inputs, ivp, sched, sync is not None) if with_schedule \
        else (None, sched)
    if ctl is not None:
        ctl.check_budget(PIPELINE_BYTES)
    # "monitor": time series between the output times (monitor.py); absent = None = exactly the run without it
    mon = monitor.parse(modelInput, tNo)
    if mon is not None:
        mon.check_budget(len(inputs), mech.V, PIPELINE_BYTES)
    # "initial": where the run starts (initial.py); absent = None = the reference's cold start, exactly the run without it
    ini = initial.parse(modelInput, sync is not None) if with_schedule else None
    # "axial-profile": catalyst activity and coolant zones along the bed (profile.py); absent = None = exactly the run
    # without it
    profile.check_model(modelInput)
    prof = profile.parse(modelInput, members_inputs, ivp, sync is not None) if with_schedule else None
    # "sensitivity": parametric sensitivities of the steady state the run starts from (sensitivity.py); absent = None =
    # exactly the run without it
    sens = sensitivity.parse(modelInput, members_inputs, sync is not None) if with_schedule else None
    # the ONE launch list of the run; a sample that fell on a mark carries that mark's time from here on (result entries)
    walk, sample_times, control_times = launches.merge(
        opT, tNo, forced_by.times if forced_by is not None else (), mon.times if mon is not None else None,
        ctl.times if ctl is not None else None)
    if mon is not None:
        mon.times = sample_times
    if ctl is not None:
        ctl.times = control_times
    forcing = None
    if forced_by is not None:
        if ivp in ("hip-ros4", "hip-auto") and ros4_quad(mech, fp32):
            raise NotImplementedError("solver-config 'schedule' with the stiff stepper needs a mechanism of at most 8 "
                                      "variables per node (this one has %d): its four-lane form does not carry the "
                                      "forcing - use ivp 'hip-rk45' or 'hip-rk4'" % mech.V)
        forcing = Forcing(forced_by if sync is None else forced_by.members(sync.lo, sync.hi), walk, zNo,
                          cfg.get('device-mode'))
        if ivp == "hip-rk4" and block is None:
            # the geometry of ONE workgroup per reactor (no chunks: the chained kernels do not carry the forcing)
            block, npt = choose_geometry(zNo, mech.V, fp32)
    if prof is not None:
        if ivp in ("hip-ros4", "hip-auto") and ros4_quad(mech, fp32):
            raise NotImplementedError("solver-config 'axial-profile' with the stiff stepper needs a mechanism of at most 8 "
                                      "variables per node (this one has %d): its four-lane form does not carry the "
                                      "profile - use ivp 'hip-rk45' or 'hip-rk4'" % mech.V)
        prof.want_mode, prof.modes = cfg.get('device-mode'), {}
        if ivp == "hip-rk4" and block is None:          # ONE workgroup per reactor, as for a forced run
            block, npt = choose_geometry(zNo, mech.V, fp32)
    if ivp == "hip-ros4" and block is None:
        block, npt = ros4_block(mech.V, zNo, fp32, ros4_quad(mech, fp32)), 1
    defines = dict(defines or {})
    if ivp == "hip-rk45" and block is None:
        block, npt, geo_defs = rk45_geometry(mech.V, zNo, fp32, **({"chain": False} if forcing is not None or prof is not None
                                                                 else {"E": E_gpu}))
        defines.update(geo_defs)
    if ivp == "hip-auto":
        dev, named_local, IV = open_auto(mech, inputs, zNo, pack, init, sync, fp32, defines, block, npt, forcing=forcing,
                                         march=ini is not None, prof=prof, sens=sens)
    else:
        dev, named_local, IV = open_members(mech, inputs, zNo, pack, init, sync, fp32=fp32, block=block, npt=npt,
                                            defines=defines, features=("ros4",) if ivp == "hip-ros4" else (),
                                            forcing=forcing, march=ini is not None, prof=prof, sens=sens)
    # the process that returns the results (rank 0, or the only one) packs EVERY member
    packer = sync is None or sync.rank == 0
    try:
        if sync is None:
            named = named_local
        else:
            named = guarded(sync, lambda: [pack(mi, mech, zNo)[0] for mi in inputs] if packer else [])
        y = guarded(sync, dev.to_device, IV)
        # (the device rows are those of t = 0: a forced run's were attached for its first launch, which starts there)
        started = start_steady(dev, y, ini, mech) if ini is not None else None
        sensed = start_sensitivity(dev, y, sens, named) if sens is not None else None
        packs = [[] for _ in named]

        def on_interval(i, t1, Yh):
            Yg = Yh if sync is None else sync.gather(Yh)               # [E_total][V*N] (or [V]: outlet) on rank 0
            if Yg is not None:
                for e, pk in enumerate(pack_all(Yg, named, mech, 1 if outlet else zNo, t1)):
                    packs[e].append(pk)
        stats, raw = integrate_intervals(dev, y, cfg, ivp, walk, len(named_local), zNo, quiet or not packer,
                                         on_interval, sync, outlet, forcing, mon, ctl)
        logs = raw["control"]                                          # [K][E][4]
        monitors = attach_monitor(raw["monitor"], sync, lambda e, r: monitor.result_entry(
            r, mon.times, mech, zNo, named[e], model, inputs[e]['reactor']['ReLe'], mon.residual))
        if forcing is not None:
            # which kernel forms ran: "reg" = the on-chip steppers, "mem" = the memory-resident ones; and what
            # rmt_n2_last_geometry reports for the last launch (workgroups per reactor, teams)
            stats["device-mode"] = dict(forcing.modes)
            stats.setdefault("launches", len(walk))            # (a monitored or controlled run has it already)
            stats["last-geometry"] = dev.last_geometry()
        elif prof is not None:
            stats["device-mode"] = dict(prof.modes)
            stats["last-geometry"] = dev.last_geometry()
    finally:
        dev.close()
    res = result(packs[0] if packs else [], modelInput, zNo, opTSpan)
    res["computation-time"] = np.round(timer() - start, ROUND_FUN_ACCURACY)
    res["device-stats"] = stats
    if sched is not None:
        res["schedule"] = schedule.result_entry(sched, opTSpan[1:])
    if members_inputs:
        # multi-rank: rank 0 holds the whole sweep, the other ranks None (and an empty dataPack)
        res["ensemble"] = [result(p, mi, zNo, opTSpan) for p, mi in zip(packs, inputs)] if packer else None
    if ctl is not None:
        entries = [ctl.result_entry(logs[:, e]) for e in range(logs.shape[1])]
        res["control"] = entries[0]
        if members_inputs:
            for entry, c in zip(res["ensemble"], entries):
                entry["control"] = c
    if prof is not None:
        res["axial-profile"] = profile.result_entry(prof, 0)
        if members_inputs:
            for e, entry in enumerate(res["ensemble"]):
                entry["axial-profile"] = profile.result_entry(prof, e)
    if started is not None:
        res["initial"] = started[0]
        if members_inputs:
            for entry, st in zip(res["ensemble"], started):
                entry["initial"] = st
    if sensed is not None:
        res[sensitivity.KEY] = sensed[0]
        if members_inputs:
            for entry, se in zip(res["ensemble"], sensed):
                entry[sensitivity.KEY] = se
    if monitors:
        res["monitor"] = monitors[0]
        if members_inputs:
            for entry, m in zip(res["ensemble"], monitors):
                entry["monitor"] = m
    if sync is not None:
        res["ensemble-shard"] = {"rank": sync.rank, "world": sync.world, "members": [sync.lo, sync.hi]}
    if display and packer:
        from .plotting import plot_results_dynamic
        plot_results_dynamic(res, tNo)
    return res


def run_n2(modelInput, members_inputs=None):
    """runN2 on the device.  ``members_inputs``: optional list of modelInput dicts (one per
    ensemble member, same mechanism); default = the single reactor described by modelInput."""
    cfg = modelInput['solver-config']
    displayResult = cfg['display-result'] == "True"        # KeyError like the reference (:3337)
    modelId = modelInput['model']
    plan.check_model_setting_n2()          # the reference's N2 RHS raises under any setting but "MAX" - so does this
    outlet = outlet_only(cfg) if members_inputs else False

    def pack_all(Yg, named, mech, zNo, t1):
        if len(named) == 1 and not outlet:
            return [pack_interval(Yg[0], named[0], mech, zNo, t1, modelId)]
        return pack_intervals(Yg, named, mech, zNo, t1, modelId)
    sensitivity.parse(modelInput, members_inputs)      # (validation before any device work: not with "deactivation")
    # "deactivation": a time-on-stream run of the quasi-steady bed (campaign.py) - no integration in time; absent = None =
    # exactly the run without it
    cam = campaign.parse(modelInput, members_inputs, active_ranks(len(members_inputs)) is not None if members_inputs else False)
    if cam is not None:
        if outlet:
            raise ValueError("solver-config 'deactivation' cannot be combined with 'ensemble-output': 'outlet' - the "
                             "campaign returns whole states (the outlet per step is in resModel['deactivation'])")
        return run_campaign(modelInput, members_inputs, cam, pack_all, lambda dataPack, mi, zNo, opTSpan: {"dataPack": dataPack})
    return run_dynamic(modelInput, members_inputs, "N2", plan.member_constants, plan.initial_state, pack_all,
                       lambda dataPack, mi, zNo, opTSpan: {"dataPack": dataPack},
                       fp32=cfg.get('dtype', 'fp64') in ('fp32', 'float32'),
                       # "strict-flags": test the Python-exception conditions on every RK stage (default: stage 1 only)
                       defines={"RMT_CHECK_ALL_STAGES": "1"} if cfg.get('strict-flags') else {},
                       with_schedule=True, outlet=outlet, display=displayResult)
