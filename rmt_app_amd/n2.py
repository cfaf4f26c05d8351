"""Device-side driver of model N2: the replacement for the time loop of
PackedBedHomoReactorClass.runN2 (PyREMOT/docs/pbHomoReactor.py:3556-3704).

The reference calls scipy's solve_ivp once per output interval with a Python RHS
(:3589-3610); here each interval is ONE launch of a device-resident explicit stepper
(fixed-step RK4 or adaptive Dormand-Prince RK45) over all mesh nodes of all ensemble members.
torch is used only as the owner of device memory and streams.
"""
from collections import namedtuple
from timeit import default_timer as timer

import numpy as np

from . import campaign, control, fit, frequency, hipbind, initial, launches, monitor, plan, profile, schedule, sensitivity
# (the two lists below are also the re-exports: every public name of codeplan and device stays importable from here)
from .codeplan import (  # noqa: F401
    FEATURE_DEFINES, KC_MAX_AGE, KC_REFRESH, MARCH_BLOCK, MAX_CHUNKS, N_CUS, CodePlan, campaign_plan, campaign_policy_plan,
    choose_geometry, code_plan, code_plans, compile_mechanism, compile_options, compile_plan, device_arch, device_source,
    forced_literals, forced_mode, forced_tail, forcing_level, is_campaign, is_forced, is_profiled, kc_period, kcache_choice,
    freq_plan, march_plan, plan_unit, precompile, rk45_block, rk45_geometry, ros4_block, ros4_quad, sens_plan)
from .device import FLAG_PRESSURE, AutoStepper, N2Device, flag_error, step_counts, stepper_args  # noqa: F401
from .ensemble import DistributedEnsemble, active_ranks, guarded
from .settings import DEVICE_DEFAULTS, ROUND_FUN_ACCURACY, solverSetting

DEVICE_IVPS = ("hip-rk4", "hip-rk45", "hip-ros4", "hip-auto", "AM", "hip-ab3")


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
                 features=(), forcing=None, march=False, prof=None, sens=None, freq=None):
    """Device + initial state for the members THIS process integrates.

    Single process: all of ``inputs``.  As one rank of a torch.distributed job (``sync``, see
    ensemble.RankSync): the rank's contiguous block; rank 0 compiles, every rank loads the broadcast
    code object, sweep-invariant member fields agreed over all ranks become kernel literals.
    Returns (device, named constants of the local members, local initial states [E_local][V*N]).
    ``forcing`` (a Forcing, solver-config "schedule"): the code object is generated with RMT_FORCING (2 when the schedule
    moves the feed composition, else 1), the rows get their tail, and the host fixes the kernel form (forced_mode).
    ``march`` (solver-config "initial", single process): a second handle on the same rows holds the steady-state march
    (N2Device.attach_march); with ``sens`` (a sensitivity.Sensitivity, solver-config "sensitivity") that handle's code
    object is the sensitivity unit (sens_plan) and ``sens.mech`` / ``sens.rows`` receive its mechanism and rows; with
    ``freq`` (a frequency.FrequencyResponse, solver-config "frequency-response") one more handle holds the frequency unit
    (N2Device.attach_frequency) and ``freq.rows`` receives the rows.
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
            forcing.fix_mode(dev, features)
        elif prof is not None:
            fix_mode(dev, prof, zNo, features, "axial-profile", "profile")
        if march:
            try:
                if sens is not None:
                    sens.mech = mech if sens.unit_params(mech.params) == tuple(mech.params) \
                        else plan.Mechanism(inputs[0], params=sens.unit_params(mech.params))
                    sens.rows = sens.widen(rows, mech, sens.mech, inputs)
                dev.attach_march(None if sens is None else (sens.NP, sens.mech, sens.rows))
                if freq is not None:
                    freq.rows = rows
                    dev.attach_frequency(freq.NP)
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
        guarded(sync, forcing.fix_mode, dev, features)
    return dev, ens.named, ens.IV


def open_auto(mech, inputs, zNo, pack, init, sync, fp32, defines, block=None, npt=None, forcing=None, march=False,
              prof=None, sens=None, freq=None):
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
                                          sens=sens, freq=freq)
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


def fix_mode(dev, by, N, features, key="schedule", what="forcing"):
    """Fix the kernel form of a forced or profiled device (forced_mode) and record it in ``by.modes``.  ``by``: the run's
    Forcing or profile.Profile, whose ``want_mode`` is solver-config "device-mode"."""
    stiff = "ros4" in features              # (all forced_mode tells apart: the stiff stepper always runs its "mem" form)
    mode = forced_mode("hip-ros4" if stiff else "explicit", N, dev.block, dev.npt, by.want_mode, key, what)
    dev.set_mode(mode)
    by.modes["ros4" if stiff else "explicit"] = mode


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

    def fix_mode(self, dev, features):
        fix_mode(dev, self, self.N, features)

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


def attach_entries(res, key, entries):
    """The members' result entries of one solver-config key: the first member's under ``res[key]`` and, where the result
    has an "ensemble" list, every member's under the same key of its own result."""
    res[key] = entries[0]
    if "ensemble" in res:
        for member, entry in zip(res["ensemble"], entries):
            member[key] = entry


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


def start_frequency(dev, y, fr, named, mech):
    """solver-config "frequency-response": ONE launch of rmt_n2_steady_freq on the frequency handle over the marched state y,
    the rows come back once.  Raises FloatingPointError naming member, frequency and node when a node of the shifted
    tangent march is singular or not finite.  Returns the members' result entries."""
    kinds, indices = fr.descriptors(mech)
    Yh = y.cpu().numpy()
    peaks = [frequency.peak_node(Yh[e], mech, named[e]) for e in range(Yh.shape[0])]
    rows, table, failed = dev.steady_freq(y, kinds, indices, fr.omegas, peaks, fr.profile)
    flags = dev.freq_status()
    if np.any(flags) or np.any(failed >= 0):
        e = int(np.nonzero(flags)[0][0]) if np.any(flags) else int(np.argwhere(failed >= 0)[0][0])
        bad = np.nonzero(failed[e] >= 0)[0]
        f = int(bad[0]) if len(bad) else 0
        raise FloatingPointError("solver-config 'frequency-response': the shifted node Jacobian is singular (or a response "
                                 "is not finite) at node %d of member %d at frequency %d (w = %g, flags=0x%x)"
                                 % (int(failed[e, f]), e, f, fr.omegas[f], int(flags[e])))
    return [frequency.result_entry(fr, rows[e], None if table is None else table[e], Yh[e], fr.rows[e], named[e], mech)
            for e in range(Yh.shape[0])]


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
    attach_entries(res, campaign.KEY, entries)
    if prof is not None:
        attach_entries(res, "axial-profile", [profile.result_entry(prof, e) for e in range(E)])
    return res


class FitLoop:
    """The device side of one fit (fit.Fit): the kernels' module and their buffers - the measurement table [E][MQ][3], the
    experiments' contributions [E][46] and predictions [E][MQ], the LM state [80] and the log [passes][68], read once per
    batch of iterations.  A spec with log-scaled or bounded parameters or data along the bed (ft.extended) takes the
    sibling kernels: the position table ``pos`` [E][MQ][2], the scale flags, the box, and a log 70 wide; any other spec
    (``pos`` None) takes rmt_n2_fit_step as before."""

    def __init__(self, ft, dev, columns, passes):
        torch = dev.torch
        self.E, self.MQ, self.columns = ft.E, ft.MQ, list(columns)
        self.tolerance, self.damping = ft.tolerance, ft.damping
        self.pos, width = None, fit.LOG
        if ft.extended:
            self.pos = torch.from_numpy(np.ascontiguousarray(ft.position_table(dev.N))).to(dev.device)
            self.flags, self.box, width = list(ft.flags), ft.box(), fit.LOG_EX
        with torch.cuda.device(dev.device):
            self.kernel = hipbind.Fit(device_arch(dev.device))
        self.meas = torch.from_numpy(np.ascontiguousarray(ft.table())).to(dev.device)
        self.contrib = torch.zeros((ft.E, fit.CONTRIB), dtype=torch.float64, device=dev.device)
        self.pred = torch.zeros((ft.E, ft.MQ), dtype=torch.float64, device=dev.device)
        self.state = torch.zeros(fit.STATE, dtype=torch.float64, device=dev.device)
        self.log = torch.zeros((passes, width), dtype=torch.float64, device=dev.device)

    def close(self):
        self.kernel.close()


def run_fit(modelInput, ft, pack_all, result):
    """solver-config "fit" (fit.py): Levenberg-Marquardt over the steady states of all experiments at once.  Opens the
    experiments' rows on ONE handle of the sensitivity unit whose per-reactor inputs hold the fitted constants (sens_plan)
    and queues per iteration rmt_n2_steady_march, rmt_n2_steady_sens and rmt_n2_fit_step back to back; the log comes to the
    host once per "batch" of iterations, and a finishing pass behind `converged` leaves state, sensitivities, predictions
    and J^T J of the accepted parameters on the device.  March flags of rejected trials are expected: failures are judged
    from the log, the sticky flag words are cleared before the finishing pass and checked after it."""
    start = timer()
    cfg = modelInput['solver-config']
    zNo = int(cfg.get('zNo', solverSetting['N2']['zNo']))
    inputs = ft.members(modelInput)
    sens = ft.sensitivity()
    mech = plan.Mechanism(modelInput, params=sens.unit_params(mechanism_for(modelInput, inputs, cfg).params))
    pairs = [plan.member_constants(mi, mech, zNo) for mi in inputs]
    named, rows = [nm for nm, _ in pairs], np.array([r for _, r in pairs])
    columns = ft.columns(mech)
    initial_values = rows[0, plan.MEMBER_FIXED + mech.S + np.array(columns)].copy()
    kinds, indices = sens.descriptors(mech)
    cp = sens_plan(mech, zNo, ft.NP, None, rows)
    dev = device_cls()(mech, rows, zNo, block=cp.block, npt=cp.npt, defines=cp.defines, specialize=False,
                       features=cp.features)
    loop = None
    try:
        loop = FitLoop(ft, dev, columns, ft.max_iterations + 1)
        y = dev.to_device(plan.initial_states(named, mech, zNo, plan.initial_state))
        raw = dev.torch.zeros((ft.E, ft.NP, mech.V + 1, zNo), dtype=dev.torch.float64, device=dev.device)
        tol, its = initial.DEFAULTS["tolerance"], initial.DEFAULTS["max-iterations"]

        def queue(k):
            dev.steady_march(y, tol, its)
            dev.steady_sens(y, kinds, indices, raw)
            dev.fit_step(y, raw, loop, k, extended=ft.extended)

        def describe(row):
            return "cost %.12g at %s%s" % (row[1], ", ".join("%s = %.12g" % (nm, v) for nm, v in
                                                             zip(ft.names, row[fit.LOG_PCUR:fit.LOG_PCUR + ft.NP])),
                                           ft.bounds_text(row))
        logs, n, done = [], 0, False
        while n < ft.max_iterations and not done:
            hi = min(ft.max_iterations, n + ft.batch)
            for k in range(n, hi):
                queue(k)
            for row in loop.log[n:hi].cpu().numpy():
                logs.append(row)
                status = int(row[7])
                if status & fit.FIRST_FAILED:
                    raise RuntimeError("solver-config 'fit': the steady-state march failed (or a prediction is not finite) "
                                       "for %d of the %d experiments at the starting values" % (int(row[6]), ft.E))
                if status & fit.NOT_POSITIVE:
                    raise RuntimeError("solver-config 'fit': J^T J + lambda D is not positive definite after 8 increases of "
                                       "lambda in iteration %d (%s): the parameters are not identifiable from these data"
                                       % (len(logs), describe(row)))
                if row[5] != 0.0:
                    done = True
                    break
            n = hi
        if not done:
            raise RuntimeError("solver-config 'fit': no convergence within %d iterations ('max-iterations'): last %s"
                               % (len(logs), describe(logs[-1])))
        dev.status()                                    # (read and cleared: what rejected trials flagged)
        queue(ft.max_iterations)                        # the finishing pass: frozen, everything at the accepted values
        last = loop.log[ft.max_iterations].cpu().numpy()
        flags = dev.status()
        err = flag_error(flags)
        if err is not None or last[6] != 0.0:
            st = dev.march_result()[0]
            e = int(np.nonzero(flags)[0][0]) if err is not None else -1
            raise RuntimeError("solver-config 'fit': the steady-state march failed at the accepted parameters (%s)%s"
                               % (describe(last), "" if e < 0 else ": node %d of experiment %d: %s"
                                  % (int(st["failed-node"][e]), e, err)))
        Yh, pred = y.cpu().numpy(), loop.pred.cpu().numpy()
        dstats = {"launches": 4*(n + 1), "iterations": len(logs), "passes": n + 1,
                  "accepted": int(sum(r[4] for r in logs)), "rejected": int(sum(1 - r[4] for r in logs))}
    finally:
        if loop is not None:
            loop.close()
        dev.close()
    packs = pack_all(Yh, named, mech, zNo, 0.0)
    res = result([packs[0]], modelInput, zNo, None)
    res["computation-time"] = np.round(timer() - start, ROUND_FUN_ACCURACY)
    res["device-stats"] = dstats
    res["ensemble"] = [result([p], mi, zNo, None) for p, mi in zip(packs, inputs)]
    for e, member in enumerate(res["ensemble"]):
        member[fit.KEY] = ft.member_entry(e, pred[e])
    res[fit.KEY] = ft.result_entry(np.array(logs), initial_values, last)
    return res


RunKeys = namedtuple("RunKeys", "sched ctl forced_by mon ini prof sens freq")


def parse_keys(modelInput, members_inputs, ivp, tNo, E, V, ranked, with_schedule):
    """The optional solver-config keys of a dynamic run, parsed and checked against their budgets; absent = None = exactly
    the run without it.  ``ranked``: one rank of a multi-rank job; ``with_schedule``: the model takes more than "monitor".
      sched  "schedule": time-varying inlet / coolant conditions (schedule.py)
      ctl    "control": a sampled PI controller per member on the device (control.py).  A controlled run is a forced run:
             without a "schedule" it gets a constant one of every member's own values - ``forced_by`` is what forces the run
      mon    "monitor": time series between the output times (monitor.py)
      ini    "initial": where the run starts (initial.py); None = the reference's cold start
      prof   "axial-profile": catalyst activity and coolant zones along the bed (profile.py); knows the "device-mode"
      sens   "sensitivity": parametric sensitivities of the steady state the run starts from (sensitivity.py)
      freq   "frequency-response": the harmonic response of that steady state (frequency.py)"""
    sched = schedule.parse(modelInput, members_inputs, ivp) if with_schedule else None
    control.check_model(modelInput)
    ctl, forced_by = control.parse(modelInput, members_inputs, ivp, sched, ranked) if with_schedule else (None, sched)
    if ctl is not None:
        ctl.check_budget(PIPELINE_BYTES)
    mon = monitor.parse(modelInput, tNo)
    if mon is not None:
        mon.check_budget(E, V, PIPELINE_BYTES)
    ini = initial.parse(modelInput, ranked) if with_schedule else None
    profile.check_model(modelInput)
    prof = profile.parse(modelInput, members_inputs, ivp, ranked) if with_schedule else None
    if prof is not None:
        prof.want_mode = modelInput['solver-config'].get('device-mode')
    sens = sensitivity.parse(modelInput, members_inputs, ranked) if with_schedule else None
    freq = frequency.parse(modelInput, members_inputs, ranked, V) if with_schedule else None
    return RunKeys(sched, ctl, forced_by, mon, ini, prof, sens, freq)


def run_geometry(ivp, mech, zNo, fp32, block, npt, defines, E_gpu, carried=()):
    """(block, nodes per thread, prelude defines) of the stepper of `ivp`; an explicit ``block`` / ``npt`` of the solver-config
    is left alone.  ``carried``: a (solver-config key, what it adds) pair for each of "schedule" and "axial-profile" the run
    has: neither the stiff stepper's four-lane form nor the chained kernels carry the forcing or the profile."""
    for key, what in carried:
        if ivp in ("hip-ros4", "hip-auto") and ros4_quad(mech, fp32):
            raise NotImplementedError("solver-config '%s' with the stiff stepper needs a mechanism of at most 8 "
                                      "variables per node (this one has %d): its four-lane form does not carry the "
                                      "%s - use ivp 'hip-rk45' or 'hip-rk4'" % (key, mech.V, what))
    defines = dict(defines or {})
    if block is not None:
        return block, npt, defines
    if ivp == "hip-rk4" and carried:          # the geometry of ONE workgroup per reactor (no chunks)
        block, npt = choose_geometry(zNo, mech.V, fp32)
    elif ivp == "hip-ros4":
        block, npt = ros4_block(mech.V, zNo, fp32, ros4_quad(mech, fp32)), 1
    elif ivp == "hip-rk45":
        block, npt, geo_defs = rk45_geometry(mech.V, zNo, fp32, **({"chain": False} if carried else {"E": E_gpu}))
        defines.update(geo_defs)
    return block, npt, defines


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
    sched, ctl, forced_by, mon, ini, prof, sens, freq = parse_keys(modelInput, members_inputs, ivp, tNo, len(inputs),
                                                                   mech.V, sync is not None, with_schedule)
    # the ONE launch list of the run; a sample that fell on a mark carries that mark's time from here on (result entries)
    walk, sample_times, control_times = launches.merge(
        opT, tNo, forced_by.times if forced_by is not None else (), mon.times if mon is not None else None,
        ctl.times if ctl is not None else None)
    if mon is not None:
        mon.times = sample_times
    if ctl is not None:
        ctl.times = control_times
    carried = ([("schedule", "forcing")] if forced_by is not None else []) \
        + ([("axial-profile", "profile")] if prof is not None else [])
    block, npt, defines = run_geometry(ivp, mech, zNo, fp32, cfg.get('block'), cfg.get('nodes-per-thread'), defines, E_gpu,
                                       carried)
    forcing = None
    if forced_by is not None:
        forcing = Forcing(forced_by if sync is None else forced_by.members(sync.lo, sync.hi), walk, zNo,
                          cfg.get('device-mode'))
    if ivp == "hip-auto":
        dev, named_local, IV = open_auto(mech, inputs, zNo, pack, init, sync, fp32, defines, block, npt, forcing=forcing,
                                         march=ini is not None, prof=prof, sens=sens, freq=freq)
    else:
        dev, named_local, IV = open_members(mech, inputs, zNo, pack, init, sync, fp32=fp32, block=block, npt=npt,
                                            defines=defines, features=("ros4",) if ivp == "hip-ros4" else (),
                                            forcing=forcing, march=ini is not None, prof=prof, sens=sens, freq=freq)
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
        swept = start_frequency(dev, y, freq, named, mech) if freq is not None else None
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
        attach_entries(res, "control", [ctl.result_entry(logs[:, e]) for e in range(logs.shape[1])])
    if prof is not None:
        attach_entries(res, "axial-profile", [profile.result_entry(prof, e) for e in range(len(inputs))])
    if started is not None:
        attach_entries(res, "initial", started)
    if sensed is not None:
        attach_entries(res, sensitivity.KEY, sensed)
    if swept is not None:
        attach_entries(res, frequency.KEY, swept)
    if monitors:
        attach_entries(res, "monitor", monitors)
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
    # "fit": kinetic parameter estimation from steady-state data (fit.py) - no integration in time; absent = None = exactly
    # the run without it
    frequency.parse(modelInput, members_inputs)        # (validation before any device work: not with "fit", "deactivation")
    ft = fit.parse(modelInput)
    if ft is not None:
        fit.parse(modelInput, multi_rank=active_ranks(ft.E) is not None)
        return run_fit(modelInput, ft, pack_all, lambda dataPack, mi, zNo, opTSpan: {"dataPack": dataPack})
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
