"""The ctypes handle of the device models (N2Device), the two-device AutoStepper of ivp "hip-auto" and the decoder of the
device status words.  torch is used only as the owner of device memory and streams."""
import ctypes as C

import numpy as np

from . import campaign, fit, frequency, hipbind, initial, monitor, plan, sensitivity
from .codeplan import code_plan, compile_plan, device_arch, forced_tail, freq_plan, is_forced, is_profiled, march_plan, sens_plan
from .lowering import FLAG_DIV0, FLAG_DOMAIN, FLAG_NONFINITE, FLAG_OVERFLOW, FLAG_STEP
from .settings import DEVICE_DEFAULTS

FLAG_PRESSURE = 32


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


def _doubles(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ptr(t):
    return C.c_void_p(t.data_ptr())


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
        self.freq = None        # ... and one with the frequency unit (attach_frequency)
        self.use_current_stream()
        self.profile = None
        if profile is not None:
            try:
                self.set_profile(profile)
            except Exception:
                self.close()
                raise

    # -- plumbing
    def _call(self, name, *args):
        """entry point ``name`` of the C library on this handle; a non-zero return raises its last error"""
        hipbind.check(getattr(hipbind.lib(), name)(self.h, *args))

    def _march_dev(self):
        """the handle that owns the steady-state march: the attached one, unless this one has it (or there is none)"""
        return self if "march" in self.features or self.march is None else self.march

    def _sens_dev(self):
        """the handle that owns the sensitivity sweep: the third handle where there is one, else the march's"""
        return self.sens if self.sens is not None else self._march_dev()

    def use_current_stream(self):
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        self._call("rmt_n2_set_stream", C.c_void_p(s))
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
        self._call("rmt_n2_set_members", _doubles(members))

    def set_members_async(self, members):
        """set_members queued on the current stream without waiting for it (between two queued launches: the rows of a
        forced run are refreshed before every launch).  Returns the page-locked staging tensor, which the caller keeps
        alive until the stream has passed the copy."""
        members = np.ascontiguousarray(members, dtype=np.float64).reshape(self.E, self.row_width)
        pinned = self.torch.empty(members.shape, dtype=self.torch.float64, pin_memory=True)
        pinned.copy_(self.torch.from_numpy(members))
        self.members = members
        self._call("rmt_n2_set_members_async", _ptr(pinned))
        return pinned

    def set_profile(self, table):
        """Upload the axial profile [E][2][N] (rmt_n2_set_profile: one synchronous copy, before the first launch).  Only
        for a device whose code object was generated with RMT_PROFILE."""
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.shape != (self.E, 2, self.N):
            raise hipbind.RmtN2Error("the profile table must be [E][2][N] = %r doubles (got %r)"
                                     % ((self.E, 2, self.N), table.shape))
        self._call("rmt_n2_set_profile", _doubles(table))
        self.profile = table
        for dev in (self.march, self.sens, self.freq):
            if dev is not None:
                dev.set_profile(table)

    def get_members(self):
        """The device rows as they are now [E][row_width] (synchronises the stream): what the last refresh uploaded and
        the controller's kernel wrote since."""
        out = np.zeros((self.E, self.row_width))
        self._call("rmt_n2_get_members", _doubles(out))
        return out

    def set_mode(self, mode):
        self._call("rmt_n2_set_mode", {"auto": 0, "reg": 1, "mem": 2, "chain": 3}[mode])

    def close(self):
        if getattr(self, "_mon", None) is not None:
            self._mon.close()
            self._mon = None
        for dev in (getattr(self, "march", None), getattr(self, "sens", None), getattr(self, "freq", None)):
            if dev is not None:
                dev.close()
        self.march = self.sens = self.freq = None
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
        self._call("rmt_n2_rhs", float(t), _ptr(y), _ptr(out))
        return out

    def rk4(self, y, dt, nsteps, t0=0.0):
        """In place: nsteps RK4 steps of size dt."""
        self._chk_state(y)
        self._call("rmt_n2_rk4", _ptr(y), float(t0), float(dt), int(nsteps))

    def multistep(self, y, dt, nsteps, method="PreCorr3", t0=0.0):
        """In place: the reference's AdBash3 / PreCorr3 (odeSolver.py:43-102), nsteps >= 3."""
        self._chk_state(y)
        self._call("rmt_n2_multistep", _ptr(y), float(t0), float(dt), int(nsteps), {"AdBash3": 0, "PreCorr3": 1}[method])

    def rk45(self, y, t0, t1, rtol, atol, h0, max_steps):
        self._chk_state(y)
        self._call("rmt_n2_rk45", _ptr(y), float(t0), float(t1), float(rtol), float(atol), float(h0), int(max_steps),
                   _ptr(self._stats))

    def ros4(self, y, t0, t1, rtol, atol, h0, max_steps):
        """In place: stiff integration (RODAS4, order 4(3)) from t0 to t1 with per-reactor step control
        (needs a code object generated with features=("ros4",) and block <= 512; 256 is fastest)."""
        self._chk_state(y)
        if "ros4" not in self.features:
            raise hipbind.RmtN2Error("create the device with features=('ros4',) to use the stiff stepper")
        self._call("rmt_n2_ros4", _ptr(y), float(t0), float(t1), float(rtol), float(atol), float(h0), int(max_steps),
                   _ptr(self._stats))

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

    def steady_sens(self, y, kinds, indices, out=None):
        """Parametric sensitivities of the steady state y (rmt_n2_steady_sens, behind steady_march on the same handle):
        returns the device tensor [E][NP][V+1][N] - per member and parameter d(scaled state)/d(row value) and, in row V,
        dP/d(row value).  ``kinds`` / ``indices``: sensitivity.Sensitivity.descriptors.  Queued on the stream, nothing is
        synchronised; status() reads the flags.  Needs a code object of sens_plan with RMT_SENS_NP = len(kinds).
        ``out``: a device tensor of that shape to write into (default: a new one, zeroed)."""
        if self._sens_dev() is not self:
            return self._sens_dev().steady_sens(y, kinds, indices, out)
        self._chk_state(y)
        if str(self.defines.get(sensitivity.DEFINE, "0")) != "1" or int(self.defines[sensitivity.DEFINE_NP]) != len(kinds):
            raise hipbind.RmtN2Error("steady_sens needs the sensitivity unit (sens_plan) with RMT_SENS_NP = %d" % len(kinds))
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        assert kinds.shape == indices.shape and kinds.ndim == 1
        if out is None:
            out = self.torch.zeros((self.E, len(kinds), self.mech.V + 1, self.N), dtype=self.torch.float64,
                                   device=self.device)
        assert out.is_cuda and out.dtype == self.torch.float64 and out.is_contiguous() \
            and out.numel() == self.E*len(kinds)*(self.mech.V + 1)*self.N, "sensitivity buffer must be [E][NP][V+1][N]"
        self._call("rmt_n2_steady_sens", _ptr(y), len(kinds), kinds.ctypes.data_as(C.POINTER(C.c_int)),
                   indices.ctypes.data_as(C.POINTER(C.c_int)), _ptr(out))
        return out

    def attach_frequency(self, n_inputs):
        """A handle of its own on the same member rows whose code object is the frequency unit (freq_plan, solver-config
        "frequency-response"): the stepper's, the march's and the sensitivity unit's code objects stay what they are without
        the key.  steady_freq then goes through it."""
        if self.freq is None:
            if self.fp32 or getattr(self.mech, "model", "N2") != "N2":
                raise hipbind.RmtN2Error("the frequency sweep is for model N2 in fp64")
            cp = freq_plan(self.mech, self.N, n_inputs, self.defines, self.members)
            self.freq = N2Device(self.mech, self.members, self.N, block=cp.block, npt=cp.npt, device=self.device.index,
                                 defines=cp.defines, specialize=False, features=cp.features, profile=self.profile)
        return self

    def steady_freq(self, y, kinds, indices, omegas, peak_nodes, profile=False):
        """Frequency response of the steady state y (rmt_n2_steady_freq): (rows [E][F][NP][2][V+1] complex - slot 0 the
        outlet node, slot 1 node peak_nodes[e] -, table [E][F][NP][V+1][N] complex or None without ``profile``, failed
        [E][F] ints: the node a lane stopped at, -1 none) as numpy arrays, in the scaled units of the state per unit of the
        row value (row V: the pressure).  ``omegas`` [F] in radians per unit of model time.  Blocking: one upload, ONE launch,
        one copy back; status() reads the flags.  Needs the frequency unit (freq_plan) with RMT_FREQ_NP = len(kinds) -
        this handle's own, or the one attach_frequency made."""
        if self.freq is not None:
            return self.freq.steady_freq(y, kinds, indices, omegas, peak_nodes, profile)
        self._chk_state(y)
        if str(self.defines.get(frequency.DEFINE, "0")) != "1" or int(self.defines[frequency.DEFINE_NP]) != len(kinds):
            raise hipbind.RmtN2Error("steady_freq needs the frequency unit (freq_plan) with RMT_FREQ_NP = %d" % len(kinds))
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        omegas = np.ascontiguousarray(omegas, dtype=np.float64)
        peak_nodes = np.ascontiguousarray(peak_nodes, dtype=np.int32)
        assert kinds.shape == indices.shape and kinds.ndim == 1 and omegas.ndim == 1 and peak_nodes.shape == (self.E,)
        E, F, NP, V1, N = self.E, len(omegas), len(kinds), self.mech.V + 1, self.N
        n_out, n_tab = E*F*NP*2*V1*2, E*F*NP*V1*N*2 if profile else 0
        buf = np.zeros(n_out + n_tab + E*F)
        ints = C.POINTER(C.c_int)
        self._call("rmt_n2_steady_freq", _ptr(y), NP, kinds.ctypes.data_as(ints), indices.ctypes.data_as(ints), F,
                   _doubles(omegas), peak_nodes.ctypes.data_as(ints), int(bool(profile)), _doubles(buf))
        rows = buf[:n_out].view(np.complex128).reshape(E, F, NP, 2, V1)
        table = buf[n_out:n_out + n_tab].view(np.complex128).reshape(E, F, NP, V1, N) if profile else None
        return rows, table, buf[n_out + n_tab:].astype(np.int64).reshape(E, F)

    def freq_status(self):
        """The status words of the handle steady_freq ran on, read and cleared (synchronises)."""
        return (self.freq if self.freq is not None else self).status()

    def fit_step(self, y, sens, loop, k, extended=False):
        """Queue pass ``k`` of a fit on the device's stream, behind steady_march and steady_sens on this handle
        (csrc/fit_kernels.inc): the residuals and their reduction over the members (the experiments) from the state y and
        the sensitivity buffer ``sens``, then the Levenberg-Marquardt step, which writes slice k of the loop's log and the
        trial values into the fitted columns of this device's rows.  ``loop``: the run's FitLoop (n2.py); ``extended``: the
        loop carries the position table, the scale flags and the box, and the sibling kernels run (rmt_n2_fit_step_ex).  Nothing is
        copied or synchronised.  Needs the sensitivity unit (sens_plan) in fp64."""
        self._chk_state(y)
        if str(self.defines.get(sensitivity.DEFINE, "0")) != "1" or self.fp32:
            raise hipbind.RmtN2Error("fit_step needs the sensitivity unit (sens_plan) in fp64")
        P = len(loop.columns)
        assert loop.E == self.E and sens.is_cuda and sens.dtype == self.torch.float64 and sens.is_contiguous() \
            and sens.numel() == self.E*P*(self.mech.V + 1)*self.N, "sensitivity buffer must be [E][NP][V+1][N]"
        args = (self.h, y.data_ptr(), sens.data_ptr(), self._stats.data_ptr(), self.mech.S, self.mech.V, self.N,
                loop.columns, loop.meas.data_ptr(), loop.MQ, loop.contrib.data_ptr(), loop.pred.data_ptr(),
                loop.state.data_ptr(), loop.log[k].data_ptr(), loop.tolerance, loop.damping)
        if not extended:                                # a loop without the new data: the present call
            loop.kernel.step(*args)
        else:                                           # log-scaled or bounded parameters, data along the bed
            assert loop.log.shape[1] == fit.LOG_EX and loop.pos.numel() == self.E*loop.MQ*2
            loop.kernel.step_ex(*args, loop.pos.data_ptr(), loop.flags, loop.box)

    def sens_status(self):
        """The status words of the handle steady_sens ran on, read and cleared (synchronises)."""
        return self._sens_dev().status()

    def steady_march(self, y, tol=initial.DEFAULTS["tolerance"], max_iter=initial.DEFAULTS["max-iterations"]):
        """In place: every member's state becomes the discrete steady state f(y) = 0 of its device rows (a forced row: its
        values at the row's reference time), found by marching from the inlet with one V x V solve per node
        (rmt_n2_steady_march).  Queued on the stream, nothing is synchronised; march_result reads what came of it.
        Needs features=("march",), or attach_march()."""
        self._chk_state(y)
        if self._march_dev() is not self:
            return self._march_dev().steady_march(y, tol, max_iter)
        if "march" not in self.features:
            raise hipbind.RmtN2Error("create the device with features=('march',) or call attach_march() to use the "
                                     "steady-state march")
        self._call("rmt_n2_steady_march", _ptr(y), float(tol), int(max_iter), _ptr(self._stats))

    def march_result(self):
        """(stats, flags) of the last steady_march (synchronises): per member the worst node's scaled residual, the node
        that failed (-1: none), the largest per-node step count and the number of nodes that needed a rejected step; the
        status words, read and cleared."""
        if self._march_dev() is not self:
            return self._march_dev().march_result()
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
        self._call("rmt_n2_set_campaign_law", _doubles(law))
        self.law = law

    def _chk_campaign(self, y, stats, buffers, message):
        """the argument check of the two campaign steps (``buffers``: (tensor, doubles it holds) pairs) -> the stats tensor"""
        self._chk_state(y)
        stats = self._stats if stats is None else stats
        for t, n in buffers + ((stats, self.E*4),):
            assert t.is_cuda and t.dtype == self.torch.float64 and t.is_contiguous() and t.numel() == n, message
        return stats

    def campaign_step(self, y, dt, log_row, stats=None, tol=initial.DEFAULTS["tolerance"],
                      max_iter=initial.DEFAULTS["max-iterations"]):
        """One step of a campaign (rmt_n2_campaign_step): y becomes every member's steady state for the activities in the
        handle's table, which then move over ``dt`` seconds at the node temperatures of that state.  ``log_row``: device
        doubles [E][V+6]; ``stats``: device doubles [E][4] (default: the device's own, march_result reads them).  Queued on
        the stream, nothing is synchronised."""
        stats = self._chk_campaign(y, stats, ((log_row, self.E*(self.mech.V + campaign.LOG_EXTRA)),),
                                   "campaign_step: the log row is [E][V+6], the stats [E][4] device doubles")
        self._call("rmt_n2_campaign_step", _ptr(y), float(dt), float(tol), int(max_iter), _ptr(log_row), _ptr(stats))

    def set_campaign_policy(self, rows, component, levels):
        """Upload the policy rows [E][4] = {target, lo, hi, tolerance}, the index of the held component and the levels
        [E] step 0 carries in (rmt_n2_set_campaign_policy: one blocking copy).  Needs the policy unit
        (campaign_policy_plan), a profile table and a law."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        levels = np.ascontiguousarray(levels, dtype=np.float64)
        if rows.shape != (self.E, campaign.POLICY_ROW) or levels.shape != (self.E,):
            raise hipbind.RmtN2Error("the policy rows must be [E][4] = %r doubles and the levels [E] (got %r and %r)"
                                     % ((self.E, 4), rows.shape, levels.shape))
        self._call("rmt_n2_set_campaign_policy", _doubles(rows), int(component), _doubles(levels))

    def campaign_policy_step(self, y, dt, log_row, policy_row, stats=None, tol=initial.DEFAULTS["tolerance"],
                             max_iter=initial.DEFAULTS["max-iterations"],
                             max_evaluations=campaign.POLICY_DEFAULTS["max-evaluations"]):
        """campaign_step with the coolant policy (rmt_n2_campaign_policy_step): y becomes every member's steady state at the
        coolant level that holds the target (or at the better limit), the activities then move over ``dt`` seconds.
        ``policy_row``: device doubles [E][4] = {level, held, marches, saturated}.  Queued on the stream, nothing is
        synchronised."""
        stats = self._chk_campaign(
            y, stats, ((log_row, self.E*(self.mech.V + campaign.LOG_EXTRA)), (policy_row, self.E*campaign.POLICY_LOG)),
            "campaign_policy_step: the log row is [E][V+6], the policy row [E][4], the stats [E][4] device doubles")
        self._call("rmt_n2_campaign_policy_step", _ptr(y), float(dt), float(tol), int(max_iter), int(max_evaluations),
                   _ptr(log_row), _ptr(policy_row), _ptr(stats))

    def get_campaign_level(self):
        """The carried coolant levels [E] as they are now (rmt_n2_get_campaign_level; synchronises the stream)."""
        out = np.zeros(self.E)
        self._call("rmt_n2_get_campaign_level", _doubles(out))
        return out

    def get_profile(self):
        """The handle's table [E][2][N] as it is now (rmt_n2_get_profile; synchronises the stream): the activities the
        campaign steps have written, and the coolant offsets."""
        out = np.zeros((self.E, 2, self.N))
        self._call("rmt_n2_get_profile", _doubles(out))
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
        self._call("rmt_n1_profile", _doubles(rows1), _ptr(out), int(nout), float(rtol), float(atol), float(h0),
                   int(max_steps), _ptr(self._stats))
        return out.cpu().numpy()

    def rk45_stats(self):
        raw = self._stats.cpu().numpy()
        acc, rej = step_counts(raw)
        return {"t_end": raw[:, 0].copy(), "h_last": raw[:, 1].copy(), "accepted": acc, "rejected": rej}

    def status(self):
        flags = np.zeros(self.E, dtype=np.uint32)
        self._call("rmt_n2_status", flags.ctypes.data_as(C.POINTER(C.c_uint32)))
        return flags

    def last_geometry(self):
        """(workgroups per reactor, teams) of the last rk4 / rk45 / ros4 launch - what the library's auto mode chose."""
        c, t = C.c_int(), C.c_int()
        self._call("rmt_n2_last_geometry", C.byref(c), C.byref(t))
        return c.value, t.value

    def fallbacks(self):
        """Reactor-launches the cached RK4 steppers handed to their plain twins so far (rmt_n2_fallbacks): a reactor whose
        temperature left the range of its cached rate constants during a launch is integrated again in full."""
        n = C.c_uint64()
        self._call("rmt_n2_fallbacks", C.byref(n))
        return int(n.value)

    def last_kernel_ms(self):
        ms = C.c_float()
        self._call("rmt_n2_last_kernel_ms", C.byref(ms))
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

    def attach_frequency(self, n_inputs):
        self.d45.attach_frequency(n_inputs)
        return self

    def steady_freq(self, y, kinds, indices, omegas, peak_nodes, profile=False):
        return self.d45.steady_freq(y, kinds, indices, omegas, peak_nodes, profile)

    def freq_status(self):
        return self.d45.freq_status()

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
