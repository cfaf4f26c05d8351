"""ctypes binding of the C-ABI library librmt_n2.so (include/rmt_n2.h).

The library is built in-tree by ``__graft_entry__.build()`` (or ``make -C rmt_app_amd/csrc``).
There is deliberately no fallback: if the shared object is missing or no HIP device is present
the calls raise.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RMT_N2_LIBRARY selects another build of the same C ABI (the host-ASan build of `make asan`)
LIB_PATH = os.environ.get("RMT_N2_LIBRARY") or os.path.join(_HERE, "librmt_n2.so")
CACHE_DIR = os.path.join(_HERE, "_kcache")

ABI_VERSION = 2


def monitor_rows_per_block(E, V, N, real_size, n_cus):
    """Rows per workgroup rmt_n2_monitor_reduce launches with (csrc/rmt_n2.cpp RMT_N2_MONITOR_*): 4 = one wave per row, for
    rows of at most 8 KiB or when there are at least 4 rows per CU; else 1 = one workgroup per row."""
    return 4 if int(N)*int(real_size) <= 8192 or int(E)*int(V) >= 4*int(n_cus) else 1


class RmtN2Error(RuntimeError):
    pass


class Plan(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("n_species", C.c_int32), ("n_reactions", C.c_int32),
        ("n_vars", C.c_int32), ("n_nodes", C.c_int32), ("n_members", C.c_int32),
        ("fp32", C.c_int32), ("block", C.c_int32), ("nodes_per_thread", C.c_int32),
        ("n_user_params", C.c_int32), ("ros4_nodes_per_block", C.c_int32), ("profiled", C.c_int32),
        ("code_object", C.c_void_p), ("code_size", C.c_size_t), ("members", C.POINTER(C.c_double)),
    ]


class Stats(C.Structure):
    _fields_ = [("t_end", C.c_double), ("h_last", C.c_double), ("accepted", C.c_int64),
                ("rejected", C.c_int64)]


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RmtN2Error("%s is missing - run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(or make -C rmt_app_amd/csrc); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, cp, dbl, i64 = C.c_void_p, C.c_char_p, C.c_double, C.c_int64
    L.rmt_n2_last_error.restype = cp
    L.rmt_n2_abi_version.restype = C.c_int
    L.rmt_n2_kernel_template.restype = cp
    L.rmt_n2_compile.argtypes = [cp, cp, cp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp)]
    L.rmt_n2_free.argtypes = [vp]
    L.rmt_n2_free.restype = None
    L.rmt_n2_create.argtypes = [C.POINTER(Plan), C.POINTER(vp)]
    L.rmt_n2_destroy.argtypes = [vp]
    L.rmt_n2_destroy.restype = None
    L.rmt_n2_set_stream.argtypes = [vp, vp]
    L.rmt_n2_set_mode.argtypes = [vp, C.c_int]
    L.rmt_n2_set_members.argtypes = [vp, C.POINTER(dbl)]
    L.rmt_n2_set_members_async.argtypes = [vp, vp]
    L.rmt_n2_get_members.argtypes = [vp, C.POINTER(dbl)]
    L.rmt_n2_set_profile.argtypes = [vp, C.POINTER(dbl)]
    L.rmt_n2_rhs.argtypes = [vp, dbl, vp, vp]
    L.rmt_n2_rk4.argtypes = [vp, vp, dbl, dbl, i64]
    L.rmt_n2_multistep.argtypes = [vp, vp, dbl, dbl, i64, C.c_int]
    L.rmt_n2_rk45.argtypes = [vp, vp, dbl, dbl, dbl, dbl, dbl, i64, vp]
    L.rmt_n2_ros4.argtypes = [vp, vp, dbl, dbl, dbl, dbl, dbl, i64, vp]
    L.rmt_n1_profile.argtypes = [vp, C.POINTER(dbl), vp, C.c_int, dbl, dbl, dbl, i64, vp]
    L.rmt_n2_steady_march.argtypes = [vp, vp, dbl, i64, vp]
    L.rmt_n2_steady_sens.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), vp]
    L.rmt_n2_steady_freq.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(dbl),
                                     C.POINTER(C.c_int), C.c_int, C.POINTER(dbl)]
    L.rmt_n2_set_campaign_law.argtypes = [vp, C.POINTER(dbl)]
    L.rmt_n2_campaign_step.argtypes = [vp, vp, dbl, dbl, i64, vp, vp]
    L.rmt_n2_get_profile.argtypes = [vp, C.POINTER(dbl)]
    L.rmt_n2_set_campaign_policy.argtypes = [vp, C.POINTER(dbl), C.c_int, C.POINTER(dbl)]
    L.rmt_n2_campaign_policy_step.argtypes = [vp, vp, dbl, dbl, i64, C.c_int, vp, vp, vp]
    L.rmt_n2_get_campaign_level.argtypes = [vp, C.POINTER(dbl)]
    L.rmt_n2_status.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.rmt_n2_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rmt_n2_last_geometry.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rmt_n2_fallbacks.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.rmt_n2_monitor_source.restype = cp
    L.rmt_n2_monitor_create.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.rmt_n2_monitor_destroy.argtypes = [vp]
    L.rmt_n2_monitor_destroy.restype = None
    L.rmt_n2_monitor_reduce.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.rmt_n2_monitor_last_rows_per_block.argtypes = [vp]
    L.rmt_n2_control_source.restype = cp
    L.rmt_n2_control_create.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.rmt_n2_control_destroy.argtypes = [vp]
    L.rmt_n2_control_destroy.restype = None
    L.rmt_n2_control_update.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int]
    L.rmt_n2_fit_source.restype = cp
    L.rmt_n2_fit_create.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.rmt_n2_fit_destroy.argtypes = [vp]
    L.rmt_n2_fit_destroy.restype = None
    L.rmt_n2_fit_step.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), vp, C.c_int,
                                  vp, vp, vp, vp, dbl, dbl]
    L.rmt_n2_fit_step_ex.argtypes = L.rmt_n2_fit_step.argtypes + [vp, C.POINTER(C.c_int), C.POINTER(dbl)]
    L.rmt_n2_hiprtc_path.restype = cp
    L.rmt_n2_compile_options.restype = cp
    if L.rmt_n2_abi_version() != ABI_VERSION:
        raise RmtN2Error("librmt_n2.so ABI %d != binding ABI %d" % (L.rmt_n2_abi_version(), ABI_VERSION))
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise RmtN2Error(lib().rmt_n2_last_error().decode(errors="replace"))


def kernel_template():
    return lib().rmt_n2_kernel_template().decode()


def _side_code(prefix, src, arch, opts=""):
    """Code object of one of the two mechanism-independent side modules from the in-tree cache (compiled on first use;
    works without a GPU)."""
    import hashlib
    return compile_cached(src, "%s-%s" % (prefix, hashlib.sha256(src.encode()).hexdigest()[:24]), arch, opts)


class _SideModule:
    """What Monitor and Control share: the code buffer, the handle ``h`` of rmt_n2_<kind>_create on the current device,
    and its release."""
    kind = code_for = None           # "monitor" / "control", the infix of the C exports; monitor_code / control_code

    def __init__(self, arch="gfx950", code=None):
        code = self.code_for(arch) if code is None else code
        self._code = C.create_string_buffer(code, len(code))
        h = C.c_void_p()
        check(getattr(lib(), "rmt_n2_%s_create" % self.kind)(C.cast(self._code, C.c_void_p), len(code), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            getattr(lib(), "rmt_n2_%s_destroy" % self.kind)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def monitor_source():
    """The monitor's translation unit (csrc/monitor_kernels.inc, embedded in the library next to the template)."""
    return lib().rmt_n2_monitor_source().decode()


def monitor_code(arch="gfx950"):
    """Code object of the monitor kernels (_side_code)."""
    return _side_code("monitor", monitor_source(), arch)


class Monitor(_SideModule):
    """rmt_n2_monitor on the current device: row reductions of a state tensor [E][V][N] into out [E][V][5] doubles
    = {y[N-1], max, argmax, min, max|dydt|} (include/rmt_n2.h).  Independent of any mechanism."""
    kind, code_for = "monitor", staticmethod(monitor_code)

    def reduce(self, stream, y_ptr, dydt_ptr, E, V, N, fp32, out_ptr):
        """Enqueue the reduction on `stream` (a hipStream_t as integer); nothing is synchronised."""
        check(lib().rmt_n2_monitor_reduce(self.h, C.c_void_p(stream), C.c_void_p(y_ptr),
                                          C.c_void_p(dydt_ptr) if dydt_ptr else None, int(E), int(V), int(N),
                                          int(bool(fp32)), C.c_void_p(out_ptr)))

    def last_rows_per_block(self):
        """4: the last reduce ran one wave per row, 1: one workgroup per row."""
        return int(lib().rmt_n2_monitor_last_rows_per_block(self.h))


CONTROL_OPTS = "-ffp-contract=off"       # the control law: one rounded fp64 operation each, reproducible in numpy


def control_source():
    """The controller's translation unit (csrc/control_kernels.inc, embedded in the library next to the template)."""
    return lib().rmt_n2_control_source().decode()


def control_code(arch="gfx950"):
    """Code object of the control kernel, compiled with floating-point contraction off (_side_code)."""
    return _side_code("control", control_source(), arch, CONTROL_OPTS)


class Control(_SideModule):
    """rmt_n2_control on the current device: the sampled PI controller's kernel (include/rmt_n2.h).  Independent of any
    mechanism; ``update`` enqueues one kernel on the stream of the N2 handle whose device rows it writes."""
    kind, code_for = "control", staticmethod(control_code)

    def update(self, handle, y_ptr, V, N, params_ptr, setpoint_ptr, state_ptr, log_ptr, tail_at, field, hold=False):
        """Enqueue an update (or, with ``hold``, the rewrite of the held value); nothing is synchronised."""
        def ptr(p):
            return C.c_void_p(p) if p else None
        check(lib().rmt_n2_control_update(self.h, handle, ptr(y_ptr), int(V), int(N), ptr(params_ptr), ptr(setpoint_ptr),
                                          ptr(state_ptr), ptr(log_ptr), int(tail_at), int(field), int(bool(hold))))


FIT_OPTS = "-ffp-contract=off"           # both fit kernels: one rounded fp64 operation each, reproducible in numpy


def fit_source():
    """The fit's translation unit (csrc/fit_kernels.inc, embedded in the library next to the template)."""
    return lib().rmt_n2_fit_source().decode()


def fit_code(arch="gfx950"):
    """Code object of the two fit kernels, compiled with floating-point contraction off (_side_code)."""
    return _side_code("fit", fit_source(), arch, FIT_OPTS)


class Fit(_SideModule):
    """rmt_n2_fit on the current device: the residual reduction and the Levenberg-Marquardt step of solver-config "fit"
    (include/rmt_n2.h).  Independent of any mechanism; ``step`` enqueues its two kernels on the stream of the N2 handle
    whose device rows it writes."""
    kind, code_for = "fit", staticmethod(fit_code)

    def step(self, handle, y_ptr, sens_ptr, stats_ptr, S, V, N, columns, meas_ptr, MQ, contrib_ptr, pred_ptr, state_ptr,
             log_ptr, tolerance, damping):
        """Enqueue one pass (residuals, then the update); nothing is synchronised."""
        def ptr(p):
            return C.c_void_p(p) if p else None
        cols = (C.c_int*len(columns))(*[int(c) for c in columns])
        check(lib().rmt_n2_fit_step(self.h, handle, ptr(y_ptr), ptr(sens_ptr), ptr(stats_ptr), int(S), int(V), int(N),
                                    len(columns), cols, ptr(meas_ptr), int(MQ), ptr(contrib_ptr), ptr(pred_ptr),
                                    ptr(state_ptr), ptr(log_ptr), float(tolerance), float(damping)))

    def step_ex(self, handle, y_ptr, sens_ptr, stats_ptr, S, V, N, columns, meas_ptr, MQ, contrib_ptr, pred_ptr, state_ptr,
                log_ptr, tolerance, damping, pos_ptr, flags, box):
        """``step`` with the sibling kernels (rmt_n2_fit_step_ex): ``pos_ptr`` the position table on the device,
        ``flags`` [P] 1 = log-scaled, ``box`` [4][8] doubles (fit.box); the log slice is 70 doubles wide."""
        def ptr(p):
            return C.c_void_p(p) if p else None
        cols = (C.c_int*len(columns))(*[int(c) for c in columns])
        scale = (C.c_int*len(columns))(*[int(bool(f)) for f in flags])
        bx = (C.c_double*32)(*[float(v) for row in box for v in row])
        check(lib().rmt_n2_fit_step_ex(self.h, handle, ptr(y_ptr), ptr(sens_ptr), ptr(stats_ptr), int(S), int(V), int(N),
                                       len(columns), cols, ptr(meas_ptr), int(MQ), ptr(contrib_ptr), ptr(pred_ptr),
                                       ptr(state_ptr), ptr(log_ptr), float(tolerance), float(damping), ptr(pos_ptr), scale,
                                       bx))


def compile_source(source, arch="gfx950", extra_opts=""):
    """hipRTC compile -> bytes of the code object (works without a GPU)."""
    L = lib()
    code, size, log = C.c_void_p(), C.c_size_t(), C.c_void_p()
    rc = L.rmt_n2_compile(source.encode(), arch.encode(), extra_opts.encode(), C.byref(code),
                          C.byref(size), C.byref(log))
    logtxt = C.string_at(log.value).decode(errors="replace") if log.value else ""
    if log.value:
        L.rmt_n2_free(log)
    if rc != 0:
        raise RmtN2Error(L.rmt_n2_last_error().decode(errors="replace"))
    blob = C.string_at(code.value, size.value)
    L.rmt_n2_free(code)
    return blob, logtxt


_RTC_TAG = None


def hiprtc_tag():
    """Short identity of the hipRTC in this process.  The image has two - /opt/rocm's and the one bundled with
    PyTorch (used by every process that imported torch before this library); both call themselves 9.0 but
    generate different code - so the tag is derived from the library file that is actually loaded."""
    global _RTC_TAG
    if _RTC_TAG is None:
        import hashlib
        path = os.path.realpath(lib().rmt_n2_hiprtc_path().decode() or "unknown")
        try:
            size = os.path.getsize(path)
        except OSError:
            size = 0
        # ... and from the options the library compiles with by default
        _RTC_TAG = hashlib.sha256(("%s:%d:%s" % (path, size, lib().rmt_n2_compile_options().decode())).encode()
                                  ).hexdigest()[:8]
    return _RTC_TAG


def compile_cached(source, key, arch="gfx950", extra_opts=""):
    """Code objects are cached in-tree (rmt_app_amd/_kcache/<key>-rtc<compiler tag>-<arch>.hsaco): the directory
    travels with the repo snapshot, a cache under $HOME would not.  The compiler's identity is part of the name,
    so objects of the two hipRTCs of this image never stand in for each other."""
    os.makedirs(CACHE_DIR, exist_ok=True)
    key = "%s-rtc%s" % (key, hiprtc_tag())
    if extra_opts:
        import hashlib
        key = "%s-%s" % (key, hashlib.sha256(extra_opts.encode()).hexdigest()[:8])
    path = os.path.join(CACHE_DIR, "%s-%s.hsaco" % (key, arch))
    if os.path.exists(path):
        with open(path, "rb") as f:
            return f.read()
    blob, _ = compile_source(source, arch, extra_opts)
    tmp = path + ".tmp%d" % os.getpid()
    with open(tmp, "wb") as f:
        f.write(blob)
    os.replace(tmp, path)
    return blob
