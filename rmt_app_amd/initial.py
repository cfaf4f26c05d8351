"""Where a dynamic N2 run starts (solver-config "initial").

    "initial": "steady"                                   # or the dict form:
    "initial": {"kind": "steady", "tolerance": 1e-10, "max-iterations": 400}

* Absent: the reference's cold start - the feed composition along the whole bed at inlet temperature - and nothing of
  the run changes: no code object, no launch, no result entry.
* "steady": every member starts at the discrete steady state f(y*) = 0 of its OWN constants: with "schedule" the forced
  values at t = 0, with "control" the member's own value of the manipulated quantity (the controller's u0; the loop's
  state starts as it does without the key, I = 0).  t = 0 of the result, the output times and the launch list stay; only
  the state uploaded before the first launch differs.
* The steady state is found on the device by marching from the inlet (csrc/kernels/71_steady_march.inc,
  rmt_n2_steady_march): the discretisation is first-order upwind and the Ergun recurrence runs downstream, so node z
  depends on the nodes before it only, and every node is one V x V nonlinear solve - pseudo-transient continuation with
  the analytic node Jacobian.  "tolerance" bounds the scaled node residual max_i |f_i| / (F1 (zNo-1) max(|y_i|, 1e-6)) AND
  the last relative update of every node (a node whose residual stays above it at the noise of its own evaluation ends
  after three updates in a row within the bound); "max-iterations" the pseudo-time steps per node.
* A member whose march does not converge raises (device.flag_error: RMT_N2_FLAG_STEP / RMT_N2_FLAG_NONFINITE, the message
  names the member and the node).  There is no fallback to the cold start.
* On a coarse mesh a node may have several steady states.  The march follows the branch reached by relaxing from the
  upstream state.
* resModel["initial"] = {"kind", "residual", "iterations", "nodes-damped"}: max_n |dy/dt| of the started state as
  rmt_n2_rhs and the monitor's reduction measure it (not the solver's own estimate), the largest per-node step count and
  the number of nodes that needed a rejected pseudo-time step.

Host side only: parsing and validation, and the result entry.
"""
import numpy as np

KINDS = ("steady",)
KEYS = ("kind", "tolerance", "max-iterations")
MODELS = ("N2",)
DEFAULTS = {"tolerance": 1e-10, "max-iterations": 400}


def check_model(modelInput):
    """ValueError when the input asks for a start state on a model that has none (rmtExe, before any device work)."""
    if (modelInput.get('solver-config') or {}).get('initial') is not None and modelInput.get('model') not in MODELS:
        raise ValueError("solver-config 'initial' (start from the steady state) is only available for model 'N2' "
                         "(got model %r)" % (modelInput.get('model'),))


class Initial:
    """A parsed "initial" spec: ``kind``, ``tolerance``, ``max_iterations``."""

    def __init__(self, kind, tolerance, max_iterations):
        self.kind, self.tolerance, self.max_iterations = kind, float(tolerance), int(max_iterations)

    def result_entry(self, residual, iterations, damped):
        return {"kind": self.kind, "residual": float(residual), "iterations": int(iterations), "nodes-damped": int(damped)}


def parse(modelInput, multi_rank=False):
    """The Initial of a run (None when the input has no "initial"), or ValueError / NotImplementedError naming the
    offending key."""
    cfg = modelInput['solver-config']
    spec = cfg.get('initial')
    if spec is None:
        return None
    check_model(modelInput)
    if isinstance(spec, str):
        spec = {"kind": spec}
    if not isinstance(spec, dict):
        raise ValueError("solver-config 'initial' must be %r or a dict with the keys %s" % (KINDS[0], KEYS))
    for k in spec:
        if k not in KEYS:
            raise ValueError("solver-config 'initial': unknown key %r (known: %s)" % (k, ", ".join(KEYS)))
    kind = spec.get('kind')
    if kind not in KINDS:
        raise ValueError("solver-config 'initial': 'kind' must be one of %s (got %r)" % (KINDS, kind))
    tol = spec.get('tolerance', DEFAULTS['tolerance'])
    if isinstance(tol, (bool, np.bool_)) or not isinstance(tol, (int, float, np.integer, np.floating)) \
            or not np.isfinite(tol) or not tol > 0:
        raise ValueError("solver-config 'initial': 'tolerance' must be a positive number (got %r)" % (tol,))
    it = spec.get('max-iterations', DEFAULTS['max-iterations'])
    if isinstance(it, (bool, np.bool_)) or not isinstance(it, (int, np.integer)) or it < 1:
        raise ValueError("solver-config 'initial': 'max-iterations' must be an integer >= 1 (got %r)" % (it,))
    if cfg.get('dtype', 'fp64') in ('fp32', 'float32'):
        raise NotImplementedError("solver-config 'initial' is not available with 'dtype': 'fp32': the steady-state march "
                                  "is an fp64 kernel")
    if multi_rank:
        raise NotImplementedError("solver-config 'initial' is not available in a multi-rank run")
    return Initial(kind, tol, it)
