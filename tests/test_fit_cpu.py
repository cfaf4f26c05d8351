"""solver-config "fit" without a GPU: validation (before any device work), the measurement table, the numpy restatements
of the two kernels - the Levenberg-Marquardt law on a linear and on a Rosenbrock-type problem, a failed trial, the frozen
state; the residual kernel's arithmetic against a direct evaluation of the formulas - the cross-compilation of the kernels'
translation unit, the C exports and the header, the reference of golden G22 (tools/make_golden.py fit, tests/fit_ref.py)
and the result-entry arithmetic on the golden's J^T J."""
import ctypes
import os

import numpy as np
import pytest

import fit_ref as FR
import inputs as INP
from rmt_app_amd import fit, hipbind, isa, plan, rmtExe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fit_input(**over):
    """case FA's input on made-up data (the validation never looks at the values)"""
    mi = FR.case_input("FA", measured=[np.full(len(FR.labels(e)), 0.5) for e in range(8)])
    mi["solver-config"]["fit"].update(over)
    return mi


def raises(exc, text, mi):
    with pytest.raises(exc) as err:
        out = rmtExe(mi)
        if isinstance(out, dict) and out.get("resModel") is None:          # (rmtExe may hand an exception back)
            raise AssertionError("no result")
    assert text in str(err.value), str(err.value)


# ----------------------------------------------------------------------------- validation
def test_absent_key_parses_to_none():
    mi = FR.base_input()
    assert "fit" not in mi["solver-config"] and fit.parse(mi) is None
    fit.check_model(dict(mi, model="M2"))


def test_parsed_spec_and_table():
    ft = fit.parse(fit_input())
    assert ft.names == ["A1", "A3"] and ft.labels == ["rate-constant:A1", "rate-constant:A3"]
    assert (ft.E, ft.MQ, ft.M) == (8, 6, sum(len(FR.labels(e)) for e in range(8)))
    assert [[q[0] for q in x] for x in ft.experiments] == [FR.labels(e) for e in range(8)]
    assert (ft.max_iterations, ft.tolerance, ft.damping, ft.batch) == (30, 1e-8, 1e-3, 8)
    tab = ft.table()
    S = 6
    assert tab.shape == (8, 6, 3)
    assert list(tab[1, :, 0]) == [4, 5, 3, 2, S, S + 1] and list(tab[4, :, 0]) == [5, S, 0, 0, 0, 0]
    assert list(tab[4, :, 2]) == [1e4, 10.0, 0, 0, 0, 0] and np.all(tab[4, 2:] == 0)
    members = ft.members(fit_input())
    assert len(members) == 8 and members[0]["external-heat"]["MeTe"] == 508.0
    assert members[0]["feed"]["volumetric-flowrate"] == FR.FLOW


def _exp(**kw):
    return [dict({"measured": {"outlet-temperature": 600.0}}, **kw)]


@pytest.mark.parametrize("over, exc, text", [
    ({"bounds": [0, 1]}, ValueError, "unknown key 'bounds'"),
    ({"experiments": _exp(weight=1)}, ValueError, "unknown key 'weight'"),
    ({"experiments": _exp(measured={"outlet-pressure": 1.0})}, ValueError, "unknown key 'outlet-pressure' in 'measured'"),
    ({"parameters": [{"rate-constant": "A9"}]}, ValueError, "'A9' is not an entry of reaction-rates.VARS"),
    ({"parameters": [{"rate-constant": "K1"}]}, NotImplementedError, "VARS['K1'] is not a scalar constant"),
    ({"parameters": ["medium-temperature"]}, ValueError, "a parameter is a dict {'rate-constant': VARS name}"),
    ({"experiments": _exp(measured={"outlet-mole-fraction": {"N2": 0.1}})}, ValueError, "'N2' is not a shell component"),
    ({"experiments": _exp(measured={})}, ValueError, "experiment 0 has no measured value at all"),
    ({"experiments": _exp(sigma={"outlet-temperature": 0.0})}, ValueError, "'sigma' of 'outlet-temperature' must be > 0"),
    ({"experiments": _exp(sigma={"outlet-temperature": -1.0})}, ValueError, "must be > 0"),
    ({"parameters": [{"rate-constant": "A1"}]*9}, ValueError, "holds 9 entries, at most 8"),
    ({"experiments": _exp()*4097}, ValueError, "holds 4097 entries, at most 4096"),
    ({"experiments": _exp(conditions={"reaction-rates": {"VARS": {"A1": 1.0}}})}, ValueError,
     "gives the fitted constant 'A1' a value of its own"),
    ({"max-iterations": 0}, ValueError, "'max-iterations' must be an integer >= 1"),
])
def test_bad_specs_raise_before_any_device_work(over, exc, text):
    raises(exc, text, fit_input(**over))


def test_temperature_measurement_in_an_isothermal_run_raises():
    mi = fit_input(experiments=_exp())
    mi["operating-conditions"]["process-type"] = "iso-thermal"
    raises(ValueError, "measures 'outlet-temperature' in an iso-thermal run", mi)


@pytest.mark.parametrize("key, value", [
    ("ensemble", [{}]), ("schedule", {"times": [0.0]}), ("control", {}), ("monitor", {"samples": 4}), ("initial", "steady"),
    ("sensitivity", {"parameters": ["medium-temperature"]}), ("deactivation", {}), ("axial-profile", {})])
def test_keys_that_cannot_stand_beside_fit(key, value):
    mi = fit_input()
    mi["solver-config"][key] = value
    raises(NotImplementedError, "solver-config 'fit' is not available with %r" % key, mi)


def test_fp32_multi_rank_and_other_models_raise():
    mi = fit_input()
    mi["solver-config"]["dtype"] = "fp32"
    raises(NotImplementedError, "not available with 'dtype': 'fp32'", mi)
    with pytest.raises(NotImplementedError, match="multi-rank"):
        fit.parse(fit_input(), multi_rank=True)
    mi = fit_input()
    mi["model"] = "M2"
    raises(NotImplementedError, "solver-config 'fit' is only available for model 'N2'", mi)


# ----------------------------------------------------------------------------- the law in numpy
def sums_of(r, J):
    P = J.shape[1]
    s = np.zeros(fit.CONTRIB)
    s[0] = 0.5*float(r @ r)
    s[1:1 + P] = J.T @ r
    H = J.T @ J
    for a in range(P):
        for b in range(a, P):
            s[1 + 8 + fit.tri(a, b)] = H[a, b]
    return s


def iterate(fun, p0, passes, tol=1e-10, damping=1e-3, failed=()):
    """emulate_update around ``fun(p) -> (r, J)``: the log slices"""
    p0 = np.asarray(p0, dtype=float)
    state, at, logs = np.zeros(fit.STATE), p0, []
    for k in range(passes):
        s = sums_of(*fun(at))
        if k in failed:
            s[0], s[fit.CONTRIB - 1] = 0.0, 1.0             # the lowest cost there is - with a failed experiment
        logs.append(fit.emulate_update(s, state, len(p0), p0, tol, damping))
        at = logs[-1][fit.LOG_PTRIAL:fit.LOG_PTRIAL + len(p0)].copy()
    return np.array(logs), state


def test_linear_problem_converges_in_one_accepted_step():
    rng = np.random.default_rng(1)
    A, b = rng.standard_normal((12, 3)), rng.standard_normal(12)
    want = np.linalg.lstsq(A, b, rcond=None)[0]
    logs, state = iterate(lambda p: (A @ p - b, A), [1.0, 2.0, 3.0], 5, tol=1e-6, damping=1e-12)
    assert list(logs[:2, 4]) == [1.0, 1.0]                   # the first pass sets the point, the second accepts the step
    assert np.allclose(logs[0, fit.LOG_PTRIAL:fit.LOG_PTRIAL + 3], want, rtol=1e-9, atol=1e-12)
    assert np.allclose(logs[1, fit.LOG_PCUR:fit.LOG_PCUR + 3], want, rtol=1e-9, atol=1e-12)
    assert logs[1, 5] == 1.0 and np.all(logs[1:, 5] == 1.0)  # converged with that step: the next one is below the tolerance
    assert np.isclose(logs[1, 1], 0.5*np.sum((A @ want - b)**2), rtol=1e-12)
    assert np.array_equal(logs[1, fit.LOG_PTRIAL:fit.LOG_PTRIAL + 3], logs[1, fit.LOG_PCUR:fit.LOG_PCUR + 3])


def rosenbrock(p):
    return np.array([10.0*(p[1] - p[0]**2), 1.0 - p[0]]), np.array([[-20.0*p[0], 10.0], [-1.0, 0.0]])


def test_rosenbrock_rejects_and_converges():
    logs, state = iterate(rosenbrock, [-1.2, 1.0], 60, tol=1e-10, damping=1e-3)
    n = int(np.argmax(logs[:, 5]))
    assert logs[n, 5] == 1.0 and n < 59
    assert np.sum(logs[1:n + 1, 4] == 0.0) >= 1, "no rejection"
    assert np.allclose(logs[n, fit.LOG_PCUR:fit.LOG_PCUR + 2], [1.0, 1.0], rtol=1e-8)
    cur = logs[:n + 1, 1]
    assert np.all(np.diff(cur) <= 0)                          # the current cost never rises
    rej = np.nonzero(logs[1:n + 1, 4] == 0.0)[0] + 1
    assert np.all(logs[rej, 2] > logs[rej - 1, 2])            # lambda grows at a rejection


def test_failed_trial_is_rejected_whatever_its_cost():
    logs, state = iterate(rosenbrock, [-1.2, 1.0], 4, failed=(2,))
    assert logs[2, 0] == 0.0 and logs[2, 6] == 1.0 and logs[2, 4] == 0.0
    assert logs[2, 1] == logs[1, 1] and np.array_equal(logs[2, 16:18], logs[1, 16:18])
    assert logs[2, 2] == logs[1, 2]*logs[1, 3] and logs[2, 3] == 2*logs[1, 3]
    # the new trial lies nearer to the current point than the failed one
    d_new = np.abs(logs[2, 8:10] - logs[2, 16:18])
    d_old = np.abs(logs[1, 8:10] - logs[1, 16:18])
    assert np.all(d_new <= d_old) and np.any(d_new < d_old)
    # a failed FIRST pass is flagged
    state = np.zeros(fit.STATE)
    s = sums_of(*rosenbrock(np.array([-1.2, 1.0])))
    s[fit.CONTRIB - 1] = 2.0
    log = fit.emulate_update(s, state, 2, [-1.2, 1.0], 1e-8, 1e-3)
    assert int(log[7]) & fit.FIRST_FAILED and np.array_equal(log[8:10], [-1.2, 1.0])


def test_frozen_state_changes_nothing():
    logs, state = iterate(rosenbrock, [-1.2, 1.0], 60)
    assert state[4] == 1.0
    before = state.copy()
    s = sums_of(*rosenbrock(np.array([3.0, -2.0])))
    log = fit.emulate_update(s, state, 2, [0.0, 0.0], 1e-8, 1e-3)
    assert np.array_equal(state, before)
    assert log[4] == 0.0 and log[5] == 1.0 and log[0] == s[0] and log[1] == before[1]
    assert np.array_equal(log[8:16], before[fit.ST_PCUR:fit.ST_PCUR + 8]) and np.array_equal(log[8:16], log[16:24])
    assert np.array_equal(log[24:32], s[1:9]) and np.array_equal(log[32:68], s[9:45])


def test_not_positive_definite_is_a_status():
    J = np.array([[1.0, np.nan], [0.0, 1.0]])
    state = np.zeros(fit.STATE)
    s = sums_of(np.array([1.0, 1.0]), np.array([[1.0, 0.0], [0.0, 1.0]]))
    s[1 + 8 + fit.tri(1, 1)] = -1.0                           # floored to 1e-300: the pivot stays negative
    log = fit.emulate_update(s, state, 2, [1.0, 1.0], 1e-8, 1e-3)
    assert int(log[7]) == fit.NOT_POSITIVE and np.array_equal(log[8:10], [1.0, 1.0])
    assert log[2] == 1e-3*1e8


# ----------------------------------------------------------------------------- the residual kernel in numpy
def synthetic(E, P, MQ, S=6, N=20, seed=0):
    """random buffers of the residual kernel: a clamped species, a tied maximum, a padded tail, a NaN in a temperature row"""
    rng = np.random.default_rng(seed)
    V = S + 1
    y = rng.uniform(0.05, 1.0, (E, V, N))
    y[:, S] = rng.uniform(0.0, 0.3, (E, N))
    sens = rng.standard_normal((E, P, V + 1, N))
    rows = rng.uniform(0.5, 2.0, (E, 16 + S + 8))
    rows[:, 0], rows[:, 1] = rng.uniform(100, 600, E), rng.uniform(450, 550, E)
    meas = np.zeros((E, MQ, 3))
    for e in range(E):
        y[e, e % S, N - 1] = 0.0 if e % 3 == 0 else 1e-31          # at and below the clamp
        a, b = sorted(rng.choice(N, 2, replace=False))
        y[e, S, a] = y[e, S, b] = 0.5                                # a tied maximum: the lower node wins
        if e % 4 == 1 and N > 3:
            y[e, S, (a + 1) % N if (a + 1) % N != b else (a + 2) % N] = np.nan
        n = 1 + (e % MQ)
        codes = rng.permutation(S + 2)[:n] if n <= S + 2 else np.resize(rng.permutation(S + 2), n)
        meas[e, :n, 0] = codes
        meas[e, :n, 1] = rng.uniform(0, 1, n)
        meas[e, :n, 2] = rng.uniform(1, 100, n)
    stats = np.zeros((E, 4))
    stats[:, 1] = -1.0
    return y, sens, stats, rows, meas


def direct(y, sens, rows, meas, S):
    """the formulas of sensitivity.result_entry, vectorised, for one experiment: (pred, r, J)"""
    cmax, tf = rows[0], rows[1]
    N = y.shape[1]
    yo = y[:S, N - 1]
    conc = np.maximum(yo, 1e-30)*cmax
    dconc = np.where(yo > 1e-30, sens[:, :S, N - 1]*cmax, 0.0)              # [P][S]
    ctot = conc.sum()
    x = conc/ctot
    dx = dconc/ctot - conc[None, :]*dconc.sum(axis=1, keepdims=True)/ctot**2
    T = y[S]
    peak = int(np.argmax(np.where(np.isnan(T), -np.inf, T)))
    pred, J = [], []
    for code, value, w in meas:
        code = int(code)
        if w == 0:
            pred.append(0.0)
            J.append(np.zeros(sens.shape[0]))
        elif code < S:
            pred.append(x[code])
            J.append(dx[:, code]*w)
        else:
            n = N - 1 if code == S else peak
            pred.append(T[n]*tf + tf)
            J.append(sens[:, S, n]*tf*w)
    pred, J = np.array(pred), np.array(J)
    return pred, (pred - meas[:, 1])*meas[:, 2], J


def test_emulate_residuals_against_the_formulas():
    S, P = 6, 3
    y, sens, stats, rows, meas = synthetic(9, P, 7)
    stats[5, 1] = 3.0                                               # a failed march
    sens[7, 1, S, 19] = np.inf                                      # a number that is not finite
    meas[7, 0] = S, 0.2, 5.0
    pred, contrib = fit.emulate_residuals(y, sens, stats, rows, meas, S)
    for e in range(9):
        p, r, J = direct(y[e], sens[e], rows[e], meas[e], S)
        assert np.allclose(pred[e], p, rtol=1e-14, atol=0, equal_nan=True)
        if e == 7:
            continue
        assert np.isclose(contrib[e, 0], 0.5*r @ r, rtol=1e-13)
        assert np.allclose(contrib[e, 1:1 + P], J.T @ r, rtol=1e-12, atol=1e-12*np.abs(J).max()*np.abs(r).max())
        H = J.T @ J
        assert np.allclose(fit.full(contrib[e, 9:45], P), H, rtol=1e-12, atol=1e-12*np.abs(H).max())
        assert np.all(contrib[e, 1 + P:9] == 0)
    assert list(contrib[:, 45]) == [0, 0, 0, 0, 0, 1, 0, 1, 0]
    # the tied maximum: the lower of the two nodes
    T = y[0, S]
    assert np.sum(T == T.max()) == 2
    # sums in index order
    sums = fit.column_sums(contrib[:5])
    acc = np.zeros(46)
    for e in range(5):
        acc += contrib[e]
    assert np.array_equal(sums, acc)


# ----------------------------------------------------------------------------- the unit, the exports, the header
def test_fit_kernels_cross_compile_without_contraction():
    src = hipbind.fit_source()
    assert src == open(os.path.join(ROOT, "rmt_app_amd", "csrc", "fit_kernels.inc")).read()
    assert hipbind.FIT_OPTS == "-ffp-contract=off"
    blob = hipbind.fit_code("gfx950")
    assert blob[:4] == b"\x7fELF"
    assert any(f.startswith("fit-") and f.endswith("-gfx950.hsaco") for f in os.listdir(hipbind.CACHE_DIR))
    for kernel in ("rmt_n2_fit_residuals_f64", "rmt_n2_fit_update_f64"):
        assert kernel.encode() in blob
        res = isa.kernel_resources(blob, kernel)
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (kernel, res)
    assert isa.kernel_resources(blob, "rmt_n2_fit_residuals_f64")["group_segment_fixed_size"] == 0
    F = plan.MEMBER_FIELDS
    for name, val in (("RMT_FIT_M_CMAX", F["CMAX"]), ("RMT_FIT_M_TF", F["TF"]), ("RMT_FIT_M_USER", F["CIN"]),
                      ("RMT_FIT_CONTRIB", fit.CONTRIB), ("RMT_FIT_STATE", fit.STATE), ("RMT_FIT_LOG", fit.LOG),
                      ("RMT_FIT_TRI", fit.TRI), ("RMT_FIT_ST_PCUR", fit.ST_PCUR), ("RMT_FIT_ST_PTRIAL", fit.ST_PTRIAL),
                      ("RMT_FIT_ST_G", fit.ST_G), ("RMT_FIT_ST_H", fit.ST_H), ("RMT_FIT_ST_DELTA", fit.ST_DELTA),
                      ("RMT_FIT_FIRST_FAILED", fit.FIRST_FAILED), ("RMT_FIT_NOT_POSITIVE", fit.NOT_POSITIVE)):
        assert "#define %s %d" % (name, val) in src, name
    # the template and its ORDER do not know the unit
    assert "fit_kernels" not in open(os.path.join(ROOT, "rmt_app_amd", "csrc", "kernels", "ORDER")).read()
    assert "rmt_n2_fit" not in hipbind.kernel_template()


def test_exports_and_header():
    L = ctypes.CDLL(hipbind.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rmt_n2.h")).read()
    for name in ("rmt_n2_fit_source", "rmt_n2_fit_create", "rmt_n2_fit_destroy", "rmt_n2_fit_step"):
        assert hasattr(L, name), name
        assert name + "(" in header, name
    assert hipbind.lib().rmt_n2_abi_version() == 2 and "#define RMT_N2_ABI_VERSION 2" in header     # additions only
    # argument errors name the function
    lib = hipbind.lib()
    assert lib.rmt_n2_fit_create(None, 0, None) != 0 and b"rmt_n2_fit_create" in lib.rmt_n2_last_error()
    cols = (ctypes.c_int*1)(0)
    assert lib.rmt_n2_fit_step(None, None, None, None, None, 6, 7, 20, 1, cols, None, 1, None, None, None, None, 1e-8,
                               1e-3) != 0
    assert b"rmt_n2_fit_step: null argument" in lib.rmt_n2_last_error()


# ----------------------------------------------------------------------------- golden G22
@pytest.mark.slow
def test_reference_reproduces_the_golden_optimum():
    """fit_ref's reference on the oracle, from the golden steady states (about half a minute: 40 steady states): at the
    golden's p_ref the predictions are the golden's data and the reference's own Gauss-Newton step vanishes - p_ref is the
    optimum of the reference.  (A whole refit from the start takes minutes: tools/make_golden.py fit=FA.)"""
    from oracle import n2_oracle as O
    gold = FR.golden("FA")
    ref = FR.Reference(O, FR.CASES["FA"]["parameters"])
    ref.last = list(np.load(os.path.join(FR.GOLD, "g22_fit_states.npz"))["states"])
    truth = []
    for e in range(8):
        n = len(FR.labels(e))
        assert np.array_equal(gold["measured"][e][:n], gold["predicted_true"][e][:n])       # noise-free
        assert np.all(np.isnan(gold["measured"][e][n:]))
        truth.append(gold["measured"][e][:n])
    p_ref = np.array(gold["p_ref"])
    r = ref.residual(p_ref, truth)
    assert ref.worst <= FR.CR.GATE
    assert np.max(np.abs(r)) <= 1e-6, r                    # weighted: 1e-10 of a mole fraction, 1e-7 K
    J = ref.jacobian(p_ref, truth)
    step = np.linalg.solve(J.T @ J, -J.T @ r)
    print("G22 FA: p_ref %s, reference step there %s, cost %.3e (golden %.3e)" % (p_ref, step/p_ref, 0.5*r @ r, gold["cost"]))
    assert np.all(np.abs(step) <= 1e-7*np.abs(p_ref))
    assert np.all(np.abs(p_ref - FR.p_true("FA")) <= FR.TRUE_CAP*FR.p_true("FA"))
    assert np.allclose(J.T @ J, gold["hessian"], rtol=1e-5)
    meta = FR.meta()
    assert meta["cases"]["FA"]["cond"] <= FR.COND_CAP and meta["p_true"] == FR.P_TRUE


def test_statistics_against_numpy_on_the_golden_hessian():
    gold = FR.golden("FN")
    H, cost = np.array(gold["hessian"]), float(gold["cost"])
    ft = fit.parse(FR.case_input("FN"))
    st = fit.statistics(H, cost, ft.M)
    cov = 2*cost/(ft.M - 2)*np.linalg.inv(H)
    assert np.allclose(st["covariance"], cov, rtol=1e-12)
    assert np.allclose(st["covariance"], gold["covariance"], rtol=1e-9)
    assert np.allclose(st["standard-error"], np.sqrt(np.diag(cov)), rtol=1e-12)
    assert np.allclose(st["correlation"], cov/np.sqrt(np.outer(np.diag(cov), np.diag(cov))), rtol=1e-12)
    assert np.allclose(np.diag(st["correlation"]), 1.0)
    assert fit.statistics(H, cost, 2) == {"covariance": None, "standard-error": None, "correlation": None}
    # the result entry: from the log slices
    last = np.zeros(fit.LOG)
    last[1], last[5] = cost, 1.0
    last[fit.LOG_PCUR:fit.LOG_PCUR + 2] = gold["p_ref"]
    for a in range(2):
        for b in range(a, 2):
            last[fit.LOG_H + fit.tri(a, b)] = H[a, b]
    entry = ft.result_entry(np.array([last]), [1.0, 2.0], last)
    assert np.array_equal(entry["hessian"], H) and np.array_equal(entry["values"], gold["p_ref"])
    assert entry["cost"] == cost and entry["iterations"] == 1 and entry["converged"] is True
    assert np.allclose(entry["covariance"], cov, rtol=1e-12) and entry["parameters"] == ft.labels
    assert list(entry["initial"]) == [1.0, 2.0] and len(entry["history"]) == 1
