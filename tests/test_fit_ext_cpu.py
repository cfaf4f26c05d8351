"""solver-config "fit" with log-scaled and bounded parameters and measurements along the bed, without a GPU: the new
keys' validation (before any device work), the table of a spec without them, the numpy restatements of the extended
kernels (fit.emulate_residuals_ex, fit.emulate_update_ex) - identical to the plain law without flags and bounds, a bounded
linear problem against scipy.optimize.lsq_linear, Rosenbrock in a box, a log-scaled exponential fit, all parameters on
bounds - the interpolation against the direct formula, the cross-compilation of the four kernels, the export and the header,
and the result-entry arithmetic on a bound."""
import ctypes
import os

import numpy as np
import pytest

import fit_ext_ref as FX
import fit_ref as FR
from test_fit_cpu import ROOT, fit_input, iterate, raises, rosenbrock, sums_of, synthetic
from rmt_app_amd import fit, hipbind, isa

INF = np.inf


def with_parameters(params, **over):
    mi = fit_input(**over)
    mi["solver-config"]["fit"]["parameters"] = params
    return mi


# ----------------------------------------------------------------------------- validation
def test_parameter_entry_with_scale_and_bounds_parses():
    """(the first test that fails without the feature: such an entry raised "a parameter is a dict")"""
    a3 = FR.P_TRUE["A3"]*0.7
    ft = fit.parse(with_parameters([{"rate-constant": "A1"},
                                    {"rate-constant": "A3", "scale": "log", "bounds": [1e3, None]}]))
    assert ft.names == ["A1", "A3"] and ft.scales == ["linear", "log"] and ft.flags == [0, 1] and ft.extended
    assert np.array_equal(ft.lo, [-INF, 1e3]) and np.array_equal(ft.hi, [INF, INF])
    bx = ft.box()
    assert bx.shape == (4, 8) and bx[0, 1] == 1e3 and bx[2, 1] == np.log(1e3) and bx[2, 0] == -INF and bx[3, 1] == INF
    assert np.all(bx[0::2, 2:] == -INF) and np.all(bx[1::2, 2:] == INF)
    assert a3 > 1e3


@pytest.mark.parametrize("entry, text", [
    ({"rate-constant": "A3", "scale": "sqrt"}, "parameter 'A3': 'scale' must be 'linear' or 'log'"),
    ({"rate-constant": "A3", "bounds": [1.0]}, "parameter 'A3': 'bounds' must be [lo, hi]"),
    ({"rate-constant": "A3", "bounds": [1e5, 1e4]}, "parameter 'A3': 'bounds' must be lo < hi"),
    ({"rate-constant": "A3", "bounds": [1e4, 1e4]}, "parameter 'A3': 'bounds' must be lo < hi"),
    ({"rate-constant": "A3", "bounds": [1e6, None]}, "parameter 'A3': the starting value"),
    ({"rate-constant": "A3", "bounds": [None, 1.0]}, "parameter 'A3': the starting value"),
    ({"rate-constant": "A3", "scale": "log", "bounds": [0.0, 1e6]}, "parameter 'A3': the lower bound of a 'log' parameter"),
    ({"rate-constant": "A3", "scale": "log", "bounds": [-1.0, None]}, "parameter 'A3': the lower bound of a 'log' parameter"),
    ({"rate-constant": "A3", "bounds": [float("nan"), None]}, "parameter 'A3': 'bounds' must be a finite number"),
])
def test_bad_parameter_entries_raise_before_any_device_work(entry, text):
    raises(ValueError, text, with_parameters([{"rate-constant": "A1"}, entry]))


def test_log_scale_needs_a_positive_start():
    for start in (0.0, -2.0):
        mi = with_parameters([{"rate-constant": "A3", "scale": "log"}])
        mi["reaction-rates"]["VARS"]["A3"] = start
        raises(ValueError, "parameter 'A3': 'scale': 'log' needs a starting value > 0", mi)


def _exp(measured, **kw):
    return [dict({"measured": measured}, **kw)]


@pytest.mark.parametrize("measured, text", [
    ({"temperature-profile": {"position": [0.1, 0.2], "value": [500.0]}}, "'temperature-profile' must be a dict"),
    ({"temperature-profile": [0.1, 500.0]}, "'temperature-profile' must be a dict"),
    ({"temperature-profile": {"position": [1.5], "value": [500.0]}}, "a position is z/L in [0, 1]"),
    ({"temperature-profile": {"position": [-0.1], "value": [500.0]}}, "a position is z/L in [0, 1]"),
    ({"mole-fraction-profile": {"N2": {"position": [0.5], "value": [0.1]}}}, "'N2' is not a shell component"),
    ({"mole-fraction-profile": {"DME": {"position": [0.5]}}}, "'mole-fraction-profile' of 'DME' must be a dict"),
    ({"temperature-profile": {"position": [0.01*k for k in range(65)], "value": [500.0]*65}}, "holds 65 measured values"),
    ({"temperature-profile": {"position": [0.5, 0.5], "value": [500.0, 501.0]}}, "'temperature-profile:0.5' twice"),
    ({"mole-fraction-profile": {"DME": {"position": [0.25, 0.2500000001], "value": [0.1, 0.1]}}},
     "'mole-fraction-profile:DME:0.25' twice"),
])
def test_bad_profiles_raise_before_any_device_work(measured, text):
    raises(ValueError, text, fit_input(experiments=_exp(measured)))


def test_profile_sigma_and_isothermal():
    raises(ValueError, "'sigma' of 'temperature-profile' must be > 0",
           fit_input(experiments=_exp({"outlet-temperature": 600.0}, sigma={"temperature-profile": 0.0})))
    mi = fit_input(experiments=_exp({"temperature-profile": {"position": [0.5], "value": [500.0]}}))
    mi["operating-conditions"]["process-type"] = "iso-thermal"
    raises(ValueError, "measures 'temperature-profile' in an iso-thermal run", mi)


def test_profile_entries_labels_table_and_positions():
    measured = {"outlet-mole-fraction": {"DME": 0.01}, "outlet-temperature": 520.0,
                "temperature-profile": {"position": [0.0, 0.25, 1.0], "value": [528.1, 531.0, 526.2]},
                "mole-fraction-profile": {"DME": {"position": [0.5, 1.0], "value": [0.008, 0.015]}}}
    sigma = {"temperature-profile": 0.5, "mole-fraction-profile": 1e-3}
    ft = fit.parse(fit_input(experiments=_exp(measured, sigma=sigma)))
    S = 6
    assert [q[0] for q in ft.experiments[0]] == ["outlet-mole-fraction:DME", "outlet-temperature", "temperature-profile:0",
                                                 "temperature-profile:0.25", "temperature-profile:1",
                                                 "mole-fraction-profile:DME:0.5", "mole-fraction-profile:DME:1"]
    tab = ft.table()
    assert tab.shape == (1, 7, 3)                                   # the [E][MQ][3] layout does not change
    assert list(tab[0, :, 0]) == [5, S, S + 2, S + 2, S + 2, S + 3 + 5, S + 3 + 5]
    assert list(tab[0, :, 2]) == [1.0, 1.0, 2.0, 2.0, 2.0, 1e3, 1e3]
    assert ft.extended and ft.scales == ["linear", "linear"]
    pos = ft.position_table(20)
    assert pos.shape == (1, 7, 2) and np.all(pos[0, :2] == 0)
    assert list(pos[0, 2]) == [0.0, 0.0] and list(pos[0, 4]) == [18.0, 1.0] and list(pos[0, 6]) == [18.0, 1.0]
    assert pos[0, 3, 0] == 4.0 and pos[0, 3, 1] == 0.25*19 - 4 and list(pos[0, 5]) == [9.0, 0.5]


def test_input_without_new_keys_parses_as_before():
    ft = fit.parse(fit_input())
    assert not ft.extended and ft.scales == ["linear"]*2 and ft.flags == [0, 0]
    assert np.all(ft.lo == -INF) and np.all(ft.hi == INF)
    assert all(z is None for zs in ft.positions for z in zs)
    tab = ft.table()
    assert tab.shape == (8, 6, 3) and list(tab[1, :, 0]) == [4, 5, 3, 2, 6, 7]
    plain = fit.Fit(ft.names, ft.experiments, ft.conditions, ft.S, 30, 1e-8, 1e-3, 8)       # the constructor of before
    assert not plain.extended and np.array_equal(plain.table(), tab)


# ----------------------------------------------------------------------------- the extended law in numpy
def iterate_ex(fun, p0, passes, flags, lo, hi, tol=1e-10, damping=1e-3):
    """emulate_update_ex around ``fun(p) -> (r, J)`` with J = d r / d p: the log slices and the state"""
    p0 = np.asarray(p0, dtype=float)
    P = len(p0)
    bx = fit.box(lo, hi, flags)
    state, at, logs = np.zeros(fit.STATE), p0, []
    for k in range(passes):
        r, J = fun(at)
        J = J*np.where(np.array(flags) != 0, at, 1.0)[None, :]          # d / d theta = p d / d p
        logs.append(fit.emulate_update_ex(sums_of(r, J), state, P, p0, tol, damping, flags, bx))
        at = logs[-1][fit.LOG_PTRIAL:fit.LOG_PTRIAL + P].copy()
    return np.array(logs), state


def test_without_flags_and_bounds_the_extended_law_is_the_plain_law():
    rng = np.random.default_rng(1)
    A, b = rng.standard_normal((12, 3)), rng.standard_normal(12)
    problems = [(lambda p: (A @ p - b, A), [1.0, 2.0, 3.0], 5, 1e-6, 1e-12), (rosenbrock, [-1.2, 1.0], 60, 1e-10, 1e-3)]
    for fun, p0, passes, tol, damping in problems:
        P = len(p0)
        logs, state = iterate(fun, p0, passes, tol=tol, damping=damping)
        ex, state_ex = iterate_ex(fun, p0, passes, [0]*P, [-INF]*P, [INF]*P, tol=tol, damping=damping)
        assert ex.shape == (passes, fit.LOG_EX) and np.array_equal(ex[:, :fit.LOG], logs)
        assert np.all(ex[:, fit.LOG:] == 0) and np.array_equal(state_ex, state)
    # a failed trial and a failed first pass, slice by slice on the same sums
    state, state_ex, bx = np.zeros(fit.STATE), np.zeros(fit.STATE), fit.box([-INF]*2, [INF]*2, [0, 0])
    at = np.array([-1.2, 1.0])
    for k in range(6):
        s = sums_of(*rosenbrock(at))
        if k == 2:
            s[0], s[fit.CONTRIB - 1] = 0.0, 1.0
        a = fit.emulate_update(s, state, 2, [-1.2, 1.0], 1e-8, 1e-3)
        b2 = fit.emulate_update_ex(s, state_ex, 2, [-1.2, 1.0], 1e-8, 1e-3, [0, 0], bx)
        assert np.array_equal(a, b2[:fit.LOG]) and np.array_equal(state, state_ex), k
        at = a[8:10].copy()
    s = sums_of(np.array([1.0, 1.0]), np.eye(2))
    s[1 + 8 + fit.tri(1, 1)] = -1.0
    a = fit.emulate_update(s, np.zeros(fit.STATE), 2, [1.0, 1.0], 1e-8, 1e-3)
    b2 = fit.emulate_update_ex(s, np.zeros(fit.STATE), 2, [1.0, 1.0], 1e-8, 1e-3, [0, 0], bx)
    assert int(a[7]) == fit.NOT_POSITIVE and np.array_equal(a, b2[:fit.LOG])


def active(row, P):
    return [(int(row[fit.LOG_UPPER]) >> j & 1) - (int(row[fit.LOG_LOWER]) >> j & 1) for j in range(P)]


def test_bounded_linear_problem_against_lsq_linear():
    import scipy.optimize
    rng = np.random.default_rng(3)
    A, b = rng.standard_normal((15, 4)), rng.standard_normal(15)
    free = np.linalg.lstsq(A, b, rcond=None)[0]
    lo = np.array([-INF, free[1] + 0.3, -INF, -5.0])                 # the free optimum violates lo[1] and hi[2]
    hi = np.array([INF, INF, free[2] - 0.2, 5.0])
    want = scipy.optimize.lsq_linear(A, b, bounds=(lo, hi), method="bvls", tol=1e-14)
    assert want.success and want.active_mask[1] == -1 and want.active_mask[2] == 1
    p0 = np.array([0.0, free[1] + 1.0, free[2] - 1.0, 0.0])
    logs, state = iterate_ex(lambda p: (A @ p - b, A), p0, 30, [0]*4, lo, hi, tol=1e-10, damping=1e-9)
    n = int(np.argmax(logs[:, 5]))
    got = logs[n, fit.LOG_PCUR:fit.LOG_PCUR + 4]
    assert logs[n, 5] == 1.0 and logs[n, 7] == 0.0
    assert got[1] == lo[1] and got[2] == hi[2]                       # exactly the bounds
    assert np.allclose(got, want.x, rtol=1e-8, atol=1e-10)
    assert active(logs[n], 4) == [0, -1, 1, 0] == list(want.active_mask)
    assert np.isclose(logs[n, 1], want.cost, rtol=1e-10)
    assert np.all(np.diff(logs[:n + 1, 1]) <= 0)
    trials = logs[:, fit.LOG_PTRIAL:fit.LOG_PTRIAL + 4]
    assert np.all(trials >= lo) and np.all(trials <= hi)             # no trial leaves the box


def test_rosenbrock_in_a_box_ends_on_a_face():
    """min over x <= 0.5: on the face x = 0.5 the optimum is y = x^2 = 0.25, cost 1/2 (1 - 0.5)^2"""
    lo, hi = [-1.5, -0.5], [0.5, 2.0]
    logs, state = iterate_ex(rosenbrock, [-1.2, 1.0], 80, [0, 0], lo, hi, tol=1e-10)
    n = int(np.argmax(logs[:, 5]))
    got = logs[n, fit.LOG_PCUR:fit.LOG_PCUR + 2]
    assert logs[n, 5] == 1.0 and n < 79 and logs[n, 7] == 0.0
    assert got[0] == 0.5 and abs(got[1] - 0.25) <= 1e-8
    assert active(logs[n], 2) == [1, 0] and state[fit.ST_UPPER] == 1.0 and state[fit.ST_LOWER] == 0.0
    assert np.isclose(logs[n, 1], 0.125, rtol=1e-9)
    assert np.all(np.diff(logs[:n + 1, 1]) <= 0)
    trials = logs[:, fit.LOG_PTRIAL:fit.LOG_PTRIAL + 2]
    assert np.all(trials >= lo) and np.all(trials <= hi)


def exponential(t, y):
    def fun(p):
        e = np.exp(-p[1]*t)
        return p[0]*e - y, np.stack([e, -p[0]*t*e], axis=1)
    return fun


def test_log_scaled_exponential_fit_from_a_start_whose_linear_step_is_negative():
    t = np.linspace(0.0, 4.0, 9)
    truth = np.array([2.0, 1.5])
    fun = exponential(t, truth[0]*np.exp(-truth[1]*t))
    p0 = np.array([0.5, 4.0])
    r, J = fun(p0)
    gn = p0 + np.linalg.solve(J.T @ J, -J.T @ r)
    assert gn[1] < 0                                                 # the Gauss-Newton step in p walks b through zero
    logs, state = iterate_ex(fun, p0, 60, [1, 1], [-INF]*2, [INF]*2, tol=1e-12)
    n = int(np.argmax(logs[:, 5]))
    assert logs[n, 5] == 1.0 and logs[n, 7] == 0.0
    assert np.allclose(logs[n, fit.LOG_PCUR:fit.LOG_PCUR + 2], truth, rtol=1e-9)
    assert np.all(logs[:, fit.LOG_PTRIAL:fit.LOG_PTRIAL + 2] > 0)    # every trial stays positive
    assert active(logs[n], 2) == [0, 0]
    # the same with a box that holds the optimum: the same optimum
    boxed, _ = iterate_ex(fun, p0, 60, [1, 1], [0.05, 1e-3], [5.0, 10.0], tol=1e-12)
    m = int(np.argmax(boxed[:, 5]))
    assert boxed[m, 5] == 1.0 and np.allclose(boxed[m, fit.LOG_PCUR:fit.LOG_PCUR + 2], truth, rtol=1e-9)
    trials = boxed[:, fit.LOG_PTRIAL:fit.LOG_PTRIAL + 2]
    assert np.all(trials >= [0.05, 1e-3]) and np.all(trials <= [5.0, 10.0])


def test_all_parameters_on_bounds_is_converged_with_zero_step():
    """the free optimum of the exponential lies beyond both bounds the start sits on"""
    t = np.linspace(0.0, 4.0, 9)
    fun = exponential(t, 2.0*np.exp(-1.5*t))
    for flags in ([0, 0], [1, 1], [0, 1]):
        p0 = np.array([1.0, 3.0])                                    # a wants to grow past hi = 1, b to fall below lo = 3
        logs, state = iterate_ex(fun, p0, 3, flags, [0.1, 3.0], [1.0, 9.0])
        assert logs[0, 5] == 1.0 and logs[0, 4] == 1.0 and logs[0, 7] == 0.0, flags
        assert active(logs[0], 2) == [1, -1]
        assert np.array_equal(logs[0, 8:10], p0) and np.array_equal(logs[0, 16:18], p0)
        assert np.all(state[fit.ST_DELTA:fit.ST_DELTA + 2] == 0.0)
        assert np.array_equal(logs[1, 8:24], logs[0, 8:24]) and np.array_equal(logs[1, 68:], logs[0, 68:])    # frozen


def test_clamped_step_uses_the_models_own_reduction():
    """one component clamped: the logged trial is the bound itself and the predicted reduction in the state is
    -(g^T d + 1/2 d^T H d) of the clamped step"""
    rng = np.random.default_rng(5)
    A, b = rng.standard_normal((10, 2)), rng.standard_normal(10)
    free = np.linalg.lstsq(A, b, rcond=None)[0]
    p0 = free + np.array([1.0, -1.0])
    lo, hi = np.array([free[0] + 0.5, -INF]), np.array([INF, INF])
    state = np.zeros(fit.STATE)
    r = A @ p0 - b
    log = fit.emulate_update_ex(sums_of(r, A), state, 2, p0, 1e-10, 1e-9, [0, 0], fit.box(lo, hi, [0, 0]))
    assert log[fit.LOG_PTRIAL] == lo[0]
    d = state[fit.ST_DELTA:fit.ST_DELTA + 2]
    g, H = A.T @ r, A.T @ A
    assert np.isclose(d[0], lo[0] - p0[0], rtol=1e-15) and np.isclose(state[7], -(g @ d + 0.5*d @ H @ d), rtol=1e-12)
    assert state[7] > 0 and log[7] == 0.0


# ----------------------------------------------------------------------------- interpolation
def profile_buffers(E=3, P=2, S=6, N=20, seed=2):
    y, sens, stats, rows, meas = synthetic(E, P, 8, S=S, N=N, seed=seed)
    y[:, S][np.isnan(y[:, S])] = 0.2
    places = [0.0, 1.0, 7.0/19.0, 0.5*(3 + 4)/19.0]                  # z = 0, z = 1, node 7, midway between 3 and 4
    pos = np.zeros((E, 8, 2))
    meas[:] = 0.0
    for e in range(E):
        for q, z in enumerate(places):
            meas[e, q] = S + 2, 0.3, 2.0
            meas[e, 4 + q] = S + 3 + (e + q) % S, 0.1, 50.0
            pos[e, q] = pos[e, 4 + q] = fit.position(z, N)
    return y, sens, stats, rows, meas, pos, places


def test_interpolation_against_the_direct_formula():
    S, N, P = 6, 20, 2
    y, sens, stats, rows, meas, pos, places = profile_buffers()
    assert fit.position(0.0, N) == (0.0, 0.0) and fit.position(1.0, N) == (18.0, 1.0)
    assert fit.position(0.5*7/19.0, N)[0] == 3.0 and abs(fit.position(0.5*7/19.0, N)[1] - 0.5) <= 1e-14
    pos[:, 2] = pos[:, 6] = 7.0, 0.0                                 # exactly node 7, whatever 7/19*19 rounds to
    pred, contrib = fit.emulate_residuals_ex(y, sens, stats, rows, meas, S, pos, [1, 0], [0, 0])
    for e in range(3):
        cmax, tf = rows[e, 0], rows[e, 1]
        T = y[e, S]*tf + tf
        dT = sens[e, :, S]*tf
        conc = np.maximum(y[e, :S], 1e-30)*cmax
        X = conc/conc.sum(axis=0)
        dconc = np.where(y[e, :S] > 1e-30, sens[e, :, :S]*cmax, 0.0)                    # [P][S][N]
        dX = dconc/conc.sum(axis=0) - conc[None]*dconc.sum(axis=1, keepdims=True)/conc.sum(axis=0)**2
        # f = 0 and f = 1: the node value bit for bit
        assert pred[e, 0] == T[0] and pred[e, 1] == T[N - 1] and pred[e, 2] == T[7]
        for q in range(4):
            sp = (e + q) % S
            assert pred[e, 4 + q] == pytest.approx(FX.interpolate(X[sp], places[q]), rel=1e-14)
        assert pred[e, 4] == X[e % S, 0] and pred[e, 5] == X[(e + 1) % S, N - 1] and pred[e, 6] == X[(e + 2) % S, 7]
        assert pred[e, 3] == pytest.approx(0.5*(T[3] + T[4]), rel=1e-15)
        assert pred[e, 7] == pytest.approx(0.5*(X[(e + 3) % S, 3] + X[(e + 3) % S, 4]), rel=1e-14)
        # the Jacobian rows: the same combination, weighted
        J = np.zeros((8, P))
        J[0], J[1], J[2], J[3] = dT[:, 0], dT[:, N - 1], dT[:, 7], 0.5*(dT[:, 3] + dT[:, 4])
        for q, (a, f) in enumerate([(0, 0.0), (N - 2, 1.0), (7, 0.0), (3, 0.5)]):
            sp = (e + q) % S
            J[4 + q] = (1 - f)*dX[:, sp, a] + f*dX[:, sp, a + 1]
        J = J*meas[e, :, 2:3]
        r = (pred[e] - meas[e, :, 1])*meas[e, :, 2]
        assert np.isclose(contrib[e, 0], 0.5*r @ r, rtol=1e-13)
        assert np.allclose(contrib[e, 1:1 + P], J.T @ r, rtol=1e-11, atol=1e-12*np.abs(J).max()*np.abs(r).max())
        H = J.T @ J
        assert np.allclose(fit.full(contrib[e, 9:45], P), H, rtol=1e-11, atol=1e-12*np.abs(H).max())
        assert contrib[e, 45] == 0.0


def test_log_flags_scale_the_jacobian_by_the_members_own_value_and_old_codes_are_unchanged():
    S = 6
    y, sens, stats, rows, meas = synthetic(9, 3, 7)
    pos = np.zeros((9, 7, 2))
    plain = fit.emulate_residuals(y, sens, stats, rows, meas, S)
    same = fit.emulate_residuals_ex(y, sens, stats, rows, meas, S, pos, [2, 0, 1], [0, 0, 0])
    assert np.array_equal(plain[0], same[0], equal_nan=True) and np.array_equal(plain[1], same[1], equal_nan=True)
    cols = [2, 0, 1]
    pred, contrib = fit.emulate_residuals_ex(y, sens, stats, rows, meas, S, pos, cols, [1, 0, 1])
    assert np.array_equal(pred, plain[0], equal_nan=True) and np.array_equal(contrib[:, 0], plain[1][:, 0], equal_nan=True)
    for e in (0, 2, 3):
        s = np.array([rows[e, 16 + S + cols[0]], 1.0, rows[e, 16 + S + cols[2]]])
        assert np.allclose(contrib[e, 1:4], plain[1][e, 1:4]*s, rtol=1e-12)
        assert np.allclose(fit.full(contrib[e, 9:45], 3), fit.full(plain[1][e, 9:45], 3)*np.outer(s, s), rtol=1e-12)
    # a record outside the mesh, or a code the table must not hold, fails the member
    meas[0, 0] = S + 2, 0.5, 1.0
    pos[0, 0] = 19.0, 0.0
    assert fit.emulate_residuals_ex(y, sens, stats, rows, meas, S, pos, cols, [0, 0, 0])[1][0, 45] == 1.0
    pos[0, 0] = 18.0, 1.0
    assert fit.emulate_residuals_ex(y, sens, stats, rows, meas, S, pos, cols, [0, 0, 0])[1][0, 45] == 0.0
    meas[0, 0, 0] = 2*S + 3
    assert fit.emulate_residuals_ex(y, sens, stats, rows, meas, S, pos, cols, [0, 0, 0])[1][0, 45] == 1.0


# ----------------------------------------------------------------------------- the result entry
def test_result_entry_on_a_bound_and_in_log_scale():
    mi = with_parameters([{"rate-constant": "A1", "scale": "log"}, {"rate-constant": "A3", "bounds": [None, 7.5e4]}])
    ft = fit.parse(mi)
    values = np.array([35.0, 7.5e4])
    Ht = np.array([[4.0e2, 3.0e-3], [3.0e-3, 9.0e-8]])              # in (ln A1, A3)
    last = np.zeros(fit.LOG_EX)
    last[1], last[5], last[fit.LOG_UPPER] = 12.5, 1.0, 2.0
    last[fit.LOG_PCUR:fit.LOG_PCUR + 2] = values
    for a in range(2):
        for b in range(a, 2):
            last[fit.LOG_H + fit.tri(a, b)] = Ht[a, b]
    entry = ft.result_entry(np.array([last]), [45.0, 5.8e4], last)
    assert entry["scale"] == ["log", "linear"] and list(entry["active-bounds"]) == [0, 1]
    assert np.array_equal(entry["bounds"], [[-INF, INF], [-INF, 7.5e4]])
    Hp = Ht*np.outer([1/35.0, 1.0], [1/35.0, 1.0])
    assert np.allclose(entry["hessian"], Hp, rtol=1e-15)
    var = 2*12.5/(ft.M - 1)/Hp[0, 0]                                 # one free parameter: M - P counts the free ones
    cov = entry["covariance"]
    assert np.isclose(cov[0, 0], var, rtol=1e-13) and np.all(np.isnan(cov[1])) and np.all(np.isnan(cov[:, 1]))
    assert np.isclose(entry["standard-error"][0], np.sqrt(var), rtol=1e-13) and np.isnan(entry["standard-error"][1])
    assert entry["correlation"][0, 0] == 1.0 and np.isnan(entry["correlation"][0, 1])
    assert "A3 at the upper 75000" in ft.bounds_text(last) and ft.bounds_text(np.zeros(fit.LOG)) == ""
    # a plain spec: the three entries are there, the statistics are the old ones
    plain = fit.parse(fit_input())
    e2 = plain.result_entry(np.array([last[:fit.LOG]]), [1.0, 2.0], last[:fit.LOG])
    assert e2["scale"] == ["linear"]*2 and list(e2["active-bounds"]) == [0, 0] and np.all(np.isinf(e2["bounds"]))
    assert np.array_equal(e2["hessian"], Ht)
    assert np.allclose(e2["covariance"], fit.statistics(Ht, 12.5, plain.M)["covariance"], rtol=0)


# ----------------------------------------------------------------------------- the unit, the export, the header
def test_four_kernels_cross_compile_with_the_resource_conditions():
    blob = hipbind.fit_code("gfx950")
    src = hipbind.fit_source()
    kernels = ("rmt_n2_fit_residuals_f64", "rmt_n2_fit_update_f64", "rmt_n2_fit_residuals_ex_f64",
               "rmt_n2_fit_update_ex_f64")
    for kernel in kernels:
        assert kernel.encode() in blob
        res = isa.kernel_resources(blob, kernel)
        print(kernel, res)
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (kernel, res)
    for kernel in kernels[::2]:
        assert isa.kernel_resources(blob, kernel)["group_segment_fixed_size"] == 0
    assert "template <bool EX>" in src and src.count("rmt_fit_cholesky(s_a, P)") == 1          # one law
    for name, val in (("RMT_FIT_LOG_EX", fit.LOG_EX), ("RMT_FIT_ST_LOWER", fit.ST_LOWER), ("RMT_FIT_ST_UPPER", fit.ST_UPPER),
                      ("RMT_FIT_M_USER", fit.MEMBER_USER)):
        assert "#define %s %d" % (name, val) in src, name
    assert fit.LOG_LOWER == fit.LOG and fit.LOG_UPPER == fit.LOG + 1


def test_export_header_and_argument_errors():
    L = ctypes.CDLL(hipbind.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rmt_n2.h")).read()
    assert hasattr(L, "rmt_n2_fit_step_ex") and "rmt_n2_fit_step_ex(" in header
    assert hipbind.lib().rmt_n2_abi_version() == 2 and "#define RMT_N2_ABI_VERSION 2" in header     # additions only
    lib = hipbind.lib()
    cols, flags = (ctypes.c_int*1)(0), (ctypes.c_int*1)(0)
    bx = (ctypes.c_double*32)(*fit.box([-INF], [INF], [0]).ravel())
    head = (None, None, None, None, None, 6, 7, 20, 1, cols, None, 1, None, None, None, None, 1e-8, 1e-3)
    assert lib.rmt_n2_fit_step_ex(*head, None, flags, bx) != 0
    assert b"rmt_n2_fit_step_ex: null argument" in lib.rmt_n2_last_error()
    assert lib.rmt_n2_fit_step_ex(*head, ctypes.c_void_p(8), flags, bx) != 0
    assert b"rmt_n2_fit_step_ex: null argument" in lib.rmt_n2_last_error()
    assert lib.rmt_n2_fit_step(*head) != 0 and b"rmt_n2_fit_step: null argument" in lib.rmt_n2_last_error()


# ----------------------------------------------------------------------------- goldens G24
def test_goldens_fc_and_fp_are_what_the_recipe_promises():
    meta = FX.meta()
    fc, fp = FX.golden("FC"), FX.golden("FP")
    hi = 0.9*FR.P_TRUE["A3"]
    assert fc["p_ref"][1] == hi == fc["hi"][1] and list(fc["active"]) == [0, 1] and np.isinf(fc["lo"]).all()
    assert np.isnan(fc["covariance"][1]).all() and np.isfinite(fc["covariance"][0, 0])
    assert float(fc["residual_gate"]) <= FR.CR.GATE and float(fp["residual_gate"]) <= FR.CR.GATE
    assert float(fp["cond"]) <= FR.COND_CAP and list(fp["active"]) == [0, 0]
    assert meta["cases"]["FC"]["p_ref"] == list(fc["p_ref"]) and meta["cases"]["FP"]["p_ref"] == list(fp["p_ref"])
    for e in range(8):
        assert len(FX.ext_labels("FP", e)) == len(FR.labels(e)) + 6
        assert FX.ext_labels("FP", e)[-6:] == ["temperature-profile:0", "temperature-profile:0.263158",
                                               "temperature-profile:0.3", "temperature-profile:0.62",
                                               "temperature-profile:1", "mole-fraction-profile:DME:0.5"]
        # the old entries are G22's noisy data
        n = len(FR.labels(e))
        assert np.array_equal(fp["measured"][e][:n], FR.golden("FN")["measured"][e][:n])
    ft = fit.parse(FX.case_input("FP"))
    assert [[q[0] for q in x] for x in ft.experiments] == [FX.ext_labels("FP", e) for e in range(8)]
    assert ft.extended and ft.MQ == 12
    fc_in = fit.parse(FX.case_input("FC"))
    assert fc_in.hi[1] == hi and np.isinf(fc_in.hi[0]) and fc_in.extended
    assert not fit.parse(FX.case_input("FC", plain=True)).extended
