"""solver-config "fit" on the device: the two kernels of csrc/fit_kernels.inc on synthetic buffers against their numpy
restatements (fit.emulate_residuals, fit.emulate_update), and the fit through rmtExe against the goldens G22
(tools/make_golden.py fit, tests/fit_ref.py).  zNo = 20 throughout.

Bounds:
* kernels alone: pred, contrib, the 46 sums and the log bit for bit (the kernels are compiled with contraction off; fp64
  division and square root are correctly rounded on the device);
* fitted values against their target (p_true; case FN: the reference's p_ref): 10 |p_ref - p_true| of the golden plus
  fit_ref.FLOOR_REL of the target (10 x the first measured discrepancy, never above 1e-6: profiles/fit.md);
* predictions against the golden's at p_true: STATE_BOUND of tests/test_gpu_initial.py (1e-8) of the value's magnitude;
* FN: cost within 1e-6 relative, covariance entries within fit_ref.COV_BOUND of sqrt(C_ii C_jj).
Each test prints its figures."""
import numpy as np
import pytest

import fit_ref as FR
from test_fit_cpu import synthetic
from rmt_app_amd import fit, n2, plan, rmtExe

pytestmark = pytest.mark.gpu

STATE_BOUND = 1e-8       # tests/test_gpu_initial.py
N = FR.ZNO


def open_unit(mi, names, members=None, NP=None):
    """a handle of the sensitivity unit with ``names`` as per-reactor inputs on the members' rows: (device, mech, rows)"""
    inputs = members or [mi]
    mech = plan.Mechanism(mi, params=tuple(names))
    rows = np.array([plan.member_constants(m, mech, N)[1] for m in inputs])
    cp = n2.sens_plan(mech, N, NP or len(names), None, rows)
    dev = n2.N2Device(mech, rows, N, block=cp.block, npt=cp.npt, specialize=False, features=cp.features, defines=cp.defines)
    return dev, mech, rows


class Loop:
    """the buffers rmt_n2_fit_step takes, as n2.FitLoop holds them, on given data"""

    def __init__(self, dev, E, MQ, columns, meas, passes, tolerance=1e-8, damping=1e-3):
        torch = dev.torch
        self.E, self.MQ, self.columns, self.tolerance, self.damping = E, MQ, list(columns), tolerance, damping
        self.kernel = n2.hipbind.Fit(n2.device_arch(dev.device))
        self.meas = torch.from_numpy(np.ascontiguousarray(meas)).to(dev.device)
        self.contrib = torch.full((E, fit.CONTRIB), -7.0, dtype=torch.float64, device=dev.device)
        self.pred = torch.full((E, MQ), -7.0, dtype=torch.float64, device=dev.device)
        self.state = torch.zeros(fit.STATE, dtype=torch.float64, device=dev.device)
        self.log = torch.zeros((passes, fit.LOG), dtype=torch.float64, device=dev.device)

    def close(self):
        self.kernel.close()


# ----------------------------------------------------------------------------- 1. the kernels alone
@pytest.mark.parametrize("E, P, MQ", [(1, 1, 3), (65, 3, 5), (130, 8, 7)])
def test_kernels_on_synthetic_buffers(E, P, MQ):
    mi = FR.wide_input()
    dev, mech, rows = open_unit(mi, FR.WIDE, [mi]*E, NP=1)
    S = mech.S
    try:
        rng = np.random.default_rng(E)
        rows[:, 0] *= rng.uniform(0.5, 1.5, E)
        rows[:, 1] *= rng.uniform(0.9, 1.1, E)
        at = plan.MEMBER_FIXED + S
        rows[:, at:at + 8] = np.linspace(1.0, 2.0, 8)[None, :]          # (one value per column for all members)
        dev.set_members(rows)
        y, sens, stats, _, meas = synthetic(E, P, MQ, S=S, N=N, seed=E)
        if E > 1:
            y[1:, S][np.isnan(y[1:, S])] = 0.1                          # (member 0 alone may fail: passes 1.. are trials)
        columns = list(range(P))[::-1]                                  # not in row order
        loop = Loop(dev, E, MQ, columns, meas, 3)
        torch = dev.torch
        d_y = torch.from_numpy(y.reshape(E, -1)).to(dev.device)
        d_s = torch.from_numpy(sens).to(dev.device)
        state, want_rows, p0 = np.zeros(fit.STATE), rows.copy(), rows[0, at + np.array(columns)]
        for k in range(3):
            if k == 1:
                stats[E//2, 1] = 4.0                                    # a member whose march failed
            if k == 2:
                stats[E//2, 1] = -1.0
                d_y.mul_(1.0 + 1e-3)
                y = d_y.cpu().numpy().reshape(E, S + 1, N)
            dev._stats.copy_(torch.from_numpy(stats))
            dev.fit_step(d_y, d_s, loop, k)
            pred, contrib = fit.emulate_residuals(y, sens, stats, want_rows, meas, S)
            got_pred, got_contrib = loop.pred.cpu().numpy(), loop.contrib.cpu().numpy()
            assert np.array_equal(got_pred, pred, equal_nan=True), (k, np.argwhere(got_pred != pred)[:4])
            assert np.array_equal(got_contrib, contrib, equal_nan=True), (k, np.argwhere(got_contrib != contrib)[:4])
            log = loop.log[k].cpu().numpy()
            sums = fit.column_sums(contrib)
            assert np.array_equal(log[fit.LOG_G:fit.LOG_G + 8], sums[1:9], equal_nan=True)
            assert np.array_equal(log[fit.LOG_H:], sums[9:45], equal_nan=True)
            assert np.array_equal(log[[0, 6]], sums[[0, 45]], equal_nan=True)
            want = fit.emulate_update(sums, state, P, p0, loop.tolerance, loop.damping)
            assert np.array_equal(log, want, equal_nan=True), (k, log[:16], want[:16])
            assert np.array_equal(loop.state.cpu().numpy(), state, equal_nan=True)
            # the user columns of every member are the logged p_trial, every other row entry is untouched
            for j, c in enumerate(columns):
                want_rows[:, at + c] = log[fit.LOG_PTRIAL + j]
            assert np.array_equal(dev.get_members(), want_rows, equal_nan=True), k
        print("E = %d, P = %d, MQ = %d: failed members per pass %s, accepted %s, lambda %s"
              % (E, P, MQ, loop.log[:, 6].cpu().numpy(), loop.log[:, 4].cpu().numpy(), loop.log[:, 2].cpu().numpy()))
        loop.close()
    finally:
        dev.close()


# ----------------------------------------------------------------------------- 2. / 3. the law on the device
def drive(name, passes, fail_at=None, **cfg):
    """the hot loop by hand on the golden case's data: (logs [passes][68], rows after every pass)"""
    mi = FR.case_input(name, **cfg)
    ft = fit.parse(mi)
    dev, mech, rows = open_unit(mi, ft.names, ft.members(mi))
    try:
        loop = Loop(dev, ft.E, ft.MQ, ft.columns(mech), ft.table(), passes, ft.tolerance, ft.damping)
        kinds, idx = ft.sensitivity().descriptors(mech)
        y = dev.to_device(np.zeros((ft.E, mech.V*N)))
        for k in range(passes):
            dev.steady_march(y)
            raw = dev.steady_sens(y, kinds, idx)
            if k == fail_at:
                dev._stats[3, 1] = 3.0                           # plain data: member 3 counts as failed in this pass
            dev.fit_step(y, raw, loop, k)
        logs = loop.log.cpu().numpy()
        loop.close()
        return logs, ft, rows[0, plan.MEMBER_FIXED + mech.S + np.array(ft.columns(mech))]
    finally:
        dev.close()


def test_failed_member_rejects_the_trial():
    logs, ft, p0 = drive("FA", 3, fail_at=1)
    a, b = logs[0], logs[1]
    assert a[4] == 1.0 and a[6] == 0.0
    assert b[6] == 1.0 and b[4] == 0.0 and b[1] == a[1] and b[7] == 0.0
    assert b[2] == a[2]*a[3] and b[3] == 2*a[3]                   # lambda grows
    P = ft.NP
    cur = a[fit.LOG_PCUR:fit.LOG_PCUR + P]
    assert np.array_equal(b[fit.LOG_PCUR:fit.LOG_PCUR + P], cur)
    d0 = np.abs(a[fit.LOG_PTRIAL:fit.LOG_PTRIAL + P] - cur)
    d1 = np.abs(b[fit.LOG_PTRIAL:fit.LOG_PTRIAL + P] - cur)
    print("failed member in pass 1: lambda %.3e -> %.3e, |trial - current| %s -> %s" % (a[2], b[2], d0, d1))
    assert np.all(d1 <= d0) and np.any(d1 < d0)
    assert logs[2, 6] == 0.0                                       # the next pass is an ordinary trial again


def test_law_on_the_device_against_the_emulation():
    logs, ft, p0 = drive("FA", 12)
    state, worst = np.zeros(fit.STATE), 0.0
    P = ft.NP
    for k, row in enumerate(logs):
        sums = np.zeros(fit.CONTRIB)
        sums[0], sums[1:9], sums[9:45], sums[45] = row[0], row[24:32], row[32:68], row[6]
        want = fit.emulate_update(sums, state, P, p0, ft.tolerance, ft.damping)
        assert np.array_equal(want[[4, 5, 6, 7]], row[[4, 5, 6, 7]]), (k, want[:8], row[:8])
        rel = np.max(np.abs(want[8:8 + P] - row[8:8 + P])/np.abs(row[8:8 + P]))
        worst = max(worst, rel)
        assert rel <= 1e-12, (k, rel)
        # (the emulation follows the device's own trial from here on)
        state[fit.ST_PTRIAL:fit.ST_PTRIAL + 8] = row[8:16]
        state[fit.ST_PCUR:fit.ST_PCUR + 8] = row[16:24]
        state[1:4] = row[1:4]
    print("law on the device: %d passes, accepted %s, converged at pass %d, largest |p_trial - emulation| / |p_trial| = %.3e"
          % (len(logs), logs[:, 4], int(np.argmax(logs[:, 5])), worst))
    assert logs[-1, 5] == 1.0


# ----------------------------------------------------------------------------- 4. - 8. through rmtExe
_RUNS = {}


def run(name, **cfg):
    key = (name, tuple(sorted(cfg.items())))
    if key not in _RUNS:
        _RUNS[key] = rmtExe(FR.case_input(name, **dict(FR.CASES[name].get("config", {}), **cfg)))["resModel"]
    return _RUNS[key]


@pytest.mark.parametrize("name", ["FA", "FB"])
def test_rmtexe_recovers_p_true(name):
    """Both cases converge in 7 iterations, all accepted (profiles/fit.md).  The experiments' feed rate matters: between 15
    and 40 times the notebook's the law walks A3 through zero from these starts and does not come back (no bounds, no
    log-parameters: README, not built)."""
    res, gold = run(name), FR.golden(name)
    f = res["fit"]
    target = FR.p_true(name)
    err, bound = np.abs(f["values"] - target), FR.value_bound(name, gold)
    print("G22 %s on the device: %d iterations (%d accepted, %d rejected), cost %.3e, |value - p_true| / p_true = %s (bound %s; "
          "the reference's own %s)" % (name, f["iterations"], res["device-stats"]["accepted"], res["device-stats"]["rejected"],
                                       f["cost"], err/target, bound/target,
                                       np.abs(gold["p_ref_noise_free"] - target)/target))
    assert f["converged"] is True and f["parameters"] == ["rate-constant:%s" % nm for nm in FR.CASES[name]["parameters"]]
    assert np.allclose(f["initial"], np.array(FR.CASES[name]["start"])*target, rtol=1e-15)
    assert np.all(err <= bound), (err, bound)
    assert len(res["ensemble"]) == 8 and len(res["dataPack"]) == 1
    worst = 0.0
    for e, member in enumerate(res["ensemble"]):
        entry = member["fit"]
        want = gold["predicted_true"][e][:len(entry["labels"])]
        assert entry["labels"] == FR.labels(e) and len(member["dataPack"]) == 1
        rel = np.abs(entry["predicted"] - want)/np.abs(want)
        worst = max(worst, rel.max())
        assert np.all(rel <= STATE_BOUND), (e, rel)
        assert np.array_equal(entry["residual"], (entry["predicted"] - entry["measured"])/FR.sigmas(e))
    print("  largest |predicted - golden at p_true| / |value| = %.3e" % worst)
    assert f["hessian"].shape == (len(target),)*2 and f["covariance"].shape == f["hessian"].shape
    assert len(f["history"]) == f["iterations"]


def test_rmtexe_on_noisy_data_against_the_reference():
    res, gold = run("FN"), FR.golden("FN")
    f = res["fit"]
    p_ref = np.array(gold["p_ref"])
    err, bound = np.abs(f["values"] - p_ref), FR.value_bound("FN", gold)
    cov, want = f["covariance"], np.array(gold["covariance"])
    scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
    crel = np.abs(cov - want)/scale
    print("G22 FN on the device: %d iterations, |value - p_ref| / p_ref = %s (bound %s), cost %.9e against %.9e (%.2e), "
          "|covariance - reference| / sqrt(C_ii C_jj) at most %.3e, standard errors %s, correlation %.4f"
          % (f["iterations"], err/p_ref, bound/p_ref, f["cost"], float(gold["cost"]), abs(f["cost"]/float(gold["cost"]) - 1),
             crel.max(), f["standard-error"], f["correlation"][0, 1]))
    assert f["converged"] is True
    assert np.all(err <= bound), (err, bound)
    assert abs(f["cost"] - float(gold["cost"])) <= 1e-6*float(gold["cost"])
    assert FR.COV_BOUND <= 1e-3 and np.all(crel <= FR.COV_BOUND), crel


def test_batching_and_size_do_not_matter():
    a, b = run("FA", batch=1)["fit"], run("FA")["fit"]
    assert a["iterations"] == b["iterations"] and np.array_equal(a["values"], b["values"]) and a["cost"] == b["cost"]
    for x, y in zip(a["history"], b["history"]):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), k
    assert np.array_equal(a["hessian"], b["hessian"])
    # every experiment nine times: the same optimum, nine times the cost
    noisy, many = run("FN")["fit"], run("FN", repeat=9)["fit"]
    rel = np.abs(many["values"] - noisy["values"])/np.abs(noisy["values"])
    crel = abs(many["cost"]/(9*noisy["cost"]) - 1)
    print("E = 72 against E = 8: values differ by %s relative, cost / (9 cost) - 1 = %.3e, iterations %d and %d"
          % (rel, crel, many["iterations"], noisy["iterations"]))
    assert np.all(rel <= 1e-10) and crel <= 1e-12


def test_finishing_pass_leaves_the_state_of_the_fitted_values():
    """every member's dataPack against rmt_n2_steady_march on a handle of the same unit (the sensitivity unit with the fitted
    constants as per-reactor inputs - the code object the fit itself marches on) whose rows hold the fitted values: bit for
    bit"""
    res = run("FA")
    mi = FR.case_input("FA")
    ft = fit.parse(mi)
    for nm, v in zip(ft.names, res["fit"]["values"]):
        mi["reaction-rates"]["VARS"][nm] = float(v)
    dev, mech, rows = open_unit(mi, ft.names, ft.members(mi))
    try:
        y = dev.to_device(np.zeros((ft.E, mech.V*N)))
        dev.steady_march(y)
        st, flags = dev.march_result()
        assert not np.any(flags)
        Y = y.cpu().numpy().reshape(ft.E, mech.V, N)
    finally:
        dev.close()
    for e, member in enumerate(res["ensemble"]):
        pk = member["dataPack"][0]
        assert np.array_equal(pk["dataYCons1"], Y[e, :-1]) and np.array_equal(pk["dataYTemp1"], Y[e, -1]), e
    assert np.array_equal(res["dataPack"][0]["dataYs"], res["ensemble"][0]["dataPack"][0]["dataYs"])


def test_no_convergence_raises():
    with pytest.raises(RuntimeError) as err:
        rmtExe(FR.case_input("FA", **{"max-iterations": 2}))
    msg = str(err.value)
    print(msg)
    assert "no convergence within 2 iterations" in msg and "last cost" in msg and "A1 = " in msg and "A3 = " in msg
