"""solver-config "fit" with log-scaled and bounded parameters and measurements along the bed, on the device: the sibling
kernels of csrc/fit_kernels.inc on synthetic buffers against their numpy restatements (fit.emulate_residuals_ex,
fit.emulate_update_ex), and the fit through rmtExe against the goldens G24 (tools/make_golden.py fit_ext,
tests/fit_ext_ref.py).  zNo = 20 throughout.

Bounds:
* kernels alone: pred, contrib, the 46 sums, the state, the log and the member rows bit for bit wherever no exp or log of
  the device is involved (the kernels are compiled with contraction off).  With log-scaled parameters the device takes
  ln p_cur and exp(delta) itself: the trial values, the clamped step and its predicted reduction are then compared with
  numpy's within EXP_BOUND relative - 10 x the largest difference first measured, never above 1e-13
  (profiles/fit_constraints.md) - pass by pass from the device's own previous state;
* fitted values against their target: fit_ref.value_bound's construction, 10 x the reference's own miss of p_true plus
  FLOOR_REL of the target (10 x the first measured discrepancy, never above 1e-6);
* FP: cost within 1e-6 relative, covariance entries within COV_BOUND of sqrt(C_ii C_jj) (10 x the first measured value,
  never above 1e-3).
Each test prints its figures."""
import numpy as np
import pytest

import fit_ext_ref as FX
import fit_ref as FR
from test_gpu_fit import Loop, open_unit, run as run_g22
from rmt_app_amd import fit, plan, rmtExe

pytestmark = pytest.mark.gpu

N = FR.ZNO
PASSES = 5
# 10 x the first measured figures (profiles/fit_constraints.md): 3.811e-16 (cap 1e-13); FC 4.104e-10, FP 1.411e-10,
# FL 4.603e-11 (cap 1e-6); 1.298e-8 (cap 1e-3)
EXP_BOUND = 3.9e-15
FLOOR_REL = {"FC": 4.2e-9, "FP": 1.5e-9, "FL": 4.7e-10}
COV_BOUND = 1.3e-7


class LoopEx(Loop):
    """the buffers rmt_n2_fit_step_ex takes, as n2.FitLoop holds them for an extended spec"""

    def __init__(self, dev, E, MQ, columns, meas, passes, pos, flags, box, **kw):
        Loop.__init__(self, dev, E, MQ, columns, meas, passes, **kw)
        torch = dev.torch
        self.pos = torch.from_numpy(np.ascontiguousarray(pos)).to(dev.device)
        self.flags, self.box = list(flags), box
        self.log = torch.zeros((passes, fit.LOG_EX), dtype=torch.float64, device=dev.device)


def synthetic_ex(E, P, MQ, S, seed):
    """random buffers with every code, old and new: species, outlet and peak temperature, temperature and mole fraction at
    positions with f = 0, f = 1, the last interval and interior ones; padded tails; a clamped species at a port"""
    from test_fit_cpu import synthetic
    y, sens, stats, _, _ = synthetic(E, P, MQ, S=S, N=N, seed=seed)
    y[:, S][np.isnan(y[:, S])] = 0.1
    rng = np.random.default_rng(seed + 1000)
    meas, pos = np.zeros((E, MQ, 3)), np.zeros((E, MQ, 2))
    codes = np.arange(2*S + 3)
    for e in range(E):
        n = MQ if e % 2 == 0 else 1 + (e % MQ)                       # full tables (lane MQ-1) and padded ones
        c = np.resize(np.roll(codes, e), n)
        meas[e, :n, 0] = c
        meas[e, :n, 1] = rng.uniform(0, 1, n)
        meas[e, :n, 2] = rng.uniform(1, 100, n)
        n0 = rng.integers(0, N - 1, n)
        f = rng.uniform(0, 1, n)
        kind = rng.integers(0, 4, n)
        f[kind == 0], f[kind == 1] = 0.0, 1.0
        n0[kind == 1] = N - 2
        pos[e, :n, 0], pos[e, :n, 1] = n0, f
        y[e, (e + 1) % S, 3] = 0.0 if e % 3 == 0 else 1e-31          # at and below the clamp at an interior node
    return y, sens, stats, meas, pos


def rel_diff(a, b, floor=1e-300):
    """largest |a - b| / max(|b|, floor) (0 where both are equal, NaNs and infinities included)"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    with np.errstate(all="ignore"):
        rel = np.abs(a - b)/np.maximum(np.abs(b), floor)
    rel = np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0.0, rel)
    return float(np.max(rel)) if rel.size else 0.0


# ----------------------------------------------------------------------------- 1. the kernels alone
@pytest.mark.parametrize("E, P, MQ", [(1, 1, 64), (65, 3, 5), (130, 8, 7)])
def test_sibling_kernels_on_synthetic_buffers(E, P, MQ):
    mi = FR.wide_input()
    dev, mech, rows0 = open_unit(mi, FR.WIDE, [mi]*E, NP=1)
    S = mech.S
    try:
        rng = np.random.default_rng(E)
        rows0[:, 0] *= rng.uniform(0.5, 1.5, E)
        rows0[:, 1] *= rng.uniform(0.9, 1.1, E)
        at = plan.MEMBER_FIXED + S
        rows0[:, at:at + 8] = np.linspace(1.0, 2.0, 8)[None, :]
        y0, sens, stats0, meas0, pos = synthetic_ex(E, P, MQ, S, seed=E)
        columns = list(range(P))[::-1]                                  # not in row order
        start = rows0[0, at + np.array(columns)]
        # a box around the start on every other parameter, open elsewhere: the random steps are clamped
        lo = np.where(np.arange(P) % 2 == 0, 0.9*start, -np.inf)
        hi = np.where(np.arange(P) % 3 != 1, 1.1*start, np.inf)
        torch = dev.torch
        d_s = torch.from_numpy(sens).to(dev.device)
        worst = 0.0
        for flags in ([0]*P, [(j + 1) % 2 for j in range(P)]):           # all linear (bit for bit), then mixed
            exact = not any(flags)
            rows, y, stats, meas = rows0.copy(), y0.copy(), stats0.copy(), meas0.copy()
            dev.set_members(rows)
            bx = fit.box(lo, hi, flags)
            loop = LoopEx(dev, E, MQ, columns, meas, PASSES, pos, flags, bx)
            d_y = torch.from_numpy(y.reshape(E, -1)).to(dev.device)
            state, want_rows = np.zeros(fit.STATE), rows.copy()
            clamps = []
            for k in range(PASSES):
                if k == 1:
                    stats[E//2, 1] = 4.0                                # a member whose march failed: rejected
                if k == 2:
                    stats[E//2, 1] = -1.0
                    d_y.mul_(1.0 + 1e-3)
                    y = d_y.cpu().numpy().reshape(E, S + 1, N)
                if k >= 2:
                    # half the weights: a quarter of the cost, so the trial - with components on their bounds - is
                    # accepted and the next step starts from the box's faces (the active set)
                    meas[:, :, 2] *= 0.5
                    loop.meas.copy_(torch.from_numpy(meas))
                dev._stats.copy_(torch.from_numpy(stats))
                dev.fit_step(d_y, d_s, loop, k, extended=True)
                pred, contrib = fit.emulate_residuals_ex(y, sens, stats, want_rows, meas, S, pos, columns, flags)
                got_pred, got_contrib = loop.pred.cpu().numpy(), loop.contrib.cpu().numpy()
                assert np.array_equal(got_pred, pred, equal_nan=True), (k, np.argwhere(got_pred != pred)[:4])
                assert np.array_equal(got_contrib, contrib, equal_nan=True), (k, np.argwhere(got_contrib != contrib)[:4])
                log, got_state = loop.log[k].cpu().numpy(), loop.state.cpu().numpy()
                sums = fit.column_sums(contrib)
                assert np.array_equal(log[fit.LOG_G:fit.LOG_G + 8], sums[1:9], equal_nan=True)
                assert np.array_equal(log[fit.LOG_H:fit.LOG], sums[9:45], equal_nan=True)
                assert np.array_equal(log[[0, 6]], sums[[0, 45]], equal_nan=True)
                want = fit.emulate_update_ex(sums, state, P, start, loop.tolerance, loop.damping, flags, bx)
                if exact:
                    assert np.array_equal(log, want, equal_nan=True), (k, log[:16], want[:16])
                    assert np.array_equal(got_state, state, equal_nan=True)
                else:
                    soft = np.zeros(fit.LOG_EX, dtype=bool)
                    soft[fit.LOG_PTRIAL:fit.LOG_PTRIAL + 8] = True
                    assert np.array_equal(log[~soft], want[~soft], equal_nan=True), (k, log[:8], want[:8])
                    ssoft, dsoft = np.zeros(fit.STATE, dtype=bool), np.zeros(fit.STATE, dtype=bool)
                    ssoft[7] = True
                    ssoft[fit.ST_PTRIAL:fit.ST_PTRIAL + 8] = dsoft[fit.ST_DELTA:fit.ST_DELTA + 8] = True
                    assert np.array_equal(got_state[~(ssoft | dsoft)], state[~(ssoft | dsoft)], equal_nan=True), k
                    # (a clamped step in theta is hi - ln p_cur, a difference: its error is that of ln p = O(1), so the
                    # step is compared on the scale max(|step|, 1))
                    rel = max(rel_diff(log[soft], want[soft]), rel_diff(got_state[ssoft], state[ssoft]),
                              rel_diff(got_state[dsoft], state[dsoft], floor=1.0))
                    worst = max(worst, rel)
                    assert rel <= EXP_BOUND, (k, rel)
                    linear = [fit.LOG_PTRIAL + j for j in range(P) if not flags[j]]
                    assert np.array_equal(log[linear], want[linear])    # a linear parameter's trial: no exp, bit for bit
                    state[:] = got_state                                # (the emulation follows the device from here on)
                trial = log[fit.LOG_PTRIAL:fit.LOG_PTRIAL + P]
                assert np.all(trial >= lo) and np.all(trial <= hi)
                clamps.append(int(np.sum((trial == lo) | (trial == hi))))
                for j, c in enumerate(columns):
                    want_rows[:, at + c] = log[fit.LOG_PTRIAL + j]
                assert np.array_equal(dev.get_members(), want_rows, equal_nan=True), k
            print("E = %d, P = %d, MQ = %d, log flags %s: failed members per pass %s, accepted %s, lambda %s, status %s, "
                  "trial values on a bound %s, active lower/upper %s"
                  % (E, P, MQ, flags, loop.log[:, 6].cpu().numpy(), loop.log[:, 4].cpu().numpy(),
                     loop.log[:, 2].cpu().numpy(), loop.log[:, 7].cpu().numpy(), clamps,
                     loop.log[:, 68:].cpu().numpy().tolist()))
            # the box was hit: a trial on a bound, and an accepted point with a non-empty active set
            masks = loop.log[:, fit.LOG_LOWER:].cpu().numpy()
            assert max(clamps) >= 1 and np.any(masks != 0.0), (clamps, masks)
            loop.close()
        print("  largest |device - numpy| / |numpy| of trial, step and predicted reduction with log flags: %.3e (bound %.1e)"
              % (worst, EXP_BOUND))
    finally:
        dev.close()


# ----------------------------------------------------------------------------- 2. through rmtExe
_RUNS = {}


def run(name, plain=False, **cfg):
    key = (name, plain, tuple(sorted(cfg.items())))
    if key not in _RUNS:
        _RUNS[key] = rmtExe(FX.case_input(name, plain=plain, **cfg))["resModel"]
    return _RUNS[key]


def value_bound(name, gold, target):
    """[P]: 10 |p_ref_noise_free - p_true| of the underlying G22 case + FLOOR_REL |target|"""
    assert FLOOR_REL[name] <= 1e-6
    base = FX.CASES[name]["base"]
    miss = np.abs(np.asarray(gold["p_ref_noise_free"]) - FR.p_true(base))
    return 10*miss + FLOOR_REL[name]*np.abs(target)


def test_rmtexe_log_scaled_and_bounded_recovers_p_true_where_the_linear_law_does_not():
    """FL: FB's data at the feed rate of the golden (between 15 and 40 times the notebook's, where the linear law walks A3
    through zero: profiles/fit.md), all three constants log-scaled inside [start/10, 10 start]"""
    res, gold = run("FL"), FX.golden("FL")
    f = res["fit"]
    target = FR.p_true("FB")
    miss = np.abs(np.asarray(gold["p_ref"]) - target)
    assert FLOOR_REL["FL"] <= 1e-6
    err, bound = np.abs(f["values"] - target), 10*miss + FLOOR_REL["FL"]*target
    print("G24 FL on the device at %g times the notebook's feed rate: %d iterations (%d accepted, %d rejected), cost %.3e, "
          "|value - p_true| / p_true = %s (bound %s; the reference law's own %s in %d iterations)"
          % (float(gold["feed"]), f["iterations"], res["device-stats"]["accepted"], res["device-stats"]["rejected"],
             f["cost"], err/target, bound/target, miss/target, int(gold["iterations"])))
    assert f["converged"] is True and f["scale"] == ["log"]*3
    assert np.all(err <= bound), (err, bound)
    lo, hi = np.asarray(gold["lo"]), np.asarray(gold["hi"])
    for h in f["history"]:
        for key in ("parameters", "trial-parameters"):
            assert np.all(h[key] > 0) and np.all(h[key] >= lo) and np.all(h[key] <= hi), h
    assert list(f["active-bounds"]) == [0, 0, 0] and np.isfinite(f["covariance"]).all()
    # the same input without "scale" and "bounds": raises, or ends with A3 <= 0
    try:
        plain = run("FL", plain=True)["fit"]
    except RuntimeError as exc:
        print("  without 'scale' and 'bounds': %s" % exc)
    else:
        print("  without 'scale' and 'bounds': 'converged' at %s" % plain["values"])
        assert plain["values"][2] <= 0


def test_rmtexe_ends_on_the_bound():
    res, gold = run("FC"), FX.golden("FC")
    f = res["fit"]
    p_ref, hi = np.array(gold["p_ref"]), float(gold["hi"][1])
    err, bound = np.abs(f["values"] - p_ref), value_bound("FC", gold, p_ref)
    print("G24 FC on the device: %d iterations (%d accepted, %d rejected), cost %.9e against %.9e, A3 = %r (bound %r), "
          "|A1 - p_ref| / p_ref = %.3e (bound %.3e), active %s, standard errors %s"
          % (f["iterations"], res["device-stats"]["accepted"], res["device-stats"]["rejected"], f["cost"],
             float(gold["cost"]), f["values"][1], hi, err[0]/p_ref[0], bound[0]/p_ref[0], f["active-bounds"],
             f["standard-error"]))
    assert f["converged"] is True and f["values"][1] == hi
    assert list(f["active-bounds"]) == [0, 1] == list(gold["active"])
    assert err[0] <= bound[0], (err, bound)
    assert f["scale"] == ["linear", "linear"] and np.array_equal(f["bounds"], [[-np.inf, np.inf], [-np.inf, hi]])
    cov, se, corr = f["covariance"], f["standard-error"], f["correlation"]
    assert np.isnan(cov[1]).all() and np.isnan(cov[:, 1]).all() and np.isnan(se[1]) and np.isnan(corr[0, 1])
    assert np.isfinite(cov[0, 0]) and se[0] > 0 and corr[0, 0] == 1.0
    assert abs(f["cost"] - float(gold["cost"])) <= 1e-6*float(gold["cost"])
    for h in f["history"]:
        assert h["trial-parameters"][1] <= hi and h["parameters"][1] <= hi


def test_rmtexe_with_data_along_the_bed_against_the_reference():
    res, gold = run("FP"), FX.golden("FP")
    f = res["fit"]
    p_ref = np.array(gold["p_ref"])
    err, bound = np.abs(f["values"] - p_ref), value_bound("FP", gold, p_ref)
    cov, want = f["covariance"], np.array(gold["covariance"])
    scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
    crel = np.abs(cov - want)/scale
    print("G24 FP on the device: %d iterations, |value - p_ref| / p_ref = %s (bound %s), cost %.9e against %.9e (%.2e), "
          "|covariance - reference| / sqrt(C_ii C_jj) at most %.3e (bound %.1e), standard errors %s"
          % (f["iterations"], err/p_ref, bound/p_ref, f["cost"], float(gold["cost"]), abs(f["cost"]/float(gold["cost"]) - 1),
             crel.max(), COV_BOUND, f["standard-error"]))
    assert f["converged"] is True and list(f["active-bounds"]) == [0, 0]
    assert np.all(err <= bound), (err, bound)
    assert abs(f["cost"] - float(gold["cost"])) <= 1e-6*float(gold["cost"])
    assert COV_BOUND <= 1e-3 and np.all(crel <= COV_BOUND), crel
    assert f["experiments"] == [len(FX.ext_labels("FP", e)) for e in range(8)]
    for e, member in enumerate(res["ensemble"]):
        entry = member["fit"]
        assert entry["labels"] == FX.ext_labels("FP", e)
        assert np.array_equal(entry["residual"], (entry["predicted"] - entry["measured"])*(1.0/FX.ext_sigmas("FP", e)))
        # the prediction at position 1 is the outlet temperature's, at position 0 the inlet node's
        lb = entry["labels"]
        assert entry["predicted"][lb.index("temperature-profile:1")] == entry["predicted"][lb.index("outlet-temperature")]
        T = member["dataPack"][0]["dataYTemp1"]
        tf = (entry["predicted"][lb.index("outlet-temperature")])/(T[-1] + 1.0)
        assert entry["predicted"][lb.index("temperature-profile:0")] == pytest.approx(T[0]*tf + tf, rel=1e-14)


def test_keys_absent_or_without_effect_change_nothing():
    """the same input without the new keys is the run of tests/test_gpu_fit.py; with bounds nothing ever touches, the
    sibling kernels run the whole fit - and end bit for bit where the plain ones do"""
    want = run_g22("FA")["fit"]
    again = rmtExe(FR.case_input("FA"))["resModel"]["fit"]
    mi = FR.case_input("FA")
    for p in mi["solver-config"]["fit"]["parameters"]:
        p.update({"scale": "linear", "bounds": [-1e300, 1e300]})
    assert fit.parse(mi).extended
    boxed = rmtExe(mi)["resModel"]["fit"]
    for got in (again, boxed):
        assert got["iterations"] == want["iterations"] and got["cost"] == want["cost"]
        assert np.array_equal(got["values"], want["values"]) and np.array_equal(got["hessian"], want["hessian"])
        assert np.array_equal(got["covariance"], want["covariance"])
        for x, y in zip(got["history"], want["history"]):
            assert x.keys() == y.keys()
            for k in x:
                assert np.array_equal(x[k], y[k]), k
        assert list(got["active-bounds"]) == [0, 0] and got["scale"] == ["linear", "linear"]
    print("FA without the new keys and with bounds of +-1e300: %d iterations, values %s - identical"
          % (want["iterations"], want["values"]))
