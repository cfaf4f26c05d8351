"""What the axial-profile tests share (tests/test_profile_cpu.py, tests/test_gpu_profile.py): the reference right-hand
side of a profiled bed on the unchanged oracle, the node rule restated, the goldens G18 and the test tables.

The two helpers are those of tools/make_golden.py (target ``profile``):

* activity: every entry of pr["RATES"] wrapped in a closure that multiplies it by the node array a [N]
  (vectorised_kinetics rebinds the user lambda through the closure cell and broadcasts a over the nodes);
* coolant: pr["Tm"] must stay a scalar (make_local_rhs tests pr["Tm"] == 0) and the right-hand side is affine in Tm, so
  f(Tm(z)) = f0 + (f1 - f0) delta(z) on the temperature row, f0 / f1 evaluated at MeTe and MeTe + 1.

Against rhs_loop node by node with scalar a_z and Tm(z_n) the combination agrees to 2.1e-15 relative (DME, 20 nodes).
"""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLD, "g18_profile.json")) as _f:
    G18 = json.load(_f)
CASES = G18["cases"]
BED_A = CASES["A"]["axial-profile"]


def golden(name):
    return np.load(os.path.join(GOLD, "g18_profile_%s.npz" % name))


def nodes(position, values, N):
    """the piecewise-linear function at z_n = n/(N-1): right-continuous at a jump, the last value at z = 1 (restated,
    not imported from the product)"""
    p, v = np.asarray(position, dtype=float), np.asarray(values, dtype=float)
    out = np.zeros(N)
    for n in range(N):
        z = n/float(N - 1)
        k = int(np.searchsorted(p, z, side="right")) - 1
        out[n] = v[-1] if k >= len(p) - 1 else v[k] + (v[k + 1] - v[k])*(z - p[k])/(p[k + 1] - p[k])
    return out


def bed(spec, N, MeTe):
    """(activities [N], coolant offsets [N]) of an "axial-profile" spec for a member with that MeTe"""
    a = nodes(spec["position"], spec["catalyst-activity"], N) if "catalyst-activity" in spec else np.ones(N)
    d = nodes(spec["position"], spec["medium-temperature"], N) - MeTe if "medium-temperature" in spec else np.zeros(N)
    return a, d


def profiled_pr(pr, a):
    def wrap(f, a):
        return lambda x: a*f(x)
    out = dict(pr)
    out["RATES"] = {k: wrap(f, a) for k, f in pr["RATES"].items()}
    return out


def profiled_rhs(O, pr, a, delta):
    """f(t, y) of the profiled bed on the oracle's vectorised right-hand side"""
    p0 = profiled_pr(pr, np.asarray(a, dtype=float))
    p1 = dict(p0)
    p1["Tm"] = p0["Tm"] + 1.0
    f0, f1 = O.make_rhs_vec(p0), O.make_rhs_vec(p1)
    S, N, V = pr["compNo"], pr["zNo"], pr["varNo"]
    delta = np.asarray(delta, dtype=float)
    if pr["iso"] or pr["Tm"] == 0 or not np.any(delta != 0):
        return f0

    def f(t, y):
        r0 = np.array(f0(t, y), dtype=float)
        r1 = np.asarray(f1(t, y), dtype=float)
        R0, R1 = r0.reshape((-1, V, N)), r1.reshape((-1, V, N))
        R0[:, S, :] += (R1[:, S, :] - R0[:, S, :])*delta
        return r0
    return f


def make_tables(N, E=3, seed=18):
    """E different tables [E][2][N]: table 0 has a zero-activity zone in front, a jump and both signs of the coolant
    offset; the others are smooth and differ from it and from each other at every node."""
    z = np.arange(N)/float(N - 1)
    rng = np.random.default_rng(seed + N)
    T = np.zeros((E, 2, N))
    T[0, 0] = np.where(z < 0.25, 0.0, np.where(z < 0.6, 0.5, 1.0))
    T[0, 1] = np.where(z < 0.5, 10.0, -10.0)
    for e in range(1, E):
        T[e, 0] = 0.3 + 0.2*e + 0.5*z + 0.05*rng.uniform(size=N)
        T[e, 1] = (-1)**e*(4.0*e + 6.0*z)
    return T
