"""Shared by tests/test_ekf_reference_host.py and test_ekf_reference_gpu.py: the fixture tests/golden/ekf_reference.npz (60 digits:
tests/golden/make_golden_ekf.py), the error measure, the gates, and the restatement's own run over the fixture.

Gate rule (as tests/ocpnlp_gates.py): tests/ekf_ref.py is a plain float64 numpy restatement that shares nothing with the oracle or
the headers; its worst error against the 60-digit values, per bucket, is what float64 delivers on these inputs, and the gate of a
bucket is MARGIN = 4 times that.  Error of one filter: max |got - ref| / max |ref| over the array; of a bucket: the worst over its
filters.  Buckets are (class, dof[, ny], level), written "class/dof/level" and "class/dofxny/level"; classes: euler, rk4, rk4_tv
(by dof), update_P, update_delta, fused_P, fused_delta, ticks_P, ticks_delta (by pair; the issue's class "ticks" is the third
tick's P and delta, gated apart because their scales differ).  Levels: cond(P) = 1e1 (c1), 1e6 (c6), 1e10 (c10).

MEASURED is the restatement's run on the CPU this was written on (test_ekf_reference_host.py::
test_gate_is_four_times_the_float64_restatements_error prints it and checks that the restatement still delivers it); neither the
oracle nor a kernel is its source.  RAISED holds the buckets in which the oracle, with every convention agreeing (it passes all
others, and the negative controls miss by 1e6 and more), came out over four times the restatement's error on the CPU: a bucket of a
few draws catches the restatement on a good day.  The issue allows up to 16 there; the measured oracle / restatement ratio stands
next to each.

REF_ROUNDING: the fixture holds the 60-digit results rounded to float64, so the stored reference is itself off by up to 2^-53 of
its largest entry, and an error is only resolved in steps of that size.  Where the restatement happens to land on the stored
roundings (0 or a fraction of 2^-53 in some predict buckets of a few small matrices) the gate is taken from 2^-53 instead: four
roundings of the reference, below which no float64 result can be told from a correct one."""
import os

import numpy as np

import ekf_ref as ER

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ekf_reference.npz")
MARGIN = 4.0
MAX_MARGIN = 16.0
REF_ROUNDING = 2.0 ** -53
FX = np.load(FIXTURE)
PAIRS = [(int(n), int(m)) for n, m in FX["pairs"]]
DOFS = [int(n) for n in FX["dofs"]]
PREDICT_DOFS = [int(n) for n in FX["predict_dofs"]]
DRAWS = {n: int(d) for n, d in zip(DOFS, FX["draws"])}
LEVELS = [str(s) for s in FX["level.names"]]
CHAIN = [str(s) for s in FX["chain.levels"]]
PREDICT_CLASSES = ("euler", "rk4", "rk4_tv")
PAIR_CLASSES = ("update_P", "update_delta", "fused_P", "fused_delta")
TICK_CLASSES = ("ticks_P", "ticks_delta")
META = ("pairs", "dofs", "predict_dofs", "draws", "level.names", "level.cond", "chain.levels")


def levels(n):
    return [L for L in LEVELS if not (n > 10 and L == "c6")]


def chain_levels(n):
    return [L for L in levels(n) if L in CHAIN]


def unpack(U, n):
    """(D, n(n+1)/2) packed upper triangles, column by column -> (D, n*n) symmetric, column-major flat"""
    out = np.zeros((U.shape[0], n, n))
    k = 0
    for j in range(n):
        for i in range(j + 1):
            out[:, i, j] = out[:, j, i] = U[:, k]
            k += 1
    return out.reshape(U.shape[0], n * n)


def _walk():
    """slice the flat arrays in the order the generator wrote them; every array must be used up"""
    pos = {}
    blocks = {}

    def take(key, D, w):
        a = pos.get(key, 0)
        pos[key] = a + D * w
        return FX[key][a:a + D * w].reshape(D, w)

    for n in DOFS:
        for L in levels(n):
            D = DRAWS[n]
            b = {"P": take("state.P", D, n * n), "A": take("state.A", D, n * n), "Q": take("state.Q", D, n * n), "dt": take("state.dt", D, 1)[:, 0]}
            b["Qc"] = b["Q"] * take("state.qchain", D, 1)                                  # the chain's Q: a power of two times Q, exact
            if n in PREDICT_DOFS:
                for k in ("Am", "Ae") + PREDICT_CLASSES:
                    b[k] = take("predict." + k, D, n * n)
            blocks[n, L] = b
    for n, m in PAIRS:
        t = n * (n + 1) // 2
        for L in levels(n):
            D = DRAWS[n]
            b = {"H": take("update.H", D, m * n), "R": take("update.R", D, m * m), "r": take("update.r", D, m),
                 "update_P": unpack(take("update.P", D, t), n), "update_delta": take("update.delta", D, n),
                 "fused_P": unpack(take("fused.P", D, t), n), "fused_delta": take("fused.delta", D, n)}
            if L in CHAIN:
                b["ticks_P"] = unpack(take("ticks.P", D, t), n)
                b["ticks_delta"] = take("ticks.delta", D, n)
            blocks[n, m, L] = b
    left = sorted(k for k in FX.files if k not in META and pos.get(k, 0) != FX[k].size)
    assert not left, left
    return blocks, set(pos) | set(META)


BLOCKS, VISITED = _walk()


def state(n, L):
    """the draws of one dof at one level: P, A, Q, Qc (the chain's Q) (D, n*n) column-major flat, dt (D,); for PREDICT_DOFS also Am, Ae, euler, rk4, rk4_tv"""
    return BLOCKS[n, L]


def pair(n, m, L):
    """one pair at one level: H (D, m*n), R (D, m*m), r (D, m) and the results, P as (D, n*n) column-major flat"""
    return BLOCKS[n, m, L]


def key(cls, n, m, L):
    return "%s/%d/%s" % (cls, n, L) if m is None else "%s/%dx%d/%s" % (cls, n, m, L)


def errors(got, ref):
    """per filter: max |got - ref| / max |ref|"""
    got = np.asarray(got, dtype=np.float64).reshape(len(ref), -1)
    ref = np.asarray(ref, dtype=np.float64).reshape(len(ref), -1)
    return np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)


def bucket_error(got, ref):
    return float(errors(got, ref).max())


def margin(k):
    return RAISED.get(k, (MARGIN,))[0]


def gate(k):
    return margin(k) * max(MEASURED[k], REF_ROUNDING)


def check(k, got, ref, who):
    """a bucket (draws tiled over any number of filters) within its gate; the figure is printed first"""
    err = bucket_error(got, ref)
    print("%-26s %-18s %.2e (gate %.2e, ratio %.2f)" % (k, who, err, gate(k), err / gate(k)))
    assert err <= gate(k), "%s (%s): %.3e over the gate %.3e" % (k, who, err, gate(k))
    return err / gate(k)


def mat(flat, rows, cols):
    return np.asarray(flat).reshape(cols, rows).T


def unmat(X):
    return np.ascontiguousarray(X.T).ravel()


def restatement_rows(**wrong):
    """[(bucket key, got, ref)] of tests/ekf_ref.py on every result of the fixture; `wrong`: a negative control of ER.update"""
    rows = []
    for n in PREDICT_DOFS:
        for L in levels(n):
            s = state(n, L)
            D = DRAWS[n]
            P, A, Q, Am, Ae = ([mat(s[k][d], n, n) for d in range(D)] for k in ("P", "A", "Q", "Am", "Ae"))
            rows.append((key("euler", n, None, L), [unmat(ER.euler(P[d], A[d], Q[d], s["dt"][d])) for d in range(D)], s["euler"]))
            rows.append((key("rk4", n, None, L), [unmat(ER.rk4(P[d], A[d], Q[d], s["dt"][d])) for d in range(D)], s["rk4"]))
            rows.append((key("rk4_tv", n, None, L), [unmat(ER.rk4(P[d], A[d], Q[d], s["dt"][d], Am[d], Ae[d])) for d in range(D)], s["rk4_tv"]))
    for n, m in PAIRS:
        for L in levels(n):
            s, p = state(n, L), pair(n, m, L)
            got = {c: [] for c in PAIR_CLASSES + TICK_CLASSES}
            for d in range(DRAWS[n]):
                P, A, Q, dt = mat(s["P"][d], n, n), mat(s["A"][d], n, n), mat(s["Q"][d], n, n), s["dt"][d]
                H, R, r = mat(p["H"][d], m, n), mat(p["R"][d], m, m), p["r"][d]
                Pu, du = ER.update(P, H, R, r, **wrong)
                got["update_P"].append(unmat(Pu)); got["update_delta"].append(du)
                if not wrong:
                    Pf, df = ER.fused(P, A, Q, dt, H, R, r)
                    got["fused_P"].append(unmat(Pf)); got["fused_delta"].append(df)
                    if L in CHAIN:
                        Pt, dk = ER.ticks(P, A, mat(s["Qc"][d], n, n), dt, H, R, r)
                        got["ticks_P"].append(unmat(Pt)); got["ticks_delta"].append(dk)
            rows += [(key(c, n, m, L), np.array(v), p[c]) for c, v in got.items() if v]
    return rows


def measure():
    """{bucket: worst error of the restatement}"""
    return {k: bucket_error(got, ref) for k, got, ref in restatement_rows()}


def all_keys():
    ks = [key(c, n, None, L) for n in PREDICT_DOFS for L in levels(n) for c in PREDICT_CLASSES]
    ks += [key(c, n, m, L) for n, m in PAIRS for L in levels(n) for c in PAIR_CLASSES]
    ks += [key(c, n, m, L) for n, m in PAIRS for L in chain_levels(n) for c in TICK_CLASSES]
    return ks


# bucket: (margin, oracle / restatement ratio measured on the CPU)
RAISED = {
    "ticks_P/9x4/c6": (8.0, 5.86), "ticks_delta/5x5/c6": (8.0, 4.51), "update_delta/4x1/c6": (8.0, 4.05),
}

MEASURED = {
    "euler/1/c1": 0.00e+00, "rk4/1/c1": 0.00e+00, "rk4_tv/1/c1": 0.00e+00, "euler/1/c6": 0.00e+00,
    "rk4/1/c6": 0.00e+00, "rk4_tv/1/c6": 0.00e+00, "euler/1/c10": 0.00e+00, "rk4/1/c10": 1.17e-16,
    "rk4_tv/1/c10": 2.01e-16, "euler/2/c1": 1.94e-16, "rk4/2/c1": 1.40e-17, "rk4_tv/2/c1": 0.00e+00,
    "euler/2/c6": 1.90e-16, "rk4/2/c6": 3.89e-18, "rk4_tv/2/c6": 1.54e-17, "euler/2/c10": 6.44e-17,
    "rk4/2/c10": 1.47e-16, "rk4_tv/2/c10": 0.00e+00, "euler/3/c1": 6.94e-18, "rk4/3/c1": 1.49e-16,
    "rk4_tv/3/c1": 6.88e-17, "euler/3/c6": 7.62e-18, "rk4/3/c6": 1.70e-17, "rk4_tv/3/c6": 4.05e-17,
    "euler/3/c10": 1.05e-16, "rk4/3/c10": 2.10e-16, "rk4_tv/3/c10": 1.64e-16, "euler/4/c1": 3.79e-17,
    "rk4/4/c1": 1.34e-16, "rk4_tv/4/c1": 1.18e-16, "euler/4/c6": 1.21e-16, "rk4/4/c6": 1.20e-16,
    "rk4_tv/4/c6": 1.23e-16, "euler/4/c10": 5.96e-17, "rk4/4/c10": 5.55e-17, "rk4_tv/4/c10": 1.11e-16,
    "euler/6/c1": 1.86e-16, "rk4/6/c1": 8.96e-17, "rk4_tv/6/c1": 1.76e-16, "euler/6/c6": 1.79e-16,
    "rk4/6/c6": 1.79e-16, "rk4_tv/6/c6": 1.29e-16, "euler/6/c10": 4.66e-17, "rk4/6/c10": 1.18e-16,
    "rk4_tv/6/c10": 7.74e-17, "euler/7/c1": 9.02e-17, "rk4/7/c1": 2.04e-16, "rk4_tv/7/c1": 4.55e-17,
    "euler/7/c6": 5.48e-17, "rk4/7/c6": 9.87e-17, "rk4_tv/7/c6": 6.04e-17, "euler/7/c10": 7.26e-17,
    "rk4/7/c10": 9.66e-17, "rk4_tv/7/c10": 3.98e-17, "euler/8/c1": 8.75e-17, "rk4/8/c1": 1.75e-16,
    "rk4_tv/8/c1": 4.36e-17, "euler/8/c6": 7.34e-17, "rk4/8/c6": 7.29e-17, "rk4_tv/8/c6": 6.62e-17,
    "euler/8/c10": 5.79e-17, "rk4/8/c10": 5.79e-17, "rk4_tv/8/c10": 1.53e-17, "euler/9/c1": 4.98e-17,
    "rk4/9/c1": 4.94e-17, "rk4_tv/9/c1": 1.71e-16, "euler/9/c6": 8.97e-17, "rk4/9/c6": 1.57e-16,
    "rk4_tv/9/c6": 9.99e-17, "euler/9/c10": 9.54e-18, "rk4/9/c10": 3.82e-17, "rk4_tv/9/c10": 7.90e-17,
    "euler/11/c1": 9.15e-17, "rk4/11/c1": 1.82e-16, "rk4_tv/11/c1": 7.98e-17, "euler/11/c10": 4.42e-17,
    "rk4/11/c10": 1.77e-16, "rk4_tv/11/c10": 9.21e-17, "euler/16/c1": 2.21e-16, "rk4/16/c1": 2.15e-16,
    "rk4_tv/16/c1": 4.67e-17, "euler/16/c10": 7.03e-17, "rk4/16/c10": 1.25e-16, "rk4_tv/16/c10": 1.45e-16,
    "update_P/2x1/c1": 1.97e-16, "update_delta/2x1/c1": 1.84e-16, "fused_P/2x1/c1": 1.86e-16, "fused_delta/2x1/c1": 1.75e-16,
    "update_P/2x1/c6": 1.12e-10, "update_delta/2x1/c6": 4.60e-16, "fused_P/2x1/c6": 4.45e-11, "fused_delta/2x1/c6": 4.61e-16,
    "update_P/2x1/c10": 8.59e-07, "update_delta/2x1/c10": 2.29e-16, "fused_P/2x1/c10": 1.57e-12, "fused_delta/2x1/c10": 4.60e-15,
    "update_P/2x2/c1": 1.17e-15, "update_delta/2x2/c1": 2.98e-16, "fused_P/2x2/c1": 1.02e-15, "fused_delta/2x2/c1": 6.43e-16,
    "update_P/2x2/c6": 1.21e-10, "update_delta/2x2/c6": 1.35e-11, "fused_P/2x2/c6": 8.67e-11, "fused_delta/2x2/c6": 8.52e-12,
    "update_P/2x2/c10": 1.11e-06, "update_delta/2x2/c10": 5.35e-07, "fused_P/2x2/c10": 4.62e-07, "fused_delta/2x2/c10": 5.34e-09,
    "update_P/2x3/c1": 7.51e-16, "update_delta/2x3/c1": 9.58e-16, "fused_P/2x3/c1": 9.69e-16, "fused_delta/2x3/c1": 2.11e-15,
    "update_P/2x3/c6": 1.31e-10, "update_delta/2x3/c6": 4.03e-11, "fused_P/2x3/c6": 1.19e-10, "fused_delta/2x3/c6": 3.05e-11,
    "update_P/2x3/c10": 8.03e-07, "update_delta/2x3/c10": 1.14e-06, "fused_P/2x3/c10": 7.97e-07, "fused_delta/2x3/c10": 1.23e-06,
    "update_P/3x1/c1": 5.37e-16, "update_delta/3x1/c1": 2.21e-16, "fused_P/3x1/c1": 3.67e-16, "fused_delta/3x1/c1": 3.74e-16,
    "update_P/3x1/c6": 1.24e-13, "update_delta/3x1/c6": 4.37e-16, "fused_P/3x1/c6": 9.86e-14, "fused_delta/3x1/c6": 1.34e-15,
    "update_P/3x1/c10": 5.20e-11, "update_delta/3x1/c10": 2.91e-16, "fused_P/3x1/c10": 4.32e-13, "fused_delta/3x1/c10": 1.66e-16,
    "update_P/3x2/c1": 1.72e-15, "update_delta/3x2/c1": 2.60e-16, "fused_P/3x2/c1": 1.11e-15, "fused_delta/3x2/c1": 4.42e-16,
    "update_P/3x2/c6": 5.65e-11, "update_delta/3x2/c6": 3.30e-12, "fused_P/3x2/c6": 2.35e-11, "fused_delta/3x2/c6": 2.76e-11,
    "update_P/3x2/c10": 3.82e-07, "update_delta/3x2/c10": 4.20e-11, "fused_P/3x2/c10": 1.16e-09, "fused_delta/3x2/c10": 5.79e-14,
    "update_P/3x3/c1": 1.52e-15, "update_delta/3x3/c1": 1.58e-15, "fused_P/3x3/c1": 1.08e-15, "fused_delta/3x3/c1": 8.43e-16,
    "update_P/3x3/c6": 5.25e-11, "update_delta/3x3/c6": 3.94e-10, "fused_P/3x3/c6": 2.82e-10, "fused_delta/3x3/c6": 2.55e-10,
    "update_P/3x3/c10": 1.06e-06, "update_delta/3x3/c10": 9.10e-07, "fused_P/3x3/c10": 6.62e-07, "fused_delta/3x3/c10": 4.95e-09,
    "update_P/4x1/c1": 3.65e-16, "update_delta/4x1/c1": 1.80e-16, "fused_P/4x1/c1": 1.63e-16, "fused_delta/4x1/c1": 2.22e-16,
    "update_P/4x1/c6": 1.93e-13, "update_delta/4x1/c6": 1.13e-15, "fused_P/4x1/c6": 1.92e-13, "fused_delta/4x1/c6": 2.07e-14,
    "update_P/4x1/c10": 4.24e-13, "update_delta/4x1/c10": 4.93e-16, "fused_P/4x1/c10": 4.72e-13, "fused_delta/4x1/c10": 8.63e-16,
    "update_P/4x2/c1": 2.50e-16, "update_delta/4x2/c1": 3.97e-16, "fused_P/4x2/c1": 2.51e-16, "fused_delta/4x2/c1": 5.92e-16,
    "update_P/4x2/c6": 3.07e-12, "update_delta/4x2/c6": 2.61e-14, "fused_P/4x2/c6": 7.25e-13, "fused_delta/4x2/c6": 2.28e-14,
    "update_P/4x2/c10": 4.46e-10, "update_delta/4x2/c10": 8.30e-12, "fused_P/4x2/c10": 2.03e-12, "fused_delta/4x2/c10": 2.43e-13,
    "update_P/4x3/c1": 4.36e-16, "update_delta/4x3/c1": 5.90e-16, "fused_P/4x3/c1": 5.49e-16, "fused_delta/4x3/c1": 3.54e-16,
    "update_P/4x3/c6": 6.64e-11, "update_delta/4x3/c6": 9.21e-12, "fused_P/4x3/c6": 4.06e-12, "fused_delta/4x3/c6": 9.56e-12,
    "update_P/4x3/c10": 9.16e-07, "update_delta/4x3/c10": 5.83e-09, "fused_P/4x3/c10": 2.95e-09, "fused_delta/4x3/c10": 6.17e-12,
    "update_P/6x1/c1": 3.20e-16, "update_delta/6x1/c1": 3.58e-16, "fused_P/6x1/c1": 2.18e-16, "fused_delta/6x1/c1": 1.88e-16,
    "update_P/6x1/c6": 3.19e-15, "update_delta/6x1/c6": 7.03e-16, "fused_P/6x1/c6": 4.29e-15, "fused_delta/6x1/c6": 5.72e-16,
    "update_P/6x1/c10": 1.65e-14, "update_delta/6x1/c10": 1.54e-16, "fused_P/6x1/c10": 1.92e-14, "fused_delta/6x1/c10": 4.81e-16,
    "update_P/6x2/c1": 3.13e-16, "update_delta/6x2/c1": 4.79e-16, "fused_P/6x2/c1": 3.96e-16, "fused_delta/6x2/c1": 4.35e-16,
    "update_P/6x2/c6": 2.54e-14, "update_delta/6x2/c6": 6.69e-15, "fused_P/6x2/c6": 1.78e-13, "fused_delta/6x2/c6": 3.71e-14,
    "update_P/6x2/c10": 3.61e-12, "update_delta/6x2/c10": 1.33e-13, "fused_P/6x2/c10": 6.36e-13, "fused_delta/6x2/c10": 2.26e-14,
    "update_P/6x3/c1": 2.78e-16, "update_delta/6x3/c1": 5.15e-16, "fused_P/6x3/c1": 2.51e-16, "fused_delta/6x3/c1": 6.30e-16,
    "update_P/6x3/c6": 2.43e-13, "update_delta/6x3/c6": 1.84e-13, "fused_P/6x3/c6": 1.64e-13, "fused_delta/6x3/c6": 1.37e-13,
    "update_P/6x3/c10": 3.19e-10, "update_delta/6x3/c10": 5.89e-11, "fused_P/6x3/c10": 3.18e-11, "fused_delta/6x3/c10": 2.60e-12,
    "update_P/6x6/c1": 9.74e-16, "update_delta/6x6/c1": 7.54e-16, "fused_P/6x6/c1": 1.65e-15, "fused_delta/6x6/c1": 7.11e-16,
    "update_P/6x6/c6": 4.54e-11, "update_delta/6x6/c6": 1.05e-10, "fused_P/6x6/c6": 5.31e-11, "fused_delta/6x6/c6": 7.24e-11,
    "update_P/6x6/c10": 1.03e-06, "update_delta/6x6/c10": 3.68e-07, "fused_P/6x6/c10": 2.35e-06, "fused_delta/6x6/c10": 1.77e-07,
    "update_P/4x4/c1": 1.44e-15, "update_delta/4x4/c1": 5.82e-16, "fused_P/4x4/c1": 5.26e-16, "fused_delta/4x4/c1": 9.52e-16,
    "update_P/4x4/c6": 2.61e-10, "update_delta/4x4/c6": 5.77e-11, "fused_P/4x4/c6": 6.69e-11, "fused_delta/4x4/c6": 5.55e-11,
    "update_P/4x4/c10": 1.69e-07, "update_delta/4x4/c10": 7.06e-07, "fused_P/4x4/c10": 1.86e-07, "fused_delta/4x4/c10": 2.84e-08,
    "update_P/7x1/c1": 1.16e-16, "update_delta/7x1/c1": 2.52e-16, "fused_P/7x1/c1": 2.41e-16, "fused_delta/7x1/c1": 3.30e-16,
    "update_P/7x1/c6": 9.83e-16, "update_delta/7x1/c6": 2.51e-16, "fused_P/7x1/c6": 7.74e-16, "fused_delta/7x1/c6": 1.82e-16,
    "update_P/7x1/c10": 6.12e-15, "update_delta/7x1/c10": 3.90e-16, "fused_P/7x1/c10": 1.04e-14, "fused_delta/7x1/c10": 1.19e-15,
    "update_P/7x2/c1": 2.05e-16, "update_delta/7x2/c1": 2.35e-16, "fused_P/7x2/c1": 2.61e-16, "fused_delta/7x2/c1": 3.62e-16,
    "update_P/7x2/c6": 1.26e-14, "update_delta/7x2/c6": 6.52e-16, "fused_P/7x2/c6": 1.59e-14, "fused_delta/7x2/c6": 1.49e-15,
    "update_P/7x2/c10": 8.27e-12, "update_delta/7x2/c10": 1.79e-13, "fused_P/7x2/c10": 1.37e-13, "fused_delta/7x2/c10": 5.47e-14,
    "update_P/7x3/c1": 3.27e-16, "update_delta/7x3/c1": 4.03e-16, "fused_P/7x3/c1": 2.62e-16, "fused_delta/7x3/c1": 3.81e-16,
    "update_P/7x3/c6": 5.36e-14, "update_delta/7x3/c6": 9.56e-14, "fused_P/7x3/c6": 6.16e-12, "fused_delta/7x3/c6": 6.18e-12,
    "update_P/7x3/c10": 4.53e-11, "update_delta/7x3/c10": 1.31e-12, "fused_P/7x3/c10": 1.40e-12, "fused_delta/7x3/c10": 1.78e-13,
    "update_P/8x1/c1": 9.12e-17, "update_delta/8x1/c1": 2.44e-16, "fused_P/8x1/c1": 9.30e-17, "fused_delta/8x1/c1": 1.16e-16,
    "update_P/8x1/c6": 2.19e-16, "update_delta/8x1/c6": 3.20e-16, "fused_P/8x1/c6": 2.40e-16, "fused_delta/8x1/c6": 2.04e-16,
    "update_P/8x1/c10": 4.01e-15, "update_delta/8x1/c10": 6.73e-16, "fused_P/8x1/c10": 5.15e-15, "fused_delta/8x1/c10": 7.76e-16,
    "update_P/8x2/c1": 2.88e-16, "update_delta/8x2/c1": 1.28e-16, "fused_P/8x2/c1": 3.68e-16, "fused_delta/8x2/c1": 1.68e-16,
    "update_P/8x2/c6": 3.24e-14, "update_delta/8x2/c6": 1.40e-15, "fused_P/8x2/c6": 5.20e-14, "fused_delta/8x2/c6": 1.02e-15,
    "update_P/8x2/c10": 9.52e-12, "update_delta/8x2/c10": 8.48e-14, "fused_P/8x2/c10": 8.98e-13, "fused_delta/8x2/c10": 4.19e-14,
    "update_P/8x3/c1": 2.21e-16, "update_delta/8x3/c1": 1.71e-16, "fused_P/8x3/c1": 2.17e-16, "fused_delta/8x3/c1": 1.68e-16,
    "update_P/8x3/c6": 1.13e-14, "update_delta/8x3/c6": 2.10e-14, "fused_P/8x3/c6": 4.53e-14, "fused_delta/8x3/c6": 1.62e-14,
    "update_P/8x3/c10": 1.76e-12, "update_delta/8x3/c10": 1.17e-13, "fused_P/8x3/c10": 5.28e-13, "fused_delta/8x3/c10": 3.32e-14,
    "update_P/9x1/c1": 2.47e-16, "update_delta/9x1/c1": 2.18e-16, "fused_P/9x1/c1": 2.44e-16, "fused_delta/9x1/c1": 2.20e-16,
    "update_P/9x1/c6": 9.62e-16, "update_delta/9x1/c6": 3.78e-16, "fused_P/9x1/c6": 8.17e-16, "fused_delta/9x1/c6": 7.78e-16,
    "update_P/9x1/c10": 6.67e-15, "update_delta/9x1/c10": 2.84e-16, "fused_P/9x1/c10": 3.48e-15, "fused_delta/9x1/c10": 1.42e-16,
    "update_P/9x2/c1": 1.41e-16, "update_delta/9x2/c1": 2.13e-16, "fused_P/9x2/c1": 1.25e-16, "fused_delta/9x2/c1": 1.59e-16,
    "update_P/9x2/c6": 4.26e-15, "update_delta/9x2/c6": 1.28e-15, "fused_P/9x2/c6": 2.71e-15, "fused_delta/9x2/c6": 9.84e-16,
    "update_P/9x2/c10": 1.93e-13, "update_delta/9x2/c10": 1.83e-15, "fused_P/9x2/c10": 1.47e-13, "fused_delta/9x2/c10": 2.31e-15,
    "update_P/9x3/c1": 4.15e-16, "update_delta/9x3/c1": 5.56e-16, "fused_P/9x3/c1": 3.28e-16, "fused_delta/9x3/c1": 9.84e-16,
    "update_P/9x3/c6": 1.41e-14, "update_delta/9x3/c6": 1.81e-15, "fused_P/9x3/c6": 5.97e-15, "fused_delta/9x3/c6": 5.87e-15,
    "update_P/9x3/c10": 3.22e-12, "update_delta/9x3/c10": 7.08e-14, "fused_P/9x3/c10": 4.20e-13, "fused_delta/9x3/c10": 5.43e-14,
    "update_P/10x1/c1": 1.68e-16, "update_delta/10x1/c1": 2.30e-16, "fused_P/10x1/c1": 2.36e-16, "fused_delta/10x1/c1": 2.58e-16,
    "update_P/10x1/c6": 1.40e-15, "update_delta/10x1/c6": 4.83e-16, "fused_P/10x1/c6": 1.37e-15, "fused_delta/10x1/c6": 2.34e-16,
    "update_P/10x1/c10": 1.91e-15, "update_delta/10x1/c10": 6.50e-16, "fused_P/10x1/c10": 6.06e-15, "fused_delta/10x1/c10": 8.03e-15,
    "update_P/10x2/c1": 3.37e-16, "update_delta/10x2/c1": 3.54e-16, "fused_P/10x2/c1": 3.45e-16, "fused_delta/10x2/c1": 1.64e-16,
    "update_P/10x2/c6": 8.74e-16, "update_delta/10x2/c6": 2.00e-15, "fused_P/10x2/c6": 1.03e-15, "fused_delta/10x2/c6": 1.39e-15,
    "update_P/10x2/c10": 1.86e-14, "update_delta/10x2/c10": 4.29e-15, "fused_P/10x2/c10": 5.82e-15, "fused_delta/10x2/c10": 2.86e-15,
    "update_P/10x3/c1": 2.28e-16, "update_delta/10x3/c1": 4.07e-16, "fused_P/10x3/c1": 3.50e-16, "fused_delta/10x3/c1": 3.74e-16,
    "update_P/10x3/c6": 4.87e-15, "update_delta/10x3/c6": 8.56e-15, "fused_P/10x3/c6": 1.19e-14, "fused_delta/10x3/c6": 9.41e-15,
    "update_P/10x3/c10": 7.88e-13, "update_delta/10x3/c10": 1.29e-13, "fused_P/10x3/c10": 1.48e-14, "fused_delta/10x3/c10": 2.06e-14,
    "update_P/3x10/c1": 5.19e-15, "update_delta/3x10/c1": 4.80e-15, "fused_P/3x10/c1": 6.81e-15, "fused_delta/3x10/c1": 3.94e-15,
    "update_P/3x10/c6": 2.93e-10, "update_delta/3x10/c6": 2.95e-10, "fused_P/3x10/c6": 3.73e-10, "fused_delta/3x10/c6": 4.29e-10,
    "update_P/3x10/c10": 2.90e-06, "update_delta/3x10/c10": 9.64e-06, "fused_P/3x10/c10": 2.25e-06, "fused_delta/3x10/c10": 1.01e-05,
    "update_P/5x9/c1": 1.31e-15, "update_delta/5x9/c1": 1.83e-15, "fused_P/5x9/c1": 1.88e-15, "fused_delta/5x9/c1": 1.14e-15,
    "update_P/5x9/c6": 1.72e-10, "update_delta/5x9/c6": 1.43e-10, "fused_P/5x9/c6": 1.33e-10, "fused_delta/5x9/c6": 1.72e-10,
    "update_P/5x9/c10": 1.37e-06, "update_delta/5x9/c10": 1.36e-06, "fused_P/5x9/c10": 1.17e-06, "fused_delta/5x9/c10": 1.48e-06,
    "update_P/5x5/c1": 8.04e-16, "update_delta/5x5/c1": 4.92e-16, "fused_P/5x5/c1": 6.28e-16, "fused_delta/5x5/c1": 6.30e-16,
    "update_P/5x5/c6": 1.18e-10, "update_delta/5x5/c6": 5.39e-11, "fused_P/5x5/c6": 4.03e-11, "fused_delta/5x5/c6": 1.38e-11,
    "update_P/5x5/c10": 3.65e-07, "update_delta/5x5/c10": 2.10e-07, "fused_P/5x5/c10": 2.33e-07, "fused_delta/5x5/c10": 6.85e-08,
    "update_P/9x4/c1": 2.48e-16, "update_delta/9x4/c1": 1.86e-16, "fused_P/9x4/c1": 2.36e-16, "fused_delta/9x4/c1": 2.98e-16,
    "update_P/9x4/c6": 4.02e-14, "update_delta/9x4/c6": 2.88e-14, "fused_P/9x4/c6": 2.96e-14, "fused_delta/9x4/c6": 8.19e-15,
    "update_P/9x4/c10": 8.04e-12, "update_delta/9x4/c10": 3.39e-12, "fused_P/9x4/c10": 1.06e-12, "fused_delta/9x4/c10": 1.18e-12,
    "update_P/11x3/c1": 1.39e-16, "update_delta/11x3/c1": 3.01e-16, "fused_P/11x3/c1": 2.70e-16, "fused_delta/11x3/c1": 4.68e-16,
    "update_P/11x3/c10": 9.32e-14, "update_delta/11x3/c10": 9.02e-15, "fused_P/11x3/c10": 3.68e-13, "fused_delta/11x3/c10": 5.89e-14,
    "update_P/16x16/c1": 1.16e-15, "update_delta/16x16/c1": 4.38e-15, "fused_P/16x16/c1": 1.74e-15, "fused_delta/16x16/c1": 3.08e-15,
    "update_P/16x16/c10": 5.92e-07, "update_delta/16x16/c10": 1.46e-06, "fused_P/16x16/c10": 1.41e-06, "fused_delta/16x16/c10": 6.07e-07,
    "update_P/1x1/c1": 1.19e-16, "update_delta/1x1/c1": 1.57e-16, "fused_P/1x1/c1": 2.07e-16, "fused_delta/1x1/c1": 1.62e-16,
    "update_P/1x1/c6": 2.08e-16, "update_delta/1x1/c6": 1.74e-16, "fused_P/1x1/c6": 2.20e-16, "fused_delta/1x1/c6": 1.13e-16,
    "update_P/1x1/c10": 1.46e-16, "update_delta/1x1/c10": 1.96e-16, "fused_P/1x1/c10": 3.76e-16, "fused_delta/1x1/c10": 1.64e-16,
    "ticks_P/2x1/c1": 2.63e-16, "ticks_delta/2x1/c1": 4.34e-16, "ticks_P/2x1/c6": 1.52e-15, "ticks_delta/2x1/c6": 1.65e-15,
    "ticks_P/2x2/c1": 2.65e-16, "ticks_delta/2x2/c1": 5.24e-16, "ticks_P/2x2/c6": 1.98e-12, "ticks_delta/2x2/c6": 6.54e-14,
    "ticks_P/2x3/c1": 3.55e-16, "ticks_delta/2x3/c1": 6.64e-16, "ticks_P/2x3/c6": 1.07e-11, "ticks_delta/2x3/c6": 4.22e-12,
    "ticks_P/3x1/c1": 2.17e-16, "ticks_delta/3x1/c1": 6.17e-16, "ticks_P/3x1/c6": 2.25e-15, "ticks_delta/3x1/c6": 2.88e-16,
    "ticks_P/3x2/c1": 3.67e-16, "ticks_delta/3x2/c1": 8.00e-16, "ticks_P/3x2/c6": 1.14e-12, "ticks_delta/3x2/c6": 3.72e-13,
    "ticks_P/3x3/c1": 2.30e-16, "ticks_delta/3x3/c1": 4.94e-16, "ticks_P/3x3/c6": 4.28e-12, "ticks_delta/3x3/c6": 4.96e-15,
    "ticks_P/4x1/c1": 4.10e-16, "ticks_delta/4x1/c1": 7.61e-16, "ticks_P/4x1/c6": 7.79e-16, "ticks_delta/4x1/c6": 3.87e-15,
    "ticks_P/4x2/c1": 3.10e-16, "ticks_delta/4x2/c1": 5.77e-16, "ticks_P/4x2/c6": 3.94e-16, "ticks_delta/4x2/c6": 7.91e-16,
    "ticks_P/4x3/c1": 2.27e-16, "ticks_delta/4x3/c1": 4.68e-16, "ticks_P/4x3/c6": 2.89e-15, "ticks_delta/4x3/c6": 3.03e-15,
    "ticks_P/6x1/c1": 3.88e-16, "ticks_delta/6x1/c1": 3.64e-16, "ticks_P/6x1/c6": 3.06e-16, "ticks_delta/6x1/c6": 7.90e-16,
    "ticks_P/6x2/c1": 3.72e-16, "ticks_delta/6x2/c1": 6.31e-16, "ticks_P/6x2/c6": 2.40e-16, "ticks_delta/6x2/c6": 4.81e-16,
    "ticks_P/6x3/c1": 3.01e-16, "ticks_delta/6x3/c1": 4.81e-16, "ticks_P/6x3/c6": 2.92e-16, "ticks_delta/6x3/c6": 8.32e-16,
    "ticks_P/6x6/c1": 3.55e-16, "ticks_delta/6x6/c1": 1.10e-15, "ticks_P/6x6/c6": 3.98e-11, "ticks_delta/6x6/c6": 1.78e-12,
    "ticks_P/4x4/c1": 4.29e-16, "ticks_delta/4x4/c1": 4.68e-16, "ticks_P/4x4/c6": 5.40e-11, "ticks_delta/4x4/c6": 6.78e-13,
    "ticks_P/7x1/c1": 2.14e-16, "ticks_delta/7x1/c1": 5.29e-16, "ticks_P/7x1/c6": 2.57e-16, "ticks_delta/7x1/c6": 7.59e-16,
    "ticks_P/7x2/c1": 4.05e-16, "ticks_delta/7x2/c1": 3.91e-16, "ticks_P/7x2/c6": 3.11e-16, "ticks_delta/7x2/c6": 5.92e-16,
    "ticks_P/7x3/c1": 3.11e-16, "ticks_delta/7x3/c1": 5.03e-16, "ticks_P/7x3/c6": 6.35e-16, "ticks_delta/7x3/c6": 1.08e-15,
    "ticks_P/8x1/c1": 3.06e-16, "ticks_delta/8x1/c1": 4.24e-16, "ticks_P/8x1/c6": 4.06e-16, "ticks_delta/8x1/c6": 4.03e-16,
    "ticks_P/8x2/c1": 2.81e-16, "ticks_delta/8x2/c1": 8.04e-16, "ticks_P/8x2/c6": 6.84e-16, "ticks_delta/8x2/c6": 3.06e-15,
    "ticks_P/8x3/c1": 3.42e-16, "ticks_delta/8x3/c1": 4.19e-16, "ticks_P/8x3/c6": 1.94e-16, "ticks_delta/8x3/c6": 5.33e-16,
    "ticks_P/9x1/c1": 2.65e-16, "ticks_delta/9x1/c1": 5.49e-16, "ticks_P/9x1/c6": 4.06e-16, "ticks_delta/9x1/c6": 4.92e-16,
    "ticks_P/9x2/c1": 1.95e-16, "ticks_delta/9x2/c1": 5.54e-16, "ticks_P/9x2/c6": 5.26e-16, "ticks_delta/9x2/c6": 6.61e-16,
    "ticks_P/9x3/c1": 5.33e-16, "ticks_delta/9x3/c1": 1.26e-15, "ticks_P/9x3/c6": 1.27e-15, "ticks_delta/9x3/c6": 9.92e-16,
    "ticks_P/10x1/c1": 4.72e-16, "ticks_delta/10x1/c1": 4.33e-16, "ticks_P/10x1/c6": 3.25e-16, "ticks_delta/10x1/c6": 3.79e-16,
    "ticks_P/10x2/c1": 3.33e-16, "ticks_delta/10x2/c1": 4.13e-16, "ticks_P/10x2/c6": 3.37e-16, "ticks_delta/10x2/c6": 1.08e-15,
    "ticks_P/10x3/c1": 4.22e-16, "ticks_delta/10x3/c1": 8.59e-16, "ticks_P/10x3/c6": 3.57e-16, "ticks_delta/10x3/c6": 2.23e-15,
    "ticks_P/3x10/c1": 4.42e-16, "ticks_delta/3x10/c1": 1.09e-15, "ticks_P/3x10/c6": 4.80e-11, "ticks_delta/3x10/c6": 6.34e-11,
    "ticks_P/5x9/c1": 7.00e-16, "ticks_delta/5x9/c1": 3.88e-16, "ticks_P/5x9/c6": 1.10e-10, "ticks_delta/5x9/c6": 7.04e-11,
    "ticks_P/5x5/c1": 3.56e-16, "ticks_delta/5x5/c1": 6.43e-16, "ticks_P/5x5/c6": 4.18e-11, "ticks_delta/5x5/c6": 1.50e-14,
    "ticks_P/9x4/c1": 3.82e-16, "ticks_delta/9x4/c1": 9.02e-16, "ticks_P/9x4/c6": 1.11e-14, "ticks_delta/9x4/c6": 1.83e-14,
    "ticks_P/11x3/c1": 9.30e-16, "ticks_delta/11x3/c1": 5.31e-16, "ticks_P/16x16/c1": 2.05e-14, "ticks_delta/16x16/c1": 9.82e-15,
    "ticks_P/1x1/c1": 1.89e-16, "ticks_delta/1x1/c1": 3.02e-16, "ticks_P/1x1/c6": 2.09e-16, "ticks_delta/1x1/c6": 3.49e-16,
}
