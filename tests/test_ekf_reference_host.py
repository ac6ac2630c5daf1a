"""The EKF matrix formulas against the 60-digit fixture tests/golden/ekf_reference.npz on the CPU: the float64 restatement
tests/ekf_ref.py (whose error sets the gates of tests/ekf_gates.py), the C oracle oracle/ekf_oracle.c on every fixture input --
which ties the oracle, and with it every bitwise oracle-parity test of the kernels, to a reference that shares nothing with it --
and two negative controls that show the inputs tell the conventions of ekf.hpp:129-138 apart.  No GPU."""
import os

import numpy as np

import ekf_gates as G
import ekf_ref as ER


def test_gate_is_four_times_the_float64_restatements_error():
    worst = G.measure()
    for k in G.all_keys():
        print("%-26s measured %.2e recorded %.2e margin %4.1f gate %.2e" % (k, worst[k], G.MEASURED[k], G.margin(k), G.gate(k)))
    assert G.VISITED == set(G.FX.files)                                             # no fixture array is left unvisited (and each is used up)
    assert set(worst) == set(G.MEASURED) == set(G.all_keys())
    # the restatement still delivers what was recorded: a bucket is the worst of 2 to 8 draws, and another BLAS build moves the last
    # bits of every product, so it is held to what everything else is held to, its bucket's gate
    for k, v in worst.items():
        assert v <= G.gate(k), (k, v, G.MEASURED[k])
        assert G.gate(k) == G.margin(k) * max(G.MEASURED[k], G.REF_ROUNDING)
        assert G.margin(k) == G.MARGIN or (k in G.RAISED and G.MARGIN < G.margin(k) <= G.MAX_MARGIN and G.RAISED[k][1] > G.MARGIN)


def test_fixture_covers_what_the_issue_asks_for():
    case = [(2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (3, 3), (4, 1), (4, 2), (4, 3), (6, 1), (6, 2), (6, 3), (6, 6), (4, 4), (7, 1), (7, 2), (7, 3)]
    wide = [(n, m) for n in (8, 9, 10) for m in (1, 2, 3)]
    generic = [(3, 10), (5, 9), (5, 5), (9, 4), (11, 3), (16, 16), (1, 1)]
    assert G.PAIRS == case + wide + generic                                         # SFB_EKF_CASE (8,1): predict only, under PREDICT_DOFS
    assert G.PREDICT_DOFS == [1, 2, 3, 4, 6, 7, 8, 9, 11, 16]
    assert G.LEVELS == ["c1", "c6", "c10"] and list(G.FX["level.cond"]) == [1e1, 1e6, 1e10] and G.CHAIN == ["c1", "c6"]
    golden = os.path.dirname(G.FIXTURE)
    assert os.path.getsize(G.FIXTURE) <= os.path.getsize(os.path.join(golden, "meshfn_reference.npz"))
    for n in G.DOFS:
        assert G.levels(n) == (["c1", "c10"] if n > 10 else G.LEVELS)
        for L, cond in zip(G.LEVELS, G.FX["level.cond"]):
            if L not in G.levels(n):
                continue
            s = G.state(n, L)
            assert ((s["dt"] >= 0.005) & (s["dt"] <= 0.1)).all() and np.abs(s["A"]).max() <= 1.0
            for d in range(G.DRAWS[n]):
                P, Q = G.mat(s["P"][d], n, n), G.mat(s["Q"][d], n, n)
                lam = np.linalg.eigvalsh(ER.symU(P))
                if n > 1:
                    assert 0.5 * cond < lam[-1] / lam[0] < 2.0 * cond                 # the chosen spectrum
                    low = np.abs(P - P.T)[np.tril_indices(n, -1)]
                    assert 0 < low.max() <= 0.11 * lam[0] and (n < 4 or low.max() > 0.01 * lam[0])   # lower triangle off by O(0.1 lambda_min)
                    assert np.abs(Q - Q.T).max() > 0.0                             # Q non-symmetric
    for n, m in G.PAIRS:
        for L in G.levels(n):
            p, s = G.pair(n, m, L), G.state(n, L)
            assert np.abs(p["H"]).max() <= 1.0 and np.abs(p["r"]).max() <= 1.0
            below = 0.0
            for d in range(G.DRAWS[n]):
                R = G.mat(p["R"][d], m, m)
                lmin = np.linalg.eigvalsh(ER.symU(G.mat(s["P"][d], n, n)))[0]
                assert (np.diag(R) > 0.3 * lmin).all() and (np.diag(R) < 3.0 * lmin).all() or n == 1
                below = max(below, np.abs(np.tril(R, -1)).max())
            assert m == 1 or below > 0.05                                           # unrelated numbers of order one below the diagonal
            assert ("ticks_P" in p) == (L in G.CHAIN)


def _oracle_rows(oracle):
    """[(bucket key, got, ref)] of the oracle on every fixture input"""
    rows = []
    for n in G.PREDICT_DOFS:
        for L in G.levels(n):
            s = G.state(n, L)
            rows.append((G.key("euler", n, None, L), oracle.ekf_predict_batch(s["A"], s["Q"], s["dt"], s["P"]), s["euler"]))
            rows.append((G.key("rk4", n, None, L), oracle.ekf_predict_batch(s["A"], s["Q"], s["dt"], s["P"], stepper="rk4"), s["rk4"]))
            rows.append((G.key("rk4_tv", n, None, L), oracle.ekf_predict_batch(s["A"], s["Q"], s["dt"], s["P"], stepper="rk4", A_mid=s["Am"],
                                                                              A_end=s["Ae"]), s["rk4_tv"]))
    for n, m in G.PAIRS:
        for L in G.levels(n):
            s, p = G.state(n, L), G.pair(n, m, L)
            Pu, du, info = oracle.ekf_update_batch(p["H"], p["R"], p["r"], s["P"], n)
            assert (info == 0).all()
            Pf, df, info = oracle.ekf_update_batch(p["H"], p["R"], p["r"], oracle.ekf_predict_batch(s["A"], s["Q"], s["dt"], s["P"]), n)
            assert (info == 0).all()
            rows += [(G.key("update_P", n, m, L), Pu, p["update_P"]), (G.key("update_delta", n, m, L), du, p["update_delta"]),
                     (G.key("fused_P", n, m, L), Pf, p["fused_P"]), (G.key("fused_delta", n, m, L), df, p["fused_delta"])]
            if L in G.CHAIN:
                Pt = s["P"]
                for _ in range(3):
                    Pt, dk, info = oracle.ekf_update_batch(p["H"], p["R"], p["r"], oracle.ekf_predict_batch(s["A"], s["Qc"], s["dt"], Pt), n)
                    assert (info == 0).all()
                rows += [(G.key("ticks_P", n, m, L), Pt, p["ticks_P"]), (G.key("ticks_delta", n, m, L), dk, p["ticks_delta"])]
    return rows


def test_oracle_is_within_the_gates_on_every_fixture_input(oracle):
    """oracle.ekf_predict_batch / ekf_update_batch on all 600 buckets.  The oracle / restatement ratio is printed with each: the
    CPU pre-flight that decides RAISED in tests/ekf_gates.py."""
    rows = _oracle_rows(oracle)
    assert sorted(k for k, _, _ in rows) == sorted(G.all_keys())
    worst, over = {}, []
    for k, got, ref in rows:
        err = G.bucket_error(got, ref)
        print("%-26s oracle %.2e gate %.2e  of the gate %.2f  of the restatement %.2f" % (k, err, G.gate(k), err / G.gate(k),
                                                                                           err / max(G.MEASURED[k], G.REF_ROUNDING)))
        c = k.split("/")[0]
        worst[c] = max(worst.get(c, 0.0), err / G.gate(k))
        if err > G.gate(k):
            over.append((k, err, G.gate(k)))
    print("worst oracle error / gate per class:", {c: round(v, 3) for c, v in worst.items()})
    assert not over, over


# how far a slipped convention must miss: 1e6 times the gate at c1 and c6.  At c10 the issue's own design caps it: the lower triangle
# of P is moved by 0.1 lambda_min = 1e-11 of the results' scale, R is of the order of lambda_min = 1e-10, and the gates there reach
# 1e-7; the controls still miss every c10 gate by more than 100 times.
FACTOR = {"c1": 1e6, "c6": 1e6, "c10": 1e2}


def _control(applies, **wrong):
    seen = 0
    for k, got, ref in G.restatement_rows(**wrong):
        c, size, L = k.split("/")
        if c not in ("update_P", "update_delta"):
            continue
        n, m = (int(v) for v in size.split("x"))
        by = G.bucket_error(got, ref) / G.gate(k)
        print("%-26s misses the gate by %.1e" % (k, by))
        if applies(n, m):
            assert by >= FACTOR[L], (k, by)
            seen += 1
        else:
            assert by <= 1.0, (k, by)                                               # nothing to tell apart there: the control is the formula
    return seen


def test_negative_control_symU_of_P_in_H_P():
    """H symU(P) in place of H P (:134): every update bucket with an off-diagonal in P, i.e. dof >= 2"""
    assert _control(lambda n, m: n >= 2, wrong_hp=True) == 2 * sum(len(G.levels(n)) for n, m in G.PAIRS if n >= 2)


def test_negative_control_lower_triangle_of_R():
    """R's lower triangle mirrored in place of its upper one (:130): every update bucket with ny >= 2"""
    assert _control(lambda n, m: m >= 2, wrong_r=True) == 2 * sum(len(G.levels(n)) for n, m in G.PAIRS if m >= 2)
