"""tests/jac_ref.py -- the reference of the analytic Jacobians -- proved on the
CPU before tests/test_gpu_jacobian.py holds the kernels to it.

1. Against the oracle's forward differences (h = 1e-10) at the bar of
   tests/test_oracle.py::test_fd_jacobian_vs_analytic (2e-3), every num_a.
2. Against long double central differences of the true projection with step
   CD_STEP: 1e-5 for the Euclidean models (truncation h^2 / 6 times the third
   derivative, cancellation 2^-64 |x| / h ~ 1e-12 px), 1e-8 for the projective
   one, whose third row is ~1 / f.  Measured here, the largest difference as a
   fraction of the row's largest entry (bar 1e-9): 6.5e-11 Euclidean (6.5e-9 at
   ten times the step, 6.8e-13 at a tenth), 4.2e-11 projective (4.2e-9, 1.4e-12).
3. dR/dw against long double central differences of Rodrigues' formula,
   Richardson-extrapolated to 2e-15, over the angles where the evaluation
   changes (the R = I rule, the series switch-over).
4. The bound's cap: at most 1e-12 of the largest |entry| of the observation's
   [A | B] on every scene of tests/test_gpu_jacobian.py.  Measured: 1.0e-14 on
   the banded scenes, 2.6e-14 on the ladders, 3.2e-14 on ladybug.
5. The dense analytic LM frees cameras that start at w = 0 (e2e_check).
6. include/vlgba.h declares the entry points.
"""
import os
import re

import numpy as np
import pytest

import jac_ref as jr
import test_gpu_robust as scenes          # the scenes only: nothing here runs on a GPU
from conftest import random_problem, random_projective_problem

LD = jr.LD
# a projective camera's third row is ~1 / f: a step of 1e-5 there moves the
# depth by half a percent, so its step is scaled down with it
CD_STEP = {6: 1e-5, 7: 1e-5, 10: 1e-5, 12: 1e-8}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _obs(vis):
    pt, cam = np.nonzero(vis)
    return pt, cam


@pytest.mark.parametrize("na", [6, 7, 10, 12])
def test_against_the_oracles_forward_differences(oracle, poracle, na):
    if na == 12:
        a, b, X, vis, *_ = random_projective_problem(3)
        K = None
        ref1 = poracle.mex1(a, b, X, vis)
    else:
        K, a, b, X, vis, _ = random_problem(3, num_a=na, zero_w_cam=True)
        ref1 = oracle.mex1(K, a, b, X, vis)
    pt, cam = _obs(vis)
    Afd = ref1[1][:, :, pt, cam].transpose(2, 0, 1)
    Bfd = ref1[2][:, :, pt, cam].transpose(2, 0, 1)
    Ao, Bo, _, _ = jr.jacobians(K, a, b, pt, cam, na)
    Ao, Bo = Ao.astype(np.float64), Bo.astype(np.float64)
    if na != 12:
        # camera 0 has w = 0: the FD rotation columns are exactly zero (App. A
        # Q2), the analytic ones are the generators' -- compared elsewhere
        z = cam == 0
        assert z.any() and np.all(Afd[z][:, :, 0:3] == 0) and np.any(Ao[z][:, :, 0:3] != 0)
        Ao[z, :, 0:3] = 0
    for got, want in ((Afd, Ao), (Bfd, Bo)):
        amax = np.abs(want).reshape(len(pt), -1).max(1)[:, None, None]
        assert np.all(np.abs(got - want) <= 2e-3 * np.abs(want) + 2e-3 * amax)


@pytest.mark.parametrize("na", [6, 7, 10, 12])
def test_against_long_double_central_differences(na):
    if na == 12:
        a, b, X, vis, *_ = random_projective_problem(5)
        K = None
    else:
        K, a, b, X, vis, _ = random_problem(5, num_a=na, zero_w_cam=False)
    pt, cam = _obs(vis)
    Ao, Bo, Ab, Bb = jr.jacobians(K, a, b, pt, cam, na)
    top = jr.row_max(Ao, Bo)[:, None, None]
    fig = {}
    for h in (10 * CD_STEP[na], CD_STEP[na], 0.1 * CD_STEP[na]):
        Ac, Bc = jr.central_differences(K, a, b, pt, cam, na, h)
        fig[h] = float(max((np.abs(Ac - Ao) / top).max(), (np.abs(Bc - Bo) / top).max()))
    print(f"JACREF central differences num_a {na}: largest |diff| / row max by step "
          + " ".join(f"{h:g}: {v:.2e}" for h, v in fig.items()))
    assert fig[CD_STEP[na]] <= 1e-9, fig


def _direction(seed=11):
    d = np.random.default_rng(seed).standard_normal(3)
    return d / np.linalg.norm(d)


ANGLES = [0.0, 1e-7, 0.99e-6, 1.01e-6, 1e-4, 0.99 * jr.SWITCH, 1.01 * jr.SWITCH, 0.1, 1.0, 3.0]


def _rodrigues_derivative(w, k, h):
    """d rodrigues / d w_k at w (3,) by long double central differences with steps
    h, h / 2, h / 4 and two Richardson extrapolations: truncation O(h^6)."""
    def cd(step):
        wp, wm = w.astype(LD).reshape(3, 1).copy(), w.astype(LD).reshape(3, 1).copy()
        wp[k] += step
        wm[k] -= step
        return (jr.rodrigues(wp) - jr.rodrigues(wm))[:, :, 0] / (2 * step)
    d0, d1, d2 = cd(LD(h)), cd(LD(h) / 2), cd(LD(h) / 4)
    r0, r1 = (4 * d1 - d0) / 3, (4 * d2 - d1) / 3
    return (16 * r1 - r0) / 15


RICH_STEP = 4e-3
RICH_ERR = 2e-15


def test_drodrigues_against_central_differences():
    """dR/dw_k at every angle where the evaluation changes, against an
    evaluation that shares nothing with the device's formula: Rodrigues'
    formula itself, differenced.  With steps 4e-3, 2e-3, 1e-3 and two
    extrapolations the truncation is h^6 |R^(7)| / 1344 < 1e-17 and the long
    double cancellation 2^-64 / 1e-3 times the extrapolations' weights, about
    1e-15: RICH_ERR = 2e-15, a tenth of the reference's own bound (at most 200 u
    = 2.2e-14).  Measured: the largest difference is 3e-16 at every angle above
    1e-6.  Below 1e-6 the rule returns the limit G_k, from which the true
    derivative differs by O(th): bar 2 th + the same."""
    w = (_direction()[:, None] * np.array(ANGLES)[None, :]).astype(np.float64)
    w[:, 0] = 0.0
    D, Db = jr.drodrigues(w)
    worst = {}
    for q, th in enumerate(ANGLES):
        for k in range(3):
            diff = np.abs(_rodrigues_derivative(w[:, q], k, RICH_STEP) - D[:, :, k, q])
            bar = Db[:, :, k, q] + RICH_ERR + (2 * th if th < jr.SMALL else 0)
            worst[th] = max(worst.get(th, 0.0), float(diff.max()))
            assert np.all(diff <= bar), (th, k, diff.max())
        if th < jr.SMALL:       # exactly the generators, exact bound
            assert np.all(Db[:, :, :, q] == 0)
            assert D[2, 1, 0, q] == 1 and D[1, 2, 0, q] == -1 and D[0, 2, 1, q] == 1
            assert np.abs(D[:, :, :, q]).sum() == 6
    print("JACREF dR/dw: largest |diff| by angle " +
          " ".join(f"{t:g}: {v:.1e}" for t, v in worst.items()))
    print("JACREF dR/dw: largest bound by angle " +
          " ".join(f"{t:g}: {float(Db[:, :, :, q].max()):.1e}" for q, t in enumerate(ANGLES)))
    assert float(Db[:, :, :, 1:].max()) <= 200 * float(jr.U53)
    # the step's own check: a coarser and a finer one agree with it to RICH_ERR
    for h in (2 * RICH_STEP, RICH_STEP / 2):
        for q in (4, 6, 8):
            d = np.abs(_rodrigues_derivative(w[:, q], 1, h) -
                       _rodrigues_derivative(w[:, q], 1, RICH_STEP)).max()
            assert d <= RICH_ERR, (h, ANGLES[q], d)


def _test_scenes():
    out = [("banded", na) for na in (6, 7, 10, 12)] + [("long", 6)]
    out += [("ladder", na) for na in (7, 10, 12)]
    return out


@pytest.mark.parametrize("name,na", _test_scenes() + [("ladybug", 6), ("e2e", 6)])
def test_bound_is_capped(name, na):
    if name == "e2e":
        s = jr.e2e_scene()
        K, a, b, pt, cam = s["K"], s["a0"], s["b0"], s["pt"], s["cam"]
    else:
        sc, pt, cam, ox = scenes._scene(name, na)
        K, a, b, _ = scenes._problem(sc, na)
    Ao, Bo, Ab, Bb = jr.jacobians(K, a, b, pt, cam, na)
    top = jr.row_max(Ao, Bo)
    cap = float(max((Ab.reshape(len(pt), -1).max(1) / top).max(),
                    (Bb.reshape(len(pt), -1).max(1) / top).max()))
    print(f"JACREF bound cap {name} num_a {na}: largest bound / row max {cap:.2e} over "
          f"{len(pt)} observations")
    assert cap <= 1e-12


def _dense(s):
    X = np.zeros((2, s["n"], s["m"]), order="F")
    X[0, s["pt"], s["cam"]], X[1, s["pt"], s["cam"]] = s["obs_x"][:, 0], s["obs_x"][:, 1]
    vis = np.zeros((s["n"], s["m"]), order="F")
    vis[s["pt"], s["cam"]] = 1.0
    return X, vis


def test_analytic_lm_frees_the_cameras_at_w_zero(oracle):
    s = jr.e2e_scene()
    X, vis = _dense(s)
    res = {}
    for jac in ("fd", "analytic"):
        res[jac] = jr.analytic_lm(s["K"], s["a0"], s["b0"], X, vis, jac=jac, pivot=s["pivot"],
                                  **jr.E2E["stop"], **jr.E2E["lm"])
    fig = jr.e2e_figures(s, res["fd"][0], res["fd"][2], res["analytic"][0], res["analytic"][2])
    print("JACREF w = 0 on the CPU: FD leaves |w| %.3g; analytic moves them to |w| >= %.4f, "
          "within %.2e of the truth; error_ FD %.6g analytic %.6g" % fig)
    print(f"JACREF w = 0 on the CPU: error_ analytic {res['analytic'][2]}")
    jr.e2e_check(fig)
    # the pivots stayed where they started
    assert np.array_equal(res["analytic"][0][:, s["pivot"]], s["a0"][:, s["pivot"]])


def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "vlgba.h")) as f:
        h = f.read()
    assert re.search(r"int\s+vlgba_set_jacobian\s*\(\s*vlgba_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", h)
    assert re.search(r"int\s+vlgba_get_jacobian\s*\(\s*vlgba_ctx\s*\*\s*\w*\s*,\s*int\s*\*\s*\w+\s*\)\s*;", h)
    assert re.search(r"#define\s+VLGBA_JAC_FD\s+0\b", h)
    assert re.search(r"#define\s+VLGBA_JAC_ANALYTIC\s+1\b", h)
    assert re.search(r"#define\s+VLGBA_ABI_VERSION\s+6\b", h)     # entry points only
