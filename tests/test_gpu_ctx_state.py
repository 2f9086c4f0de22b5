"""State that moved when ba_solver.cpp was split (ba_ctx.h): the dense scratch
the recovery paths and the dense covariance share (ba_dense), the covariance
state the context owns (ba_cov_state), and the stage entries' context guard.
Everything here is bit-for-bit: a context that used the shared state in one
order is compared with contexts that used it in another order or not at all.

1. scratch    the 11-camera banded scene of test_gpu_cov_selected (sel6-11):
              covariance, a forced pinv pass, covariance again in one context;
              the pinv pass first in another; both against a fresh context's
              covariance and against the pinv pass of a context that never
              called the covariance.  Then the same with the selected method,
              whose reported scratch stays the reduction's tiles.
2. reuse      three contexts in a row (create, set_params, two passes,
              covariance, destroy) on test_gpu_covariance's two cameras / one
              point and on sel6-11: equal results; and once more in a fresh
              child process with VLGBA_POISON=1 (every block handed out filled
              with 0xff): equal to the unpoisoned results, so nothing reads a
              block of an earlier context before writing it.
3. stage      vlgba_mex_bundle_3 with a null W returns VLGBA_E_ARG and a valid
              call after it gives the bits of the call before it (a 3-camera,
              5-point scene of conftest.random_problem, as test_mex_gateways).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_cov_selected as tcs
from conftest import random_problem
from test_gpu_stage_ref import ROWS, _params, _two_one

pytestmark = pytest.mark.gpu

KEY = "sel6-11"
COV_KEYS = ("cam", "pts", "blk_jk", "blocks")
E_ARG = -1001


def _same(x, y, what):
    assert sorted(x) == sorted(y), what
    for k in x:
        assert np.array_equal(x[k], y[k]), (what, k)


def _cov(ba, **kw):
    c = ba.covariance(scale=False, blocks=True, **kw)
    out = {k: c[k] for k in COV_KEYS}
    out["scalars"] = np.array([c["sse"], c["dof"], c["sigma2"], c["fixed_rows"]])
    return out, c["scratch_bytes"]


def _pinv_pass(ba):
    """One pass with the pivot word forced: it takes the pinv step.  The state
    is left alone (update_lm = False), so the parameters stay the case's."""
    ba.force_status(4, 1)
    info = ba.step(relinearize=True, update_lm=False)
    assert info.pinv == 1 and info.chol_failed == 1
    da, db = ba.last_step()
    return dict(info=np.frombuffer(bytes(info), dtype=np.uint8), da=da, db=db)


def _ctx(gpu, method):
    ba, r = tcs._make(gpu, KEY)
    ba.set_params(r["a"], r["b"])
    if method == "selected":
        assert tcs._is_cr32(ba, r["na"])
    ba.set_covariance_method(method)
    return ba, r


@pytest.mark.parametrize("method", ["dense", "selected"])
def test_scratch_shared_by_fallback_and_covariance(gpu, method):
    ba, r = _ctx(gpu, method)
    with ba:                                  # a fresh context's covariance
        cov_ref, scratch = _cov(ba)
    ba, _ = _ctx(gpu, method)
    with ba:                                  # a pinv pass without any covariance
        pass_ref = _pinv_pass(ba)
    ba, _ = _ctx(gpu, method)
    with ba:                                  # (a) covariance, pinv pass, covariance
        cov1, s1 = _cov(ba)
        pass_a = _pinv_pass(ba)
        cov2, s2 = _cov(ba)
        assert ba.get_covariance_method() == method
    na, m = r["na"], r["m"]
    tiles = 3 * 32 * 32 * 8 * -(-na * m // ROWS[na])
    print(f"CTXSTATE {method}: scratch_bytes {scratch} (dense {8 * (na * m) ** 2}, tiles {tiles})")
    assert scratch == s1 == s2 == (tiles if method == "selected" else 8 * (na * m) ** 2)
    _same(cov1, cov_ref, "covariance before the pinv pass")
    _same(cov2, cov_ref, "covariance after the pinv pass")
    _same(pass_a, pass_ref, "pinv pass after a covariance")
    if method == "selected":
        return
    ba, _ = _ctx(gpu, method)
    with ba:                                  # (b) the pinv pass first
        pass_b = _pinv_pass(ba)
        cov_b, _ = _cov(ba)
    _same(pass_b, pass_ref, "pinv pass before the covariance")
    _same(cov_b, cov_ref, "covariance after a pinv pass")


def _two_one_make(gpu):
    sc, pt, cam, ox = _two_one()
    a, b = _params(sc, 6)
    return gpu.BundleAdjuster(sc.K, pt, cam, ox, sc.n, 6), dict(a=a, b=b)


def _lifecycles(gpu):
    """Three contexts in a row per scene, each from create to destroy; the
    results as one flat dict of arrays."""
    out = {}
    for name, make in (("two-one", _two_one_make), (KEY, lambda g: tcs._make(g, KEY))):
        for q in range(3):
            ba, r = make(gpu)
            with ba:
                ba.set_params(r["a"], r["b"])
                res = {}
                for p in range(2):
                    info = ba.step(relinearize=True, update_lm=True)
                    res[f"info{p}"] = np.frombuffer(bytes(info), dtype=np.uint8)
                    res[f"da{p}"], res[f"db{p}"] = ba.last_step()
                try:                          # two-one: nothing fixes the gauge, so
                    cov, _ = _cov(ba)         # VLGBA_E_SINGULAR is a result as well
                    res.update(cov, rc=np.array(0))
                except gpu._lib.VlgbaError as exc:
                    assert "(-1007)" in str(exc), exc
                    res["rc"] = np.array(-1007)
                res["a"], res["b"] = ba.get_params()
            out.update({f"{name}|{q}|{k}": np.asarray(v) for k, v in res.items()})
    return out


_PLAIN = {}


def _plain(gpu):
    if not _PLAIN:
        _PLAIN.update(_lifecycles(gpu))
    return _PLAIN


def test_contexts_in_a_row_repeat(gpu):
    res = _plain(gpu)
    for key, v in res.items():
        name, q, k = key.split("|")
        assert np.array_equal(v, res[f"{name}|0|{k}"]), key
    assert res[f"{KEY}|0|rc"] == 0 and np.all(np.isfinite(res[f"{KEY}|0|cam"]))


def test_contexts_in_a_row_poisoned(gpu, tmp_path):
    """The same in a fresh child process with VLGBA_POISON=1."""
    out = tmp_path / "poisoned.npz"
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.pathsep.join([os.path.dirname(here), here] + sys.path)
    env = dict(os.environ, VLGBA_POISON="1", PYTHONPATH=path)
    run = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    with np.load(out) as got:
        _same(dict(got), _plain(gpu), "VLGBA_POISON=1")


def test_stage_entry_after_argument_error(gpu):
    K, a, b, X, vis, sc = random_problem(3, m=3, n=5)
    num_a, m, n = 6, sc.m, sc.n
    assert (m, n) == (3, 5)
    _, _, _, _, _, V, W, _, eB = gpu.mex_bundle_1_XABeUVWeAeB(K, a, b, X, vis)
    Vinv = np.asfortranarray(np.linalg.inv((V + 1e-3 * np.eye(3)[:, :, None]).transpose(2, 0, 1))
                             .transpose(1, 2, 0))
    da = np.asfortranarray(1e-3 * np.random.default_rng(5).standard_normal((num_a, m)))
    args = (W, da, eB, Vinv, K, a, b, X, vis)
    before = gpu.mex_bundle_3_db_new(*args)
    dp = gpu.bundle._dp
    F = [np.asfortranarray(x, dtype=np.float64) for x in args]
    outs = [np.zeros(s, order="F") for s in ((3, n), (num_a, m), (3, n), (2, n, m))]
    rc = gpu.lib().vlgba_mex_bundle_3(m, n, num_a, None, *[dp(x) for x in F[1:]],
                                      *[dp(x) for x in outs])
    assert rc == E_ARG
    assert all(np.all(x == 0.0) for x in outs)
    after = gpu.mex_bundle_3_db_new(*args)
    for x, y in zip(before, after):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y)


if __name__ == "__main__":      # the poisoned child of test_contexts_in_a_row_poisoned
    import bundleadjustmentmatlab_amd as pkg
    assert os.environ.get("VLGBA_POISON") == "1"
    pkg.lib()
    np.savez(sys.argv[1], **_lifecycles(pkg))
