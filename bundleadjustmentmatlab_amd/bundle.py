"""Host mirror of the reference's MATLAB entry points, running on libvlgba.

``bundle_euclid`` keeps the signature, option names, argument meaning and
output semantics of toolbox/bundle/bundle_euclid.m:1-269::

    K_, Te_, w_, Xe_, error_ = bundle_euclid(K, Te, w, Xe, x, 'fix_calibration',
                                             'visibility', vis, 'verbose')

with arrays MATLAB-shaped (K 4xm, Te 3xm, w 3xm, Xe 4xn, x 3xnxm).  The whole
LM loop (bundle_euclid.m:111-249) runs on the GPU through ``vlgba_solve``.

``bundle_euclid_obs`` takes the same problem as a COO observation list, the
form that scales to the 1000-camera / 500k-point configs (a dense x at that
size is 12 GB).

``bundle_euclid_nomex`` is the same drop-in for the reference's pure-MATLAB
twin toolbox/bundle/bundle_euclid_nomex.m (full-da back substitution, no
'fix_pivot', Xe_(4,:) = 1).

``mex_bundle_1_XABeUVWeAeB`` / ``mex_bundle_2_Se_`` / ``mex_bundle_3_db_new``
mirror the three MEX stages with their exact argument layouts.
"""
from __future__ import annotations

import ctypes
import numpy as np

from ._lib import (ALLREDUCE_FN, COV_METHODS, JACOBIANS, LOSSES, MODEL_EUCLIDEAN, MODEL_PROJECTIVE, NKERNELS, ON_PASS_FN,
                   VlgbaOptions,
                   VlgbaProblem, VlgbaResectProblem, VlgbaStats,
                   VlgbaStepInfo, c_dp, c_ip, c_up, check, lib)

__all__ = ["bundle_euclid", "bundle_euclid_nomex", "bundle_euclid_obs", "BundleAdjuster",
           "bundle_euclid_resect", "bundle_euclid_intersect", "triangulate_points",
           "parse_options", "pivot_mask",
           "mex_bundle_1_XABeUVWeAeB", "mex_bundle_2_Se_", "mex_bundle_3_db_new"]


def _F(a):
    return np.asfortranarray(a, dtype=np.float64)


def _dp(a):
    return a.ctypes.data_as(c_dp)


# ---------------------------------------------------------------------------
# options (bundle_euclid.m:44-82)
# ---------------------------------------------------------------------------
def pivot_mask(pivot, m):
    """The cameras ``U(:,:,pivot) = 0`` fixes (bundle_euclid.m:150-153), read
    the way MATLAB indexes with ``pivot``: a logical mask (bool dtype) of any
    length -- entries past m must be false -- or a list of 1-based camera
    numbers (``'fix_pivot', 1`` or ``[1 3]``; duplicates allowed).  MATLAB
    would grow U / W / eA for a true entry or an index past m, and errors on
    an index that is not a positive integer; both are errors here.  Returns
    the (m,) bool mask."""
    p = np.asarray(pivot)
    mask = np.zeros(m, dtype=bool)
    flat = p.reshape(-1)
    if p.dtype == bool:
        if flat[m:].any():
            raise ValueError("fix_pivot: logical index past the camera count")
        mask[:min(flat.size, m)] = flat[:m]
        return mask
    if flat.size == 0:
        return mask
    v = flat.astype(np.float64)
    if not np.all(np.isfinite(v)) or np.any(v != np.floor(v)) or v.min() < 1 or v.max() > m:
        raise ValueError("fix_pivot: camera indices must be integers in 1..m")
    mask[v.astype(np.int64) - 1] = True
    return mask


def parse_options(m, n, varargin, x=None, nomex=False):
    """Name/value options of bundle_euclid.m:53-78.  Unknown names are
    ignored, as the reference's switch statement ignores them.  'fix_pivot'
    takes a logical mask or 1-based camera numbers (pivot_mask).  nomex=True
    parses bundle_euclid_nomex.m:50-70 instead, which has no 'fix_pivot': the
    name and its argument fall through its switch and are ignored."""
    o = dict(fix_structure=False, fix_motion=False, fix_pivot=False,
             pivot=np.zeros(m, dtype=bool), num_variableK=4, visible=None, verbose=False)
    k = 0
    varargin = list(varargin)
    while k < len(varargin):
        name = varargin[k]
        name = name.lower() if isinstance(name, str) else name
        if name == "fix_structure":
            o["fix_structure"] = True
        elif name == "fix_motion":
            o["fix_motion"] = True
        elif name == "fix_pivot":
            if not nomex:
                o["fix_pivot"] = True
                o["pivot"] = pivot_mask(varargin[k + 1], m)
            k += 1
        elif name == "fix_calibration":
            o["num_variableK"] = 0
        elif name == "fix_principal":
            o["num_variableK"] = 1
        elif name == "visibility":
            o["visible"] = np.asarray(varargin[k + 1])
            k += 1
        elif name == "verbose":
            o["verbose"] = True
        k += 1
    if o["visible"] is None and x is not None:
        o["visible"] = (x[0] != 0) | (x[1] != 0)          # bundle_euclid.m:50
    if o["visible"] is not None:
        o["visible"] = np.asarray(o["visible"], dtype=np.float64).reshape(n, m, order="F")
    return o


RADIAL_NVK = 3   # the radial model's variable calibration: a[6:9] = f, k1, k2


def pack_a(K, Te, w, nvk, kd=None):
    """a = [w; T; (K)] (bundle_euclid.m:89-96); the radial model (nvk =
    RADIAL_NVK, kd 2 x m): a = [w; T; f; k1; k2] with f = K[0]."""
    m = w.shape[1]
    a = np.zeros((6 + nvk, m), order="F")
    a[0:3] = w
    a[3:6] = Te
    if nvk == RADIAL_NVK:
        kd = np.asarray(kd, dtype=np.float64)
        if kd.shape != (2, m):
            raise ValueError(f"radial: expected 2 x {m} coefficients, got {kd.shape}")
        a[6] = K[0]
        a[7:9] = kd
    elif nvk == 1:
        a[6] = K[0]
    elif nvk == 4:
        a[6:10] = K
    return a


def unpack(K, a, b, Xe4, nvk):
    """bundle_euclid.m:255-267 (Xe_(4,:) is the input Xe(4,:), App. A Q5)."""
    K_ = np.array(K, dtype=np.float64, order="F")
    if nvk == 1 or nvk == RADIAL_NVK:   # (radial: a[7:9] = k1, k2 are the caller's)
        K_[0] = a[6]
        K_[1] = a[6]
    elif nvk == 4:
        K_[:] = a[6:10]
    return K_, a[3:6].copy(order="F"), a[0:3].copy(order="F"), np.vstack([b, Xe4])


# ---------------------------------------------------------------------------
# per-pass JSON log ("Tracing")
# ---------------------------------------------------------------------------
class _PassLog:
    """Callable for vlgba_options.on_pass: one JSON line per LM pass."""

    def __init__(self, sink, num_vis, projective):
        import json
        self._json = json
        self._own = False
        self._fn = None
        self._fh = None
        if callable(sink) and not hasattr(sink, "write"):
            self._fn = sink
        elif hasattr(sink, "write"):
            self._fh = sink
        else:
            self._fh = open(sink, "a", encoding="utf-8")
            self._own = True
        self.num_vis = float(num_vis)
        self.projective = projective
        self.records = []

    def __call__(self, npass, it, info_p, _user):
        i = info_p.contents
        # bundle_euclid.m:219-220 error_ = SSE / num_vis (projective: SSE * (1 / num_vis))
        sc = (lambda v: 1 / self.num_vis * v) if self.projective else (lambda v: v / self.num_vis)
        rec = {"pass": int(npass), "iter": int(it), "lambda": i.lambda_,
               "old_sse": i.old_sse, "new_sse": i.new_sse, "error_old": sc(i.old_sse),
               "error_new": sc(i.new_sse), "dpg": i.dpg, "rho": i.rho,
               "accepted": bool(i.accepted), "chol_failed": bool(i.chol_failed),
               "pinv": bool(i.pinv), "spin_retry": bool(i.spin_retry)}
        self.records.append(rec)
        try:
            if self._fn is not None:
                self._fn(rec)
            else:
                self._fh.write(self._json.dumps(rec) + "\n")
        except Exception:   # noqa: BLE001 -- a failing log must not abort the solve
            pass

    def close(self):
        if self._own and self._fh is not None:
            self._fh.close()
            self._fh = None


# ---------------------------------------------------------------------------
# the GPU solver handle
# ---------------------------------------------------------------------------
class BundleAdjuster:
    """One problem resident on one GPU (vlgba_ctx).

    obs_pt / obs_cam (0-based) and obs_x (N, 2) describe the visible
    observations; K is 4 x m; num_a is 6 (fix_calibration), 7 (fix_principal),
    10 (variable K) or 9: the camera with radial distortion, a = [w; T; f; k1;
    k2] per camera, x = f d n + (K[2], K[3]) with n the normalised image point
    and d = 1 + k1 |n|^2 + k2 |n|^4.  That model has analytic Jacobians only
    (jacobian="fd" raises VlgbaError -1001), always takes all nine rows of da
    into the back substitution, and does not go with ``parity`` / ``ordered``
    (VlgbaError -1001 at creation).  Options follow bundle_euclid.m's names.  ``solver``
    picks the reduced-camera solve: "auto" (cyclic reduction when S is
    tile-tridiagonal, else envelope Cholesky -- on a nested-dissection camera
    order when that shortens its chain of steps), "envelope", "nd" (the
    nested-dissection order whenever the cameras split), "dense", or "pcg":
    block-Jacobi preconditioned conjugate gradients on the co-visible blocks
    (opt-in; an inexact step, no dense S -- device memory linear in the blocks
    and cameras; ``pcg_tol`` / ``pcg_max_iter``: set_pcg, defaults 0.1 and 500;
    not with ``parity`` / ``ordered``: VlgbaError -1001).
    ``dense_solve=True`` is the same as solver="dense".  ``schur_kernel``
    picks the fast-path Schur complement kernel: "auto" (dense per-chunk
    products on fp64 MFMA when the tracks fit) or "terms" (per-term sums).
    ``semantics`` is "mex" (bundle_euclid.m) or "nomex" (bundle_euclid_nomex.m).
    ``parity=True`` runs the parity mode (vlgba_options.ordered = 2: ordered
    sums, sequential Cholesky, LM scalars in the reference's flat order --
    the LM trajectory is bit-identical to the CPU oracle's).  ``stop_rel``
    replaces the 1e-3 of the stop rule (bundle_euclid.m:123).
    ``log`` (a path, a text file or a callable) receives one JSON record per
    LM pass of run() (vlgba_options.on_pass): pass, iter, lambda, old / new
    SSE, error_ values (SSE / num_vis), rho, accepted, chol_failed, pinv.
    ``model="projective"`` solves bundle_projective.m instead: num_a = 12
    (a = P(:) per camera), K is None and ``m`` gives the camera count.
    ``loss`` ("none", "huber" or "cauchy") with ``loss_scale`` in pixels makes
    the solve robust (set_loss; vlgba_set_loss): error_ and the pass scalars
    are then the robust cost.  Not with ``parity`` / ``ordered``.
    ``jacobian`` is "fd" (the reference's forward differences, h = 1e-10) or
    "analytic" (closed-form derivatives on the fast path: set_jacobian;
    vlgba_set_jacobian) -- the same residuals and cost, Jacobians without the
    differences' ~1e-6 noise, and a camera at w = 0 can rotate.  None (the
    default) leaves the library's default: "fd", or "analytic" where the
    environment variable VLGBA_JACOBIAN=analytic is set; a given value wins over
    the environment.  Not with ``parity`` / ``ordered`` (ValueError); on a
    problem that the planner hands to the ordered kernels all the same
    (plan_info()["ordered"] == 1) "analytic" raises VlgbaError -1001.
    """
    SOLVERS = {"auto": 0, "dense": 1, "envelope": 2, "sequential": 3, "nd": 4,
               "pcg": 5}
    SCHUR_KERNELS = {"auto": 0, "terms": 1}
    SEMANTICS = {"mex": 0, "nomex": 1}
    MODELS = {"euclidean": MODEL_EUCLIDEAN, "projective": MODEL_PROJECTIVE}

    def __init__(self, K, obs_pt, obs_cam, obs_x, n, num_a=6, *, fix_structure=False,
                 fix_motion=False, pivot=None, verbose=False, num_vis=0.0, device=0,
                 rank=0, world_size=1, comm_id=None, max_iter=0, max_iter2=0, lambda0=0.0,
                 dense_solve=False, ordered=False, allreduce=None, solver=None,
                 schur_kernel="auto", semantics="mex", model="euclidean", m=None,
                 parity=False, stop_rel=0.0, log=None, loss="none", loss_scale=0.0,
                 jacobian=None, pcg_tol=None, pcg_max_iter=None):
        L = lib()
        if jacobian is not None and jacobian not in JACOBIANS:
            raise ValueError(f"jacobian must be one of {sorted(JACOBIANS)}")
        if jacobian == "analytic" and (parity or ordered):
            raise ValueError("analytic Jacobians do not go with parity / ordered mode (bit "
                             "parity with the reference's forward differences)")
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {sorted(LOSSES)}")
        if loss != "none" and (parity or ordered):
            raise ValueError("a robust loss does not go with parity / ordered mode (bit parity "
                             "with a reference that has no loss)")
        solve_mode = self.SOLVERS[solver] if solver is not None else int(bool(dense_solve))
        self.K = _F(K) if K is not None else None
        self.m = int(m) if m is not None else self.K.shape[1]
        self.n = int(n)
        self.num_a = int(num_a)
        self.max_iter = int(max_iter) if max_iter > 0 else 20   # bundle_euclid.m:117
        self._pt = np.ascontiguousarray(obs_pt, dtype=np.int32)
        self._cam = np.ascontiguousarray(obs_cam, dtype=np.int32)
        self._x = np.ascontiguousarray(obs_x, dtype=np.float64).reshape(-1, 2)
        self.num_obs = len(self._pt)
        prob = VlgbaProblem(self.m, self.n, self.num_a, self.num_obs,
                            self._pt.ctypes.data_as(c_ip), self._cam.ctypes.data_as(c_ip),
                            _dp(self._x), _dp(self.K) if self.K is not None else None,
                            float(num_vis), self.MODELS[model])
        self._pivot = None
        if pivot is not None:
            self._pivot = np.ascontiguousarray(np.asarray(pivot, dtype=bool).reshape(-1),
                                               dtype=np.uint8)
        self._comm = None
        if comm_id is not None:
            self._comm = ctypes.create_string_buffer(bytes(comm_id), 128)
        self._ar = None
        if allreduce is not None:
            # host collective: allreduce(np.ndarray) sums in place over ranks
            def _cb(buf, count, _user, fn=allreduce):
                try:
                    fn(np.ctypeslib.as_array(buf, shape=(count,)))
                    return 0
                except Exception:   # noqa: BLE001 -- reported to the library as failure
                    return 1
            self._ar = ALLREDUCE_FN(_cb)
        self._log = self._log_fn = None
        if log is not None:
            self._log = _PassLog(log, num_vis if num_vis > 0 else float(self.num_obs),
                                 model == "projective")
            self._log_fn = ON_PASS_FN(self._log)
        opt = VlgbaOptions(int(fix_structure), int(fix_motion),
                           self._pivot.ctypes.data_as(c_up) if self._pivot is not None else None,
                           int(verbose), int(max_iter), int(max_iter2), float(lambda0),
                           int(device), int(rank), int(world_size),
                           ctypes.cast(self._comm, ctypes.c_void_p) if self._comm else None,
                           solve_mode, 2 if parity else int(ordered),
                           ctypes.cast(self._ar, ctypes.c_void_p) if self._ar else None, None,
                           self.SCHUR_KERNELS[schur_kernel], self.SEMANTICS[semantics],
                           float(stop_rel),
                           ctypes.cast(self._log_fn, ctypes.c_void_p) if self._log_fn else None,
                           None)
        h = ctypes.c_void_p()
        check(L.vlgba_create(ctypes.byref(prob), ctypes.byref(opt), ctypes.byref(h)),
              "vlgba_create")
        self._h = h
        self._L = L
        try:
            if loss != "none":
                self.set_loss(loss, loss_scale)
            if jacobian is not None and self.get_jacobian() != jacobian:
                self.set_jacobian(jacobian)       # (over the environment's default)
            if pcg_tol is not None or pcg_max_iter is not None:
                self.set_pcg(pcg_tol, pcg_max_iter)
        except Exception:
            self.close()
            raise

    def set_loss(self, loss="none", scale=0.0):
        """The robust loss of the passes from here on (vlgba_set_loss): "none",
        "huber" or "cauchy" with ``scale`` in pixels.  The next pass or getter
        linearises again with the new weights."""
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {sorted(LOSSES)}")
        check(self._L.vlgba_set_loss(self._h, LOSSES[loss], float(scale)), "vlgba_set_loss")

    def get_loss(self):
        """(loss name, scale) of the context (vlgba_get_loss)."""
        kind, scale = ctypes.c_int(), ctypes.c_double()
        check(self._L.vlgba_get_loss(self._h, ctypes.byref(kind), ctypes.byref(scale)),
              "vlgba_get_loss")
        return {v: k for k, v in LOSSES.items()}[kind.value], scale.value

    def set_jacobian(self, jacobian="fd"):
        """The Jacobians of the passes from here on (vlgba_set_jacobian): "fd" or
        "analytic".  The next pass or getter linearises again."""
        if jacobian not in JACOBIANS:
            raise ValueError(f"jacobian must be one of {sorted(JACOBIANS)}")
        check(self._L.vlgba_set_jacobian(self._h, JACOBIANS[jacobian]), "vlgba_set_jacobian")

    def get_jacobian(self):
        """"fd" or "analytic" (vlgba_get_jacobian)."""
        kind = ctypes.c_int()
        check(self._L.vlgba_get_jacobian(self._h, ctypes.byref(kind)), "vlgba_get_jacobian")
        return {v: k for k, v in JACOBIANS.items()}[kind.value]

    def set_pcg(self, tol=None, max_iter=None):
        """The stop rule of a solver="pcg" context from here on (vlgba_set_pcg):
        the relative residual sqrt(r'M^-1 r / e_'M^-1 e_) to reach (0 < tol < 1)
        and the iteration limit; None keeps the current value."""
        check(self._L.vlgba_set_pcg(self._h, 0.0 if tol is None else float(tol),
                                    0 if max_iter is None else int(max_iter)), "vlgba_set_pcg")

    def get_pcg(self):
        """(tol, max_iter) of a solver="pcg" context (vlgba_get_pcg)."""
        tol, it = ctypes.c_double(), ctypes.c_int()
        check(self._L.vlgba_get_pcg(self._h, ctypes.byref(tol), ctypes.byref(it)),
              "vlgba_get_pcg")
        return tol.value, it.value

    def pcg_stats(self):
        """The last pass's PCG solve (vlgba_get_pcg_stats): dict of iterations,
        relres (the recurrence's sqrt(rz_k / rz_0) at its end), converged (the
        tolerance was met; False: the iteration limit ended the solve and the
        iterate was the step) and total (iterations over the context's passes)."""
        it, conv, rel, tot = ctypes.c_int(), ctypes.c_int(), ctypes.c_double(), ctypes.c_longlong()
        check(self._L.vlgba_get_pcg_stats(self._h, ctypes.byref(it), ctypes.byref(rel),
                                          ctypes.byref(conv), ctypes.byref(tot)),
              "vlgba_get_pcg_stats")
        return dict(iterations=it.value, relres=rel.value, converged=bool(conv.value),
                    total=tot.value)

    def residuals(self):
        """Per observation at the current parameters (vlgba_get_residuals), in
        linearization()'s W order: e (N, 2) the unweighted residuals x - x_hat,
        w (N,) the loss's weights and rho (N,) its costs (no loss: 1 and
        e0^2 + e1^2)."""
        e = np.zeros((self.num_obs, 2))
        w = np.zeros(self.num_obs)
        rho = np.zeros(self.num_obs)
        check(self._L.vlgba_get_residuals(self._h, _dp(e), _dp(w), _dp(rho)),
              "vlgba_get_residuals")
        return e, w, rho

    def close(self):
        if getattr(self, "_h", None):
            self._L.vlgba_destroy(self._h)
            self._h = None
        if getattr(self, "_log", None) is not None:
            self._log.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_params(self, a, b):
        a = np.ascontiguousarray(_F(a).reshape(-1, order="F"))
        b = np.ascontiguousarray(_F(b).reshape(-1, order="F"))
        assert a.size == self.num_a * self.m and b.size == 3 * self.n
        check(self._L.vlgba_set_params(self._h, _dp(a), _dp(b)), "vlgba_set_params")

    def get_params(self):
        a = np.zeros(self.num_a * self.m)
        b = np.zeros(3 * self.n)
        check(self._L.vlgba_get_params(self._h, _dp(a), _dp(b)), "vlgba_get_params")
        return a.reshape(self.num_a, self.m, order="F"), b.reshape(3, self.n, order="F")

    def force_status(self, word, passes=1):
        """Fault injection: the next ``passes`` passes report a non-positive
        pivot (word 4: pinv step) or a hand-off timeout (word 5: re-solve);
        word 6: the next ``passes`` starts of the envelope runner fail (the
        factorization then runs with the column launches alone)."""
        check(self._L.vlgba_debug_force_status(self._h, int(word), int(passes)),
              "vlgba_debug_force_status")

    def step(self, relinearize=True, update_lm=True):
        info = VlgbaStepInfo()
        check(self._L.vlgba_step(self._h, int(relinearize), int(update_lm), ctypes.byref(info)),
              "vlgba_step")
        return info

    def passes(self, n):
        """n full passes at the current parameters and lambda, each
        relinearising, none changing the state (vlgba_run_passes); the last
        pass's info."""
        info = VlgbaStepInfo()
        check(self._L.vlgba_run_passes(self._h, int(n), ctypes.byref(info)), "vlgba_run_passes")
        return info

    def run(self):
        """The LM loop (vlgba_run): (error_, stats).  error_ has at most
        max_iter entries (bundle_euclid.m:117-123)."""
        err = np.zeros(self.max_iter + 1)
        st = VlgbaStats()
        check(self._L.vlgba_run(self._h, _dp(err), err.size, ctypes.byref(st)), "vlgba_run")
        assert st.num_error <= err.size
        return err[: st.num_error].copy(), st

    def last_step(self):
        """(da (num_a, m), db (3, n)) of the last pass (vlgba_get_step)."""
        da = np.zeros(self.num_a * self.m)
        db = np.zeros(3 * self.n)
        check(self._L.vlgba_get_step(self._h, _dp(da), _dp(db)), "vlgba_get_step")
        return da.reshape(self.num_a, self.m, order="F"), db.reshape(3, self.n, order="F")

    def reduced_system(self, dense=True):
        """S (lower triangle: blocks j >= k; dense (na m) x (na m) if dense,
        else (blk_jk (nb, 2), blocks (nb, na, na))) and e_ at the current
        lambda (vlgba_get_reduced_system)."""
        nb = self.plan_info()["blocks"]
        na = self.num_a
        jk = np.zeros(2 * nb, dtype=np.int32)
        blocks = np.zeros(na * na * nb)
        e_ = np.zeros(na * self.m)
        check(self._L.vlgba_get_reduced_system(self._h, jk.ctypes.data_as(c_ip), _dp(blocks),
                                               _dp(e_)), "vlgba_get_reduced_system")
        jk = jk.reshape(nb, 2)
        blocks = blocks.reshape(nb, na, na).transpose(0, 2, 1)   # [b, r, c]
        if not dense:
            return jk, blocks, e_
        S = np.zeros((na * self.m, na * self.m))
        for (j, k), B in zip(jk, blocks):
            if j == k:
                S[na * j:na * j + na, na * k:na * k + na] = np.tril(B)
            else:
                S[na * j:na * j + na, na * k:na * k + na] = B
        return S, e_

    def set_covariance_method(self, method="dense"):
        """How covariance() forms the camera covariance from here on
        (vlgba_set_covariance_method): "dense" (rocSOLVER inverse of the dense
        reduced system, 8 ld^2 bytes of scratch) or "selected" (a selected
        inverse on the camera-aligned cyclic reduction's factors: only the
        co-visible blocks, three 32 x 32 tiles of scratch per reduction tile).
        "selected" raises VlgbaError (-1001) unless plan_info() shows the
        camera-aligned cyclic reduction (cr_levels > 0, cr_rows == num_a *
        (32 // num_a)) on one rank outside ordered / parity mode."""
        if method not in COV_METHODS:
            raise ValueError(f"method must be one of {sorted(COV_METHODS)}")
        check(self._L.vlgba_set_covariance_method(self._h, COV_METHODS[method]),
              "vlgba_set_covariance_method")

    def get_covariance_method(self):
        """"dense" or "selected" (vlgba_get_covariance_method)."""
        kind = ctypes.c_int()
        check(self._L.vlgba_get_covariance_method(self._h, ctypes.byref(kind)),
              "vlgba_get_covariance_method")
        return {v: k for k, v in COV_METHODS.items()}[kind.value]

    def covariance(self, scale=True, full=False, method=None, blocks=False):
        """Posterior covariance at the current parameters (vlgba_covariance:
        undamped, conditional on the fixed parameters, single rank): dict of
        cam (na, na, m) the diagonal blocks of the camera covariance, pts
        (3, 3, n) the point covariances, full (na m, na m) if ``full``, and
        sse, dof, sigma2 = sse / dof, fixed_rows, ms (camera stage, point
        kernel) and scratch_bytes.  ``scale`` multiplies the matrices by
        sigma2.  ``method`` ("dense" or "selected", see
        set_covariance_method) holds for this call only; ``full`` is the dense
        method's (VlgbaError -1001 with "selected").  ``blocks`` adds the
        co-visible blocks of the camera covariance
        (vlgba_get_covariance_blocks): blk_jk (nb, 2) camera pairs j >= k and
        blocks (nb, na, na) indexed [b, r, c], in reduced_system()'s order.
        Raises VlgbaError (-1007) when the gauge is not fixed."""
        if method is not None and method not in COV_METHODS:
            raise ValueError(f"method must be one of {sorted(COV_METHODS)}")
        prev = None
        if method is not None and method != self.get_covariance_method():
            prev = self.get_covariance_method()
            self.set_covariance_method(method)
        try:
            na, ld = self.num_a, self.num_a * self.m
            cam = np.zeros((na, na, self.m), order="F")
            pts = np.zeros((3, 3, self.n), order="F")
            S = np.zeros((ld, ld), order="F") if full else None
            info = np.zeros(8)
            check(self._L.vlgba_covariance(self._h, int(bool(scale)), _dp(cam),
                                           _dp(S) if full else None, _dp(pts), _dp(info)),
                  "vlgba_covariance")
            out = dict(cam=cam, pts=pts, sse=float(info[0]), dof=float(info[1]),
                       sigma2=float(info[2]), fixed_rows=int(info[3]),
                       ms=(float(info[4]), float(info[5])), scratch_bytes=int(info[6]))
            if full:
                out["full"] = S
            if blocks:
                nb = self.plan_info()["blocks"]
                jk = np.zeros(2 * nb, dtype=np.int32)
                blk = np.zeros(na * na * nb)
                check(self._L.vlgba_get_covariance_blocks(self._h, jk.ctypes.data_as(c_ip),
                                                          _dp(blk)),
                      "vlgba_get_covariance_blocks")
                out["blk_jk"] = jk.reshape(nb, 2)
                out["blocks"] = blk.reshape(nb, na, na).transpose(0, 2, 1)   # [b, r, c]
            return out
        finally:
            if prev is not None:
                self.set_covariance_method(prev)

    def sync(self):
        check(self._L.vlgba_sync(self._h), "vlgba_sync")

    def linearization(self):
        """Stage 1 at the current parameters: dict of U (na, na, m), eA (na, m),
        V (3, 3, n), eB (3, n) and W (na, 3, N) with observations point-major
        (points ascending, cameras ascending within a point)."""
        na, m, n, N = self.num_a, self.m, self.n, self.num_obs
        U = np.zeros((na, na, m), order="F")
        eA = np.zeros((na, m), order="F")
        V = np.zeros((3, 3, n), order="F")
        eB = np.zeros((3, n), order="F")
        W = np.zeros((na, 3, N), order="F")
        check(self._L.vlgba_get_linearization(self._h, _dp(U), _dp(eA), _dp(V), _dp(eB),
                                              _dp(W)), "vlgba_get_linearization")
        return dict(U=U, eA=eA, V=V, eB=eB, W=W)

    def set_timing(self, on=True):
        check(self._L.vlgba_set_timing(self._h, int(on)), "vlgba_set_timing")

    def kernel_ms(self, reset=True):
        """{kernel: (total ms, launches)} accumulated since the last reset over
        the passes run with set_timing(True)."""
        n = NKERNELS
        ms = np.zeros(n)
        calls = (ctypes.c_longlong * n)()
        check(self._L.vlgba_kernel_ms(self._h, _dp(ms), calls, int(reset)), "vlgba_kernel_ms")
        return {self._L.vlgba_kernel_name(k).decode(): (float(ms[k]), int(calls[k]))
                for k in range(n) if calls[k] > 0}

    PLAN_KEYS = ("obs", "points", "cameras", "num_a", "chunks", "chunk_slots",
                 "chunk_eslots", "groups", "group_slots", "group_eslots", "blocks",
                 "tiles", "cr_levels", "cr_elim", "cr_keep", "ordered", "schur_terms",
                 "blob_words", "mfma", "cr_rows", "mfma_groups", "reordered", "long_points",
                 "nd_arcs", "nd_sep_tiles", "solve_flops_factor", "solve_flops_syrk",
                 "solve_flops_back", "env_runner_runs", "vinv_fold", "camupd_fold", "pcg",
                 "solve_bytes")

    def plan_info(self):
        """Execution-plan sizes of this rank (vlgba_plan_info)."""
        n = len(self.PLAN_KEYS)
        buf = (ctypes.c_longlong * n)()
        rc = self._L.vlgba_plan_info(self._h, buf, n)
        check(min(rc, 0), "vlgba_plan_info")
        return dict(zip(self.PLAN_KEYS, [int(v) for v in buf]))

    def phase_ms(self):
        ms = np.zeros(7)
        check(self._L.vlgba_phase_ms(self._h, _dp(ms)), "vlgba_phase_ms")
        return dict(zip(["linearize", "camera_reduce", "damp_y", "schur", "assemble",
                         "cholesky_solve", "update"], ms.tolist()))


# ---------------------------------------------------------------------------
# drop-in drivers
# ---------------------------------------------------------------------------
def euclid_obs_adjuster(K, m, n, obs_pt, obs_cam, obs_x, *varargin, num_vis=0.0, device=0,
                        rank=0, world_size=1, comm_id=None, semantics="mex", loss="none",
                        loss_scale=0.0, jacobian=None, radial=False, **solver):
    """The BundleAdjuster that bundle_euclid_obs would create for this problem
    and these options (its structure only: no parameter values; ``radial``:
    the num_a = 9 model, whatever the calibration options say), so a caller
    can build it ahead of time -- the host plan of vlgba_create runs with the
    GIL released (ctypes), e.g. on a worker thread while the previous solve
    runs (incremental.py) -- and hand it to bundle_euclid_obs(adjuster=...)."""
    o = parse_options(m, n, varargin, nomex=semantics == "nomex")
    if radial:
        o["num_variableK"] = RADIAL_NVK
    ba = BundleAdjuster(K, obs_pt, obs_cam, obs_x, n, 6 + o["num_variableK"],
                        fix_structure=o["fix_structure"], fix_motion=o["fix_motion"],
                        pivot=o["pivot"] if o["fix_pivot"] else None, verbose=o["verbose"],
                        num_vis=num_vis, device=device, rank=rank, world_size=world_size,
                        comm_id=comm_id, semantics=semantics, loss=loss, loss_scale=loss_scale,
                        jacobian=jacobian, **solver)
    ba.fingerprint = _adjuster_fingerprint(K, m, n, obs_pt, obs_cam, obs_x, o, num_vis,
                                           semantics, rank, world_size, device, comm_id,
                                           loss, loss_scale, ba.get_jacobian())
    return ba


def _adjuster_fingerprint(K, m, n, obs_pt, obs_cam, obs_x, o, num_vis, semantics, rank,
                          world_size, device, comm_id, loss="none", loss_scale=0.0,
                          jacobian="fd"):
    """What a prebuilt adjuster was made for: sizes, the parsed
    options, K, a hash of the observation list, the device and the RCCL id
    -- a context built for another subset, other options, another GPU or
    another communicator with the same counts must not be used."""
    # xxh3 (~25x blake2b's speed; the growing replay fingerprints every solve's
    # observations twice, at build and at use), over the arrays' own buffers
    try:
        import xxhash
        h = xxhash.xxh3_128()
    except ImportError:
        import hashlib
        h = hashlib.blake2b(digest_size=16)
    for arr, dt in ((obs_pt, np.int32), (obs_cam, np.int32), (obs_x, np.float64),
                    (K, np.float64)):
        h.update(memoryview(np.ascontiguousarray(arr, dtype=dt)).cast("B"))
    piv = o["pivot"] if o["fix_pivot"] else None
    if piv is not None:
        h.update(np.asarray(piv, dtype=bool).tobytes())
    if comm_id is not None:
        h.update(bytes(comm_id))
    return (int(m), int(n), int(o["num_variableK"]), bool(o["fix_structure"]),
            bool(o["fix_motion"]), bool(o["fix_pivot"]), bool(o["verbose"]), float(num_vis),
            semantics, int(rank), int(world_size), int(device), comm_id is not None,
            h.hexdigest(), str(loss), float(loss_scale) if loss != "none" else 0.0,
            str(jacobian))


def bundle_euclid_obs(K, Te, w, Xe, obs_pt, obs_cam, obs_x, *varargin, num_vis=0.0, device=0,
                      rank=0, world_size=1, comm_id=None, return_stats=False,
                      semantics="mex", adjuster=None, return_covariance=False, loss="none",
                      loss_scale=0.0, jacobian=None, covariance_method=None, radial=None,
                      **solver):
    """bundle_euclid on a COO observation list (0-based point / camera ids).
    ``radial``: 2 x m initial radial coefficients (k1; k2) -- the solve then
    refines a = [w; T; f; k1; k2] per camera (num_a = 9, f from K(1,:), the
    principal point fixed, whatever 'fix_calibration' / 'fix_principal' say)
    with analytic Jacobians, and the refined 2 x m coefficients are returned as
    an extra last output.
    ``jacobian``: "fd", "analytic" or None (BundleAdjuster); a prebuilt adjuster
    must have been made in the mode asked for here (None: its own).
    ``loss`` / ``loss_scale``: the robust loss (BundleAdjuster); error_ is then
    the robust cost / num_vis, and a returned covariance is the unscaled one.
    ``solver`` keywords go to BundleAdjuster (parity, stop_rel, max_iter,
    max_iter2, lambda0, solver, ordered, schur_kernel).  ``adjuster``: a handle
    made beforehand by euclid_obs_adjuster for the same problem and options
    (or a concurrent.futures.Future of one); it is used and closed here.
    ``return_covariance`` appends BundleAdjuster.covariance() at the returned
    parameters (after the stats, when both are asked for), by
    ``covariance_method`` ("dense", "selected" or None: the adjuster's)."""
    K, Te, w, Xe = _F(K), _F(Te), _F(w), _F(Xe)
    m, n = w.shape[1], Xe.shape[1]
    nomex = semantics == "nomex"
    o = parse_options(m, n, varargin, nomex=nomex)
    if radial is not None:
        if jacobian == "fd":
            raise ValueError("radial distortion has analytic Jacobians only")
        o["num_variableK"] = RADIAL_NVK
    nvk = o["num_variableK"]
    a = pack_a(K, Te, w, nvk, radial)
    b = _F(Xe[0:3])
    if adjuster is not None:
        if solver:
            raise ValueError("bundle_euclid_obs: solver options belong to the prebuilt adjuster")
        ba = adjuster.result() if hasattr(adjuster, "result") else adjuster
        want = _adjuster_fingerprint(K, m, n, obs_pt, obs_cam, obs_x, o, num_vis, semantics,
                                     rank, world_size, device, comm_id, loss, loss_scale,
                                     jacobian if jacobian is not None else
                                     ba.get_jacobian())
        if getattr(ba, "fingerprint", None) != want:
            ba.close()
            raise ValueError("bundle_euclid_obs: the prebuilt adjuster is for another problem "
                             "or other options (make it with euclid_obs_adjuster)")
    else:
        ba = euclid_obs_adjuster(K, m, n, obs_pt, obs_cam, obs_x, *varargin, num_vis=num_vis,
                                 device=device, rank=rank, world_size=world_size,
                                 comm_id=comm_id, semantics=semantics, loss=loss,
                                 loss_scale=loss_scale, jacobian=jacobian,
                                 radial=radial is not None, **solver)
    with ba:
        ba.set_params(a, b)
        err, st = ba.run()
        a, b = ba.get_params()
        if return_covariance:
            ba.set_params(a, b)   # a linearisation of its own at the returned point
            cov = ba.covariance(scale=loss == "none", method=covariance_method)
    # Xe_(4,:): the input's (bundle_euclid.m:267) or ones (bundle_euclid_nomex.m:364)
    out = unpack(K, a, b, np.ones((1, n)) if nomex else Xe[3:4], nvk) + (err,)
    out = out + (st,) if return_stats else out
    out = out + (cov,) if return_covariance else out
    return out + (a[7:9].copy(order="F"),) if radial is not None else out


def bundle_euclid(K, Te, w, Xe, x, *varargin, device=0, return_stats=False, semantics="mex",
                  return_covariance=False, loss="none", loss_scale=0.0, covariance_method=None,
                  **solver):
    """[K_ Te_ w_ Xe_ error_] = bundle_euclid(K, Te, w, Xe, x, ...)  (bundle_euclid.m:1);
    ``loss`` / ``loss_scale``, ``covariance_method`` and ``jacobian="fd" |
    "analytic"`` and ``radial=kd0`` (among the solver keywords) as
    bundle_euclid_obs."""
    x = _F(x)
    m, n = np.shape(w)[1], x.shape[1]
    o = parse_options(m, n, varargin, x=x, nomex=semantics == "nomex")
    vis = o["visible"]
    num_vis = float(vis.sum())                                     # bundle_euclid.m:82
    pt, cam = np.nonzero(vis)                                      # point-major
    obs_x = np.stack([x[0, pt, cam], x[1, pt, cam]], axis=1)
    # re-emit the options without 'visibility' (already applied)
    rest, k = [], 0
    while k < len(varargin):
        nm = varargin[k].lower() if isinstance(varargin[k], str) else varargin[k]
        if nm == "visibility":
            k += 2
            continue
        if nm == "fix_pivot":
            rest += [varargin[k], varargin[k + 1]]
            k += 2
            continue
        rest.append(varargin[k])
        k += 1
    return bundle_euclid_obs(K, Te, w, Xe, pt, cam, obs_x, *rest, num_vis=num_vis,
                             device=device, return_stats=return_stats, semantics=semantics,
                             return_covariance=return_covariance, loss=loss,
                             loss_scale=loss_scale, covariance_method=covariance_method,
                             **solver)


def bundle_euclid_nomex(K, Te, w, Xe, x, *varargin, device=0, return_stats=False,
                        return_covariance=False, loss="none", loss_scale=0.0,
                        covariance_method=None, **solver):
    """[K_ Te_ w_ Xe_ error_] = bundle_euclid_nomex(K, Te, w, Xe, x, ...)
    (bundle_euclid_nomex.m:1): the same LM loop with the twin's semantics --
    db from every camera parameter (:268-277), no 'fix_pivot', Xe_(4,:) = 1."""
    return bundle_euclid(K, Te, w, Xe, x, *varargin, device=device,
                         return_stats=return_stats, semantics="nomex",
                         return_covariance=return_covariance, loss=loss,
                         loss_scale=loss_scale, covariance_method=covariance_method, **solver)


def _block_mode(radial, jacobian, loss, loss_scale, return_residuals):
    """(extended, jacobian kind, loss kind, scale) of the batched one-block
    entries' mode keywords: extended is False with every keyword at its default
    (the plain entry is called then, exactly as before).  jacobian None: "fd",
    or "analytic" with radial= (that model has no other)."""
    if jacobian is None:
        jacobian = "fd" if radial is None else "analytic"
    if jacobian not in JACOBIANS:
        raise ValueError(f"jacobian must be one of {sorted(JACOBIANS)}, got {jacobian!r}")
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {sorted(LOSSES)}, got {loss!r}")
    ex = radial is not None or jacobian != "fd" or loss != "none" or bool(return_residuals)
    return ex, JACOBIANS[jacobian], LOSSES[loss], float(loss_scale)


def _block_solve(name, head, head_ex, mode, x, count, N, residuals, return_stats, device,
                 max_iter, max_iter2, lambda0, stop_rel):
    """The call both batched one-block functions make: ``name`` (head..., opt, x,
    error_, ..., stats), or with mode = (True, jacobian, loss, scale) ``name``_ex
    (head_ex..., opt, jacobian, loss, scale, x, error_, ..., res, w, stats), on
    ``count`` problems with N observations in all; x (the parameters) is
    updated in place.  residuals: None, or what turns res (N x 2) and w (N) into
    the returned residuals.  Returns the outputs after the parameters:
    (errs[, stats][, residuals])."""
    ex, jac, lk, ls = mode
    cap = (max_iter if max_iter > 0 else 20) + 1
    err = np.zeros((count, cap))
    nerr = np.zeros(count, dtype=np.int32)
    opt = VlgbaOptions()
    opt.max_iter, opt.max_iter2, opt.lambda0 = int(max_iter), int(max_iter2), float(lambda0)
    opt.device, opt.stop_rel = int(device), float(stop_rel)
    st = VlgbaStats()
    tail = (_dp(x), _dp(err), cap, nerr.ctypes.data_as(c_ip))
    if not ex:
        check(getattr(lib(), name)(*head, ctypes.byref(opt), *tail, ctypes.byref(st)), name)
    else:
        res, wts = np.zeros((N, 2)), np.zeros(N)
        check(getattr(lib(), name + "_ex")(*head_ex, ctypes.byref(opt), jac, lk, ls, *tail,
                                           _dp(res) if residuals else None,
                                           _dp(wts) if residuals else None, ctypes.byref(st)),
              name + "_ex")
    out = ([err[q, : nerr[q]].copy() for q in range(count)],) + ((st,) if return_stats else ())
    return out + (residuals(res, wts),) if residuals else out


def bundle_euclid_resect(K, Te, w, Xs, xs, *varargin, device=0, max_iter=0, max_iter2=0,
                         lambda0=0.0, stop_rel=0.0, return_stats=False, radial=None,
                         jacobian=None, loss="none", loss_scale=0.0, return_residuals=False):
    """Batched one-camera refinement with the structure fixed -- the call of
    estimate_camera.m:247-253,

        [K T Omega] = bundle_euclid(K, T, Omega, X, x0, 'fix_calibration',
                                    'fix_structure', 'visibility', inlier')

    for every camera q at once on the GPU (vlgba_resect).  K (4 x c), Te, w
    (3 x c); Xs[q] the fixed points camera q sees (3 or 4 x n_q), xs[q] their
    measured image points (2 or 3 x n_q; only the inliers).  Options as
    bundle_euclid.m: 'fix_calibration' (num_a 6), 'fix_principal' (7), neither
    (10); 'fix_structure' is implied.  Returns K_, Te_, w_ and the list of
    per-camera error_ (SSE / n_q per accepted step).

    Beyond the reference (vlgba_resect_ex; with all of them at their defaults
    the call is vlgba_resect's, as before): ``radial`` = kd0 (2 x c start
    coefficients k1; k2) refines the radial-distortion camera [w; T; f; k1; k2]
    from the focal length K[0] (the calibration options do not apply; analytic
    Jacobians only) and returns the refined 2 x c coefficients as an extra last
    output; ``jacobian`` "fd" | "analytic"; ``loss`` "none" | "huber" |
    "cauchy" at ``loss_scale`` pixels (error_ is then the robust cost / n_q);
    ``return_residuals`` appends a list of (e (2 x n_q) the unweighted residuals
    x - x_hat, w (n_q) the loss's weights) at the returned parameters.  Output
    order: K_, Te_, w_, errs[, stats][, residuals][, kd_]."""
    K, Te, w = _F(K), _F(Te), _F(w)
    c = w.shape[1]
    mode = _block_mode(radial, jacobian, loss, loss_scale, return_residuals)
    o = parse_options(c, 0, varargin)
    nvk = o["num_variableK"] if radial is None else RADIAL_NVK
    na = 6 + nvk
    a = np.ascontiguousarray(pack_a(K, Te, w, nvk, radial).reshape(-1, order="F"))
    assert len(Xs) == len(xs) == c
    cnt = [np.shape(X)[1] for X in Xs]
    assert all(np.shape(x)[1] == k for x, k in zip(xs, cnt))
    ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum(cnt)]), dtype=np.int64)
    Xo = np.ascontiguousarray(np.concatenate([np.asarray(X, dtype=np.float64)[:3].T for X in Xs]
                                             if c else np.zeros((0, 3))))
    xo = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64)[:2].T for x in xs]
                                             if c else np.zeros((0, 2))))
    Kc = np.ascontiguousarray(K.reshape(-1, order="F"))
    pr = VlgbaResectProblem(c, na, ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                            _dp(Xo), _dp(xo), _dp(Kc))

    def per_camera(res, wts):
        return [(res[ptr[q]:ptr[q + 1]].T.copy(), wts[ptr[q]:ptr[q + 1]].copy())
                for q in range(c)]
    out = _block_solve("vlgba_resect", (ctypes.byref(pr),), (ctypes.byref(pr),), mode, a, c,
                       int(ptr[-1]), per_camera if return_residuals else None, return_stats,
                       device, max_iter, max_iter2, lambda0, stop_rel)
    a = a.reshape(na, c, order="F")
    K_, Te_, w_, _ = unpack(K, a, np.zeros((3, 0)), np.zeros((1, 0)), nvk)
    out = (K_, Te_, w_) + out
    if radial is not None:
        out += (a[7:9].copy(order="F"),)
    return out


def _tracks(K, Te, w, obs_ptr, obs_cam, obs_x):
    """The camera and CSR track arguments of vlgba_triangulate / vlgba_intersect
    as contiguous buffers (and the ctypes pointers to them)."""
    K, Te, w = _F(K), _F(Te), _F(w)
    m = w.shape[1]
    assert K.shape == (4, m) and Te.shape == (3, m)
    ptr = np.ascontiguousarray(obs_ptr, dtype=np.int64).reshape(-1)
    cam = np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
    ox = np.ascontiguousarray(obs_x, dtype=np.float64).reshape(-1, 2)
    assert len(ptr) >= 1 and len(cam) == len(ox) and (len(ptr) == 1 or ptr[-1] == len(cam))
    keep = (K, Te, w, ptr, cam, ox)
    args = (m, _dp(K), _dp(Te), _dp(w), len(ptr) - 1,
            ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), cam.ctypes.data_as(c_ip),
            _dp(ox))
    return keep, args


def _radial_kd(radial, m):
    """radial= of the per-point entries as a contiguous 2 x m (k1; k2) buffer"""
    kd = np.ascontiguousarray(np.asarray(radial, dtype=np.float64).reshape(2, -1).T)
    if kd.shape != (m, 2):
        raise ValueError(f"radial: expected 2 x {m} coefficients, got {np.shape(radial)}")
    return kd


def triangulate_points(K, Te, w, obs_ptr, obs_cam, obs_x, device=0, return_status=False,
                       radial=None):
    """X = triangulation(P, x) (toolbox/geometry/triangulation.m:19-53) for every
    point of a batch on the GPU (vlgba_triangulate).  K (4 x m), Te, w (3 x m):
    the pinhole cameras; point i has the views obs_ptr[i] .. obs_ptr[i+1]-1 of
    obs_cam (camera ids, any order within a point) / obs_x (N x 2 measured
    image points).  Returns X (4 x n): the point over its 4th entry, or zeros
    when a view sees it at negative depth (status 0), when it has fewer than two
    views or the result is not finite (status 2; the reference would return
    inf / nan for a point at infinity).  ``return_status``: (X, status).
    ``radial`` = kd (2 x m: k1; k2): the cameras have radial distortion with
    f = K[0]; every measurement is undistorted first (vlgba_triangulate_ex), and
    a point with a view at or past the fold of its lens gets status 2."""
    keep, args = _tracks(K, Te, w, obs_ptr, obs_cam, obs_x)
    n = args[4]
    X = np.zeros((4, n), order="F")
    status = np.zeros(n, dtype=np.int32)
    if radial is None:
        check(lib().vlgba_triangulate(*args, int(device), _dp(X), status.ctypes.data_as(c_ip)),
              "vlgba_triangulate")
    else:
        kd = _radial_kd(radial, args[0])
        check(lib().vlgba_triangulate_ex(*args[:4], _dp(kd), *args[4:], int(device), _dp(X),
                                         status.ctypes.data_as(c_ip)), "vlgba_triangulate_ex")
    return (X, status) if return_status else X


def bundle_euclid_intersect(K, Te, w, X, obs_ptr, obs_cam, obs_x, device=0, max_iter=0,
                            max_iter2=0, lambda0=0.0, stop_rel=0.0, return_stats=False,
                            radial=None, jacobian=None, loss="none", loss_scale=0.0,
                            return_residuals=False):
    """Batched one-point refinement with the motion fixed --

        [~, ~, ~, X_i] = bundle_euclid(K, T, Omega, X_i, x_i, 'fix_calibration',
                                       'fix_motion', 'visibility', ones(1, k))

    for every point i at once on the GPU (vlgba_intersect), each point with its
    own lambda: the mirror image of bundle_euclid_resect.  Cameras and tracks as
    triangulate_points; X (3 or 4 x n) the start points.  Returns X_ (the same
    row count; a 4th row is passed through) and the list of per-point error_
    (SSE / views per accepted step; empty for a point without views, which is
    left untouched).

    Beyond the reference (vlgba_intersect_ex; with all of them at their
    defaults the call is vlgba_intersect's, as before): ``radial`` = kd (2 x m)
    as triangulate_points, ``jacobian``, ``loss`` / ``loss_scale`` and
    ``return_residuals`` as bundle_euclid_resect; the residuals are one pair
    (e (N x 2), w (N)) in the order of obs_x, appended last."""
    mode = _block_mode(radial, jacobian, loss, loss_scale, return_residuals)
    keep, args = _tracks(K, Te, w, obs_ptr, obs_cam, obs_x)
    n = args[4]
    X = np.asarray(X, dtype=np.float64)
    assert X.shape[0] in (3, 4) and X.shape[1] == n
    b = np.ascontiguousarray(X[:3].T).reshape(-1)      # 3 x n column major
    kd = None if radial is None else _radial_kd(radial, args[0])
    out = _block_solve("vlgba_intersect", args,
                       args[:4] + (None if kd is None else _dp(kd),) + args[4:], mode, b, n,
                       len(keep[4]), (lambda res, wts: (res, wts)) if return_residuals else None,
                       return_stats, device, max_iter, max_iter2, lambda0, stop_rel)
    X_ = np.array(X, order="F")
    X_[:3] = b.reshape(n, 3).T
    return (X_,) + out


# ---------------------------------------------------------------------------
# MEX stage mirrors (exact argument layouts of the reference MEX files)
# ---------------------------------------------------------------------------
def mex_bundle_1_XABeUVWeAeB(K, a, b, X, visible):
    """[X_hat A B e U V W eA eB] = mex_bundle_1_XABeUVWeAeB(K, a, b, X, visible)."""
    K, a, b, X, vis = map(_F, (K, a, b, X, visible))
    num_a, m = a.shape
    n = b.shape[1]
    z = lambda *s: np.zeros(s, order="F")
    out = [z(2, n, m), z(2, num_a, n, m), z(2, 3, n, m), z(2, n, m), z(num_a, num_a, m),
           z(3, 3, n), z(num_a, 3, n, m), z(num_a, m), z(3, n)]
    check(lib().vlgba_mex_bundle_1(m, n, num_a, _dp(K), _dp(a), _dp(b), _dp(X), _dp(vis),
                                   *[_dp(q) for q in out]), "mex_bundle_1_XABeUVWeAeB")
    return tuple(out)


def mex_bundle_2_Se_(Y, W, U, eA, eB):
    """[S e_] = mex_bundle_2_Se_(Y, W, U, eA, eB)."""
    Y, W, U, eA, eB = map(_F, (Y, W, U, eA, eB))
    num_a, m = eA.shape
    n = eB.shape[1]
    S = np.zeros((num_a * m, num_a * m), order="F")
    e_ = np.zeros((num_a * m, 1), order="F")
    check(lib().vlgba_mex_bundle_2(m, n, num_a, _dp(Y), _dp(W), _dp(U), _dp(eA), _dp(eB),
                                   _dp(S), _dp(e_)), "mex_bundle_2_Se_")
    return S, e_


def mex_bundle_3_db_new(W, da, eB, V_inv, K, a, b, X, visible):
    """[db a_new b_new X_hat] = mex_bundle_3_db_new(W, da, eB, V_inv, K, a, b, X, visible)."""
    W, da, eB, Vinv, K, a, b, X, vis = map(_F, (W, da, eB, V_inv, K, a, b, X, visible))
    num_a, m = a.shape
    n = b.shape[1]
    db = np.zeros((3, n), order="F")
    a_new = np.zeros((num_a, m), order="F")
    b_new = np.zeros((3, n), order="F")
    X_hat = np.zeros((2, n, m), order="F")
    check(lib().vlgba_mex_bundle_3(m, n, num_a, _dp(W), _dp(da), _dp(eB), _dp(Vinv), _dp(K),
                                   _dp(a), _dp(b), _dp(X), _dp(vis), _dp(db), _dp(a_new),
                                   _dp(b_new), _dp(X_hat)), "mex_bundle_3_db_new")
    return db, a_new, b_new, X_hat
