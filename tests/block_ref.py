"""One-block references of the batched entries with a model, a Jacobian mode
and a loss (vlgba_resect_ex, vlgba_intersect_ex, vlgba_triangulate_ex) -- TEST
INFRASTRUCTURE ONLY, in the style of jac_ref.py / radial_ref.py / robust_ref.py,
from whose functions everything here is built:

    jac_ref     jacobians (num_a 6 / 7 / 10), project (the true projection, for
                central differences), linearization, table_rotation, E
    radial_ref  jacobians, residuals, cost, linearization (num_a 9)
    robust_ref  loss, weighted (the weighted sums and the fix masks)

A problem is a dict (``camera`` / ``point`` below) that holds one camera and
the fixed points it sees (m = 1, the mask fix_structure: the block is U, eA) or
one point and the fixed cameras that see it (n = 1, fix_motion: V, eB), as the
observation list (pt, cam) those functions take.

Residuals of the pinhole models.  radial_ref.residuals gives the radial model's
kernel-order residuals with their bound; ``residuals`` restates the pinhole
projection the same way, operation by operation in the kernel's order
(vlg_project_h: x = (fx Xc0 + 0 Xc1 + cx Xc2) / Xc2 on the table's R(w)), on
jac_ref's (value, bound) arithmetic, so that R = I below |w| = 1e-6 and every
fp64 rounding is in the bound.

``block_lm`` is a dense NA x NA (or 3 x 3) LM with the reference's LM and stop
rules (bundle_euclid.m:117-123, 205-249), as radial_ref.radial_lm: an exactly
zero row of the block is fixed (pinv rule), the block is damped on its diagonal
by (1 + lambda), the gain ratio uses dp'(lambda dp + g) with the (robust)
gradient g.

``undistort_mp`` restates the undistortion of vlgba_triangulate_ex in mpmath.
"""
import numpy as np

import jac_ref as jr
import radial_ref as rad
import robust_ref as rr

LD = jr.LD
E = jr.E
U53 = jr.U53
UNDIST_ITERS = 20            # TRI_UNDIST_ITERS
UNDIST_TOL = 2.0 ** -49      # TRI_UNDIST_TOL


def camera(K4, a, Xw, x):
    """One camera a (na,) with K4 (4,) seeing the fixed points Xw (3, N) at x
    (N, 2): the problem dict."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 1)
    N = np.shape(Xw)[1]
    return dict(which="camera", na=a.shape[0], K=np.asarray(K4, dtype=np.float64).reshape(4, 1),
                a=a.copy(order="F"), b=np.array(np.asarray(Xw)[:3], dtype=np.float64, order="F"),
                pt=np.arange(N, dtype=np.int64), cam=np.zeros(N, dtype=np.int64),
                obs_x=np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(N, 2)),
                m=1, n=N, masks=dict(fix_structure=True))


def point(K, a, X, cams, x):
    """One point X (3,) seen by the fixed cameras a (na, m), K (4, m) with ids
    ``cams`` (views in that order) at x (k, 2)."""
    a = np.array(a, dtype=np.float64, order="F")
    cams = np.asarray(cams, dtype=np.int64)
    return dict(which="point", na=a.shape[0], K=np.array(K, dtype=np.float64, order="F"), a=a,
                b=np.asarray(X, dtype=np.float64).reshape(3, 1).copy(order="F"),
                pt=np.zeros(len(cams), dtype=np.int64), cam=cams,
                obs_x=np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(len(cams), 2)),
                m=a.shape[1], n=1, masks=dict(fix_motion=True))


def radial_cameras(K, T, w, kd):
    """(K, a (9, m)) of the per-point entries' radial cameras: f = K[0]."""
    return np.asarray(K, dtype=np.float64), rad.pack(K, w, T, kd)


def pinhole_cameras(K, T, w):
    """(K, a (6, m)) of the per-point entries' pinhole cameras."""
    a = np.zeros((6, np.shape(w)[1]), order="F")
    a[0:3], a[3:6] = w, T
    return np.asarray(K, dtype=np.float64), a


def free(P):
    """the free parameter vector of the problem (a copy)"""
    return (P["a"][:, 0] if P["which"] == "camera" else P["b"][:, 0]).copy()


def with_free(P, x):
    """(a, b) of the problem with its free parameters replaced by x"""
    a, b = P["a"].copy(order="F"), P["b"].copy(order="F")
    if P["which"] == "camera":
        a[:, 0] = x
    else:
        b[:, 0] = x
    return a, b


def _project_pinhole(K, a, b, pt, cam, na):
    """(x (N, 2), bound): the kernel's pinhole projection on E arithmetic."""
    a, b, K = (np.asarray(q, dtype=np.float64) for q in (a, b, K))
    Rm, Rmb = jr.table_rotation(a[0:3])
    R = [[E(Rm[r, c, cam], Rmb[r, c, cam]) for c in range(3)] for r in range(3)]
    bo = [E(b[k, pt]) for k in range(3)]
    T = [E(a[3 + k, cam]) for k in range(3)]
    Xc = [((R[r][0] * bo[0] + R[r][1] * bo[1]) + R[r][2] * bo[2]) + T[r] for r in range(3)]
    fx, fy = (E(q) for q in jr._focal(K, a, na, cam))
    cx, cy = (E(a[8, cam]), E(a[9, cam])) if na == 10 else (E(K[2, cam]), E(K[3, cam]))
    # Kc (S + t), the zero entries of Kc as exact products (no rounding counted
    # for them: x + 0 is exact), then the division
    x0 = (fx * Xc[0] + cx * Xc[2]) / Xc[2]
    x1 = (fy * Xc[1] + cy * Xc[2]) / Xc[2]
    return np.stack([x0.v, x1.v], 1), np.stack([x0.e, x1.e], 1)


def residuals(P, a=None, b=None):
    """(e (N, 2) long double, bound) of e = x_obs - x at (a, b) (default: the
    problem's own), the kernel's evaluation with every rounding bounded."""
    a = P["a"] if a is None else a
    b = P["b"] if b is None else b
    if P["na"] == rad.NA:
        return rad.residuals(P["K"], a, b, P["pt"], P["cam"], P["obs_x"])
    x, xb = _project_pinhole(P["K"], a, b, P["pt"], P["cam"], P["na"])
    e = P["obs_x"].astype(LD) - x
    return e, xb + U53 * np.abs(e)


def cost(P, a=None, b=None, kind="none", c=1.0):
    """(robust cost sum rho(s), bound of an fp64 evaluation in any order)."""
    e, eb = residuals(P, a, b)
    s = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
    w, rho, mag = rr.loss(kind, c, s)
    N = len(e)
    # d rho = w ds, ds = 2 |e| de; then the loss's own roundings and the sum's
    prop = (w * (2 * np.abs(e) * eb + eb * eb).sum(1)).sum()
    return rho.sum(), prop + (max(N, 1) - 1 + rr.KRHO + 2) * U53 * mag.sum()


def _rodrigues64(w):
    """vlg_rodrigues in fp64, operation for operation, with libm's sin / cos
    (math.sin / math.cos: the device's are glibc's bit for bit)"""
    import math
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if th < 1e-6:
        return np.eye(3)
    x, y, z = w[0] / th, w[1] / th, w[2] / th
    xx, xy, xz, yy, yz, zz = x * x, x * y, x * z, y * y, y * z, z * z
    s, c = math.sin(th), math.cos(th)
    mc = 1.0 - c
    return np.array([[1 - mc * (yy + zz), -s * z + mc * xy, s * y + mc * xz],
                     [s * z + mc * xy, 1 - mc * (zz + xx), -s * x + mc * yz],
                     [-s * y + mc * xz, s * x + mc * yz, 1 - mc * (xx + yy)]])


def cost_fp64(P, a=None, b=None, kind="none", c=1.0):
    """The CPU cost in plain fp64: the kernels' projection (vlg_project /
    vlg_project_radial on vlg_rodrigues' R) and their cost sum restated operation
    for operation and in their order, so that it agrees with the device's to the
    last bits whatever the size of the residuals (the long double ``cost`` does
    not: its residuals differ from the device's by their rounding bound, which
    a near-zero residual does not forgive).  -> float"""
    import math
    a = np.asarray(P["a"] if a is None else a, dtype=np.float64)
    b = np.asarray(P["b"] if b is None else b, dtype=np.float64)
    K, pt, cam, na = P["K"], P["pt"], P["cam"], P["na"]
    R = np.stack([_rodrigues64(a[0:3, j]) for j in range(a.shape[1])], 2)[:, :, cam]
    bo = b[:, pt]
    Xc = [((R[r, 0] * bo[0] + R[r, 1] * bo[1]) + R[r, 2] * bo[2]) + a[3 + r, cam] for r in range(3)]
    if na == rad.NA:
        u, v = Xc[0] / Xc[2], Xc[1] / Xc[2]
        q = u * u + v * v
        d = (1.0 + a[7, cam] * q) + (a[8, cam] * q) * q
        x0 = a[6, cam] * (d * u) + K[2, cam]
        x1 = a[6, cam] * (d * v) + K[3, cam]
    else:
        fx, fy = jr._focal(K, a, na, cam)
        cx, cy = (a[8, cam], a[9, cam]) if na == 10 else (K[2, cam], K[3, cam])
        x0 = (fx * Xc[0] + cx * Xc[2]) / Xc[2]
        x1 = (fy * Xc[1] + cy * Xc[2]) / Xc[2]
    e0, e1 = P["obs_x"][:, 0] - x0, P["obs_x"][:, 1] - x1
    kind = rr.KINDS.get(kind, kind)
    c2 = float(c) * float(c)
    acc = 0.0
    for p, q in zip(e0.tolist(), e1.tolist()):
        s = p * p + q * q
        if kind == 0 or (kind == 1 and s <= c2):
            acc = acc + p * p
            acc = acc + q * q
        elif kind == 1:
            acc = acc + (2.0 * c * math.sqrt(s) - c2)
        else:
            acc = acc + c2 * math.log1p(s / c2)
    return acc


def weights(P, a=None, b=None, kind="none", c=1.0):
    """(w (N,), bound): the loss's weights, robust_ref's rounding bound plus the
    residuals' bound through |dw/ds| <= w / max(s, c^2) (both losses)."""
    e, eb = residuals(P, a, b)
    s = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
    w = rr.loss(kind, c, s)[0]
    ds = (2 * np.abs(e) * eb + eb * eb).sum(1)
    return w, (2 * rr.KW + 1) * U53 * w + w * ds / np.maximum(s, LD(c) * LD(c))


def jacobians(P, a=None, b=None):
    a = P["a"] if a is None else a
    b = P["b"] if b is None else b
    if P["na"] == rad.NA:
        return rad.jacobians(P["K"], a, b, P["pt"], P["cam"])
    return jr.jacobians(P["K"], a, b, P["pt"], P["cam"], P["na"])


def linearization(P, a=None, b=None, kind="none", c=1.0):
    """The weighted normal equations of the problem at (a, b) from the fp64
    residuals, with bounds: jac_ref.linearization (pinhole, no loss),
    radial_ref.linearization (radial) -- and for a pinhole model under a loss
    radial_ref.linearization's propagation restated on jac_ref.jacobians.  The
    block is R["U"][:, :, 0], R["eA"][:, 0] (camera) or R["V"][:, :, 0],
    R["eB"][:, 0] (point); the other blocks are masked to exact zeros."""
    a = P["a"] if a is None else a
    b = P["b"] if b is None else b
    eo = np.asarray(residuals(P, a, b)[0], dtype=np.float64)
    args = (P["K"], a, b, P["pt"], P["cam"], eo, P["m"], P["n"])
    if P["na"] == rad.NA:
        return rad.linearization(*args, kind=kind, c=c, **P["masks"])
    if rr.KINDS.get(kind, kind) == 0:
        R = jr.linearization(*args, P["na"], **P["masks"])
        s = eo.astype(LD)
        R["cost"] = (s * s).sum()
        return R
    Ao, Bo, Ab, Bb = jr.jacobians(P["K"], a, b, P["pt"], P["cam"], P["na"])
    Ab = Ab + U53 * np.abs(Ao)
    Bb = Bb + U53 * np.abs(Bo)
    m, n, na, pt, cam = P["m"], P["n"], P["na"], P["pt"], P["cam"]
    R = rr.weighted(m, n, na, pt, cam, Ao, Bo, eo, kind, c, **P["masks"])
    Pm = rr.weighted(m, n, na, pt, cam, np.ones_like(Ao), np.ones_like(Bo), np.ones_like(eo),
                     "none", 1.0, **P["masks"])
    eabs = np.abs(eo.astype(LD))[:, :, None]
    aA, aB = np.abs(Ao), np.abs(Bo)
    w = np.asarray(R["w"], dtype=LD)[:, None, None]
    gs = rr._group_sum
    ein = lambda x, y: w * np.einsum("okr,okc->orc", x, y)
    extra = dict(U=gs(ein(aA, Ab) + ein(Ab, aA), cam, m).transpose(1, 2, 0),
                 eA=gs(ein(Ab, eabs), cam, m)[:, :, 0].T,
                 V=gs(ein(aB, Bb) + ein(Bb, aB), pt, n).transpose(1, 2, 0),
                 eB=gs(ein(Bb, eabs), pt, n)[:, :, 0].T)
    for k, x in extra.items():
        masked = np.asarray(Pm[k], dtype=LD) == 0
        R[k + "_b"] = np.where(masked, 0, R[k + "_b"] + x)
    return R


def block(P, R):
    """(H, g, bound of H, bound of g) of the problem's block out of a
    linearization R, long double."""
    if P["which"] == "camera":
        return R["U"][:, :, 0], R["eA"][:, 0], R["U_b"][:, :, 0], R["eA_b"][:, 0]
    return R["V"][:, :, 0], R["eB"][:, 0], R["V_b"][:, :, 0], R["eB_b"][:, 0]


def damped(H, lam):
    """H with its diagonal times (1 + lambda) (bundle_euclid.m:162-173)."""
    Hs = np.array(H, copy=True)
    k = np.arange(Hs.shape[0])
    Hs[k, k] = Hs[k, k] * (1 + lam)
    return Hs


def block_lm(P, kind="none", c=1.0, *, stop_rel=1e-3, max_iter=20, max_iter2=10, lambda0=1e-3,
             trace=None):
    """Dense LM on the problem's free parameters from its start: (x, error_)
    with error_ = (robust) cost / views per accepted step."""
    x = free(P)
    num_vis = float(len(P["pt"]))
    lam, nu = lambda0, 2.0
    it, it2 = 1, 0
    err = []
    f64 = lambda q: np.asarray(q, dtype=np.float64)

    def cont():
        if not (it < max_iter and it2 < max_iter2):
            return False
        if it < 3:
            return True
        return err[it - 1] > 1e-20 and err[it - 2] - err[it - 1] > stop_rel * err[it - 2]

    lin = None
    while cont():
        if lin is None:
            a, b = with_free(P, x)
            eo = f64(residuals(P, a, b)[0])
            Ao, Bo, _, _ = jacobians(P, a, b)
            R = rr.weighted(P["m"], P["n"], P["na"], P["pt"], P["cam"], Ao, Bo, eo, kind, c,
                            **P["masks"])
            H, g, _, _ = block(P, R)
            lin = (f64(H), f64(g), float(R["cost"]))
        H, g, old_cost = lin
        Hs = damped(H, lam)
        fixed = np.diag(Hs) == 0
        Hs[fixed, :] = 0
        Hs[:, fixed] = 0
        Hs[fixed, fixed] = 1
        rhs = np.where(fixed, 0.0, g)
        dx = np.linalg.pinv(Hs, hermitian=True) @ rhs if len(x) == 3 else np.linalg.solve(Hs, rhs)
        x_new = x + dx
        new_cost = float(cost(P, *with_free(P, x_new), kind, c)[0])
        rho = (old_cost - new_cost) / float(dx @ (lam * dx + g))
        accepted = (old_cost - new_cost) > 0
        if trace is not None:
            trace.append(dict(lam=lam, accepted=bool(accepted), old=old_cost, new=new_cost,
                              rho=rho, dx=dx.copy()))
        if accepted:
            x = x_new
            lin = None
            lam = lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)
            nu = 2.0
            if len(err) < it:
                err.append(old_cost / num_vis)
            else:
                err[it - 1] = old_cost / num_vis
            it += 1
            err.append(new_cost / num_vis)
            it2 = 0
        else:
            lam = lam * nu
            nu = 2.0 * nu
            it2 += 1
    return x, np.array(err)


def true_cost(P, x, kind="none", c=1.0):
    """The robust cost at free parameters x (long double) from the TRUE
    projection (jac_ref.project / radial_ref.project_true: no R = I rule), for
    central differences."""
    a, b = P["a"].astype(LD), P["b"].astype(LD)
    if P["which"] == "camera":
        a[:, 0] = x
    else:
        b[:, 0] = x
    if P["na"] == rad.NA:
        xh = rad.project_true(P["K"], a, b, P["pt"], P["cam"])
    else:
        xh = jr.project(P["K"], a, b, P["pt"], P["cam"], P["na"])
    e = P["obs_x"].astype(LD) - xh
    return rr.loss(kind, c, e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])[1].sum()


def gradient_cd(P, x, kind="none", c=1.0, h=1e-6):
    """d cost / d x by long double central differences of true_cost; the step
    of parameter k is h max(1, |x_k|)."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    g = np.zeros(len(x), dtype=LD)
    for k in range(len(x)):
        hk = LD(h) * max(LD(1), abs(x[k]))
        xp, xm = x.copy(), x.copy()
        xp[k] += hk
        xm[k] -= hk
        g[k] = (true_cost(P, xp, kind, c) - true_cost(P, xm, kind, c)) / (2 * hk)
    return g


# ---------------------------------------------------------------------------
# seeded scenes of tests/test_block_ref.py and tests/test_gpu_block_model.py
# ---------------------------------------------------------------------------
NOISE = 0.5
K_START = (0.9, 1.2)         # the start's coefficients as multiples of the truth
K4 = {6: (800.0, 800.0, 500.0, 400.0), 7: (800.0, 800.0, 500.0, 400.0),
      9: (800.0, 800.0, 500.0, 400.0), 10: (800.0, 790.0, 500.0, 400.0)}


def _true_a(na, w, T, K4_, kd=rad.K_TRUE):
    a = np.zeros((na, 1))
    a[0:3, 0], a[3:6, 0] = w, T
    if na == 7:
        a[6, 0] = K4_[0]
    elif na == 10:
        a[6:10, 0] = K4_
    elif na == 9:
        a[6, 0], a[7:9, 0] = K4_[0], kd
    return a


def _observe(na, K, a, X, pt, cam, noise, seed):
    """fp64 observations of the true scene plus seeded Gaussian noise"""
    if na == rad.NA:
        return rad.observe(K, a, X, pt, cam, noise, seed)
    x = jr.project(K, a, np.asarray(X)[0:3], pt, cam, na).astype(np.float64)
    return np.ascontiguousarray(x + np.random.default_rng(seed).standard_normal(x.shape) * noise)


def synth_camera(N, seed, na, noise=NOISE, w0_zero=False):
    """One resection problem: a camera of model na with a seeded true pose, N
    points 4 .. 8 units in front of it that fill the image out to |n| = 0.7
    (the lens K_TRUE at na = 9), 0.5 px noise; the start is a DLT-like pose
    (rotation 2e-3, translation 2e-2 off; ``w0_zero``: the true and the start
    rotation are 0 and 0.02 rad apart, the start at exactly w = 0), the focal
    lengths 1 % off and the coefficients at K_START times the truth.
    -> (problem dict at the start, a_true (na,))"""
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 0.3, 3)
    if w0_zero:
        w = 0.02 * w / np.linalg.norm(w)
    T = np.array([rng.normal(0, 0.5), rng.normal(0, 0.5), rng.normal(0, 0.2)])
    z = rng.uniform(4, 8, N)
    uv = rng.uniform(-0.5, 0.5, (2, N))
    Xc = np.stack([uv[0] * z, uv[1] * z, z])
    R = np.asarray(jr.rodrigues(w.reshape(3, 1))[:, :, 0], dtype=np.float64)
    X = R.T @ (Xc - T[:, None])
    k4 = np.array(K4[na])
    a_true = _true_a(na, w, T, k4)
    pt, cam = np.arange(N), np.zeros(N, dtype=np.int64)
    x = _observe(na, k4.reshape(4, 1), a_true, X, pt, cam, noise, seed + 200)
    a0 = a_true.copy()
    a0[0:3, 0] = 0.0 if w0_zero else w + rng.normal(0, 2e-3, 3)
    a0[3:6, 0] = T + rng.normal(0, 2e-2, 3)
    if na == 7:
        a0[6, 0] *= 1.01
    elif na == 10:
        a0[6:8, 0] *= 1.01
    elif na == 9:
        a0[6, 0] *= 1.01
        a0[7:9, 0] = np.array(rad.K_TRUE) * np.array(K_START)
    return camera(k4, a0[:, 0], X, x), a_true[:, 0]


def synth_tracks(views, seed, radial, m=9, noise=NOISE, offset=0.05):
    """A batch of one-point problems: m cameras on a ring of radius 6 that look
    at the origin (pinhole, or with the lens K_TRUE), one point per entry of
    ``views`` (its track length; the views are the first cameras of a seeded
    permutation) in the unit cube around the origin, 0.5 px noise, the start
    ``offset`` off the truth.  -> dict K (4, m), T, w (3, m), kd (2, m) or None,
    ptr, cam, x (N, 2), X0, X_true (3, n)"""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(m) / m
    # R_y(ang) turns the optical axis to (-sin ang, 0, cos ang): towards the origin
    w = np.stack([0.1 * np.cos(3 * ang), np.where(ang > np.pi, ang - 2 * np.pi, ang),
                  0.1 * np.sin(2 * ang)])
    w[:, 0] = 0.0   # one camera at w = 0 exactly (R = I, the generators)
    R = np.asarray(jr.rodrigues(w), dtype=np.float64)              # (3, 3, m)
    C = np.stack([6 * np.sin(ang), 0.3 * np.cos(ang), -6 * np.cos(ang)])
    C[:, 0] = (0.0, 0.0, -6.0)
    T = -np.einsum("ijm,jm->im", R, C)
    K = np.tile(np.array(K4[9])[:, None], (1, m))
    kd = np.tile(np.array(rad.K_TRUE)[:, None], (1, m)) if radial else None
    n = len(views)
    X = rng.uniform(-1, 1, (3, n))
    ptr = np.concatenate([[0], np.cumsum(views)]).astype(np.int64)
    cam = np.concatenate([rng.permutation(m)[:k] for k in views] + [np.zeros(0, dtype=int)])
    cam = cam.astype(np.int32)
    pt = np.repeat(np.arange(n), views)
    if radial:
        x = rad.observe(K, rad.pack(K, w, T, kd), X, pt, cam, noise, seed + 200)
    else:
        x = _observe(6, K, pinhole_cameras(K, T, w)[1], X, pt, cam, noise, seed + 200)
    X0 = X + rng.normal(0, offset, X.shape)
    return dict(K=K, T=np.asfortranarray(T), w=np.asfortranarray(w), kd=kd, ptr=ptr, cam=cam,
                x=np.ascontiguousarray(x.reshape(-1, 2)), X0=np.asfortranarray(X0),
                X_true=X, m=m, n=n)


def track_point(s, i, X=None):
    """the problem dict of point i of a synth_tracks batch (start X, default its
    own start)"""
    sl = slice(s["ptr"][i], s["ptr"][i + 1])
    K, a = (radial_cameras(s["K"], s["T"], s["w"], s["kd"]) if s["kd"] is not None
            else pinhole_cameras(s["K"], s["T"], s["w"]))
    return point(K, a, s["X0"][:, i] if X is None else X, s["cam"][sl], s["x"][sl])


# ---------------------------------------------------------------------------
# the undistortion of vlgba_triangulate_ex
# ---------------------------------------------------------------------------
def undistort_mp(f, c, k1, k2, x, digits=40):
    """The pinhole pixel f n + c of the measurement x under the lens (f, k1, k2,
    principal point c) in mpmath, or None when the view fails: nd = (x - c) / f,
    rd = |nd|, r (1 + k1 r^2 + k2 r^4) = rd by Newton from r = rd (at most
    UNDIST_ITERS updates, settled when an update is within UNDIST_TOL |r|; the
    derivative 1 + 3 k1 r^2 + 5 k2 r^4 must stay positive), n = nd r / rd."""
    import mpmath as mp
    with mp.workdps(digits):
        f, k1, k2 = mp.mpf(float(f)), mp.mpf(float(k1)), mp.mpf(float(k2))
        nd = [(mp.mpf(float(x[k])) - mp.mpf(float(c[k]))) / f for k in range(2)]
        rd = mp.sqrt(nd[0] ** 2 + nd[1] ** 2)
        if rd == 0:
            return np.array([float(c[0]), float(c[1])])
        r, ok = rd, False
        dg = lambda r: 1 + 3 * k1 * r ** 2 + 5 * k2 * r ** 4
        for _ in range(UNDIST_ITERS):
            if dg(r) <= 0:
                return None
            dr = (r * (1 + k1 * r ** 2 + k2 * r ** 4) - rd) / dg(r)
            r = r - dr
            if abs(dr) <= UNDIST_TOL * abs(r):
                ok = True
                break
        if not ok or dg(r) <= 0 or r <= 0:
            return None
        return np.array([float(f * nd[k] * r / rd + mp.mpf(float(c[k]))) for k in range(2)])


def undistort_r_mp(k1, k2, rd, digits=40):
    """r with r (1 + k1 r^2 + k2 r^4) = rd as undistort_mp finds it (f = 1, c = 0,
    the measurement on the first axis) -> mpf, or None."""
    import mpmath as mp
    with mp.workdps(digits):
        u = undistort_mp(1.0, (0.0, 0.0), k1, k2, (rd, 0.0), digits)
        return None if u is None else mp.mpf(float(u[0]))
