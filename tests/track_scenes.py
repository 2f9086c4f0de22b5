"""Scenes with planted tracks of chosen lengths -- TEST INFRASTRUCTURE ONLY (a
plain helper module like scene_ref.py; tests/test_track_scenes.py checks what
it promises from the arrays alone).

The base is make_config("ladybug", max_track=30, long_frac=0): cameras drive
round a circle of RADIUS looking at its centre, every base track has at most 30
views (+ up to 3 loop-closure views).  A landmark within 0.1 RADIUS of the
centre is in front of every camera, so ANY camera list is a valid track: a
track's length, and which cameras share it, are chosen and not drawn.

    planted(m, base_n, tracks, seed)  one landmark per camera list
    ladder(na, top, m=280)
                      two landmarks (a window of consecutive cameras, a random
                      camera set) of every length on a threshold of the fast
                      path: BA_MF_CMAX(na) and + 1 (MFMA | per-term chunk), 8 |
                      9 and 32 | 33 (k_point_cov's bins), 90 | 91 (per-term |
                      long by the term cap), 128 | 129 (one | two segments),
                      256 | 257 (two | three segments, k_long_db's second
                      trip), and top, the longest
    shared(C)         C landmarks that all see cameras 0..89 and some of 90..99:
                      long-observation lists of exactly C, C pairs per block
"""
import functools

import numpy as np

RADIUS = 150.0
CMAX = {6: 8, 7: 9, 9: 7, 10: 6, 12: 5}   # BA_MF_CMAX(na), ba_limits.h
CH_OBS, CH_TERMS = 128, 4096           # BA_CH_OBS, BA_CH_TERMS


def is_long(k):
    """track_kind(k) == 2 (ba_plan.cpp): more than a per-term chunk holds."""
    k = np.asarray(k, dtype=np.int64)
    return (k > CH_OBS) | (k * (k + 1) // 2 > CH_TERMS)


def planted(m, base_n, tracks, seed):
    """The base scene of m cameras and base_n points with one landmark per
    entry of ``tracks`` (an ascending camera list) appended as points base_n,
    base_n + 1, ...  Returns (sc, pt, cam, ox), point-major with cameras
    ascending within a point; sc is the Scene WITH the landmarks (X, X0, n and
    the observation arrays), sc.base_n the number of base points."""
    from bundleadjustmentmatlab_amd.scene import Scene, make_config, project
    base = make_config("ladybug", m=m, n=base_n, max_track=30, long_frac=0.0, radius=RADIUS,
                       seed=seed)
    rng = np.random.default_rng([seed, 7])
    nl = len(tracks)
    lm = np.vstack([rng.uniform(-0.1 * RADIUS, 0.1 * RADIUS, size=(3, nl)), np.ones((1, nl))])
    lcam = np.concatenate([np.asarray(t, dtype=np.int64) for t in tracks])
    llen = np.array([len(t) for t in tracks])
    for t in tracks:
        t = np.asarray(t)
        assert len(t) >= 1 and t[0] >= 0 and t[-1] < m and np.all(np.diff(t) > 0), "camera list"
    X = np.hstack([base.X, lm])
    lpt = base_n + np.repeat(np.arange(nl), llen)
    lx, z = project(base.K, base.w, base.T, X, lcam, lpt)
    assert np.all(z > 0), "a landmark behind one of its cameras"
    lx = lx + rng.standard_normal(lx.shape) * 0.5          # the scene's noise (pixels)
    X0 = np.hstack([base.X0, lm])
    X0[:3, base_n:] += rng.standard_normal((3, nl)) * 1e-3   # scene._perturb
    pt = np.r_[base.obs_pt, lpt].astype(np.int32)
    cam = np.r_[base.obs_cam, lcam].astype(np.int32)
    ox = np.ascontiguousarray(np.vstack([base.obs_x, lx]))
    # base points come first and each landmark's cameras ascend: already point-major
    assert np.all((np.diff(pt) > 0) | ((np.diff(pt) == 0) & (np.diff(cam) > 0)))
    sc = Scene(base.K, base.T, base.w, X, pt, cam, ox, base.T0, base.w0, X0)
    sc.base_n = base_n
    return sc, pt, cam, ox


def ladder_lengths(na, top):
    return sorted({CMAX[na], CMAX[na] + 1, 8, 9, 32, 33, 90, 91, 128, 129, 256, 257, top})


@functools.lru_cache(maxsize=None)
def ladder(na, top, m=280):
    """m cameras, 400 base points, two landmarks of every length of
    ladder_lengths(na, top): a window of consecutive cameras at a random start
    and a random camera set of the same size (a window cut in two segments
    shares its cameras with its neighbours' tracks, a random set does not)."""
    base_n = 400
    assert 257 <= top <= m
    rng = np.random.default_rng([na, top])
    tracks = []
    for k in ladder_lengths(na, top):
        s = int(rng.integers(0, m - k + 1))
        tracks.append(np.arange(s, s + k))
        tracks.append(np.sort(rng.choice(m, size=k, replace=False)))
    return planted(m, base_n, tracks, seed=100 + na)


@functools.lru_cache(maxsize=None)
def shared(C):
    """m = 100, 300 base points, C landmarks: each sees cameras 0..89 and each
    of cameras 90..99 with probability 1 / 2 (at least one), so 91..100 views:
    long by the term cap, one segment."""
    m, base_n = 100, 300
    rng = np.random.default_rng([C, 11])
    tracks = []
    for _ in range(C):
        tail = rng.random(10) < 0.5
        if not tail.any():
            tail[rng.integers(0, 10)] = True
        tracks.append(np.r_[np.arange(90), 90 + np.flatnonzero(tail)])
    return planted(m, base_n, tracks, seed=200 + C)


def track_lengths(sc, pt):
    """(lengths of the base points, lengths of the planted landmarks)."""
    L = np.bincount(pt, minlength=sc.n)
    return L[:sc.base_n], L[sc.base_n:]
