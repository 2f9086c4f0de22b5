"""What tests/track_scenes.py promises, from the arrays alone (no GPU): the
planted lengths, the per-camera long-observation counts and the per-block
shared counts that tests/test_gpu_track_lengths.py relies on to reach the
paths it names."""
import numpy as np
import pytest

import track_scenes as ts

LADDERS = [(6, 257), (7, 257), (10, 273), (10, 274), (12, 280), (9, 303, 304), (9, 304, 304)]
# sha256 (first 16 digits) over pt, cam, ox, X, X0 of the m = 280 ladders, the
# observation count, the last observation's x and the last landmark's start z,
# recorded before ladder() took its m keyword
RECORDED = {(6, 257): ("ab04f4c67d9294f1", 4056, 266.09222295817017, -12.865866604488387),
            (7, 257): ("bb92af63ffa05c4e", 4098, 248.63849822473307, 0.03135371800370057),
            (10, 273): ("5646f97cc7294941", 4640, 273.8215188273276, 0.9300141163828215),
            (10, 274): ("a64439c9701a30e1", 4642, 273.23803925364547, 0.9282356540785651),
            (12, 280): ("faa00f00ca531d59", 4594, 243.41584476042246, 8.034343501975139)}
SHARED = [48, 49, 64, 65, 256, 257]


def _well_formed(sc, pt, cam, ox):
    assert pt.dtype == np.int32 and cam.dtype == np.int32 and ox.shape == (len(pt), 2)
    assert np.all((np.diff(pt) > 0) | ((np.diff(pt) == 0) & (np.diff(cam) > 0)))
    assert cam.min() >= 0 and cam.max() < sc.m and pt.max() == sc.n - 1
    assert sc.X.shape == sc.X0.shape == (4, sc.n) and sc.n > sc.base_n
    assert sc.obs_pt is pt and sc.obs_cam is cam and sc.obs_x is ox
    # the landmarks lie within 0.1 radius of the centre and start perturbed
    lm = sc.X[:3, sc.base_n:]
    assert np.abs(lm).max() <= 0.1 * ts.RADIUS
    d = np.abs(sc.X0[:3, sc.base_n:] - lm)
    assert 0 < d.max() < 1e-2 and np.all(sc.X0[3] == 1)
    # noisy observations: not the exact projections, but within a few pixels
    from bundleadjustmentmatlab_amd.scene import project
    x, z = project(sc.K, sc.w, sc.T, sc.X, cam, pt)
    assert np.all(z > 0)
    r = np.abs(ox - x)
    assert 0 < r[pt >= sc.base_n].min() and r.max() < 4.0


@pytest.mark.parametrize("key", list(RECORDED))
def test_ladders_of_280_cameras_are_unchanged(key):
    """The m keyword left the existing scenes bit for bit what they were."""
    import hashlib
    sc, pt, cam, ox = ts.ladder(*key)
    assert all(np.array_equal(x, y) for x, y in zip(ts.ladder(*key, m=280)[1:], (pt, cam, ox)))
    h = hashlib.sha256()
    for x in (pt, cam, ox, sc.X, sc.X0):
        h.update(np.ascontiguousarray(x).tobytes())
    digest, nobs, last_x, last_z = RECORDED[key]
    assert (len(pt), float(ox[-1, 0]), float(sc.X0[2, -1])) == (nobs, last_x, last_z)
    assert h.hexdigest()[:16] == digest


@pytest.mark.parametrize("args", LADDERS, ids=["-".join(map(str, a)) for a in LADDERS])
def test_ladder(args):
    na, top = args[:2]
    m = args[2] if len(args) > 2 else 280
    sc, pt, cam, ox = ts.ladder(*args)
    _well_formed(sc, pt, cam, ox)
    assert (sc.m, sc.base_n) == (m, 400)
    base, lad = ts.track_lengths(sc, pt)
    assert base.max() <= 30 and base.min() >= 1        # long_points is the planted ones'
    want = ts.ladder_lengths(na, top)
    assert {ts.CMAX[na], ts.CMAX[na] + 1, 8, 9, 32, 33, 90, 91, 128, 129, 256, 257, top} \
        == set(want)
    assert lad.tolist() == [k for k in want for _ in range(2)]      # two of every length
    assert lad.max() == top and (top == 257 or (lad == top).sum() == 2)
    assert int(ts.is_long(lad).sum()) == 2 * sum(k >= 91 for k in want)
    assert not ts.is_long(base).any()
    # every kind of track is present: MFMA chunks, per-term chunks, long tracks
    L = np.r_[base, lad]
    assert (L <= ts.CMAX[na]).any() and ((L > ts.CMAX[na]) & ~ts.is_long(L)).any()
    # the first copy is a window of consecutive cameras, the second is not
    for q in range(len(lad)):
        c = cam[pt == sc.base_n + q]
        window = np.all(np.diff(c) == 1)
        assert window == (q % 2 == 0) or len(c) == sc.m, (q, len(c))


@pytest.mark.parametrize("C", SHARED)
def test_shared(C):
    sc, pt, cam, ox = ts.shared(C)
    _well_formed(sc, pt, cam, ox)
    assert (sc.m, sc.base_n, sc.n) == (100, 300, 300 + C)
    base, lad = ts.track_lengths(sc, pt)
    assert base.max() <= 30 and not ts.is_long(base).any()
    assert lad.min() >= 91 and lad.max() <= 100 and ts.is_long(lad).all()
    assert np.all(lad <= ts.CH_OBS)                    # one segment each
    # per camera, the long observations: exactly C for 0..89, fewer (and some) for 90..99
    lobs = np.bincount(cam[pt >= sc.base_n], minlength=sc.m)
    assert np.all(lobs[:90] == C)
    assert np.all(lobs[90:] < C) and np.all(lobs[90:] > 0)
    # per block, the long tracks that see both cameras
    vis = np.zeros((C, sc.m), dtype=np.int64)
    vis[pt[pt >= sc.base_n] - sc.base_n, cam[pt >= sc.base_n]] = 1
    both = vis.T @ vis
    assert np.all(both[:90, :90] == C)
    assert np.array_equal(both[90:, :90], np.repeat(lobs[90:, None], 90, axis=1))
    assert both[90:, 90:].max() < C
    if C >= 48:      # the binary search of a 90..99 camera's list has misses
        assert (both[90:, 90:] < np.minimum.outer(lobs[90:], lobs[90:])).any()


def test_scenes_are_cached_and_seeded():
    assert ts.ladder(6, 257) is ts.ladder(6, 257)
    a = ts.planted(40, 50, [np.arange(3, 30), np.array([0, 5, 39])], seed=3)
    b = ts.planted(40, 50, [np.arange(3, 30), np.array([0, 5, 39])], seed=3)
    assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert np.array_equal(a[0].X0, b[0].X0)
    assert np.bincount(a[1])[50:].tolist() == [27, 3]
    with pytest.raises(AssertionError):
        ts.planted(40, 50, [np.array([5, 3])], seed=3)
