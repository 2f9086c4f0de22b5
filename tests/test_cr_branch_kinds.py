"""Which code path every cyclic-reduction scene of tests/test_gpu_cr_branches.py
takes, proven without a GPU from the host planner's own output:
tools/bench_chol_plan.cpp (--na: the scene's camera size, num_a = 9 included)
plans each scene of tests/cr_branches.py for a device of 256 compute units and
dumps the plan; the assertions read the dumped scalars and eptr / kptr.

* every 64-row scene: cr32 = 0, the tile count, cr_nlev, the per-level counts
  of eliminated / kept tiles (cr_branches.levels is the planner's cr_records),
  and per level whether k_cr_factor / k_cr_update run split or unsplit -- the
  three large scenes reach the unsplit bodies at level 0 and only there;
* the rule that puts a banded scene on the 64-row route (cr_branches.
  takes_64_rows) against the planner for every track length 2 .. 11 at num_a
  6 / 7 / 9 / 10 / 12: num_a 9 takes it for tracks of 5 to 7;
* the 3000-camera scene of the camera-aligned 32-row reduction: 600 tiles, ten
  levels, level 0 in two records a tile, k_cr32_factor unsplit, the back
  substitution level by level -- and the opposite of each on a device large
  enough, where the stored launch plan differs.
"""
import os
import subprocess

import numpy as np
import pytest

import cr_branches as cb
import plan_cases as pc
from test_solve_plan import _load

NCU = 256


def _write(path, **kw):
    """plan_cases.write_case's file of a banded scene."""
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", **kw)
    with open(path, "wb") as f:
        np.array([sc.m, sc.n, len(sc.obs_pt)], np.int32).tofile(f)
        np.asarray(sc.obs_pt, np.int32).tofile(f)
        np.asarray(sc.obs_cam, np.int32).tofile(f)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("cr_kinds")
    exe = str(out / "bench_chol_plan")
    b = pc.build_harness(exe, flags=("-O1",), sources=pc.CHOL_SOURCES)
    assert b.returncode == 0, b.stderr
    (out / "dump").mkdir()

    def plan(name, na, ncu=NCU, **kw):
        """The auto-mode plan of scene `name` (written once): (fields of the
        harness's line, the dumped vectors)."""
        path = str(out / f"{name}.bin")
        if not os.path.exists(path):
            _write(path, **kw)
        r = subprocess.run([exe, "--ncu", str(ncu), "--na", str(na), "--dump", str(out / "dump"),
                            path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("chol ")]
        assert [t[2] for t in lines] == [f"na={na}"] * 5          # only the camera size asked for
        t = [t for t in lines if t[3] == "mode=0"][0]
        f = {k: v for k, v in (x.split("=") for x in t[2:] if "=" in x)}
        f["launchplan"] = t[t.index("launchplan") + 1]
        return f, _load(str(out / "dump"), name, na, 0, ncu)
    plan.exe = exe
    return plan


def test_the_default_camera_sizes_are_unchanged(harness, tmp_path):
    """Without --na: num_a 6, 7, 10, 12, five solver modes each."""
    path = str(tmp_path / "tiny.bin")
    _write(path, m=10, n=400, track=4, seed=41)
    r = subprocess.run([harness.exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    nas = [ln.split()[2] for ln in r.stdout.splitlines() if ln.startswith("chol ")]
    assert nas == [f"na={na}" for na in (6, 7, 10, 12) for _ in range(5)]


@pytest.mark.parametrize("name", list(cb.SCENES))
def test_64_row_scene(harness, name):
    s = cb.SCENES[name]
    na = s["na"]
    assert cb.takes_64_rows(na, s["track"])
    f, p = harness(name, na, **cb.scene_kw(s))
    nt = -(-na * s["m"] // cb.TILE)
    assert nt == s["tiles"] == p["nt"]
    assert p["cr32"] == 0 and p["cr_fused"] == 0 and p["nd_np"] == 0, f
    lv = cb.levels_of(p["eptr"], p["kptr"])
    assert p["cr_nlev"] == len(s["kinds"]) == len(lv)
    assert lv == cb.levels(nt)
    assert p["eptr"][-1] == nt and len(p["elim"]) == 3 * nt
    assert cb.kinds64(lv, NCU) == s["kinds"], (name, lv)
    assert cb.update_launches(lv) == len(lv) - 1
    large = name in cb.LARGE
    assert ("u" in "".join(s["kinds"])) == large
    if large:      # ... and one solve mixes both bodies: every deeper level is split
        assert all(k in ("ss", "s-") for k in s["kinds"][1:])
    print(f"CR-KINDS {name}: ld {na * s['m']} tiles {nt} levels {lv} kinds {s['kinds']}")


def test_the_large_scenes_reach_what_the_table_says():
    k = {n: cb.SCENES[n]["kinds"][0] for n in cb.LARGE}
    assert k == {"na10-t5-m700": "us", "na12-t5-m700": "uu", "na6-t9-m1400": "uu"}
    # the thresholds themselves: 51 | 52 eliminated and 64 | 65 kept tiles on 256 compute units
    assert cb.factor_split(51, 256) and not cb.factor_split(52, 256)
    assert cb.update_split(64, 256) and not cb.update_split(65, 256)
    # a partial last tile, an odd count, a full last tile, blocks that straddle tiles
    rows = {n: s["na"] * s["m"] % cb.TILE for n, s in cb.SCENES.items()}
    assert rows["na6-t9-m11"] == 2 and rows["na6-t9-m43"] == 2 and rows["na9-t6-m33"] == 41
    assert rows["na6-t9-m64"] == 0 and rows["na10-t6-m64"] == 0
    assert cb.TILE % 12 != 0


@pytest.mark.parametrize("na", [6, 7, 9, 10, 12])
def test_the_rule_of_the_64_row_route(harness, na):
    """Banded scenes of 40 cameras, every track length 2 .. 11: the planner
    takes the camera-aligned 32-row tiles up to G + 1 cameras a track and the
    64-row reduction wherever takes_64_rows says so.  (Past na * track = 65 a
    block can span three tiles; whether one does depends on where the cameras
    fall in the tiles, and the route is the planner's to choose.)"""
    took = {}
    for track in range(2, 12):
        f, p = harness(f"rule-t{track}", na, m=40, n=480, track=track, seed=41)
        took[track] = "32" if p["cr32"] else "64" if p["cr_nlev"] > 0 else "-"
        if track - 1 <= cb.group(na):
            assert took[track] == "32", (na, track, f)
        if cb.takes_64_rows(na, track):
            assert took[track] == "64", (na, track, f)
    want = {6: range(7, 11), 7: range(6, 10), 9: range(5, 8), 10: range(5, 7), 12: range(4, 6)}
    assert [t for t in took if cb.takes_64_rows(na, t)] == list(want[na])
    print(f"CR-KINDS rule num_a {na}: " + " ".join(f"{t}:{k}" for t, k in took.items()))


def test_32_row_scene_past_the_compute_units(harness):
    s = cb.CR32
    f, p = harness("cr32-m3000", s["na"], **cb.scene_kw(s))
    assert p["cr32"] == 1 and p["tb32"] == 30 and p["cr_fused"] == 1, f
    assert p["nt32"] == s["tiles"] and p["cr_nlev"] == s["levels"]
    lv = cb.levels_of(p["eptr"], p["kptr"])
    assert lv == cb.levels(s["tiles"])
    ne0, nrec = lv[0][0], int(p["eptr"][-1])
    assert (ne0, nrec) == (300, 600)
    assert cb.cr32_l0two(ne0, NCU) and not cb.cr32_factor_split(ne0, NCU)
    assert not cb.cr32_back_one_launch(nrec, NCU)
    # a device that holds level 0 at three records a tile stores another launch plan
    big = 1024
    assert not cb.cr32_l0two(ne0, big) and cb.cr32_factor_split(ne0, big)
    assert cb.cr32_back_one_launch(nrec, big)
    g, _ = harness("cr32-m3000", s["na"], ncu=big, **cb.scene_kw(s))
    assert g["launchplan"] != f["launchplan"]
    # ... and one between the two thresholds of level 0 does not: 3 ne > ncu on both
    h, _ = harness("cr32-m3000", s["na"], ncu=512, **cb.scene_kw(s))
    assert cb.cr32_l0two(ne0, 512) and h["launchplan"] == f["launchplan"]
    print(f"CR-KINDS cr32-m3000: tiles {s['tiles']} levels {lv}")
