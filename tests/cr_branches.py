"""The cyclic reductions' code paths as functions of the device's compute-unit
count -- TEST INFRASTRUCTURE ONLY, shared by tests/test_cr_branch_kinds.py
(which proves every function here on the host planner's own output, without a
GPU) and tests/test_gpu_cr_branches.py (which evaluates them with the device's
real count), so the two cannot drift.

The five choices (csrc/ba_chol.hip ba_chol_solve / ba_cr32_factor,
csrc/ba_chol_plan.cpp cr32_fplan_build), ne / nk the eliminated / kept tiles
of a level, nrec the tiles in all:

    64-row   k_cr_factor   split (5 workgroups a tile)   5 ne <= ncu
             k_cr_update   split (4 a tile)              4 nk <= ncu
    32-row   k_cr32_factor split (3 a tile), per level   3 ne <= 2 ncu
             k_cr32_back_all (one launch) vs per level   nrec <= 2 ncu
             k_cr32_fused level 0 in 2 records a tile    3 ne > ncu
"""
TILE = 64


def levels(nt):
    """[(ne, nk)] per level of the cyclic reduction of nt tiles
    (ba_chol_plan.cpp cr_records: the even positions of the active list are
    eliminated, the odd ones kept)."""
    out = []
    while nt > 0:
        out.append(((nt + 1) // 2, nt // 2))
        nt //= 2
    return out


def levels_of(eptr, kptr):
    """The same from a plan's eptr / kptr."""
    return [(int(eptr[q + 1] - eptr[q]), int(kptr[q + 1] - kptr[q])) for q in range(len(eptr) - 1)]


def factor_split(ne, ncu):
    return 5 * ne <= ncu


def update_split(nk, ncu):
    return 4 * nk <= ncu


def cr32_factor_split(ne, ncu):
    return 3 * ne <= 2 * ncu


def cr32_back_one_launch(nrec, ncu):
    return nrec <= 2 * ncu


def cr32_l0two(ne0, ncu):
    return 3 * ne0 > ncu


def kinds64(lv, ncu):
    """Per level of the 64-row reduction "ss" / "us" / "uu" / "s-" ...: factor
    then update, s split, u unsplit, - no launch (no kept tile)."""
    return ["su"[not factor_split(ne, ncu)] + ("-" if nk == 0 else "su"[not update_split(nk, ncu)])
            for ne, nk in lv]


def update_launches(lv):
    return sum(nk > 0 for _, nk in lv)


def group(na):
    return 32 // na


def takes_64_rows(na, track):
    """Every point in `track` consecutive cameras: the band leaves the
    camera-aligned 32-row tiles (groups of G = floor(32 / na) cameras) when a
    pair track - 1 apart can lie two groups apart, track - 1 > G, and S stays
    tridiagonal in 64-row tiles while no block spans three of them: a block's
    last row is at most na * track - 1 below its first column, and 64 below
    still ends in the next tile."""
    return track - 1 > group(na) and na * track - 1 <= TILE


# name: num_a, track, cameras, 64-row tiles, levels, per level factor / update
# kinds on 256 compute units.  n = 12 m points, seed 41 (scene_kw).
SCENES = {
    "na6-t9-m11": dict(na=6, track=9, m=11, tiles=2, kinds=["ss", "s-"]),
    "na6-t9-m22": dict(na=6, track=9, m=22, tiles=3, kinds=["ss", "s-"]),
    "na6-t9-m43": dict(na=6, track=9, m=43, tiles=5, kinds=["ss", "ss", "s-"]),
    "na6-t9-m64": dict(na=6, track=9, m=64, tiles=6, kinds=["ss", "ss", "s-"]),
    "na6-t10-m43": dict(na=6, track=10, m=43, tiles=5, kinds=["ss", "ss", "s-"]),
    "na7-t8-m75": dict(na=7, track=8, m=75, tiles=9, kinds=["ss", "ss", "ss", "s-"]),
    "na10-t6-m64": dict(na=10, track=6, m=64, tiles=10, kinds=["ss", "ss", "ss", "s-"]),
    "na12-t5-m33": dict(na=12, track=5, m=33, tiles=7, kinds=["ss", "ss", "s-"]),
    # the radial camera: G = 3, tracks of 5 .. 7; 297 rows = 4 tiles and 41 rows
    "na9-t6-m33": dict(na=9, track=6, m=33, tiles=5, kinds=["ss", "ss", "s-"]),
    # level 0 past the compute units: the unsplit bodies
    "na10-t5-m700": dict(na=10, track=5, m=700, tiles=110,
                         kinds=["us", "ss", "ss", "ss", "ss", "ss", "s-"]),
    "na12-t5-m700": dict(na=12, track=5, m=700, tiles=132,
                         kinds=["uu", "ss", "ss", "ss", "ss", "ss", "ss", "s-"]),
    "na6-t9-m1400": dict(na=6, track=9, m=1400, tiles=132,
                         kinds=["uu", "ss", "ss", "ss", "ss", "ss", "ss", "s-"]),
}
LARGE = [k for k, s in SCENES.items() if s["m"] >= 100]
SMALL = [k for k in SCENES if k not in LARGE]
# the camera-aligned 32-row reduction past the compute units
# (tests/test_gpu_parity.py::test_cr_one_launch_bit_identical's m = 3000)
CR32 = dict(na=6, track=6, m=3000, n=30000, seed=43 + 3000, tiles=600, levels=10)


def scene_kw(s):
    return dict(m=s["m"], n=s.get("n", 12 * s["m"]), track=s["track"], seed=s.get("seed", 41))
