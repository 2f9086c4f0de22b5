"""k_schur_mfma's chunk head on small scenes: the chunk kinds its loads tell
apart -- direct chunks (20 points whose observation table is the identity),
table chunks, short last chunks, a chunk with a missing view -- and every
branch of its last row tile (C = 5 .. 8 cameras), against the
extended-precision reference of tests/schur_ref.py, entry by entry, exactly as
tests/test_gpu_stage_ref.py does: |diff| / bound <= 1 for every S block and e_
of vlgba_get_reduced_system.  Each case also requires two runs of one context
to agree bit for bit and the per-term kernel to lie within the same bound.

What a scene claims (its chunk kinds) is checked on the CPU first: chunk_model
restates the planner's MFMA chunking (ba_plan.cpp, build_plan) and must
reproduce the plan's chunk, camera-slot and record-word counts
(vlgba_plan_info) before its chunks are read; a scene that does not produce
the kinds its case lists fails.  group_model restates the planner's grouping
in the same way (group, block and camera counts of vlgba_plan_info).

With BA_MF_GROUPS groups a scene this small has one chunk per workgroup, so
test_one_group runs every track length again with VLGBA_SCHUR_GROUPS = 1 in a
fresh child: several chunks in one workgroup, among them a direct chunk next
to a table chunk, consecutive chunks that differ in C, chunks that share their
cameras, a flush with chunks after it and the chunk with the removed view
(ONE_GROUP, checked on the model's groups before the GPU runs).

The scenes are scene.make_config("cfg2", m, n, track, seed) with 9 <= m <= 16.
With m >= 9 and tracks of at most 8 cameras a scene has at least two camera
lists, so a chunk is full (20 points) where 20 points share a list or the
lists of its first points differ early (the planner then fills it up to 8
cameras), and only with tracks of at most 6: a chunk holds 128 observations.
So n = 19, 20, 21 and 41 give short table chunks, and the direct chunks come
from the longer scenes.  The seeds below were chosen on the CPU for the kinds
listed.

The cases here are num_a = 6 (three row tiles, the last on 4x4x4 MFMAs).  The
models, the claims and _solve take num_a (default 6):
tests/test_gpu_schur_head_na.py runs them at num_a = 7, 9, 10 and 12.

Largest |diff| / bound measured on an MI355X (pytest -s prints every case,
lines starting SCHUR-HEAD): S 0.033, e_ 0.011 for both kernels (tracks of 2);
the direct chunks' scenes 0.0021 .. 0.0057 (S), 0.0015 .. 0.0025 (e_).  With
every chunk in one group the ratios are the same to three digits (the
largest again tracks of 2: S 0.033, e_ 0.011).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import schur_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMAX, PTS, KB = 8, 20, 5        # BA_MF_CMAX(6), BA_MF_PTS, BA_MF_KB
CH_OBS, CH_TERMS = 128, 4096    # BA_CH_OBS, BA_CH_TERMS
MF_GROUPS, GROUP_CH = 768, 64   # BA_MF_GROUPS, BA_GROUP_CH
GS_CAP, GE_CAP = 1536 // 36, 24  # BA_MF_GACC / (6 x 6) blocks, BA_MF_GE_CAP cameras per group


def cmax_of(na):
    """BA_MF_CMAX(na): the cameras whose rows fit 16 * BA_MF_RT(na) slab rows."""
    return 16 * (3 if na == 6 else 4) // na


def caps_of(na):
    """(blocks, cameras) a group's LDS holds (ba_plan.cpp, build_plan's gs_cap
    and ge_cap of an MFMA group): one chunk's blocks always fit."""
    c = cmax_of(na)
    return max(1536 // na ** 2, c * (c + 1) // 2), max(24, c)


assert cmax_of(6) == CMAX and caps_of(6) == (GS_CAP, GE_CAP)


def chunk_model(pt, cam, n, na=6):
    """The MFMA chunks of build_plan for an observation list sorted
    point-major with cameras ascending, every track of at most CMAX views:
    a list of dicts np, C, words (the record's), direct (20 points, the
    table is the identity), missing (a 0xff table entry).  Of num_a only
    CMAX depends: the 128 observations, the 20 points and the record's words
    are the same for every camera model."""
    CMAX = cmax_of(na)
    ptr = np.searchsorted(pt, np.arange(n + 1))
    cams_of = [tuple(cam[ptr[i]:ptr[i + 1]]) for i in range(n)]
    assert all(0 < len(c) <= CMAX and list(c) == sorted(c) for c in cams_of)
    out, p = [], 0
    while p < n:
        q, seen, uniform, terms = p, set(), True, 0
        while (q < n and q - p < PTS and ptr[q + 1] - ptr[p] <= CH_OBS and
               terms + len(cams_of[q]) * (len(cams_of[q]) + 1) // 2 <= CH_TERMS):
            same = cams_of[q] == cams_of[p]
            if uniform and not same and q - p >= 4:
                break
            uniform = uniform and same
            if len(seen | set(cams_of[q])) > CMAX:
                break
            seen |= set(cams_of[q])
            terms += len(cams_of[q]) * (len(cams_of[q]) + 1) // 2
            q += 1
        cams = sorted(seen)
        npts, C = q - p, len(cams)
        nobs = int(ptr[q] - ptr[p])
        full = all(cams_of[i] == tuple(cams) for i in range(p, q))
        pairs = {(a, b) for i in range(p, q) for a in cams_of[i] for b in cams_of[i] if a >= b}
        out.append(dict(np=npts, C=C, words=2 + C + C * (C + 1) // 2 + (npts * C + 3) // 4,
                        direct=npts == PTS and full, missing=nobs < npts * C,
                        cams=tuple(cams), pairs=pairs))
        p = q
    return out


def group_model(chunks, G=MF_GROUPS, na=6):
    """The MFMA groups of build_plan for chunk_model's chunks: chunks spread
    over G groups (VLGBA_SCHUR_GROUPS, else BA_MF_GROUPS), a group closed
    early where its blocks or cameras would pass the LDS caps of num_a.  A
    list of (first chunk, one past the last, blocks, cameras) per group."""
    GS_CAP, GE_CAP = caps_of(na)
    n, out, c, k = len(chunks), [], 0, 0
    while c < n:
        tend = ((k + 1) * n + G - 1) // G
        gmax = min(GROUP_CH, max(1, tend - c))
        k += 1
        gs, ge, d = set(), set(), c
        while d < n and d - c < gmax:
            new_s, new_e = chunks[d]["pairs"] - gs, set(chunks[d]["cams"]) - ge
            if d > c and (len(gs) + len(new_s) > GS_CAP or len(ge) + len(new_e) > GE_CAP):
                break
            gs |= new_s
            ge |= new_e
            d += 1
            if len(gs) > GS_CAP:
                break
        out.append((c, d, len(gs), len(ge)))
        c = d
    return out


def group_kinds(chunks, groups):
    """What the chunk loop meets inside one workgroup: several chunks (the
    header read one chunk ahead is a real chunk's), a direct chunk next to a
    table chunk, a change of C, chunks that share their cameras (sums carried
    from chunk to chunk) and a change of cameras ahead of the group's end (a
    flush with chunks after it); the camera counts that occur in groups of
    several chunks."""
    k = dict(several=False, mixed=False, c_change=False, carried=False, flush_mid=False, C=set())
    for c, d, _, _ in groups:
        if d - c < 2:
            continue
        k["several"] = True
        k["C"] |= {chunks[q]["C"] for q in range(c, d)}
        for q in range(c, d - 1):
            a, b = chunks[q], chunks[q + 1]
            k["mixed"] |= a["direct"] != b["direct"]
            k["c_change"] |= a["C"] != b["C"]
            k["carried"] |= a["cams"] == b["cams"]
            k["flush_mid"] |= a["cams"] != b["cams"]
    return k


def _scene(m, n, track, seed, drop=None):
    from bundleadjustmentmatlab_amd.scene import make_config
    sc = make_config("cfg2", m=m, n=n, track=track, seed=seed)
    pt, cam, ox = sc.obs_pt, sc.obs_cam, sc.obs_x
    if drop is not None:     # one observation inside the track of point `drop`
        o = int(np.flatnonzero(pt == drop)[1])
        keep = np.arange(len(pt)) != o
        pt, cam, ox = pt[keep], cam[keep], ox[keep]
    return sc, pt, cam, ox


# name: scene arguments and what its chunks must show.  last: points of the
# last chunk; kb: points of the last chunk's last wave K-block; C: camera
# counts that must occur; direct / table: at least one such chunk;
# missing: a chunk with a 0xff table entry (never direct)
CASES = {
    # short table chunks (7 + 12, 12 + 8, 8 + 13 points)
    "n19": dict(args=(9, 19, 8, 1), table=True, last=12, kb=2, C={8}),
    "n20": dict(args=(9, 20, 8, 4), table=True, last=8, kb=3, C={8}),
    "n21": dict(args=(9, 21, 8, 1), table=True, last=13, kb=3, C={8}),
    # tracks of 8: 16 points fill a chunk's 128 observations; last chunks of 1, 9, 5 points
    "n41-kb1": dict(args=(9, 41, 8, 4), table=True, last=1, kb=1, C={8}),
    "n41-kb4": dict(args=(9, 41, 8, 1), table=True, last=9, kb=4, C={8}),
    "n41-kb5": dict(args=(9, 41, 8, 3), table=True, last=5, kb=5, C={8}),
    # C = 7 chunks and a C = 8 chunk across a camera change
    "track7": dict(args=(9, 61, 7, 2), table=True, missing=True, last=17, kb=2, C={7, 8}),
    # the config-3 pattern: direct C = 6 chunks, C = 7 chunks across a camera change
    "track6": dict(args=(9, 81, 6, 2), direct=True, missing=True, last=1, kb=1, C={6, 7}),
    # table chunks of 10, 15, 12 points, one direct chunk, a last chunk of 4
    "track6-kb4": dict(args=(9, 61, 6, 1), direct=True, table=True, last=4, kb=4, C={6}),
    "track5": dict(args=(9, 101, 5, 3), direct=True, missing=True, last=1, kb=1, C={5, 6, 7}),
    "track4": dict(args=(10, 64, 4, 2), table=True, C={4}),
    "track3": dict(args=(12, 66, 3, 4), table=True, missing=True, C={3, 4}),
    # tracks of 2 filling chunks up to 8 cameras: C = 8 with absent views
    "track2": dict(args=(16, 45, 2, 2), table=True, missing=True, last=1, kb=1, C={2, 8}),
    # "track6" without one observation of point 3: its first chunk is no longer direct
    "missing-view": dict(args=(9, 81, 6, 2), drop=3, direct=True, missing=True, last=1, kb=1),
}


def _claims(key, chunks, na=6, cases=None):
    c = (cases or CASES)[key]
    kinds = dict(direct=any(k["direct"] for k in chunks),
                 table=any(not k["direct"] for k in chunks),
                 missing=any(k["missing"] for k in chunks),
                 C={k["C"] for k in chunks}, last=chunks[-1]["np"],
                 kb=(chunks[-1]["np"] - 1) % KB + 1)
    assert not any(k["direct"] and k["missing"] for k in chunks)
    if c.get("drop") is not None:   # the removed view is in the first chunk, still 20 points
        assert chunks[0]["np"] == PTS and chunks[0]["missing"] and not chunks[0]["direct"], key
    for name in ("direct", "table", "missing"):
        if c.get(name):
            assert kinds[name], (key, name, chunks)
    assert c.get("C", set()) <= kinds["C"], (key, kinds["C"])
    for name in ("last", "kb"):
        if c.get(name) is not None:
            assert kinds[name] == c[name], (key, name, kinds[name])
    return kinds


def _env_groups():
    """The planner's group count in this process: VLGBA_SCHUR_GROUPS, else
    BA_MF_GROUPS."""
    e = os.environ.get("VLGBA_SCHUR_GROUPS", "")
    return int(e) if e.isdigit() and int(e) > 0 else MF_GROUPS


def _check_plan(key, plan, chunks, groups, na=6):
    """The models are the planner's chunking and grouping: same chunks, blocks,
    camera slots and record words, same groups with the same blocks and
    cameras; every chunk on the MFMA kernel."""
    assert plan["num_a"] == na, (key, plan)
    assert plan["mfma"] == 1 and plan["reordered"] == 0 and plan["long_points"] == 0, (key, plan)
    assert plan["chunks"] == len(chunks), (key, plan["chunks"], len(chunks))
    assert plan["chunk_slots"] == sum(len(k["pairs"]) for k in chunks), key
    assert plan["chunk_eslots"] == sum(k["C"] for k in chunks), key
    assert plan["blob_words"] == sum(k["words"] for k in chunks), key
    assert plan["groups"] == plan["mfma_groups"] == len(groups), (key, plan, groups)
    assert plan["group_slots"] == sum(g[2] for g in groups), (key, plan, groups)
    assert plan["group_eslots"] == sum(g[3] for g in groups), (key, plan, groups)


def _start(sc, na, pt, cam, ox):
    """(K, a, b, observations, constructor keywords) of a scene at num_a: the
    parameters of tests/test_gpu_stage_ref.py (6, 7, 10), the projective
    cameras of scene.projective_from (12), and for the radial camera (9)
    tests/test_gpu_radial.py's start and observations through the lens."""
    b = np.asfortranarray(sc.X0[:3])
    if na == 12:
        from bundleadjustmentmatlab_amd.scene import projective_from
        Pp, Xp = projective_from(sc)
        return (None, np.asfortranarray(Pp.reshape(12, sc.m, order="F")),
                np.asfortranarray(Xp[0:3]), ox, dict(model="projective", m=sc.m))
    if na == 9:
        from test_gpu_stage_ref import _radial
        a, b, ox = _radial(sc, pt, cam)
        return sc.K, a, b, ox, {}
    from test_gpu_stage_ref import _params
    return sc.K, _params(sc, na)[0], b, ox, {}


def _solve(pkg, key, na=6, cases=None):
    """One case on the GPU: (kinds, plan, ratios of the MFMA kernel, ratios of
    the per-term kernel); asserts the bit-for-bit repeat."""
    c = (cases or CASES)[key]
    sc, pt, cam, ox = _scene(*c["args"], drop=c.get("drop"))
    chunks = chunk_model(pt, cam, sc.n, na)
    kinds = _claims(key, chunks, na, cases)
    K, a, b, ox, kw = _start(sc, na, pt, cam, ox)
    out = {}
    for kern in ("auto", "terms"):
        with pkg.BundleAdjuster(K, pt, cam, ox, sc.n, na, schur_kernel=kern, **kw) as ba:
            ba.set_params(a, b)
            lin = ba.linearization()
            jk, blocks, e_ = (x.copy() for x in ba.reduced_system(dense=False))
            jk2, blocks2, e2 = (x.copy() for x in ba.reduced_system(dense=False))
            plan = ba.plan_info()
        assert np.array_equal(jk, jk2) and np.array_equal(blocks, blocks2), (key, kern)
        assert np.array_equal(e_, e2), (key, kern)
        if kern == "auto":
            _check_plan(key, plan, chunks, group_model(chunks, _env_groups(), na), na)
            out["plan"] = plan
        else:
            assert plan["mfma"] == 0 and plan["mfma_groups"] == 0, (key, plan)
        ref = sr.schur(sc.m, sc.n, na, pt, cam, lin["W"], lin["V"], lin["eB"], lin["U"],
                       lin["eA"], 1e-3)
        got = set(map(tuple, jk.tolist()))
        nz = np.flatnonzero(np.any(ref["S"] != 0, axis=(1, 2)))
        assert all(tuple(ref["jk"][q]) in got for q in nz), (key, kern)
        out[kern] = tuple(float(x) for x in sr.schur_ratio(ref, jk, blocks, e_))
    return kinds, out["plan"], out["auto"], out["terms"]


def _report(key, kinds, plan, mf, tm):
    print(f"SCHUR-HEAD {key}: chunks {plan['chunks']} groups {plan['mfma_groups']} "
          f"C {sorted(kinds['C'])} direct {kinds['direct']} table {kinds['table']} "
          f"missing {kinds['missing']} last {kinds['last']} kb {kinds['kb']}; "
          f"MFMA S {mf[0]:.3g} e_ {mf[1]:.3g}, terms S {tm[0]:.3g} e_ {tm[1]:.3g} of the bound")


@pytest.mark.parametrize("key", list(CASES))
def test_chunk_kinds(gpu, key):
    kinds, plan, mf, tm = _solve(gpu, key)
    _report(key, kinds, plan, mf, tm)
    assert max(mf) <= 1.0 and max(tm) <= 1.0, (key, mf, tm)


def test_cases_cover_the_kinds():
    """Between them the cases hold what the kernel tells apart (CPU only: the
    model on the scenes): direct and table chunks in one scene, a missing
    view, C = 5, 6, 7, 8, and last K-blocks of 1, 4 and 5 points."""
    seen_c, kbs, both = set(), set(), False
    for key, c in CASES.items():
        sc, pt, cam, ox = _scene(*c["args"], drop=c.get("drop"))
        kinds = _claims(key, chunk_model(pt, cam, sc.n))
        seen_c |= kinds["C"]
        kbs.add(kinds["kb"])
        both = both or (kinds["direct"] and kinds["table"])
    assert {5, 6, 7, 8} <= seen_c, seen_c
    assert {1, 4, 5} <= kbs, kbs
    assert both




# VLGBA_SCHUR_GROUPS = 1: the planner puts chunk after chunk into one group
# until the LDS caps close it, so the chunk loop runs over several chunks in a
# workgroup (with BA_MF_GROUPS groups these small scenes have one chunk each).
# name: what the model's groups must show, group_kinds' names
ONE_GROUP = {
    "track2": dict(c_change=True, flush_mid=True, C={2, 8}),
    "track3": dict(c_change=True, flush_mid=True, C={3, 4}),
    "track4": dict(flush_mid=True, C={4}),
    "track5": dict(mixed=True, c_change=True, flush_mid=True, C={5, 6, 7}),
    "track6": dict(mixed=True, c_change=True, flush_mid=True, C={6, 7}),
    "track6-kb4": dict(mixed=True, carried=True, flush_mid=True, C={6}),
    "track7": dict(c_change=True, flush_mid=True, C={7, 8}),
    "n41-kb5": dict(carried=True, C={8}),
    "missing-view": dict(mixed=True, c_change=True, flush_mid=True, C={6, 7}),
}


def _group_claims(key, G, na=6, cases=None, one_group=None):
    """The model's groups of a case with G groups asked for, and their kinds;
    fails where the groups do not show what ONE_GROUP lists (G = 1)."""
    c = (cases or CASES)[key]
    sc, pt, cam, ox = _scene(*c["args"], drop=c.get("drop"))
    chunks = chunk_model(pt, cam, sc.n, na)
    groups = group_model(chunks, G, na)
    kinds = group_kinds(chunks, groups)
    if G == 1:
        assert kinds["several"], (key, groups)
        for name, want in (one_group or ONE_GROUP)[key].items():
            assert (want <= kinds["C"]) if name == "C" else kinds[name], (key, name, kinds, groups)
        if c.get("drop") is not None:   # the chunk with the removed view has neighbours
            assert groups[0][1] - groups[0][0] >= 2, (key, groups)
    return chunks, groups, kinds


def test_one_group_cases_cover_the_kinds():
    """Between them the one-group cases run, inside a workgroup of several
    chunks (CPU only: the models on the scenes): a direct chunk next to a table
    chunk, consecutive chunks that differ in C, sums carried across chunks of
    the same cameras, a flush with chunks after it, the chunk with the removed
    view, and C = 2 .. 8."""
    seen = dict(mixed=False, c_change=False, carried=False, flush_mid=False, C=set())
    for key in ONE_GROUP:
        chunks, groups, kinds = _group_claims(key, 1)
        for name in seen:
            seen[name] = seen[name] | kinds[name]
    assert seen["mixed"] and seen["c_change"] and seen["carried"] and seen["flush_mid"], seen
    assert set(range(2, 9)) <= seen["C"], seen


_CHILD = r"""
import json, sys
sys.path[:0] = [{root!r}, {tests!r}, {oracle!r}]
import bundleadjustmentmatlab_amd as pkg
import test_gpu_schur_head as t
kinds, plan, mf, tm = t._solve(pkg, {key!r})
print("RESULT " + json.dumps(dict(groups=plan["mfma_groups"], chunks=plan["chunks"],
                                  group_slots=plan["group_slots"],
                                  group_eslots=plan["group_eslots"], mf=mf, tm=tm,
                                  direct=kinds["direct"], table=kinds["table"])))
"""


def _child(key, groups):
    """One case in a fresh child with VLGBA_SCHUR_GROUPS set (it is read once
    per process); the child's _solve holds its plan to the models as well."""
    env = dict(os.environ, VLGBA_SCHUR_GROUPS=str(groups))
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"),
                         oracle=os.path.join(ROOT, "oracle"), key=key)
    r = subprocess.run([sys.executable, "-s", "-c", code], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(f"SCHUR-HEAD {key} VLGBA_SCHUR_GROUPS={groups}: {res}")
    return res


@pytest.mark.parametrize("key", list(ONE_GROUP))
def test_one_group(gpu, key):
    """Every track length with its chunks in one workgroup: the header read a
    chunk ahead, the direct / table choice, C and the flush change from chunk
    to chunk inside one chunk loop.  The plan's groups are the model's."""
    chunks, groups, kinds = _group_claims(key, 1)
    res = _child(key, 1)
    assert res["chunks"] == len(chunks) and res["groups"] == len(groups), (res, groups)
    assert res["group_slots"] == sum(g[2] for g in groups), (res, groups)
    assert res["group_eslots"] == sum(g[3] for g in groups), (res, groups)
    assert max(res["mf"]) <= 1.0 and max(res["tm"]) <= 1.0, res


def test_one_chunk_per_group(gpu):
    """VLGBA_SCHUR_GROUPS far above the chunk count: one chunk per group,
    direct and table chunks among them (test_one_group[track6-kb4] has the same
    scene in one group)."""
    res = _child("track6-kb4", 10 ** 6)
    assert res["direct"] and res["table"]
    assert res["chunks"] > 1 and res["groups"] == res["chunks"], res
    assert max(res["mf"]) <= 1.0 and max(res["tm"]) <= 1.0, res
