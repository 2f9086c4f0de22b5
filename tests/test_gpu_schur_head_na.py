"""k_schur_mfma's chunk head at num_a = 7, 9, 10 and 12: the cases of
tests/test_gpu_schur_head.py (which stay at num_a = 6) for the instantiations
that take the kernel's other row-tile branch -- four row tiles, all on the
16x16x4 MFMA -- with blocks of NA x NA entries that straddle the 16-row tile
boundaries in the flush, lane constants (16 t + li) / NA and % NA, and the
group caps of 45 / 28 / 21 / 15 blocks.  Harness, models, checks and bars are
that module's, given num_a: every S block and e_ of vlgba_get_reduced_system
within |diff| / bound <= 1 of tests/schur_ref.py's long double reference for
the MFMA kernel and for schur_kernel="terms", every non-zero block of the
reference returned, two runs of one context bit-identical, and the plan's
chunk, slot, camera-slot, record-word and group counts (vlgba_plan_info) equal
to chunk_model's and group_model's before a chunk is read.

Parameters: num_a 7 / 10 as tests/test_gpu_stage_ref.py (_params), 12 the
projective cameras of scene.projective_from, 9 the radial camera's start and
observations through the lens of tests/test_gpu_radial.py (radial_ref.pack /
observe).

What the cases of one num_a show between them (asserted on the models, without
a GPU and without the gpu marker, by tests/test_schur_head_na_kinds.py):
  * every C from 2 to BA_MF_CMAX(na) (9 / 7 / 6 / 5) in a chunk of at least two
    points: every count of live row tiles, and at num_a = 7, C = 9 the dead
    column of the last tile;
  * a direct chunk at the largest C that allows one (6, 6, 6, 5) and at one
    less, a table chunk beside it in the scene;
  * the direct chunk's scene without one observation of point 3: the first
    chunk keeps its 20 points and reads its table;
  * last K-blocks of 1, 4 and 5 points, a chunk of at most 15 points and one of
    at most 5 (one wave, three waves without a point);
  * with VLGBA_SCHUR_GROUPS = 1: a direct chunk next to a table chunk, a change
    of C, sums carried across chunks, a flush with chunks after it -- and a
    group that the block cap closes with chunks after it (more than one group
    although one was asked for; at num_a = 12 one C = 5 chunk's 15 blocks are
    the cap, so every change of cameras does it).
The scenes are scene.make_config("cfg2", m, n, track, seed), 9 <= m <= 16,
n <= 101; the seeds were chosen on the CPU with the models, and
tests/test_schur_head_na_kinds.py holds the models to the host planner itself
(tools/bench_plan --num_a=N prints the counts of vlgba_plan_info) with
BA_MF_GROUPS groups and with one.

The one-group cases of a num_a run in ONE fresh child (VLGBA_SCHUR_GROUPS is
read once per process): four children, one after another, each under its own
time limit.

Largest |diff| / bound measured on an MI355X (pytest -s prints every case,
lines starting SCHUR-HEAD-NA); no bar was widened.  MFMA and terms kernel
alike to two digits, and the same with every chunk in one group (up to the
block cap) as with one chunk per group:
    num_a    S        e_      (the case)
    7        0.054    0.038   (tracks of 2 filled up to 9 cameras)
    9        0.043    0.042   (tracks of 2 filled up to 7 cameras)
    10       0.034    0.031   (tracks of 2 filled up to 6 cameras)
    12       0.038    0.026   (tracks of 2 filled up to 5 cameras)
The direct chunks' scenes: S 0.0028 .. 0.010, e_ 0.0016 .. 0.0078; whole
tracks of 9 / 8 / 7 views at num_a = 7: S 0.0084 / 0.012 / 0.013, of 7 views at
num_a = 9: 0.013.  vlgba_plan_info
equalled the models' counts in every case, with one chunk per group and in
the one-group children (where the block cap gave 2 .. 5 groups).
"""
import json
import os
import subprocess
import sys

import pytest

import test_gpu_schur_head as head
from test_gpu_schur_head import CH_OBS, GROUP_CH, PTS, caps_of, cmax_of

pytestmark = pytest.mark.gpu

ROOT = head.ROOT
NAS = (7, 9, 10, 12)

# num_a: name: scene arguments and what its chunks must show (the names of
# tests/test_gpu_schur_head.py's CASES; np: the points of every chunk)
CASES = {
    7: {
        "track6": dict(args=(9, 64, 6, 4), direct=True, table=True, last=16, kb=1, C={6},
                       np=[20, 16, 12, 16]),
        "missing-view": dict(args=(9, 64, 6, 4), drop=3, table=True, missing=True, last=16, kb=1,
                             C={6}, np=[20, 16, 12, 16]),
        "track5": dict(args=(9, 61, 5, 1), direct=True, table=True, last=1, kb=1, C={5},
                       np=[8, 8, 13, 11, 20, 1]),
        "track3": dict(args=(16, 64, 3, 3), table=True, missing=True, last=10, kb=5,
                       C={3, 5, 7, 8}, np=[9, 5, 20, 20, 10]),
        "track2": dict(args=(16, 21, 2, 6), table=True, missing=True, last=6, kb=1, C={2, 4, 9},
                       np=[10, 5, 6]),
        # whole tracks of 9, 8, 7 views: all four row tiles full of live rows
        "track9": dict(args=(12, 41, 9, 1), table=True, last=4, kb=4, C={9}, np=[7, 9, 7, 14, 4]),
        "track8": dict(args=(12, 41, 8, 1), table=True, last=15, kb=5, C={8}, np=[5, 5, 8, 8, 15]),
        "track7": dict(args=(12, 41, 7, 1), table=True, last=11, kb=1, C={7},
                       np=[5, 4, 7, 4, 10, 11]),
    },
    9: {
        "track6": dict(args=(9, 64, 6, 4), direct=True, table=True, last=16, kb=1, C={6},
                       np=[20, 16, 12, 16]),
        "missing-view": dict(args=(9, 64, 6, 4), drop=3, table=True, missing=True, last=16, kb=1,
                             C={6}, np=[20, 16, 12, 16]),
        "track5": dict(args=(9, 61, 5, 1), direct=True, table=True, last=1, kb=1, C={5},
                       np=[8, 8, 13, 11, 20, 1]),
        "track2": dict(args=(12, 21, 2, 2), table=True, missing=True, last=5, kb=5, C={2, 4, 7},
                       np=[9, 7, 5]),
        "track2-kb4": dict(args=(10, 45, 2, 6), table=True, missing=True, last=9, kb=4,
                           C={2, 3, 5}, np=[4, 7, 5, 20, 9]),
        # whole tracks of 7 views: 63 of the 64 slab rows live
        "track7": dict(args=(12, 41, 7, 1), table=True, last=11, kb=1, C={7},
                       np=[5, 4, 7, 4, 10, 11]),
    },
    10: {
        "track6": dict(args=(9, 81, 6, 2), direct=True, table=True, last=20, kb=5, C={6},
                       np=[20, 1, 19, 20, 1, 20]),
        "missing-view": dict(args=(9, 81, 6, 2), drop=3, direct=True, table=True, missing=True,
                             last=20, kb=5, C={6}, np=[20, 1, 19, 20, 1, 20]),
        "track5": dict(args=(9, 61, 5, 1), direct=True, table=True, last=1, kb=1, C={5},
                       np=[8, 8, 13, 11, 20, 1]),
        "track2-kb4": dict(args=(10, 45, 2, 6), table=True, missing=True, last=9, kb=4,
                           C={2, 3, 5}, np=[4, 7, 5, 20, 9]),
        "track2": dict(args=(9, 21, 2, 1), table=True, missing=True, last=11, kb=1, C={4, 6},
                       np=[10, 11]),
    },
    12: {
        "track5": dict(args=(9, 101, 5, 2), direct=True, table=True, last=17, kb=2, C={5},
                       np=[20, 4, 17, 20, 4, 19, 17]),
        "missing-view": dict(args=(9, 101, 5, 2), drop=3, direct=True, table=True, missing=True,
                             last=17, kb=2, C={5}, np=[20, 4, 17, 20, 4, 19, 17]),
        "track4": dict(args=(9, 81, 4, 1), direct=True, table=True, last=20, kb=5, C={4},
                       np=[10, 12, 13, 8, 18, 20]),
        "track2": dict(args=(12, 64, 2, 4), table=True, missing=True, last=7, kb=2, C={2, 3, 4},
                       np=[9, 5, 4, 5, 20, 4, 5, 5, 7]),
        "track2-kb4": dict(args=(9, 21, 2, 3), table=True, missing=True, last=4, kb=4,
                           C={2, 3, 5}, np=[4, 13, 4]),
        "track2-kb1": dict(args=(9, 21, 2, 5), table=True, missing=True, last=11, kb=1, C={5},
                           np=[10, 11]),
    },
}
# the direct chunks' camera counts per num_a: min(CMAX, 6) (20 C <= 128) and one less
DIRECT_C = {7: {"track6": 6, "track5": 5}, 9: {"track6": 6, "track5": 5},
            10: {"track6": 6, "track5": 5}, 12: {"track5": 5, "track4": 4}}

# VLGBA_SCHUR_GROUPS = 1.  num_a: name: what the model's groups must show
# (group_kinds' names; groups: how many the model forms; cap: a group closed
# by the block cap with chunks after it)
ONE_GROUP = {
    7: {
        "track6": dict(mixed=True, flush_mid=True, C={6}, groups=1),
        "missing-view": dict(flush_mid=True, C={6}, groups=1),
        "track5": dict(mixed=True, carried=True, flush_mid=True, C={5}, groups=1),
        "track3": dict(c_change=True, flush_mid=True, C={3, 5, 7, 8}, groups=1),
        "track2": dict(c_change=True, flush_mid=True, C={2, 4, 9}, groups=1),
        "track9": dict(carried=True, C={9}, groups=4, cap=True),
        "track8": dict(flush_mid=True, C={8}, groups=3, cap=True),
        "track7": dict(flush_mid=True, C={7}, groups=2, cap=True),
    },
    9: {
        "track6": dict(mixed=True, flush_mid=True, C={6}, groups=2, cap=True),
        "missing-view": dict(flush_mid=True, C={6}, groups=2, cap=True),
        "track5": dict(mixed=True, carried=True, flush_mid=True, C={5}, groups=2, cap=True),
        "track2": dict(c_change=True, flush_mid=True, C={2, 4, 7}, groups=1),
        "track2-kb4": dict(c_change=True, flush_mid=True, C={2, 3, 5}, groups=1),
    },
    10: {
        "track6": dict(mixed=True, carried=True, C={6}, groups=4, cap=True),
        "missing-view": dict(mixed=True, carried=True, C={6}, groups=4, cap=True),
        "track5": dict(mixed=True, carried=True, flush_mid=True, C={5}, groups=3, cap=True),
        "track2-kb4": dict(c_change=True, flush_mid=True, C={2, 3, 5}, groups=1),
        "track2": dict(c_change=True, flush_mid=True, C={4, 6}, groups=1),
    },
    12: {
        "track5": dict(mixed=True, carried=True, C={5}, groups=5, cap=True),
        "missing-view": dict(mixed=True, carried=True, C={5}, groups=5, cap=True),
        "track4": dict(mixed=True, flush_mid=True, C={4}, groups=3, cap=True),
        "track2": dict(c_change=True, flush_mid=True, C={2, 3, 4}, groups=2, cap=True),
        "track2-kb4": dict(c_change=True, flush_mid=True, C={2, 3, 5}, groups=1),
    },
}


def _chunks(na, key):
    c = CASES[na][key]
    sc, pt, cam, ox = head._scene(*c["args"], drop=c.get("drop"))
    chunks = head.chunk_model(pt, cam, sc.n, na)
    kinds = head._claims(key, chunks, na, CASES[na])
    assert [k["np"] for k in chunks] == c["np"], (na, key, [k["np"] for k in chunks])
    assert all(k["C"] <= cmax_of(na) for k in chunks)
    # a direct chunk: 20 points, every view present, 20 C observations in the chunk's 128
    assert all(k["np"] == PTS and PTS * k["C"] <= CH_OBS for k in chunks if k["direct"])
    return chunks, kinds


def closed_by_block_cap(chunks, groups, na):
    """A group of the model that ends ahead of the last chunk because the next
    chunk's new blocks would pass the group's LDS accumulators (and not for
    its cameras or its chunk count)."""
    gs_cap, ge_cap = caps_of(na)
    for c, d, nblk, ncam in groups:
        if d == len(chunks) or d - c >= GROUP_CH:
            continue
        have = set().union(*(chunks[q]["pairs"] for q in range(c, d)))
        cams = set().union(*(chunks[q]["cams"] for q in range(c, d)))
        assert len(have) == nblk and len(cams) == ncam
        if (nblk + len(chunks[d]["pairs"] - have) > gs_cap
                and ncam + len(set(chunks[d]["cams"]) - cams) <= ge_cap):
            return True
    return False


@pytest.mark.parametrize("na,key", [(na, key) for na in NAS for key in CASES[na]],
                         ids=[f"na{na}-{key}" for na in NAS for key in CASES[na]])
def test_chunk_kinds(gpu, na, key):
    kinds, plan, mf, tm = head._solve(gpu, key, na, CASES[na])
    print(f"SCHUR-HEAD-NA num_a {na} {key}: chunks {plan['chunks']} groups {plan['mfma_groups']} "
          f"points {CASES[na][key]['np']} C {sorted(kinds['C'])} direct {kinds['direct']} "
          f"table {kinds['table']} missing {kinds['missing']} last {kinds['last']} "
          f"kb {kinds['kb']}; MFMA S {mf[0]:.3g} e_ {mf[1]:.3g}, terms S {tm[0]:.3g} "
          f"e_ {tm[1]:.3g} of the bound")
    assert plan["groups"] == plan["chunks"]      # BA_MF_GROUPS groups: one chunk each
    assert max(mf) <= 1.0 and max(tm) <= 1.0, (na, key, mf, tm)


def _group_claims(na, key):
    chunks, groups, kinds = head._group_claims(key, 1, na, CASES[na], {
        k: {n: v for n, v in w.items() if n not in ("groups", "cap")}
        for k, w in ONE_GROUP[na].items()})
    want = ONE_GROUP[na][key]
    assert len(groups) == want["groups"], (na, key, groups)
    cap = closed_by_block_cap(chunks, groups, na)
    assert cap == bool(want.get("cap")), (na, key, groups)
    if cap:
        assert len(groups) > 1
    return chunks, groups, kinds, cap


_CHILD = r"""
import json, sys
sys.path[:0] = [{root!r}, {tests!r}, {oracle!r}]
import bundleadjustmentmatlab_amd as pkg
import test_gpu_schur_head as head
import test_gpu_schur_head_na as t
for key in {keys!r}:
    kinds, plan, mf, tm = head._solve(pkg, key, {na}, t.CASES[{na}])
    print("RESULT " + json.dumps(dict(key=key, groups=plan["mfma_groups"], chunks=plan["chunks"],
                                      group_slots=plan["group_slots"],
                                      group_eslots=plan["group_eslots"], mf=mf, tm=tm)),
          flush=True)
"""


@pytest.mark.parametrize("na", NAS)
def test_one_group(gpu, na):
    """Every one-group case of one num_a in one fresh child with
    VLGBA_SCHUR_GROUPS = 1 (the child's _solve holds each plan to the models
    with one group asked for): the plan's groups are the model's, more than
    one where the block cap closes a group, and both kernels within the bound."""
    keys = list(ONE_GROUP[na])
    want = {key: _group_claims(na, key) for key in keys}
    env = dict(os.environ, VLGBA_SCHUR_GROUPS="1")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"),
                         oracle=os.path.join(ROOT, "oracle"), keys=keys, na=na)
    r = subprocess.run([sys.executable, "-s", "-c", code], env=env, capture_output=True, text=True,
                       timeout=300)
    res = [json.loads(ln[7:]) for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    for x in res:
        print(f"SCHUR-HEAD-NA num_a {na} {x['key']} VLGBA_SCHUR_GROUPS=1: {x}")
    assert r.returncode == 0, r.stderr[-2000:]
    assert [x["key"] for x in res] == keys
    for x in res:
        chunks, groups, kinds, cap = want[x["key"]]
        assert x["chunks"] == len(chunks) and x["groups"] == len(groups), (x, groups)
        assert x["group_slots"] == sum(g[2] for g in groups), (x, groups)
        assert x["group_eslots"] == sum(g[3] for g in groups), (x, groups)
        assert max(x["mf"]) <= 1.0 and max(x["tm"]) <= 1.0, x
