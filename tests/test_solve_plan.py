"""The reduced solve's host planner (csrc/ba_chol_plan.cpp chol_plan_build /
chol_nd_step) without a GPU and without ROCm: tools/bench_chol_plan.cpp,
built with the host C++ compiler, plans every problem of plan_cases.SOLVE_CASES
for num_a 6 / 7 / 10 / 12, the solver modes 0 (auto) .. 4 and devices of 256
and 8 compute units.

* Each structure kind the solve can take occurs, asserted from the plan's own
  scalars: fused camera-aligned 32-row cyclic reduction (tile rows 30 / 28 / 30 /
  24 for num_a 6 / 7 / 10 / 12), 64-row cyclic reduction, the natural envelope
  with the one-launch backward solve (nt <= ncu) and without (nt > ncu), nested
  dissection with and without a separator, nested dissection refused because
  it would not shorten the chain (4 * chain > 3 * tiles), every lower tile
  (modes 1, 3) and a one-tile problem.  (ladybug_small in auto mode is the
  refused one at num_a = 6; the nested dissection with a separator that auto
  mode takes is cfg5x_300's.)
* The plans are the recorded ones (tests/golden/solve_plan_hashes.json: from
  the library before the planner moved out of ba_chol.hip where its entries say
  so, from the planner itself for the rest).
* Invariants that need no recorded value, on the dumped vectors: the
  co-visible blocks lie inside the envelope and on their tiles' block lists; the
  cyclic reduction eliminates every tile once, at a level where its neighbours
  are still live; the nested dissection's row maps are inverse permutations and
  no block couples two arcs; the chunked separator records cover each pair's
  arc columns exactly once.

Whoever changes what the planner computes on purpose regenerates the golden
file from the harness's "chol" lines and marks the entries regression only."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import plan_cases as pc

NCU = (256, 8)
NAS = (6, 7, 10, 12)
SCAL = ["nt", "n_env", "cr32", "tb32", "nt32", "cr_nlev", "asm_direct_ok", "cr_fused", "nd_np",
        "nd_grouped"] + [f"a0_{t}" for t in range(9)] + ["slds", "npair", "nrec", "one_back",
                                                         "handoff", "env_runner", "runner_flags"]
VECS = ["tfirst", "pan_ptr", "pan_list", "env", "tptr", "tblk", "elim", "keep", "eptr", "kptr",
        "frec", "srec", "fptr", "sptr", "crow", "prow", "rowsrc", "pairs", "pptr", "rec", "klist",
        "jk"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One harness process over every case: {(case, na, mode, ncu): fields}, dump dir, stderr."""
    out = tmp_path_factory.mktemp("solve_plan")
    exe = str(out / "bench_chol_plan")
    b = pc.build_harness(exe, sources=pc.CHOL_SOURCES)
    assert b.returncode == 0, b.stderr
    paths = []
    for name in pc.SOLVE_CASES:
        paths.append(str(out / f"{name}.bin"))
        pc.write_case(name, paths[-1])
    dump = out / "dump"
    dump.mkdir()
    r = subprocess.run([exe, "--ncu", ",".join(map(str, NCU)), "--dump", str(dump), *paths],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    plans = {}
    for line in r.stdout.splitlines():
        if not line.startswith("chol "):
            continue
        t = line.split()
        f = {k: v for k, v in (x.split("=") for x in t[2:] if "=" in x)}
        e = {k: int(v) for k, v in f.items() if k != "ms"}
        for w in ("solveplan", "launchplan", "launchrun"):
            e[w] = t[t.index(w) + 1]
        plans[(t[1], e["na"], e["mode"], e["ncu"])] = e
    assert len(plans) == len(pc.SOLVE_CASES) * len(NAS) * 5 * len(NCU)
    return plans, str(dump), exe, dict(zip(pc.SOLVE_CASES, paths))


def _load(dump, case, na, mode, ncu):
    raw = np.fromfile(os.path.join(dump, f"{case}_na{na}_mode{mode}_ncu{ncu}.bin"), np.int32)
    assert raw[0] == 1 + len(VECS)
    vecs, at = [], 1
    for _ in range(raw[0]):
        vecs.append(raw[at + 1:at + 1 + raw[at]].astype(np.int64))
        at += 1 + raw[at]
    assert at == len(raw)
    p = dict(zip(SCAL, vecs[0]))
    p.update(zip(VECS, vecs[1:]))
    return p


# ---- the structure kinds ----------------------------------------------------
def test_camera_aligned_cyclic_reduction(run):
    plans = run[0]
    for case, na, rows in [("banded", 6, 30), ("cr_track5", 7, 28), ("cr_track4", 10, 30),
                           ("cr_track3", 12, 24)]:
        for ncu in NCU:
            p = plans[(case, na, 0, ncu)]
            assert p["cr_nlev"] > 0 and p["cr32"] == 1 and p["tb32"] == rows, (case, p)
            assert p["cr_fused"] == 1 and p["nd_np"] == 0 and p["handoff"] == 0, (case, p)
        assert plans[(case, na, 2, 256)]["cr_nlev"] == 0      # mode 2: the envelope, no CR


def test_64_row_cyclic_reduction(run):
    for ncu in NCU:
        p = run[0][("cr64_track9", 6, 0, ncu)]
        assert p["cr_nlev"] > 0 and p["cr32"] == 0 and p["cr_fused"] == 0, p
        assert p["nd_np"] == 0 and p["handoff"] == 0 and p["one_back"] == 0, p


def test_natural_envelope_on_both_sides_of_the_cu_count(run):
    big, small = (run[0][("ladybug_small", 6, 2, ncu)] for ncu in NCU)
    for p in (big, small):
        assert p["cr_nlev"] == 0 and p["nd_np"] == 0 and p["handoff"] == 1, p
    assert 8 < big["nt"] <= 256 and big["one_back"] == 1
    assert small["one_back"] == 0
    assert big["solveplan"] != small["solveplan"]
    # the fused CR's level 0 goes from 3 to 2 records a tile once 3 tiles a CU do not fit
    assert run[0][("banded", 6, 0, 256)]["launchplan"] != run[0][("banded", 6, 0, 8)]["launchplan"]


def test_nested_dissection_with_a_separator(run):
    for key in [("cfg5x_300", 6, 0), ("cfg5x_300", 6, 4), ("ladybug_small", 6, 4)]:
        for ncu in NCU:
            p = run[0][(*key, ncu)]
            assert p["cr_nlev"] == 0 and p["nd_np"] >= 2 and p["nsep"] > 0, p
            assert p["npair"] > 0 and p["nrec"] >= p["npair"], p
    # the separator's records are chunked by the CU count
    assert run[0][("cfg5x_300", 6, 0, 8)]["nrec"] < run[0][("cfg5x_300", 6, 0, 256)]["nrec"]


def test_nested_dissection_without_a_separator(run):
    for mode in (0, 4):
        p = run[0][("two_groups", 6, mode, 256)]
        assert p["nd_np"] == 2 and p["nsep"] == 0 and p["npair"] == 0 and p["nrec"] == 0, p


def test_nested_dissection_refused_when_the_chain_does_not_shorten(run):
    plans, _, exe, paths = run
    p = plans[("ladybug_small", 6, 0, 256)]
    assert p["cr_nlev"] == 0 and p["nd_np"] == 0 and p["handoff"] == 1, p
    r = subprocess.run([exe, "--ncu", "256", "--nd-verbose", paths["ladybug_small"]],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    first = [ln for ln in r.stderr.splitlines() if "nested dissection" in ln][0]   # na 6, mode 0
    m = re.search(r"natural (\d+) tiles, (\d+) arcs -> chain (\d+), <= (\d+) separator pairs, "
                  r"(\d+) setup checks \(not taken\)", first)
    assert m, first
    nt, K, crit, pairs, checks = map(int, m.groups())
    assert nt == p["nt"] and K >= 2
    assert pairs <= 16384 and checks <= 1 << 26      # inside the setup budget ...
    assert nt >= 8 and 4 * crit > 3 * nt             # ... refused by the chain rule


def test_every_lower_tile_and_one_tile(run):
    plans = run[0]
    for mode in (1, 3):
        p = plans[("ladybug_small", 6, mode, 256)]
        assert p["n_env"] == p["nt"] * (p["nt"] + 1) // 2 and p["cr_nlev"] == 0, p
        assert p["nd_np"] == 0 and p["handoff"] == (mode == 1), p
    for mode in range(5):
        p = plans[("tiny10", 6, mode, 256)]
        assert p["nt"] == 1 and p["n_env"] == 1 and p["nd_np"] == 0, p
    assert plans[("tiny10", 6, 0, 256)]["cr32"] == 1      # two 30-row tiles
    assert plans[("tiny10", 6, 2, 256)]["one_back"] == 1


# ---- the recorded plans -------------------------------------------------------
@pytest.mark.parametrize("case", pc.SOLVE_CASES)
def test_plans_are_the_recorded_ones(run, case):
    with open(os.path.join(pc.ROOT, "tests", "golden", "solve_plan_hashes.json")) as f:
        gold = json.load(f)["entries"]
    n = from_parent = 0
    for (c, na, mode, ncu), p in run[0].items():
        if c != case:
            continue
        want = gold[f"{c} na={na} mode={mode} ncu={ncu}"]
        for w in ("solveplan", "launchplan", "launchrun"):
            assert p[w] == want[w], (c, na, mode, ncu, w)
        n += 1
        from_parent += "solveplan" in want["parent"]
    assert n == len(NAS) * 5 * len(NCU)
    assert from_parent >= 15      # num_a 6 / 7 / 10 x five solvers at 256 CUs


# ---- invariants -----------------------------------------------------------------
def _rows_of(p, na, cams):
    """First row of each camera in the plan's row order."""
    return p["crow"][cams] if p["nd_np"] > 0 else na * cams


def _env_set(p):
    return set(map(tuple, p["env"].reshape(-1, 2)))


@pytest.mark.parametrize("case,na,mode,ncu", [
    ("cfg5x_300", 6, 0, 256), ("cfg5x_300", 10, 2, 8), ("ladybug_small", 7, 4, 256),
    ("ladybug_small", 6, 0, 256), ("banded", 6, 0, 256), ("cr64_track9", 6, 0, 256),
    ("two_groups", 6, 0, 256), ("shared_257", 12, 4, 8), ("ladder6_257", 6, 1, 256),
    ("tiny10", 6, 2, 256)])
def test_blocks_inside_the_envelope(run, case, na, mode, ncu):
    p = _load(run[1], case, na, mode, ncu)
    jk = p["jk"].reshape(-1, 2)
    nt, env = p["nt"], p["env"].reshape(-1, 2)
    assert len(env) == p["n_env"] and len(set(map(tuple, env))) == len(env)
    assert np.all(env[:, 0] >= env[:, 1]) and np.all(env[:, 0] < nt)
    tid = -np.ones((nt, nt), np.int64)
    tid[env[:, 0], env[:, 1]] = np.arange(len(env))
    r0, c0 = _rows_of(p, na, jk[:, 0]), _rows_of(p, na, jk[:, 1])
    r0, c0 = np.maximum(r0, c0), np.minimum(r0, c0)
    lists = [set(p["tblk"][a:b]) for a, b in zip(p["tptr"][:-1], p["tptr"][1:])]
    assert p["tptr"][-1] == len(p["tblk"])
    seen = 0
    for dr in (0, na - 1):
        for dc in (0, na - 1):
            t, u = (r0 + dr) // 64, (c0 + dc) // 64
            low = u <= t
            assert np.all(tid[t[low], u[low]] >= 0)        # every lower tile a block touches
            for b in np.flatnonzero(low):
                assert b in lists[tid[t[b], u[b]]]
                seen += 1
    assert seen >= len(jk)
    # tfirst is the envelope's profile, the panel lists its columns
    for i in range(nt):
        assert p["tfirst"][i] == env[env[:, 0] == i, 1].min()
    for k in range(nt):
        want = np.sort(env[(env[:, 1] == k) & (env[:, 0] > k), 0])
        assert np.array_equal(p["pan_list"][p["pan_ptr"][k]:p["pan_ptr"][k + 1]], want)


@pytest.mark.parametrize("case,na", [("banded", 6), ("cr_track5", 7), ("cr_track4", 10),
                                     ("cr_track3", 12), ("cr64_track9", 6), ("tiny10", 6)])
def test_cyclic_reduction_records(run, case, na):
    p = _load(run[1], case, na, 0, 256)
    ntc = p["nt32"] if p["cr32"] else p["nt"]
    elim, keep = p["elim"].reshape(-1, 3), p["keep"].reshape(-1, 4)
    eptr, kptr, nl = p["eptr"], p["kptr"], p["cr_nlev"]
    assert len(eptr) == nl + 1 == len(kptr) and eptr[-1] == len(elim) and kptr[-1] == len(keep)
    assert sorted(elim[:, 0]) == list(range(ntc))            # every tile eliminated exactly once
    live = set(range(ntc))
    for L in range(nl):
        E, Kp = elim[eptr[L]:eptr[L + 1]], keep[kptr[L]:kptr[L + 1]]
        gone = set(E[:, 0])
        for e, a, b in E:      # neighbours: live at this level (kept at level L - 1), not eliminated
            assert e in live and all(x == -1 or (x in live and x not in gone) for x in (a, b))
        for k, em, ep, k2 in Kp:
            assert k in live and k not in gone and em in gone and (ep == -1 or ep in gone)
            assert k2 == -1 or (k2 in live and k2 not in gone)
        assert gone | set(Kp[:, 0]) == live
        live = set(Kp[:, 0])
    assert not live
    if p["cr32"]:      # the fused levels: a record per elimination / survivor of level >= 1
        frec, srec = p["frec"].reshape(-1, 5), p["srec"].reshape(-1, 3)
        assert np.array_equal(frec[:, :3], elim[eptr[1]:]) and len(srec) == len(keep) - kptr[1]
        assert p["fptr"][-1] == len(frec) and p["sptr"][-1] == len(srec)


@pytest.mark.parametrize("case,na,mode,ncu", [
    ("cfg5x_300", 6, 0, 256), ("cfg5x_300", 7, 0, 8), ("ladybug_small", 6, 4, 256),
    ("ladybug_small", 10, 4, 8), ("two_groups", 6, 0, 256), ("shared_257", 12, 4, 256),
    ("banded", 6, 4, 256)])
def test_nested_dissection_rows_and_separator_records(run, case, na, mode, ncu):
    p = _load(run[1], case, na, mode, ncu)
    np_, nt = p["nd_np"], p["nt"]
    assert np_ >= 2 and p["slds"] == 64 * nt
    jk = p["jk"].reshape(-1, 2)
    ld = na * (jk.max() + 1)
    prow, rowsrc = p["prow"], p["rowsrc"]
    assert len(rowsrc) == p["slds"] and np.all(prow[:ld] >= 0) and np.all(prow[ld:] == -1)
    assert np.array_equal(rowsrc[prow[:ld]], np.arange(ld))
    real = np.flatnonzero(rowsrc >= 0)
    assert len(real) == ld and np.array_equal(prow[rowsrc[real]], real)
    a0 = np.array([p[f"a0_{t}"] for t in range(np_ + 1)])
    s0 = a0[np_]
    part = np.searchsorted(a0, np.arange(nt), side="right") - 1      # arc of a tile; np_: separator
    tj, tk = p["crow"][jk[:, 0]] // 64, p["crow"][jk[:, 1]] // 64
    both = (tj < s0) & (tk < s0)
    assert np.all(part[tj[both]] == part[tk[both]])      # no block couples two arcs
    # separator pairs (i >= j) with a common arc column, their columns chunked
    env = _env_set(p)
    cols = {i: [k for k in range(s0) if (i, k) in env] for i in range(s0, nt)}
    want = [(i, j, sorted(set(cols[i]) & set(cols[j]))) for i in range(s0, nt)
            for j in range(s0, i + 1)]
    want = [w for w in want if w[2]]
    pairs, rec, pptr = p["pairs"].reshape(-1, 2), p["rec"].reshape(-1, 3), p["pptr"]
    assert [tuple(x) for x in pairs] == [w[:2] for w in want]
    assert len(pptr) == len(pairs) + 1 and pptr[-1] == len(rec) == p["nrec"]
    work = sum(len(w[2]) for w in want)
    kc = max(2, -(-work // ncu))
    at = 0
    for q, (_, _, ks) in enumerate(want):
        got = []
        for pr, kofs, kcnt in rec[pptr[q]:pptr[q + 1]]:
            assert pr == q and kofs == at and 1 <= kcnt <= kc
            got += list(p["klist"][kofs:kofs + kcnt])
            at += kcnt
        assert got == ks      # each arc column of the pair exactly once
    assert at == len(p["klist"])
