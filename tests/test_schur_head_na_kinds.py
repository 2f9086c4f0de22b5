"""What the cases of tests/test_gpu_schur_head_na.py claim, on the CPU alone (no
marker: these run everywhere): chunk_model and group_model of
tests/test_gpu_schur_head.py on every scene, per num_a = 7, 9, 10, 12.  The
GPU tests of that module check the same claims again before they run and hold
vlgba_plan_info to the models' counts."""
import pytest

from test_gpu_schur_head import PTS, caps_of, cmax_of
from test_gpu_schur_head_na import CASES, DIRECT_C, NAS, ONE_GROUP, _chunks, _group_claims


@pytest.mark.parametrize("na", NAS)
def test_cases_cover_the_kinds(na):
    """Between them the cases of one num_a hold what the kernel tells apart
    (CPU only: the model on the scenes)."""
    cmax = cmax_of(na)
    assert cmax == {7: 9, 9: 7, 10: 6, 12: 5}[na]
    assert caps_of(na) == {7: (45, 24), 9: (28, 24), 10: (21, 24), 12: (15, 24)}[na]
    multi_c, kbs, npts, direct_c = set(), set(), set(), set()
    for key, c in CASES[na].items():
        chunks, kinds = _chunks(na, key)
        multi_c |= {k["C"] for k in chunks if k["np"] >= 2}
        kbs.add(kinds["kb"])     # points of the last chunk's last K-block (BA_MF_KB = 5)
        npts |= {k["np"] for k in chunks}
        here = {k["C"] for k in chunks if k["direct"]}
        direct_c |= here
        if key in DIRECT_C[na]:     # the direct chunk has a table chunk beside it
            assert DIRECT_C[na][key] in here and kinds["table"], (na, key, here)
        if c.get("drop") is not None:
            # (_claims: the first chunk keeps 20 points, misses a view, is not direct)
            full, _ = _chunks(na, next(k for k, v in CASES[na].items()
                                       if v["args"] == c["args"] and v.get("drop") is None))
            assert full[0]["direct"] and full[0]["C"] == min(cmax, 6), (na, key)
            assert [k["np"] for k in full] == [k["np"] for k in chunks]
    assert set(range(2, cmax + 1)) <= multi_c, (na, multi_c)
    assert {min(cmax, 6), min(cmax, 6) - 1} <= direct_c, (na, direct_c)
    assert {1, 4, 5} <= kbs, (na, kbs)
    assert min(npts) <= 5 and any(5 < k <= 15 for k in npts) and PTS in npts, (na, npts)


@pytest.mark.parametrize("na", NAS)
def test_one_group_cases_cover_the_kinds(na):
    """Between them the one-group cases of one num_a run, inside a workgroup of
    several chunks (CPU only: the models on the scenes): a direct chunk next to a
    table chunk, chunks that differ in C, sums carried across chunks, a flush
    with chunks after it, the chunk with the removed view beside others -- and
    a group closed by the block cap with chunks after it."""
    seen = dict(mixed=False, c_change=False, carried=False, flush_mid=False)
    caps = []
    for key in ONE_GROUP[na]:
        chunks, groups, kinds, cap = _group_claims(na, key)
        for name in seen:
            seen[name] = seen[name] | kinds[name]
        caps.append(cap)
    assert all(seen.values()), (na, seen)
    assert any(caps), na
    if na == 12:     # 15 blocks: one C = 5 chunk's pairs are the cap
        chunks, groups, _, _ = _group_claims(na, "track5")
        for c, d, _, _ in groups:
            assert len({chunks[q]["cams"] for q in range(c, d)}) == 1, groups


# ---------------------------------------------------------------------------
# the models against the host planner itself (no ROCm: tools/bench_plan.cpp +
# csrc/ba_plan.cpp with the host compiler, as tests/test_plan_threads.py)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    import plan_cases as pc
    out = tmp_path_factory.mktemp("plan_na")
    exe = str(out / "bench_plan")
    r = pc.build_harness(exe)
    assert r.returncode == 0, r.stderr
    return exe, out


@pytest.mark.parametrize("na", (6,) + NAS)
def test_models_are_the_host_planner(harness, na):
    """chunk_model and group_model give the counts of plan_host (the ones
    vlgba_plan_info reports) for every case of a num_a -- the num_a = 6 cases of
    tests/test_gpu_schur_head.py too -- with BA_MF_GROUPS groups and with
    VLGBA_SCHUR_GROUPS = 1."""
    import os
    import subprocess

    import numpy as np

    import test_gpu_schur_head as head
    exe, out = harness
    for key, c in (head.CASES if na == 6 else CASES[na]).items():
        sc, pt, cam, _ = head._scene(*c["args"], drop=c.get("drop"))
        chunks = head.chunk_model(pt, cam, sc.n, na)
        path = str(out / f"na{na}-{key}.bin")
        with open(path, "wb") as f:
            np.array([sc.m, sc.n, len(pt)], np.int32).tofile(f)
            np.asarray(pt, np.int32).tofile(f)
            np.asarray(cam, np.int32).tofile(f)
        for G in (None, 1):
            env = {k: v for k, v in os.environ.items() if k != "VLGBA_SCHUR_GROUPS"}
            if G:
                env["VLGBA_SCHUR_GROUPS"] = str(G)
            r = subprocess.run([exe, f"--num_a={na}", path, "1"], check=True, capture_output=True,
                               text=True, env=env, timeout=60)
            words = [ln for ln in r.stdout.splitlines() if ln.startswith("  plan ")][-1].split()
            got = dict(zip(words[1::2], map(int, words[2::2])))
            groups = head.group_model(chunks, G or head.MF_GROUPS, na)
            want = dict(num_a=na, mfma_chunks=len(chunks), chunks=len(chunks),
                        slots=sum(len(k["pairs"]) for k in chunks),
                        eslots=sum(k["C"] for k in chunks), words=sum(k["words"] for k in chunks),
                        groups=len(groups), mfma_groups=len(groups),
                        group_slots=sum(g[2] for g in groups),
                        group_eslots=sum(g[3] for g in groups))
            assert got == want, (na, key, G, got, want)
