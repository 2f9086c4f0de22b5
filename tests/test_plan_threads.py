"""The host plan built on several threads is the single-threaded plan, bit for
bit (csrc/ba_plan.cpp plan_host: chunk lists, long-track slots, term records
and bucket sorts in work-balanced thread ranges), and it is the plan recorded
in tests/golden/plan_hashes.json.  CPU only, no ROCm: tools/bench_plan.cpp +
csrc/ba_plan.cpp, built with the host C++ compiler, run plan_host on a problem
file and hash every plan vector.

The golden hashes were recorded from the planner as it stood before it moved
out of ba_solver.cpp.  Whoever changes what the planner computes on purpose
regenerates that file: run the harness on each case below and store the hash
it prints with the case's m, n and N."""
import os
import subprocess

import pytest

import plan_cases as pc


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("plan")
    exe = str(out / "bench_plan")
    r = pc.build_harness(exe)
    assert r.returncode == 0, r.stderr
    return exe, out


def _hash(exe, path, threads):
    env = dict(os.environ, VLGBA_HOST_THREADS=str(threads))
    r = subprocess.run([exe, path, "1"], check=True, capture_output=True, text=True, env=env)
    return pc.hashes(r.stdout)[0], r.stdout


@pytest.mark.parametrize("name", pc.CASES)
def test_plan_identical_on_threads(harness, name):
    exe, out = harness
    path = str(out / f"{name}.bin")
    m, n, N = pc.write_case(name, path)
    want = pc.golden()[name]
    assert (m, n, N) == (want["m"], want["n"], want["N"])   # the scene generators' part
    h1, log1 = _hash(exe, path, 1)
    h8, log8 = _hash(exe, path, 8)
    assert "fast 1" in log1, log1          # the chunked (fast) plan, not the ordered fallback
    assert h1 == h8, (log1, log8)
    assert h1 == want["hash"], log1        # the recorded plan
