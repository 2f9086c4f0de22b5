"""ThreadSanitizer and AddressSanitizer + UndefinedBehaviorSanitizer runs of
the host planner (csrc/ba_plan.cpp): its two worker-thread pools, the
per-thread counting sorts and the storage reused from one context to the next.
tools/bench_plan.cpp + csrc/ba_plan.cpp are built as a stand-alone program
with the host C++ compiler and run on 8 threads on two problems in ONE
process, so the second plan reuses the first one's storage (host_blocks::reset
clears only the dense-table entries the first plan set).  The first problem of
each pair is large enough that the worker threads really run.  A data race,
out-of-bounds access, use-after-free, leak or undefined operation fails the
run, and the plans must still be the recorded ones.

The reduced solve's planner (csrc/ba_chol_plan.cpp) gets the same treatment:
tools/bench_chol_plan.cpp, built the same way, plans every problem of
plan_cases.SOLVE_CASES (num_a 6 / 7 / 10 / 12, the five solver modes, 256 and 8
compute units) in one process."""
import json
import os
import subprocess

import pytest

import plan_cases as pc

SANITIZERS = {
    "tsan": ["-fsanitize=thread"],
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
PAIRS = [("ladybug_small", "shared_257"), ("banded", "ladder6_257")]


@pytest.fixture(scope="module")
def problems(tmp_path_factory):
    out = tmp_path_factory.mktemp("plan_san")
    paths = {}
    for name in pc.SOLVE_CASES:
        paths[name] = str(out / f"{name}.bin")
        pc.write_case(name, paths[name])
    return paths


def _sanitized(request, tmp_path_factory, name, sources):
    out = tmp_path_factory.mktemp(name + "_" + request.param)
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", *SANITIZERS[request.param]]
    # can this sanitizer's runtime start here at all?  (TSan refuses some
    # address-space layouts.)  Only that is a skip; a report never is.
    probe = out / "probe.cpp"
    probe.write_text("int main(){return 0;}\n")
    b = subprocess.run([pc.CXX, *flags, str(probe), "-o", str(out / "probe")],
                       capture_output=True, text=True)
    if b.returncode != 0:
        pytest.skip(f"{request.param}: an empty program does not build: {b.stderr[-300:]}")
    r = subprocess.run([str(out / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"{request.param}: an empty program does not run "
                    f"(exit {r.returncode}): {r.stderr[-300:]}")
    exe = str(out / name)
    b = pc.build_harness(exe, flags, sources)
    assert b.returncode == 0, b.stderr
    return exe


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def harness(request, tmp_path_factory):
    return _sanitized(request, tmp_path_factory, "bench_plan", pc.SOURCES)


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def chol_harness(request, tmp_path_factory):
    return _sanitized(request, tmp_path_factory, "bench_chol_plan", pc.CHOL_SOURCES)


@pytest.mark.parametrize("pair", PAIRS, ids=["+".join(p) for p in PAIRS])
def test_planner_under_sanitizer(harness, problems, pair):
    env = dict(os.environ, VLGBA_HOST_THREADS="8",
               TSAN_OPTIONS="halt_on_error=1",
               ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([harness, problems[pair[0]], "1", problems[pair[1]]],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for bad in ("ThreadSanitizer", "AddressSanitizer", "runtime error"):
        assert bad not in r.stderr, r.stderr
    gold = pc.golden()
    assert pc.hashes(r.stdout) == [gold[pair[0]]["hash"], gold[pair[1]]["hash"]], r.stdout


def test_solve_planner_under_sanitizer(chol_harness, problems):
    env = dict(os.environ, VLGBA_HOST_THREADS="8",
               TSAN_OPTIONS="halt_on_error=1",
               ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([chol_harness, "--ncu", "256,8", *(problems[n] for n in pc.SOLVE_CASES)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for bad in ("ThreadSanitizer", "AddressSanitizer", "runtime error"):
        assert bad not in r.stderr, r.stderr
    with open(os.path.join(pc.ROOT, "tests", "golden", "solve_plan_hashes.json")) as f:
        want = json.load(f)["entries"]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("chol ")]
    assert len(lines) == len(want)
    for t in lines:
        e = want[" ".join(t[1:5])]      # "<case> na=.. mode=.. ncu=.."
        assert all(t[t.index(w) + 1] == e[w] for w in ("solveplan", "launchplan", "launchrun"))
