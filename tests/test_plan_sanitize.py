"""ThreadSanitizer and AddressSanitizer + UndefinedBehaviorSanitizer runs of
the host planner (csrc/ba_plan.cpp): its two worker-thread pools, the
per-thread counting sorts and the storage reused from one context to the next.
tools/bench_plan.cpp + csrc/ba_plan.cpp are built as a stand-alone program
with the host C++ compiler and run on 8 threads on two problems in ONE
process, so the second plan reuses the first one's storage (host_blocks::reset
clears only the dense-table entries the first plan set).  The first problem of
each pair is large enough that the worker threads really run.  A data race,
out-of-bounds access, use-after-free, leak or undefined operation fails the
run, and the plans must still be the recorded ones."""
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
    for name in sorted({n for pair in PAIRS for n in pair}):
        paths[name] = str(out / f"{name}.bin")
        pc.write_case(name, paths[name])
    return paths


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def harness(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("plan_" + request.param)
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
    exe = str(out / "bench_plan")
    b = pc.build_harness(exe, flags)
    assert b.returncode == 0, b.stderr
    return exe


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
