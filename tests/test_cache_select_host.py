"""CPU: the selection arithmetic of a sender-cache compaction (csrc/at2v_cache_select.h, the function
cache_select_kernel calls on the device) under AddressSanitizer + UBSan: tests/host/cache_select_host.cpp, a program of
its own. Without pins and without a room request the function returns exactly what the compaction computed before pins
existed; with them every pinned entry stays, the total kept is at most the target, and the requested room comes free."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "at2-node_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "host", "cache_select_host_asan")

EDGES = ("all_in_bucket_0", "all_in_bucket_0_room", "pins_half", "pins_half_room_half", "empty", "oldest_bucket",
         "beyond_limits")


@pytest.fixture(scope="module")
def select_exe():
    """built to a per-process name and renamed into place (parallel test workers)"""
    tmp = f"{EXE}.{os.getpid()}"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "host", "cache_select_host.cpp"), "-o", tmp], check=True)
    os.replace(tmp, EXE)
    return EXE


def _stats(out):
    f = out.stdout.split()
    return dict(zip(f[0::2], map(int, f[1::2])))


def test_header_includes_no_hip_header():
    src = open(os.path.join(CSRC, "at2v_cache_select.h")).read()
    assert "hip/" not in src and "#include <cstdint>" in src
    assert '#include "at2v_cache_select.h"' in open(os.path.join(CSRC, "at2v_kern_cache.h")).read()


@pytest.mark.parametrize("seed", [1, 0xC0FFEE])
def test_no_pins_no_room_equals_the_old_loop(select_exe, seed):
    """20,000 random histograms per seed (spread, heaped young, heaped old; capacities 1..8192): threshold and
    remainder equal a literal restatement of the loop cache_select_kernel ran before pins existed"""
    out = subprocess.run([select_exe, "legacy", str(seed), "20000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    st = _stats(out)
    assert st["rounds"] == 20000 and min(st["cuts"], st["whole"]) > 1000, st  # both outcomes exercised


@pytest.mark.parametrize("seed", [2, 0xBEEF])
def test_pins_and_room_requests(select_exe, seed):
    """20,000 random cases per seed within the context's limits (pins <= capacity / 2, room <= capacity / 2): everything
    pinned is kept, the total kept is at most min(3/4 capacity, capacity - room), at least `room` payloads come free,
    and nothing is dropped without need"""
    out = subprocess.run([select_exe, "pins", str(seed), "20000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    st = _stats(out)
    assert st["rounds"] == 20000 and st["cuts"] > 1000 and st["room_requests"] > 1000, st


def test_extremes(select_exe):
    """all entries in bucket 0, pins exactly capacity / 2 (with and without a room request of capacity / 2), an empty
    cache, the oldest bucket, and inputs beyond the context's limits (no wrap-around)"""
    out = subprocess.run([select_exe, "edges"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    got = dict(line.split() for line in out.stdout.splitlines())
    assert got == {name: "ok" for name in EDGES}
