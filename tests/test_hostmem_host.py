"""CPU: the registry of pinned host ranges (csrc/at2v_hostmem.h: what at2v_host_alloc / at2v_host_register record and
the host-buffer calls look their slices up in) under AddressSanitizer + UBSan: tests/host/hostmem_host.cpp, a program of
its own. Random insert / lookup / remove operations against a brute-force list, and the edge cases of a lookup."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "at2-node_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "host", "hostmem_host_asan")

EDGES = ("insert", "whole_range", "ends_at_end", "one_past_end", "starts_one_before", "first_byte", "last_byte",
         "byte_at_end", "zero_length_inside", "zero_length_insert_refused", "adjacent_after", "adjacent_before",
         "across_seam", "seam_sides", "overlap_inside", "overlap_covering", "overlap_start", "overlap_end",
         "overlap_same", "wraps_refused", "find_wraps", "remove_interior", "remove_unknown", "remove_start",
         "remove_twice", "gone", "reinsert")


@pytest.fixture(scope="module")
def hostmem_exe():
    """built to a per-process name and renamed into place (parallel test workers)"""
    tmp = f"{EXE}.{os.getpid()}"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "host", "hostmem_host.cpp"),
                    "-o", tmp], check=True)
    os.replace(tmp, EXE)
    return EXE


@pytest.mark.parametrize("seed", [1, 0xA72, 0x5EED])
def test_random_operations_against_brute_force(hostmem_exe, seed):
    """10,000 operations per seed in a 4 KB address space (overlaps, exact fits and neighbours are common): every
    insert, lookup, start-of-range lookup and removal agrees with a linear scan, and the ranges stay sorted and disjoint"""
    out = subprocess.run([hostmem_exe, "random", str(seed), "10000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    f = out.stdout.split()
    stats = dict(zip(f[0::2], map(int, f[1::2])))
    assert stats["ops"] == 10000
    # the run exercised every outcome, not one branch only
    assert min(stats["inserts"], stats["refused"], stats["hits"], stats["removes"]) > 100, stats


def test_lookup_edge_cases(hostmem_exe):
    """a slice ending exactly at a range's end is inside, one byte past it or starting one byte before it is not, a
    zero-length slice is in no range, adjacent ranges are accepted and a slice across their seam is in neither, every
    kind of overlap is refused, and only the start of a range removes it"""
    out = subprocess.run([hostmem_exe, "edges"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    got = dict(line.split() for line in out.stdout.splitlines())
    assert got == {name: "ok" for name in EDGES}
