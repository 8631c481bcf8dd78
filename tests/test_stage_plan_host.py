"""CPU: the arithmetic of the host-buffer pipeline (csrc/at2v_stage_plan.h: the chunk schedule, a chunk's layout, its
uploads, the device arena's size and the copy pieces, which at2v_api_pipe.h's issue_chunk trusts) under ASan + UBSan:
tests/host/stage_plan_host.cpp, a program of its own. The header includes nothing of HIP, so no GPU is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "at2-node_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "host", "stage_plan_host_asan")


@pytest.fixture(scope="module")
def stage_plan_exe():
    """built to a per-process name and renamed into place (parallel test workers)"""
    tmp = f"{EXE}.{os.getpid()}"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "host", "stage_plan_host.cpp"),
                    "-o", tmp], check=True)
    os.replace(tmp, EXE)
    return EXE


def _run(exe, mode):
    out = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    f = out.stdout.split()
    return dict(zip(f[0::2], f[1::2]))


def test_header_is_plain_cxx():
    """the header compiles alone with g++ (no HIP, HSA or RCCL include, directly or through another header)"""
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++",
                    os.path.join(CSRC, "at2v_stage_plan.h")], check=True)
    text = open(os.path.join(CSRC, "at2v_stage_plan.h")).read()
    assert [ln for ln in text.splitlines() if ln.startswith("#include") and '"' in ln] == []


def test_chunk_plans_fit_their_arena(stage_plan_exe):
    """stage_first {64, 128, 1024, 65536} x stage_max {64, 256, 4096, 131072} (raised to stage_first) x small_batch_max
    {0, 1, 64, 1000, 2048} x every m in 1..700 and 299 random m below 2,000,000 x message lengths {0, 1, 48, 100, 4097}:
    the chunks sum to m, every chunk but the last is a multiple of 64, a part of at most small_batch_max records is one
    chunk, no chunk exceeds max(stage_max, first) but by a merged remainder below `first`, and the chunks' layouts,
    256-aligned, fit arena_bytes(m, message bytes, min(stage_first, max(m, 1))): what issue_chunk relies on"""
    got = _run(stage_plan_exe, "plan")
    assert int(got["cases"]) == 4 * 4 * 5 * (700 + 299) * 5 == 399600
    assert 0.99 < float(got["tightest"]) <= 1.0, got  # (the bound is tight for one-record parts: it is not slack by luck)


def test_chunk_layout_parts(stage_plan_exe):
    """sig, off and msg are 16-byte aligned, pk | sig | offsets | messages do not overlap, upload + 16 == total"""
    got = _run(stage_plan_exe, "layout")
    assert int(got["cases"]) == 600 * 5


def test_upload_plan_and_walk(stage_plan_exe):
    """records and transfers x c in {1, 63, 64, 65, 4096} x message bytes {0, 100 c} x every direct / staged choice of the
    four parts (for records the offsets' bit must change nothing: they are never read from the caller). The uploads are
    the sequences written out in the test (pk; sig with the offsets behind it when staged, else sig and then the offsets;
    the messages if there are any; one upload per field array for transfers), their count is the signal's start value,
    they are disjoint, inside the uploaded region and cover every part's bytes once, and direct + staged bytes are
    c * 96 + message bytes (c * 136 for transfers). Then the walk with a submit that fails at every position k (and
    never): exactly the uploads before k are submitted, nothing after k is staged, and the signal, less the uploads never
    submitted, counts the ones in flight down to exactly 0"""
    got = _run(stage_plan_exe, "uploads")
    assert int(got["cases"]) == 2 * 5 * 2 * 16


def test_copy_pieces_cover_their_ranges(stage_plan_exe):
    """CopyJob::add / add_offsets cut a range into pieces of at most kCopyPiece bytes that cover it exactly once; run in
    any order they reproduce a memcpy, and for offsets the rebased values; nothing past the range is written"""
    got = _run(stage_plan_exe, "copy")
    assert int(got["cases"]) == 8 + 7
