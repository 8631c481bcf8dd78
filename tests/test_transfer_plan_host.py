"""CPU: the HIP-free arithmetic of the transfers entry points (at2v_verify_transfers*) under AddressSanitizer + UBSan:
tests/host/transfer_plan_host.cpp, a program of its own. csrc/at2v_transfer.h is the one definition of a transfer's signed
message from its fields (the prep kernel, the CPU backend and the ingest queue all use it); csrc/at2v_stage_plan.h lays a
transfers chunk out on the device and bounds the arena, which at2v_api_pipe.h's issue_chunk trusts: that part runs in
tests/host/stage_plan_host.cpp, beside the records form over the same layout code."""
import os
import subprocess

import pytest
from test_stage_plan_host import stage_plan_exe  # noqa: F401  (the fixture that builds stage_plan_host.cpp)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "at2-node_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "host", "transfer_plan_host_asan")


@pytest.fixture(scope="module")
def transfer_plan_exe():
    """built to a per-process name and renamed into place (parallel test workers)"""
    tmp = f"{EXE}.{os.getpid()}"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "host", "transfer_plan_host.cpp"), "-o", tmp], check=True)
    os.replace(tmp, EXE)
    return EXE


def _run(exe, mode):
    out = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    f = out.stdout.split()
    return dict(zip(f[0::2], f[1::2]))


def test_transfer_header_is_plain_cxx():
    """at2v_transfer.h compiles alone with g++ and includes nothing of the project (no HIP through another header)"""
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++",
                    os.path.join(CSRC, "at2v_transfer.h")], check=True)
    text = open(os.path.join(CSRC, "at2v_transfer.h")).read()
    assert [ln for ln in text.splitlines() if ln.startswith("#include") and '"' in ln] == []


def test_message_builder_against_literal_bytes(transfer_plan_exe):
    """both wires x amounts {0, 1, 2^64 - 1, 0x0807060504030201}: the bytes and the little-endian words of
    bincode(ThinTransaction{recipient, amount}) equal literal arrays, the lengths are 48 and 40 (0 for any other wire),
    and nothing is written past the message"""
    got = _run(transfer_plan_exe, "msg")
    assert int(got["cases"]) == 4 * 2


def test_transfer_chunks_fit_their_arena(stage_plan_exe):  # noqa: F811
    """stage_first {64, 128, 1024, 65536} x stage_max {64, 256, 4096, 131072} (raised to stage_first) x small_batch_max
    {0, 1, 64, 1000, 2048, 32768} x m in {1, 63, 64, 65, 4096, 131073, 1000003} x message length {48, 40}: every
    chunk's layout has 16-byte-aligned, disjoint parts with no more padding than alignment needs, uploads exactly
    136 bytes per record, and the chunks, 256-aligned, fit arena_bytes(m, m L, min(stage_first, max(m, 1)), transfers);
    the chunks also keep the size rules of the records plan"""
    got = _run(stage_plan_exe, "tplan")
    assert int(got["cases"]) == 4 * 4 * 6 * 7 * 2
    assert 0.5 < float(got["tightest"]) <= 1.0, got
