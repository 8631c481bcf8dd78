"""CPU: the joint-table form of the verify routine (verify_half_fu_joint, what the GPU's verify_kernel runs) on the
host, under AddressSanitizer + UBSan and with the unsigned field's run-time bound checks (-DAT2V_FU_CHECK):
tests/host/joint_host.cpp linked with the CPU backend (at2v_cpu.cpp) and its host tables. Every record of every golden
set under both policies against the stored verdicts and against verify_half_fu, and the signed radix-4 recoding
(sc_recode2) against Python integers."""
import os
import random
import subprocess

import pytest

import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "at2-node_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "host", "joint_host_asan")


@pytest.fixture(scope="module")
def joint_exe():
    """-O0 (the always-inline field code takes minutes at -O1 under ASan); built to a per-process name and renamed into
    place (parallel test workers)"""
    tmp = f"{EXE}.{os.getpid()}"
    subprocess.run(["g++", "-O0", "-std=c++17", "-DAT2V_FU_CHECK", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "host", "joint_host.cpp"),
                    os.path.join(CSRC, "at2v_cpu.cpp"), "-pthread", "-o", tmp], check=True)
    os.replace(tmp, EXE)
    return EXE


def test_joint_form_matches_golden_and_plain_form(joint_exe):
    """13,220 records, both policies: 0 mismatches against the stored verdicts, and verify_half_fu_joint ==
    verify_half_fu on every one. The sets hold what the joint table can get wrong: A = R and A = -R (A -+ R is the
    identity), all small-order encodings as A and as R (2A or 2R is the identity or equals A), A or R failing to
    decode, and k giving c0 = 0."""
    files = [os.path.join(golden_io.GOLDEN_DIR, s + ".bin") for s in golden_io.SETS]
    out = subprocess.run([joint_exe, "verify"] + files, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    rows = [list(map(int, line.split())) for line in out.stdout.splitlines()]
    assert len(rows) == len(files)
    assert sum(r[0] for r in rows) == 13220
    assert all(r[1:] == [0, 0, 0] for r in rows), rows


def digit_count(v):
    """the smallest m with v <= 2 (4^m - 1) / 3"""
    m = 0
    while 3 * v > 2 * (4 ** m - 1):
        m += 1
    return m


def recode_cases():
    rng = random.Random(0x4A32)
    vals = [rng.getrandbits(128) for _ in range(20000)]
    vals += [0, 1, 2, 3, 2 ** 255 - 1]
    for k in range(1, 256):  # around every digit-count boundary: the powers of two ...
        vals += [2 ** k - 1, 2 ** k] if k < 255 else [2 ** k - 1]
    for m in range(1, 128):  # ... and the largest value of m digits, 22..2 in base 4 = floor(2 4^m / 3)
        b = 2 * 4 ** m // 3
        vals += [b - 1, b, b + 1]
    return vals


def test_recode2_against_python_integers(joint_exe):
    """sum d_i 4^i equals the value, digits in {-1, 0, 1, 2}, the digit count minimal and the top digit there"""
    vals = recode_cases()
    assert all(0 <= v < 2 ** 255 for v in vals)
    out = subprocess.run([joint_exe, "recode"], input="".join(f"{v:064x}\n" for v in vals + [2 ** 256 - 1]),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(vals) + 1
    for v, line in zip(vals, lines):
        f = line.split()
        nd, words = int(f[0]), [int(x, 16) for x in f[1:]]
        digits = [((words[i >> 4] >> (2 * (i & 15))) & 3) - 1 for i in range(128)]
        assert all(-1 <= d <= 2 for d in digits)
        assert sum(d << (2 * i) for i, d in enumerate(digits)) == v, hex(v)
        assert nd == digit_count(v), hex(v)
        assert all(d == 0 for d in digits[nd:]) and (nd == 0 or digits[nd - 1] > 0), hex(v)
    assert int(lines[-1].split()[0]) == 129  # 128 digits cannot hold it: the caller fails closed
