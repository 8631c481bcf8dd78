"""CPU: every squaring of the unsigned field (at2v_fu_gen.h) with the scaled-operand set tools/gen_fu.py chose for it,
on the host under AddressSanitizer + UBSan and with the field's run-time bound checks (-DAT2V_FU_CHECK: scaled operands
below 2^32, columns below 2^64, one-MAD wrap carries below 2^32): tests/host/sq_operands_host.cpp. Inputs are drawn from
the class the generator proves for each function; the expected values are Python integers. Then the whole verify
routine over every golden record, since the squarings sit under both decodes and every doubling."""
import importlib.util
import os
import random
import subprocess

import pytest

import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "at2-node_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "host", "sq_operands_host_asan")
P = 2 ** 255 - 19
OFF = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
FUNCS = ["fu_sq", "fu_sq2", "fu_sqc", "fu_sq_x2", "fu_sq_sq2", "fu_sq_sq2_n", "fu_sqc_x2"]   # the program's fn numbers
DOUBLED = {"fu_sq": (0, 0), "fu_sq2": (1, 1), "fu_sqc": (0, 0), "fu_sq_x2": (0, 0), "fu_sq_sq2": (0, 1),
           "fu_sq_sq2_n": (0, 1), "fu_sqc_x2": (0, 0)}                                        # 1: the half computes 2 f^2
RANDOM_CASES = 20000


@pytest.fixture(scope="module")
def sq_exe():
    """-O0 as tests/test_joint_host.py; built to a per-process name and renamed into place (parallel test workers)"""
    tmp = f"{EXE}.{os.getpid()}"
    subprocess.run(["g++", "-O0", "-std=c++17", "-DAT2V_FU_CHECK", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "host", "sq_operands_host.cpp"),
                    os.path.join(CSRC, "at2v_cpu.cpp"), "-pthread", "-o", tmp], check=True)
    os.replace(tmp, EXE)
    return EXE


@pytest.fixture(scope="module")
def classes():
    spec = importlib.util.spec_from_file_location("gen_fu", os.path.join(ROOT, "tools", "gen_fu.py"))
    gen_fu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen_fu)
    return gen_fu.squaring_classes()


def value(limbs):
    return sum(v << OFF[i] for i, v in enumerate(limbs))


def inputs(fmax, rng):
    """20,000 random members of the class, then its extremes: every limb at its maximum (limb 1 of a carried element is
    2^25 - 1 + kFuLimb1Spill there), each limb alone at its maximum, and zero"""
    out = [[rng.randint(0, m) for m in fmax] for _ in range(RANDOM_CASES)]
    out.append(list(fmax))
    out += [[fmax[i] if i == j else 0 for i in range(10)] for j in range(10)]
    out += [[fmax[i] if i != j else 0 for i in range(10)] for j in range(10)]
    out.append([0] * 10)
    return out


def test_classes_fit_the_thirteen_operand_set(classes):
    """the carried class has limb 1 at 2^25 - 1 + spill, and the thirteen-operand functions' 38 f_j stays below 2^32"""
    c = classes["fu_sqc"][0]
    assert c[1] > 2 ** 25 - 1 and all(c[i] == (1 << (26 if i % 2 == 0 else 25)) - 1 for i in range(10) if i != 1)
    for name in ("fu_sqc", "fu_sqc_x2", "fu_sq", "fu_sq_x2"):
        for cl in classes[name]:
            assert all(2 * cl[i] < 2 ** 32 for i in range(8))
            assert all(38 * cl[i] < 2 ** 32 for i in (5, 7, 9)) and all(19 * cl[i] < 2 ** 32 for i in (6, 8))
    assert all(a >= 2 * b - 2 for a, b in zip(classes["fu_sq"][0], c))      # fu_sq takes a sum of two carried elements


def test_squarings_against_python_integers(sq_exe, classes):
    rng = random.Random(0x5153)
    lines = []
    for fn, name in enumerate(FUNCS):
        a, b = (inputs(cl, rng) for cl in classes[name])
        rng.shuffle(b)
        for f0, f1 in zip(a, b):
            e = [((1 + d) * value(f) ** 2) % P for f, d in zip((f0, f1), DOUBLED[name])]
            lines.append(f"{fn} " + " ".join(f"{v:x}" for v in f0 + f1) + f" {e[0]:064x} {e[1]:064x}\n")
    out = subprocess.run([sq_exe, "sq"], input="".join(lines), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert out.stdout.split() == [str(len(FUNCS) * (RANDOM_CASES + 22)), "0"]


def test_joint_verify_matches_golden(sq_exe):
    """13,220 records, both policies, through cpu_verify_one_joint: 0 mismatches with the stored verdicts"""
    files = [os.path.join(golden_io.GOLDEN_DIR, s + ".bin") for s in golden_io.SETS]
    out = subprocess.run([sq_exe, "verify"] + files, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    rows = [list(map(int, line.split())) for line in out.stdout.splitlines()]
    assert len(rows) == len(files)
    assert sum(r[0] for r in rows) == 13220
    assert all(r[1:] == [0, 0] for r in rows), rows
