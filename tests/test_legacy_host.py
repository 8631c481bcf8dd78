"""CPU: every host-compilable verify route of the shared headers under AT2V_POLICY_DALEK_V1_LEGACY, in a stand-alone
program (tests/host/legacy_host.cpp) under AddressSanitizer + UBSan with the unsigned field's run-time bound checks
(-DAT2V_FU_CHECK). The program prints verdicts; the expected ones are tests/legacy_ref.py's (the stored columns and the
oracle on R || (s - l)). The constructed records carry s = 2^253 - 1, the largest scalar the rule lets through: every
route must evaluate [s]B exactly for it (sc_mul_signed's 512-bit reduction, and the radix-2^16 / 2^20 / 2^24 recodings of
the combs with their top carry).

The comb routes pay a 4,128-entry comb per distinct key and a base ladder per comb-of-B entry on the host, some sixty
verifies per record, so they run every record with s >= l (the class the rule is about) and every 64th other record of
the big sets; the ladder routes run every record."""
import os
import subprocess

import numpy as np
import pytest

import golden_io
import legacy_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "at2-node_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "host", "legacy_host_asan")
LADDER = ["core", "half", "half_fu", "joint", "pair", "split"]
COMB = ["comb16", "comb20", "comb24", "comb_lat"]
SETS = ("adversarial", "edge", "ragged")


@pytest.fixture(scope="module")
def legacy_exe():
    """-O0 (the always-inline field code takes minutes at -O1 under ASan); built to a per-process name and renamed into
    place (parallel test workers)"""
    tmp = f"{EXE}.{os.getpid()}"
    subprocess.run(["g++", "-O0", "-std=c++17", "-DAT2V_FU_CHECK", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "host", "legacy_host.cpp"),
                    "-pthread", "-o", tmp], check=True)
    os.replace(tmp, EXE)
    return EXE


@pytest.fixture(scope="module")
def expected(golden, oracle):
    return {name: lr.legacy_expected_set(oracle, golden[name]) for name in SETS}


@pytest.fixture(scope="module")
def cases(golden, oracle):
    return lr.constructed(oracle, golden["at2_cfg1"])


def run(exe, policy, stride, routes, files):
    out = subprocess.run([exe, str(policy), str(stride), ",".join(routes)] + [str(f) for f in files],
                         capture_output=True, text=True, timeout=3000)
    assert out.returncode == 0, (out.stdout[-500:] + out.stderr)[-3000:]
    rows = {}
    for line in out.stdout.splitlines():
        f, route, bits = line.split()
        rows[(f, route)] = bits
    assert len(rows) == len(routes) * len(files)
    return rows


def compare(bits, want, what):
    got = np.frombuffer(bits.encode(), np.uint8)
    assert len(got) == len(want), what
    ran = got != ord("-")
    bad = np.nonzero(ran & ((got == ord("1")) != want))[0]
    assert bad.size == 0, (what, bad[:8])
    return ran


def test_the_class_is_in_the_fixture(golden, expected):
    g = golden["adversarial"]
    cls = np.array([lr.in_class(g.sig[i].tobytes()) for i in range(g.n)])
    assert cls.sum() == 109 and (cls & expected["adversarial"]).sum() == 108


def test_constructed_records_every_route(legacy_exe, cases, tmp_path):
    """s = l, l + 1 and 2^253 - 1 accepted, 2^253 and s + 2l rejected, on every route; under the two old policies the
    same program gives the old verdicts"""
    path = tmp_path / "constructed.bin"
    lr.write_fixture(path, *lr.pack(cases))
    assert any(lr.s_of(c.sig) == 2 ** 253 - 1 and c.verdicts[2] for c in cases)
    for p in (2, 0, 1):
        rows = run(legacy_exe, p, 1, LADDER + COMB, [path])
        want = np.array([bool(c.verdicts[p]) for c in cases])
        for route in LADDER + COMB:
            assert compare(rows[(str(path), route)], want, (p, route)).all()


@pytest.mark.parametrize("route", LADDER)
def test_ladder_routes_over_the_fixtures(legacy_exe, golden, expected, route):
    files = {name: os.path.join(golden_io.GOLDEN_DIR, name + ".bin") for name in SETS}
    rows = run(legacy_exe, 2, 1, [route], list(files.values()))
    for name, f in files.items():
        assert compare(rows[(f, route)], expected[name], (name, route)).all()


@pytest.mark.parametrize("route", COMB)
def test_comb_routes_over_the_fixtures(legacy_exe, golden, expected, route):
    files = {name: os.path.join(golden_io.GOLDEN_DIR, name + ".bin") for name in SETS}
    rows = run(legacy_exe, 2, 64, [route], list(files.values()))
    for name, f in files.items():
        g = golden[name]
        ran = compare(rows[(f, route)], expected[name], (name, route))
        cls = np.array([lr.in_class(g.sig[i].tobytes()) for i in range(g.n)])
        assert ran[cls].all() and ran[::64].all()
