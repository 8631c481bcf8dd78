"""CPU: every host-compilable verify route of the shared headers under AT2V_POLICY_ZIP215, in a stand-alone program
(tests/host/zip215_host.cpp) under AddressSanitizer + UBSan with the unsigned field's run-time bound checks
(-DAT2V_FU_CHECK). The program reads one fixture file written here, the constructed records of tests/zip215_ref.py followed
by the `edge` set, and compares each route's verdicts with the column in that file: the reference's (Python integers on
the full-length equation), never the library's.

The ladder routes (half_fu, joint, pair, split) run every record. The comb routes pay a 4,128-entry comb per distinct key
and a base ladder per comb-of-B entry on the host, so they run a stated subset: every constructed record (the 196-case
matrix, the torsion-shifted signatures, the negative cases: 30 distinct keys) and every 16th `edge` record."""
import os
import struct
import subprocess

import numpy as np
import pytest

import zip215_ref as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "at2-node_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "host", "zip215_host_asan")
LADDER = ["half_fu", "joint", "pair", "split"]
COMB = ["comb16", "comb20", "comb24", "comb_lat"]
ZIP = zr.POLICIES.index(zr.ZIP215)


@pytest.fixture(scope="module")
def zip_exe():
    """-O0 (the always-inline field code takes minutes at -O1 under ASan); built to a per-process name and renamed into
    place (parallel test workers)"""
    tmp = f"{EXE}.{os.getpid()}"
    subprocess.run(["g++", "-O0", "-std=c++17", "-DAT2V_FU_CHECK", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "host", "zip215_host.cpp"),
                    "-pthread", "-o", tmp], check=True)
    os.replace(tmp, EXE)
    return EXE


@pytest.fixture(scope="module")
def records(golden):
    """the constructed records, then `edge`: pk, sig, msg, off, bool[n, 4] expected (the old policies' columns of `edge`
    are the fixture's stored ones and are not used here), and the number of constructed records"""
    cases = zr.constructed()
    g = golden["edge"]
    pk, sig, msg, off = zr.pack(cases)
    valid = np.zeros((len(cases) + g.n, 4), bool)
    valid[:len(cases)] = [c.verdicts for c in cases]
    valid[len(cases):, 0] = g.dalek
    valid[len(cases):, ZIP] = zr.stored("edge", g.n)
    return (np.concatenate([pk, g.pk]), np.concatenate([sig, g.sig]), np.concatenate([msg, g.msg]),
            np.concatenate([off, g.off[1:] + off[-1]]).astype(np.uint32), valid, len(cases))


def write_fixture(path, pk, sig, msg, off, column):
    """the tests/golden/*.bin layout (tests/golden/README.md); verdict_dalek holds the expected column"""
    n = len(pk)
    with open(path, "wb") as f:
        f.write(struct.pack("<4I", 0x56325441, 1, n, len(msg)))
        f.write(np.ascontiguousarray(pk, np.uint8).tobytes() + np.ascontiguousarray(sig, np.uint8).tobytes())
        f.write(np.ascontiguousarray(off, "<u4").tobytes() + np.ascontiguousarray(msg, np.uint8).tobytes())
        f.write(np.asarray(column, np.uint8).tobytes() + bytes(2 * n))


def run(exe, policy, n_all, stride, routes, path):
    out = subprocess.run([exe, str(policy), str(n_all), str(stride), ",".join(routes), str(path)],
                         capture_output=True, text=True, timeout=3000)
    assert out.returncode in (0, 1), (out.stdout[-500:] + out.stderr)[-3000:]
    rows = {}
    for line in out.stdout.splitlines():
        f = line.split()
        rows[f[0]] = (int(f[1]), int(f[2]), f[3:])
    assert sorted(rows) == sorted(routes), out.stdout
    return rows


def test_new_product_sites_at_their_class_extremes(zip_exe):
    """the subtraction of a decoded point, three doublings after the last addition, the completion after the pair
    combine, on all-maximal limbs under the run-time bound checks; and their values on points of order 8"""
    out = subprocess.run([zip_exe, "bounds"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.split()[0] == "ok", out.stdout + out.stderr


def test_ladder_routes_every_record(zip_exe, records, tmp_path):
    pk, sig, msg, off, valid, nc = records
    path = tmp_path / "zip215.bin"
    write_fixture(path, pk, sig, msg, off, valid[:, ZIP])
    rows = run(zip_exe, zr.ZIP215, len(pk), 1, LADDER, path)
    for route in LADDER:
        assert rows[route][:2] == (len(pk), 0), (route, rows[route])


def test_comb_routes_stated_subset(zip_exe, records, tmp_path):
    pk, sig, msg, off, valid, nc = records
    path = tmp_path / "zip215.bin"
    write_fixture(path, pk, sig, msg, off, valid[:, ZIP])
    ran = nc + len(range(-(-nc // 16) * 16, len(pk), 16))
    rows = run(zip_exe, zr.ZIP215, nc, 16, COMB, path)
    for route in COMB:
        assert rows[route][:2] == (ran, 0), (route, rows[route])


def test_dalek_policy_on_the_same_file(zip_exe, records, tmp_path):
    """the program judges by the column it is given: under DALEK_V1 the same records give the cofactorless column on
    every route (and would fail against the ZIP215 column, on which the two differ)"""
    pk, sig, msg, off, valid, nc = records
    path = tmp_path / "dalek.bin"
    write_fixture(path, pk, sig, msg, off, valid[:, 0])
    assert (valid[:, 0] != valid[:, ZIP]).sum() > 300
    rows = run(zip_exe, zr.DALEK, nc, 16, LADDER + COMB, path)
    for route in LADDER + COMB:
        assert rows[route][1] == 0, (route, rows[route])
