"""CPU: every table of tests/probe_cases.py through the probe library with where = 0, the host compile of the csrc inline
functions (the AT2V_UMAD C form of the products, the IEEE division of lehmer_round32), against Python integers. This
checks the references and the case generators without a GPU, and is the direct integer check of the multiplications' C
form. tests/test_gpu_probe.py runs the same tables on the device. Also: the generator's multiplication classes, that
regenerating at2v_fu_gen.h changes nothing, and that the probe stays out of libat2v.so."""
import filecmp
import os
import re
import subprocess
import sys

import pytest

import probe_cases as pc
import probe_lib
import probe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = probe_lib.HOST


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(probe_lib.PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "at2-node_amd"), "probe"], check=True)
    return probe_lib.load()


def test_probe_lists_every_function(built):
    _, ops = built
    assert [n for n, _ in sorted(ops.items(), key=lambda kv: kv[1][0])][:14] == pc.PRODUCTS
    assert set(ops) == set(pc.PRODUCTS + pc.UTILS + pc.POWERS + pc.GROUP + pc.DECODES + pc.SCALARS)


def test_probe_rejects_bad_arguments(built):
    import ctypes
    lib, ops = built
    buf = (ctypes.c_uint32 * 64)()
    assert lib.at2v_probe_run(0, len(ops), 1, buf, buf, 0) == -1
    assert lib.at2v_probe_run(2, 0, 1, buf, buf, 0) == -1
    assert lib.at2v_probe_run(0, 0, 0, buf, buf, 0) == -1
    assert lib.at2v_probe_run(0, 0, 1, None, buf, 0) == -1
    assert lib.at2v_probe_run(0, ops["fu_sqn"][0], 1, buf, buf, 0) == -1    # n >= 1
    assert lib.at2v_probe_run(0, ops["fu_sub"][0], 1, buf, buf, 2) == -1


def test_probe_adds_nothing_to_the_product_library(built):
    """libat2v.so exports no probe symbol and the probe library exports only its three calls"""
    import at2v
    nm = lambda path: set(re.findall(r"\b[TDB] (\w+)", subprocess.run(
        ["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout))
    assert not [s for s in nm(at2v.LIB_PATH) if "probe" in s]
    assert {s for s in nm(probe_lib.PATH) if s.startswith("at2v_")} == {"at2v_probe_count", "at2v_probe_info",
                                                                         "at2v_probe_run"}
    assert b"amdgcn-amd-amdhsa--gfx950" in open(probe_lib.PATH, "rb").read()


def test_regenerated_header_is_byte_identical(tmp_path):
    out = str(tmp_path / "at2v_fu_gen.h")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fu.py"), out], check=True, capture_output=True)
    assert filecmp.cmp(out, os.path.join(ROOT, "at2-node_amd", "csrc", "at2v_fu_gen.h"), shallow=False)


def test_multiplication_classes():
    """the wide functions take the declared classes, fu_mulc carried x carried, the one-MAD-wrap variants the narrow sites
    of check_group_law, each with a top carry below 2^32 under the generator's own prove()"""
    g = R.GEN
    m = g.multiplication_classes()
    assert set(m) == set(pc.MULS)
    assert [(f, gg) for f, gg, _ in m["fu_mul"][0]] == [(g.MUL_F, g.MUL_G)] and m["fu_mul_x2"] == m["fu_mul"]
    assert [(f, gg) for f, gg, _ in m["fu_mulc"][0]] == [(R.CARRIED, R.CARRIED)] and m["fu_mulc_x2"] == m["fu_mulc"]
    narrow = m["fu_mul_n"][0]
    assert m["fu_mul_nn"] == (narrow, narrow) and m["fu_mul_wn"] == (m["fu_mul"][0], narrow) and len(narrow) > 1
    names = {w for _, _, w in narrow}
    assert {"add B", "add C", "add D", "madd A", "madd B"} <= names
    for f, gg, where in narrow:
        assert all(f[i] <= g.MUL_F[i] and gg[i] <= g.MUL_G[i] for i in range(10)), where
        assert g.prove(g.MCOLS, f, gg, where)[1] < 2 ** 32, where
    assert g.prove(g.MCOLS, g.MUL_F, g.MUL_G, "declared")[1] >= 2 ** 32     # the wide class does need the full wrap


def test_limb_helpers():
    for x in pc.SPECIAL + [R.D, R.SQRT_M1]:
        assert R.val(R.canon(x)) == x % R.P
        for cmax in (R.CARRIED, R.KC, R.GEN.MUL_F, pc.ANY):
            m = R.max_rep(x, cmax)
            assert (R.val(m) - x) % R.P == 0 and R.val(cmax) - R.val(m) < R.P
    assert R.is_carried(R.CARRIED) and not R.is_carried([v + (i == 3) for i, v in enumerate(R.CARRIED)])
    assert R.on_curve(R.B) and R.mul(R.L, R.B) == R.IDENT and all(R.in_torsion(t) for t in R.TORSION)
    assert len(set(R.TORSION)) == 8 and not R.in_torsion(R.B)


@pytest.mark.parametrize("name", pc.PRODUCTS)
def test_field_products(name):
    assert pc.check_product(HOST, name) > 2048


@pytest.mark.parametrize("name", pc.UTILS)
def test_field_utilities(name):
    assert pc.check_util(HOST, name) > 2048


@pytest.mark.parametrize("name", pc.POWERS)
def test_field_powers(name):
    assert pc.check_power(HOST, name) >= 2 * 517


@pytest.mark.parametrize("name", pc.GROUP)
def test_group_law(name):
    assert pc.check_group(HOST, name) >= 2 * 274


@pytest.mark.parametrize("name", pc.DECODES)
def test_decode(name):
    assert pc.check_decode(HOST, name) >= 14 + 38 + 1024


@pytest.mark.parametrize("name", pc.SCALARS)
def test_scalars(name):
    assert pc.check_scalar(HOST, name) > 2048
