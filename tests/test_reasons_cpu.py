"""CPU: per-record reject reasons (include/at2v.h at2v_reason) through the C ABI without a device: at2v_verify_one_reason,
at2v_reject_reasons on a CPU context, the CPU ingest queue with AT2V_QUEUE_REASONS, and a stand-alone host program
(tests/host/reason_host.cpp) under AddressSanitizer + UBSan. Expected bytes come from tests/reason_ref.py (Python
integers only), itself cross-checked here against the oracle and the golden verdicts."""
import os
import subprocess

import numpy as np
import pytest

import golden_io
import reason_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "at2-node_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "host", "reason_host_asan")
POLICIES = (("dalek", rr.DALEK), ("libsodium", rr.LIBSODIUM))

# the reason counts of the golden sets, recorded when the reasons were specified: a guard on the helper itself
COUNTS = {
    ("adversarial", "dalek"): {0: 7451, 1: 32, 2: 163, 5: 191, 6: 355},
    ("adversarial", "libsodium"): {0: 7426, 1: 32, 2: 163, 3: 140, 5: 103, 6: 328},
    ("edge", "dalek"): {0: 184, 1: 21, 2: 5, 5: 87, 6: 312},
    ("edge", "libsodium"): {0: 1, 1: 21, 2: 5, 3: 538, 6: 44},
    ("ragged", "dalek"): {0: 256, 2: 1, 5: 15, 6: 48},
    ("ragged", "libsodium"): {0: 256, 2: 1, 5: 15, 6: 48},
    ("rfc8032", "dalek"): {0: 3}, ("rfc8032", "libsodium"): {0: 3},
    ("at2_cfg1", "dalek"): {0: 4096}, ("at2_cfg1", "libsodium"): {0: 4096},
}


@pytest.fixture(scope="module")
def at2v_mod():
    import at2v
    at2v.load_library()
    return at2v


@pytest.fixture(scope="module")
def expected(golden):
    """(set, policy name) -> u8[n] from the helper, computed once and never modified"""
    out = {}
    for name, g in golden.items():
        for pname, pol in POLICIES:
            r = rr.reasons(g.pk, g.sig, g.dalek if pol == rr.DALEK else g.sodium, pol)
            r.setflags(write=False)
            out[(name, pname)] = r
    return out


@pytest.fixture(scope="module")
def built(golden):
    """the constructed records (reason_ref.constructed) around the first valid record of at2_cfg1, with its message"""
    g = golden["at2_cfg1"]
    assert g.dalek[0] and g.sodium[0]
    cases = rr.constructed(g.pk[0].tobytes(), g.sig[0].tobytes())
    return cases, g.message(0)


def test_helper_against_oracle_and_golden(golden, expected, oracle):
    assert {rr.y_of(oracle.small_order_encoding(i)) for i in range(14)} == set(rr.BLOCKLIST_Y)
    for (name, pname), r in expected.items():
        g = golden[name]
        assert rr.counts(r) == COUNTS[(name, pname)], (name, pname)
        assert np.array_equal(r == 0, g.dalek if pname == "dalek" else g.sodium)
        dec = np.array([oracle.decompress_ok(g.pk[i].tobytes()) for i in range(g.n)])
        assert np.array_equal(r == rr.A_DECODE, ~dec), (name, pname)
    assert all(4 not in c for c in COUNTS.values())  # reason 4 is in no fixture: the constructed records cover it


def test_constructed_records_expectations(built, oracle):
    """the constructed cases are rejected by the oracle under both policies, and their stated reasons (by specification:
    blocklisted R is 4 under libsodium, 6 under dalek for canonical encodings and 5 for y >= p; the priority cases)
    are what the helper derives from the bytes"""
    cases, msg = built
    seen = set()
    for name, pk, sig, want_d, want_s in cases:
        for pol, want in ((rr.DALEK, want_d), (rr.LIBSODIUM, want_s)):
            assert not oracle.verify(pk, sig, msg, pol), name
            assert rr.reason(pk, sig, False, pol) == want, (name, pol)
            seen.add(want)
    assert seen == {1, 2, 3, 4, 5, 6}
    by = {c[0]: c for c in cases}
    assert by["R=blocklist y=0x1 sign=0"][3:] == (rr.EQUATION, rr.R_POLICY)
    assert by["R=blocklist y=0x0+p sign=0"][3:] == (rr.R_ENCODING, rr.R_POLICY)
    assert by["R=blocklist y=0x1 sign=1"][3:] == (rr.R_ENCODING, rr.R_POLICY)  # x = 0 with the sign bit


def test_verify_one_reason_every_golden_record(at2v_mod, golden, expected, built):
    for (name, pname), want in expected.items():
        g = golden[name]
        got = np.array([at2v_mod.verify_one_reason(g.pk[i].tobytes(), g.sig[i].tobytes(), g.message(i), pname)
                        for i in range(g.n)], np.uint8)
        assert np.array_equal(got, want), (name, pname, np.nonzero(got != want)[0][:8])
    cases, msg = built
    for name, pk, sig, want_d, want_s in cases:
        assert at2v_mod.verify_one_reason(pk, sig, msg, "dalek") == want_d, name
        assert at2v_mod.verify_one_reason(pk, sig, msg, "libsodium") == want_s, name
    lib = at2v_mod.load_library()
    assert lib.at2v_verify_one_reason(None, None, None, 0, 0) == -1
    assert lib.at2v_verify_one_reason(bytes(32), bytes(64), None, 0, 7) == -1


def test_cpu_context_reject_reasons(at2v_mod, golden, expected, built):
    cases, msg = built
    for pname, pol in POLICIES:
        with at2v_mod.BatchVerifier(num_gpus=0, policy=pname, cpu_threads=4) as v:
            for name, g in golden.items():
                want = expected[(name, pname)]
                got = v.reject_reasons(g.pk, g.sig, rr.words_of(want == 0))
                assert np.array_equal(got, want), (name, pname, np.nonzero(got != want)[0][:8])
                # behind the context's own verify: reason 0 <=> the verdict bit
                ok = v.verify_batch(g.pk, g.sig, g.msg, g.off)
                got = v.reject_reasons(g.pk, g.sig, ok)
                assert np.array_equal(got == 0, ok) and np.array_equal(got, want), (name, pname)
            pk, sig, m, off = at2v_mod.pack_records([c[1] for c in cases], [c[2] for c in cases], [msg] * len(cases))
            ok = v.verify_batch(pk, sig, m, off)
            assert not ok.any()
            got = v.reject_reasons(pk, sig, ok)
            assert got.tolist() == [c[3 + pol] for c in cases]
            with pytest.raises(at2v_mod.At2vError) as e:  # a device entry point on a CPU context
                v.reject_reasons_device(16, 16, 1, 16, 16)
            assert e.value.code == -2


def test_reject_reasons_does_not_reverify_and_fails_closed(at2v_mod, golden):
    g = golden["at2_cfg1"]
    n = 70
    lib = at2v_mod.load_library()
    with at2v_mod.BatchVerifier(num_gpus=0, cpu_threads=2) as v:
        # a valid record handed in with a 0 bit is EQUATION (the header says so); guard bytes after n survive
        buf = np.full(n + 64, 0xA5, np.uint8)
        words = np.zeros(3, np.uint32)
        words[0] = 0xFFFFFFFE
        words[1] = 0xFFFFFFFF
        pk, sig = np.ascontiguousarray(g.pk[:n]), np.ascontiguousarray(g.sig[:n])
        assert lib.at2v_reject_reasons(v._h, pk.ctypes.data, sig.ctypes.data, n, words.ctypes.data, buf.ctypes.data) == 0
        assert buf[0] == rr.EQUATION and not buf[1:64].any() and (buf[64:n] == rr.EQUATION).all()
        assert (buf[n:] == 0xA5).all()
        assert lib.at2v_reject_reasons(v._h, None, None, 0, None, None) == 0  # n = 0
        assert lib.at2v_reject_reasons(v._h, None, sig.ctypes.data, n, words.ctypes.data, buf.ctypes.data) == -1
        assert (buf[:n] == 0xFF).all() and (buf[n:] == 0xA5).all()  # an error: every byte UNKNOWN
        assert lib.at2v_reject_reasons(None, pk.ctypes.data, sig.ctypes.data, n, words.ctypes.data, None) == -1


def test_reason_names_and_verify_error(at2v_mod, golden, built):
    names = [at2v_mod.reason_name(r) for r in range(7)] + [at2v_mod.reason_name(0xFF)]
    assert len(set(names)) == 8 and names[0] == "valid" and at2v_mod.reason_name(99) == "not a reason"
    assert at2v_mod.strerror(-99) == "unknown error"  # at2v_strerror is unchanged
    cases, msg = built
    g = golden["at2_cfg1"]
    at2v_mod.Signature(g.sig[0].tobytes()).verify(msg, at2v_mod.PublicKey(g.pk[0].tobytes()))
    for name, pk, sig, want_d, _ in cases:
        with pytest.raises(at2v_mod.VerifyError) as e:
            at2v_mod.Signature(sig).verify(msg, at2v_mod.PublicKey(pk))
        assert e.value.reason == want_d, name


def test_cpu_queue_poll_reasons(at2v_mod, golden, expected):
    from at2v import node
    g = golden["adversarial"]
    n = 2000
    want = expected[("adversarial", "dalek")][:n]
    with node.IngestQueue(cpu=True, reasons=True, max_batch=512, cpu_threads=4) as q:
        rng = np.random.default_rng(5)
        at, first = 0, None
        while at < n:  # ragged pieces
            m = min(n - at, int(rng.integers(1, 300)))
            off = g.off[at:at + m + 1]
            t = q.submit(g.pk[at:at + m], g.sig[at:at + m], g.msg[off[0]:off[-1]], off - off[0])
            first = t if first is None else first
            at += m
        q.flush()
        tickets, reasons = [], []
        while len(tickets) < n:
            t, r = q.poll_reasons(4096, 2_000_000)
            assert len(t), "queue stalled"
            tickets += t.tolist()
            reasons += r.tolist()
        assert tickets == list(range(first, first + n))
        assert np.array_equal(np.array(reasons, np.uint8), want)
        # plain poll on a flagged queue still returns 0/1
        q.submit(g.pk[:64], g.sig[:64], g.msg[:g.off[64]], g.off[:65])
        q.flush()
        got = []
        while len(got) < 64:
            _, v = q.poll(4096, 2_000_000)
            got += v.tolist()
        assert got == g.dalek[:64].astype(int).tolist()
    with node.IngestQueue(cpu=True, max_batch=512, cpu_threads=2) as q:  # without the flag
        with pytest.raises(at2v_mod.At2vError) as e:
            q.poll_reasons(16, 0)
        assert e.value.code == -1
        t = np.zeros(4, np.uint64)
        r = np.zeros(4, np.uint8)
        lib = at2v_mod.load_library()
        assert lib.at2v_queue_poll_reasons(None, t.ctypes.data, r.ctypes.data, 4, 0) == -1


@pytest.fixture(scope="module")
def reason_exe():
    """-O0 with the unsigned field's run-time bound checks, as tests/test_joint_host.py builds joint_host.cpp; built to
    a per-process name and renamed into place (parallel test workers)"""
    tmp = f"{EXE}.{os.getpid()}"
    subprocess.run(["g++", "-O0", "-std=c++17", "-DAT2V_FU_CHECK", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "host", "reason_host.cpp"),
                    os.path.join(CSRC, "at2v_cpu.cpp"), "-pthread", "-o", tmp], check=True)
    os.replace(tmp, EXE)
    return EXE


def test_host_program_under_sanitizers(reason_exe, golden, expected, tmp_path):
    """reject_reason and cpu_reject_reasons over every golden file, both policies, under ASan + UBSan: 0 mismatches
    against the helper, and the 64 guard bytes after reasons[n] untouched"""
    total = 0
    for name in golden_io.SETS:
        want = tmp_path / (name + ".reasons")
        want.write_bytes(expected[(name, "dalek")].tobytes() + expected[(name, "libsodium")].tobytes())
        out = subprocess.run([reason_exe, os.path.join(golden_io.GOLDEN_DIR, name + ".bin"), str(want)],
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (name, (out.stdout + out.stderr)[-3000:])
        row = list(map(int, out.stdout.split()))
        assert row[0] == golden[name].n and row[1:] == [0, 0, 0, 0, 0], (name, row)
        total += row[0]
    assert total == 13220
