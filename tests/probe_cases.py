"""Seeded case tables for the probe library and their checks against Python integers, shared by tests/test_probe_host.py
(where = 0: the host compile of the csrc inline functions) and tests/test_gpu_probe.py (where = 1: the device compile, with
the inline-asm products). Every check is an exact integer comparison. A check_* function runs one probe over its whole
table and returns the number of cases; a failure names the function, the class or site and the first failing case."""
import random

import numpy as np

import golden_io
import probe_lib
import probe_ref as R
import reason_ref as rr
import test_lattice_host as tl
import zip215_ref as zr

P, L, W, OFF = R.P, R.L, R.W, R.OFF
RANDOM_PRODUCT_CASES = 2048
U32 = 2 ** 32 - 1

MULS = ["fu_mul", "fu_mul_x2", "fu_mulc", "fu_mulc_x2", "fu_mul_n", "fu_mul_wn", "fu_mul_nn"]
SQUARES = ["fu_sq", "fu_sq2", "fu_sqc", "fu_sq_x2", "fu_sq_sq2", "fu_sq_sq2_n", "fu_sqc_x2"]
PRODUCTS = ["fu_mul", "fu_sq", "fu_sq2", "fu_mul_x2", "fu_sq_x2", "fu_sq_sq2", "fu_mulc", "fu_sqc", "fu_mulc_x2",
            "fu_mul_n", "fu_mul_wn", "fu_mul_nn", "fu_sq_sq2_n", "fu_sqc_x2"]          # the probe's numbers 0..13
TWO_WAY = {"fu_mul_x2", "fu_mulc_x2", "fu_mul_wn", "fu_mul_nn", "fu_sq_x2", "fu_sq_sq2", "fu_sq_sq2_n", "fu_sqc_x2"}
DOUBLED = {"fu_sq2": (1, 1), "fu_sq_sq2": (0, 1), "fu_sq_sq2_n": (0, 1)}            # 1: the half computes 2 f^2
SPECIAL = [0, 1, 2, 19, P - 1, P - 2, 2 ** 255 - 20]


def fail(name, site, i, ins, got, want):
    raise AssertionError(f"{name} [{site}] case {i}: in={[list(map(int, x)) for x in ins]} "
                         f"got={list(map(int, got))} want={want}")


# ------------------------------------------------------------------------------------------------ field products

def class_members(cmax, seed):
    """members of the class `cmax` (per-limb maxima): 2,048 random ones, every limb at its maximum, each limb alone at
    its maximum, each limb alone zero with the rest at maximum, zero, and the representatives of 0, 1, 2, 19, p - 1,
    p - 2, 2^255 - 20 in canonical limbs and in the largest limbs the class admits (for 0 also the limbs of p, 2p, FU_KC
    and FU_K2C where the class admits them)"""
    rs = np.random.default_rng(seed)
    cols = [rs.integers(0, m + 1, size=RANDOM_PRODUCT_CASES, dtype=np.uint64) for m in cmax]
    out = [[int(c[k]) for c in cols] for k in range(RANDOM_PRODUCT_CASES)]
    out += edge_members(cmax)
    out += representatives(cmax)
    assert all(0 <= m[i] <= cmax[i] for m in out for i in range(10))
    return out


def edge_members(cmax):
    out = [list(cmax)]
    out += [[cmax[i] if i == j else 0 for i in range(10)] for j in range(10)]
    out += [[cmax[i] if i != j else 0 for i in range(10)] for j in range(10)]
    out.append([0] * 10)
    return out


def representatives(cmax):
    out = []
    for x in SPECIAL:
        out.append(R.canon(x))
        out.append(R.max_rep(x, cmax))
    for z in (R.radix(P), R.radix(2 * P), R.KC, R.K2C):
        assert R.val(z) % P == 0
        if all(z[i] <= cmax[i] for i in range(10)):
            out.append(list(z))
    return out


def mul_pairs(fmax, gmax, seed):
    """(f, g) for one multiplication class: the members of both classes paired (random with random, extreme with the
    other side's maximum and with its own kind), zero against everything, the 100 pairs "f limb i and g limb j at maximum,
    the rest zero", and every pair of representatives"""
    rs = np.random.default_rng(seed)
    fc = [rs.integers(0, m + 1, size=RANDOM_PRODUCT_CASES, dtype=np.uint64) for m in fmax]
    gc = [rs.integers(0, m + 1, size=RANDOM_PRODUCT_CASES, dtype=np.uint64) for m in gmax]
    out = [([int(c[k]) for c in fc], [int(c[k]) for c in gc]) for k in range(RANDOM_PRODUCT_CASES)]
    fe, ge = edge_members(fmax), edge_members(gmax)
    out += [(f, list(gmax)) for f in fe] + [(list(fmax), g) for g in ge] + list(zip(fe, ge))
    out += [([fmax[i] if i == a else 0 for i in range(10)], [gmax[i] if i == b else 0 for i in range(10)])
            for a in range(10) for b in range(10)]
    out += [(f, g) for f in representatives(fmax) for g in representatives(gmax)]
    assert all(f[i] <= fmax[i] and g[i] <= gmax[i] for f, g in out for i in range(10))
    return out


def product_table(name):
    """[(site, rows, expected values per half)] for one of the fourteen products: one entry per class (or per pair of
    classes, for a two-way function, whose halves get independent operands)"""
    is_mul = name in MULS
    two = name in TWO_WAY
    dbl = DOUBLED.get(name, (0, 0))
    tables = []
    if is_mul:
        h0, h1 = R.GEN.multiplication_classes()[name]
        runs = max(len(h0), len(h1)) if two else len(h0)
        for r in range(runs):
            f0, g0, s0 = h0[r % len(h0)]
            a = mul_pairs(f0, g0, seed=(PRODUCTS.index(name), r, 0))
            if not two:
                tables.append((s0, [f + g for f, g in a], [[R.val(f) * R.val(g) % P for f, g in a]]))
                continue
            f1, g1, s1 = h1[(r + 1) % len(h1)]
            b = mul_pairs(f1, g1, seed=(PRODUCTS.index(name), r, 1))
            random.Random(r).shuffle(b)
            b = [b[i % len(b)] for i in range(len(a))]
            tables.append((f"{s0} | {s1}", [f + g + ff + gg for (f, g), (ff, gg) in zip(a, b)],
                           [[R.val(f) * R.val(g) % P for f, g in a], [R.val(f) * R.val(g) % P for f, g in b]]))
    else:
        c0, c1 = R.GEN.squaring_classes()[name]
        a = class_members(c0, seed=(PRODUCTS.index(name), 0))
        if not two:
            tables.append(("class", a, [[(1 + dbl[0]) * R.val(f) ** 2 % P for f in a]]))
        else:
            b = class_members(c1, seed=(PRODUCTS.index(name), 1))
            random.Random(1).shuffle(b)
            b = [b[i % len(b)] for i in range(len(a))]
            tables.append(("class f0 | class f1", [f + g for f, g in zip(a, b)],
                           [[(1 + dbl[0]) * R.val(f) ** 2 % P for f in a], [(1 + dbl[1]) * R.val(f) ** 2 % P for f in b]]))
    return tables


def check_product(where, name):
    """value(result) = value(f) value(g) mod p (doubled where the function doubles), every returned limb in the carried
    class (limb i < 2^W[i], limb 1 <= 2^25 - 1 + kFuLimb1Spill)"""
    n = 0
    for site, rows, want in product_table(name):
        out = probe_lib.run(where, name, rows)
        for h, exp in enumerate(want):
            for i, e in enumerate(exp):
                got = out[i, 10 * h:10 * h + 10]
                if R.val(got) % P != e or not R.is_carried(got):
                    fail(name, f"{site}, half {h}", i, [rows[i][10 * k:10 * k + 10] for k in range(len(rows[i]) // 10)],
                         got, hex(e))
        n += len(rows)
    return n


# ------------------------------------------------------------------------------------------------ field utilities

# fu_tobytes, fu_iszero, fu_isnegative and fu_carry document "any limbs < 2^32 - 2^12"
ANY = [2 ** 32 - 2 ** 12 - 1] * 10
ENCODE_VALUES = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 2 ** 255 - 1, 2 ** 255 + 18]
UTILS = ["fu_carry", "fu_pcarry_even", "fu_add", "fu_sub", "fu_neg", "fu_frombytes", "fu_tobytes", "fu_iszero",
         "fu_isnegative"]
POWERS = ["fu_sqn", "fu_sqn_x2", "fu_invert", "fu_pow22523", "fu_pow22523_x2"]
SQN = [1, 2, 3, 5, 10, 50, 100]


def limb_forms(v):
    """limb forms of the integer v inside the class ANY: its own radix limbs (what is above bit 230 in limb 9), the same
    with every limb above a non-zero one lending it one unit, the largest limbs of the class with the same residue, and
    the radix limbs plus FU_KC and plus FU_K2C (the shapes fu_sub leaves)"""
    base = R.radix(v)
    lent = list(base)
    for i in range(9, 0, -1):
        if lent[i] > 0:
            lent[i] -= 1
            lent[i - 1] += 1 << W[i - 1]
    out = [base, lent, R.max_rep(v, ANY), [a + b for a, b in zip(base, R.KC)], [a + b for a, b in zip(base, R.K2C)]]
    assert all((R.val(f) - v) % P == 0 and all(0 <= f[i] <= ANY[i] for i in range(10)) for f in out)
    assert R.val(base) == v and R.val(lent) == v
    return out


def encode_cases():
    rs = np.random.default_rng(0xE2C)
    cols = [rs.integers(0, m + 1, size=2048, dtype=np.uint64) for m in ANY]
    out = [f for v in ENCODE_VALUES for f in limb_forms(v)]
    out += [list(ANY), [0] * 10] + [[int(c[k]) for c in cols] for k in range(2048)]
    return out


def check_util(where, name):
    rng = random.Random(sum(map(ord, name)))
    if name in ("fu_tobytes", "fu_iszero", "fu_isnegative"):
        rows = encode_cases()
        out = probe_lib.run(where, name, rows)
        for i, f in enumerate(rows):
            x = R.val(f) % P
            want = {"fu_tobytes": R.words(x), "fu_iszero": [int(x == 0)], "fu_isnegative": [x & 1]}[name]
            if list(map(int, out[i])) != want:
                fail(name, "limbs < 2^32 - 2^12", i, [f], out[i], want)
        return len(rows)
    if name == "fu_carry":       # limbs < 2^32 - 2^12 -> the same value mod p, carried
        rows = encode_cases()
        out = probe_lib.run(where, name, rows)
        for i, f in enumerate(rows):
            if (R.val(out[i]) - R.val(f)) % P or not R.is_carried(out[i]):
                fail(name, "limbs < 2^32 - 2^12", i, [f], out[i], "same value, carried")
        return len(rows)
    if name == "fu_pcarry_even":  # any even limbs, odd limbs < 2^32 - 2^6: the same integer, even limbs < 2^26
        cmax = [U32 if i % 2 == 0 else U32 - 64 for i in range(10)]
        rows = [[rng.randint(0, m) for m in cmax] for _ in range(2048)] + edge_members(cmax)
        out = probe_lib.run(where, name, rows)
        for i, f in enumerate(rows):
            want = list(f)
            for j in range(0, 10, 2):
                want[j + 1] += want[j] >> 26
                want[j] &= (1 << 26) - 1
            if list(map(int, out[i])) != want or R.val(out[i]) != R.val(f):
                fail(name, "odd limbs < 2^32 - 2^6", i, [f], out[i], want)
        return len(rows)
    if name == "fu_add":          # limb sums below 2^32
        rows = [[rng.randint(0, 2 ** 31 - 1) for _ in range(20)] for _ in range(2048)]
        rows += [[2 ** 31 - 1] * 20, [0] * 20, [U32] * 10 + [0] * 10]
        out = probe_lib.run(where, name, rows)
        for i, r in enumerate(rows):
            want = [a + b for a, b in zip(r[:10], r[10:])]
            if list(map(int, out[i])) != want:
                fail(name, "sums < 2^32", i, [r[:10], r[10:]], out[i], want)
        return len(rows)
    if name in ("fu_sub", "fu_neg"):   # g <= K limb-wise (K dominates the subtrahend), f + K < 2^32
        n = 0
        for arg, K in ((0, R.KC), (1, R.K2C)):
            gs = [[rng.randint(0, k) for k in K] for _ in range(2048)] + edge_members(K)
            gs += [R.max_rep(x, K) for x in SPECIAL] + [R.canon(x) for x in SPECIAL]
            fs = [[rng.randint(0, U32 - k) for k in K] for _ in gs]
            fs[-1] = [U32 - k for k in K]
            rows = [f + g for f, g in zip(fs, gs)] if name == "fu_sub" else gs
            out = probe_lib.run(where, name, rows, arg)
            for i, g in enumerate(gs):
                f = fs[i] if name == "fu_sub" else [0] * 10
                want = [a + k - b for a, k, b in zip(f, K, g)]
                if list(map(int, out[i])) != want or (R.val(out[i]) - R.val(f) + R.val(g)) % P:
                    fail(name, "FU_K2C" if arg else "FU_KC", i, [f, g], out[i], want)
            n += len(rows)
        return n
    if name == "fu_frombytes":    # bit 255 ignored, y >= p kept as it is: the limbs of v mod 2^255, each below 2^W[i]
        ys = [0, 1, 19, P - 1, P, P + 1, P + 18, 2 ** 255 - 1, 2 ** 254, 2 ** 230 - 1, 2 ** 230]
        vs = [y | (s << 255) for y in ys for s in (0, 1)] + [rng.getrandbits(256) for _ in range(2048)]
        out = probe_lib.run(where, name, [R.words(v) for v in vs])
        for i, v in enumerate(vs):
            want = R.radix(v & (2 ** 255 - 1))
            if list(map(int, out[i])) != want:
                fail(name, "256 bits", i, [R.words(v)], out[i], want)
        return len(vs)
    raise KeyError(name)


def power_inputs():
    """0, 1, p - 1, sqrt(-1), d and 512 random elements, in canonical limbs and in the largest carried limbs"""
    rng = random.Random(0x22523)
    xs = [0, 1, P - 1, R.SQRT_M1, R.D] + [rng.randrange(P) for _ in range(512)]
    return [(x, f) for x in xs for f in (R.canon(x), R.max_rep(x, R.CARRIED))]



def check_power(where, name):
    """fu_sqn (n in SQN), fu_invert, fu_pow22523 and the two-way forms against pow(); carried inputs and outputs"""
    a = power_inputs()
    b = list(a)
    random.Random(5).shuffle(b)
    two = name.endswith("_x2")
    rows = [f + g for (_, f), (_, g) in zip(a, b)] if two else [f for _, f in a]
    n = 0
    for arg in (SQN if name.startswith("fu_sqn") else [0]):
        e = {"fu_sqn": 2 ** arg, "fu_sqn_x2": 2 ** arg, "fu_invert": P - 2, "fu_pow22523": (P - 5) // 8,
             "fu_pow22523_x2": (P - 5) // 8}[name]
        out = probe_lib.run(where, name, rows, arg)
        for h, src in enumerate((a, b) if two else (a,)):
            for i, (x, f) in enumerate(src):
                got = out[i, 10 * h:10 * h + 10]
                if R.val(got) % P != pow(x, e, P) or not R.is_carried(got):
                    fail(name, f"n={arg}, half {h}", i, [f], got, hex(pow(x, e, P)))
        n += len(rows)
    return n


# ------------------------------------------------------------------------------------------------ group law

GROUP = ["gu_dbl_p2", "gu_dbl_p3", "gu_p3_to_cached", "gu_add", "gu_niels_cneg", "gu_madd", "gu_p2_is_identity",
         "gu_p2_mul8_is_identity", "gu_cofactored_eq"]
_POINTS = None


def pts():
    global _POINTS
    if _POINTS is None:
        _POINTS = R.points()
    return _POINTS


def p3_reps(p, rng):
    """(X, Y, Z, T) limbs of the affine point p in three representations: canonical limbs with Z = 1, canonical limbs
    with a random non-zero Z, and the largest carried limbs (the operand class of every group-law function's point
    arguments) of that second form's coordinates"""
    x, y = p
    z = rng.randrange(1, P)
    c = (x * z % P, y * z % P, z, x * y * z % P)
    return [[R.canon(x), R.canon(y), R.canon(1), R.canon(x * y)], [R.canon(v) for v in c],
            [R.max_rep(v, R.CARRIED) for v in c]]


def niels_reps(p):
    """(y + x, y - x, 2 d x y) of the affine point p, carried: canonical and largest limbs"""
    x, y = p
    c = ((y + x) % P, (y - x) % P, 2 * R.D * x * y % P)
    return [[R.canon(v) for v in c], [R.max_rep(v, R.CARRIED) for v in c]]


def flat(coords):
    return [v for c in coords for v in c]


def check_point(name, site, i, ins, got, want, has_t):
    """got = (X, Y, Z[, T]) limbs: carried, Z != 0, (X/Z, Y/Z) = want, T Z = X Y"""
    vals = [R.val(got[10 * k:10 * k + 10]) % P for k in range(4 if has_t else 3)]
    ok = R.is_carried(got[:10]) and R.is_carried(got[10:20]) and R.is_carried(got[20:30]) and vals[2] != 0
    if ok:      # X/Z = x and Y/Z = y, cross-multiplied
        ok = (vals[0] - want[0] * vals[2]) % P == 0 and (vals[1] - want[1] * vals[2]) % P == 0
        if has_t:
            ok = ok and R.is_carried(got[30:40]) and (vals[3] * vals[2] - vals[0] * vals[1]) % P == 0
    if not ok:
        fail(name, site, i, ins, got, want)


def pair_list(rng):
    """(site, P, Q): for every test point P: P + P, P + (-P), P + identity, P + each small-order point, P + a random Q"""
    ps = pts()
    out = []
    for nm, p in ps:
        out.append((f"{nm} + itself", p, p))
        out.append((f"{nm} + its negative", p, R.neg(p)))
        out += [(f"{nm} + [{j}]T8", p, t) for j, t in enumerate(R.TORSION)]     # j = 0: the identity
        qn, q = ps[rng.randrange(len(ps))]
        out.append((f"{nm} + {qn}", p, q))
    return out


def check_group(where, name):
    rng = random.Random(sum(map(ord, name)))
    ps = pts()
    if name in ("gu_dbl_p2", "gu_dbl_p3"):
        cases = [(f"{nm} rep {r}", p, rep) for nm, p in ps for r, rep in enumerate(p3_reps(p, rng))]
        rows = [flat(rep[:3]) for _, _, rep in cases]
        out = probe_lib.run(where, name, rows)
        for i, (site, p, rep) in enumerate(cases):
            check_point(name, site, i, rep[:3], out[i], R.add(p, p), name == "gu_dbl_p3")
        return len(rows)
    if name in ("gu_p2_is_identity", "gu_p2_mul8_is_identity"):
        cases = [(f"{nm} rep {r}", p, rep) for nm, p in ps for r, rep in enumerate(p3_reps(p, rng))]
        rows = [flat(rep[:3]) for _, _, rep in cases]
        out = probe_lib.run(where, name, rows)
        truth = 0
        for i, (site, p, rep) in enumerate(cases):
            want = int(p == R.IDENT if name == "gu_p2_is_identity" else R.in_torsion(p))
            truth += want
            if int(out[i, 0]) != want:
                fail(name, site, i, rep[:3], out[i], want)
        assert 0 < truth < len(cases)
        return len(rows)
    if name == "gu_p3_to_cached":
        n = 0
        cases = [(f"{nm} rep {r}", p, rep) for nm, p in ps for r, rep in enumerate(p3_reps(p, rng))]
        rows = [flat(rep) for _, _, rep in cases]
        for neg in (0, 1):
            out = probe_lib.run(where, name, rows, neg)
            for i, (site, p, rep) in enumerate(cases):
                X, Y, Z, T = (R.val(c) for c in rep)
                want = [(Y + X) % P, (Y - X) % P, 2 * Z % P, 2 * R.D * T % P]
                if neg:
                    want = [want[1], want[0], want[2], (-want[3]) % P]
                if [R.val(out[i, 10 * k:10 * k + 10]) % P for k in range(4)] != want:
                    fail(name, f"{site} neg={neg}", i, rep, out[i], want)
            n += len(rows)
        return n
    if name == "gu_niels_cneg":
        n = 0
        cases = [(f"{nm} rep {r}", p, rep) for nm, p in ps for r, rep in enumerate(niels_reps(p))]
        rows = [flat(rep) for _, _, rep in cases]
        for neg in (0, 1):
            out = probe_lib.run(where, name, rows, neg)
            for i, (site, p, rep) in enumerate(cases):
                q = R.neg(p) if neg else p
                want = [(q[1] + q[0]) % P, (q[1] - q[0]) % P, 2 * R.D * q[0] * q[1] % P]
                if [R.val(out[i, 10 * k:10 * k + 10]) % P for k in range(3)] != want:
                    fail(name, f"{site} neg={neg}", i, rep, out[i], want)
            n += len(rows)
        return n
    if name in ("gu_add", "gu_madd"):
        cases = []
        for site, p, q in pair_list(rng):
            preps = p3_reps(p, rng)
            qreps = p3_reps(q, rng) if name == "gu_add" else niels_reps(q)
            for r, prep in enumerate(preps):
                cases.append((f"{site} rep {r}", p, q, prep, qreps[r % len(qreps)]))
        rows = [flat(a) + flat(b) for _, _, _, a, b in cases]
        n = 0
        for neg in (0, 1):
            out = probe_lib.run(where, name, rows, neg)
            for i, (site, p, q, a, b) in enumerate(cases):
                check_point(name, f"{site} neg={neg}", i, a + b, out[i], R.add(p, R.neg(q) if neg else q), True)
            n += len(rows)
        return n
    if name == "gu_cofactored_eq":
        # P as gu_p1p1_to_p3 leaves it (carried, any Z); R a decoded point: Z = 1, X and T carried, Y the limbs of an
        # integer below 2^255 (y, or y + p where that fits). True iff [8](P - R) is the identity.
        cases = []
        for nm, p in ps:
            others = [(f"+[{j}]T8", R.add(p, t)) for j, t in enumerate(R.TORSION)] + [("negative", R.neg(p))]
            qn, q = ps[rng.randrange(len(ps))]
            others.append((qn, q))
            preps = p3_reps(p, rng)
            for k, (on, o) in enumerate(others):
                x, y = o
                ys = [R.canon(y)] + ([R.radix(y + P)] if y + P < 2 ** 255 else [])
                rep = [R.canon(x), ys[-1], R.canon(1), R.canon(x * y)]
                if k % 2:
                    rep = [R.max_rep(x, R.CARRIED), ys[0], R.canon(1), R.max_rep(x * y, R.CARRIED)]
                cases.append((f"{nm} vs {on}", R.add(p, R.neg(o)), preps[k % 3], rep))
        rows = [flat(a) + flat(b) for _, _, a, b in cases]
        out = probe_lib.run(where, name, rows)
        truth = 0
        for i, (site, diff, a, b) in enumerate(cases):
            want = int(R.in_torsion(diff))
            truth += want
            if int(out[i, 0]) != want:
                fail(name, site, i, a + b, out[i], want)
        assert 0 < truth < len(cases)
        return len(rows)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ decode

DECODES = ["gu_frombytes", "gu_frombytes_x2"]


def decode_inputs():
    """all 14 small-order encodings (x = 0 with the sign bit among them); y = p .. 2^255 - 1 with both sign bits; the
    off-curve sweep of the `edge` fixture (its class-7 keys); 1,024 random encodings"""
    rng = random.Random(0xDEC0)
    out = list(zr.torsion_encodings())
    out += [rr.enc_y(y, s) for y in range(P, 2 ** 255) for s in (0, 1)]
    out += [rr.enc_y(1, 1), rr.enc_y(P - 1, 1)]
    g = golden_io.load("edge")
    sweep = [g.pk[i].tobytes() for i in range(g.n) if g.cls[i] == 7]
    assert 0 < sum(not rr.decode(e)[0] for e in sweep) < len(sweep)    # the sweep crosses y values on and off the curve
    out += sweep
    out += [rng.getrandbits(256).to_bytes(32, "little") for _ in range(1024)]
    return out


def check_decode(where, name):
    """ok and x against dalek's sqrt_ratio_i decode (reason_ref.decode); Y the limbs of the encoded y, unreduced; T = X Y"""
    a = decode_inputs()
    b = list(a)
    random.Random(6).shuffle(b)
    two = name == "gu_frombytes_x2"
    as_words = lambda e: R.words(int.from_bytes(e, "little"))
    rows = [as_words(e) + as_words(f) for e, f in zip(a, b)] if two else [as_words(e) for e in a]
    out = probe_lib.run(where, name, rows)
    oks = 0
    for h, src in enumerate((a, b) if two else (a,)):
        for i, e in enumerate(src):
            got = out[i, 31 * h:31 * h + 31]
            ok, x = rr.decode(e)
            oks += ok
            y = rr.y_of(e)
            good = int(got[30]) == int(ok) and list(map(int, got[10:20])) == R.radix(y)
            if good and ok:
                X, T = R.val(got[:10]) % P, R.val(got[20:30]) % P
                good = X == x and T == x * y % P and R.is_carried(got[:10]) and R.is_carried(got[20:30])
            if not good:
                fail(name, f"half {h}", i, [as_words(e)], got, (ok, hex(x)))
    assert 0 < oks < len(a) * (2 if two else 1)
    return len(rows)


# ------------------------------------------------------------------------------------------------ scalars

SCALARS = ["sc_reduce512", "lattice", "sc_recode2_joint", "sc_recode4", "sc_recode4_hi8", "sc_recode8", "sc_recode16",
           "sc_recode_w10", "sc_recode_w16", "sc_recode_w20", "sc_recode_w24"]
REC2_MAX = 2 * (4 ** 128 - 1) // 3     # the largest value 128 digits in {-1, 0, 1, 2} hold


def rec2_count(s):
    m = 0
    while s > 2 * (4 ** m - 1) // 3:
        m += 1
    return m


def recode_inputs(limit, rng):
    """0, 1, 2 (4^m - 1) / 3 and that plus one for several m, powers of two and their neighbours, the largest admitted
    value limit - 1, and 2,048 random values below limit"""
    out = [0, 1, limit - 1, limit - 2, limit // 2, limit // 2 - 1]
    for m in (1, 2, 3, 8, 16, 17, 32, 63, 64, 65, 100, 126, 127, 128):
        out += [2 * (4 ** m - 1) // 3, 2 * (4 ** m - 1) // 3 + 1]
    for b in (3, 4, 7, 8, 15, 16, 31, 32, 33, 63, 64, 127, 128, 129, 251, 252):
        out += [2 ** b - 1, 2 ** b, 2 ** b + 1, 3 * 2 ** (b - 1), 2 ** (b + 1) - 2 ** (b - 3)]
    out += [int("8" * 63, 16), int("7" * 63, 16), int("80" * 31, 16), int("7f" * 31, 16), int("8000" * 15, 16)]
    out = [v for v in out if 0 <= v < limit]
    out += [rng.randrange(limit) for _ in range(2048)] + [rng.randrange(2 ** b) for b in range(1, 250, 3)]
    return out


def digits(ws, width, count, bias):
    v = R.unwords(ws)
    return [((v >> (width * i)) & ((1 << width) - 1)) - bias for i in range(count)]


def check_scalar(where, name):
    rng = random.Random(sum(map(ord, name)))
    if name == "sc_reduce512":
        xs = [0, L - 1, L, L + 1, 2 ** 252, 2 ** 256 - 1, 2 ** 512 - 1]
        for m in (1, 2, 3, 15, 16, 2 ** 32 - 1, 2 ** 64 + 1, 2 ** 128 - 1, 2 ** 200 + 12345, 2 ** 252, 2 ** 256 + 7,
                  2 ** 258 + 2 ** 100, 2 ** 259, (2 ** 512 - 1) // L):
            xs += [m * L - 1, m * L, m * L + 1]
        xs = [x for x in xs if x < 2 ** 512]
        xs += [rng.getrandbits(512) for _ in range(2048)]
        out = probe_lib.run(where, name, [R.words(x, 16) for x in xs])
        for i, x in enumerate(xs):
            if R.unwords(out[i]) != x % L:
                fail(name, "512 bits", i, [R.words(x, 16)], out[i], hex(x % L))
        return len(xs)
    if name == "lattice":
        return check_lattice(where)
    if name == "sc_recode2_joint":   # any 256-bit values; 129 (fail closed) above REC2_MAX
        xs = recode_inputs(2 ** 256, rng) + [REC2_MAX - 1, REC2_MAX, REC2_MAX + 1, 2 ** 255 - 1, 2 ** 255, 2 ** 255 + 1]
        ys = list(xs)
        rng.shuffle(ys)
        out = probe_lib.run(where, name, [R.words(a) + R.words(b) for a, b in zip(xs, ys)])
        closed = 0
        for i, (a, b) in enumerate(zip(xs, ys)):
            cnt = [rec2_count(v) if v <= REC2_MAX else 129 for v in (a, b)]
            good = int(out[i, 16]) == max(cnt)
            closed += max(cnt) == 129
            for v, c, ws in ((a, cnt[0], out[i, :8]), (b, cnt[1], out[i, 8:16])):
                if c <= 128:     # the digits reconstruct the value, lie in {-1, 0, 1, 2}, and none is set at or above c
                    ds = digits(ws, 2, 128, 1)
                    good = good and sum(d << (2 * j) for j, d in enumerate(ds)) == v and not any(ds[c:])
                    good = good and (c == 0 or ds[c - 1] > 0)
            if not good:
                fail(name, "256 bits", i, [R.words(a), R.words(b)], out[i], cnt)
        assert closed
        return len(xs)
    # (digit width, digit count, stored bias, lowest digit, highest digit, admitted limit)
    spec = {"sc_recode4": (4, 64, 8, -8, 7, 2 ** 253), "sc_recode4_hi8": (4, 64, 7, -7, 8, 2 ** 255),
            "sc_recode8": (8, 32, 128, -128, 127, 2 ** 253), "sc_recode16": (16, 16, 2 ** 15, -2 ** 15, 2 ** 15 - 1, 2 ** 253)}
    if name in spec:
        width, count, bias, lo, hi, limit = spec[name]
        xs = recode_inputs(limit, rng)
        out = probe_lib.run(where, name, [R.words(x) for x in xs])
        for i, x in enumerate(xs):
            ds = digits(out[i], width, count, bias)
            good = sum(d << (width * j) for j, d in enumerate(ds)) == x and all(lo <= d <= hi for d in ds)
            if name == "sc_recode4":
                good = good and 0 <= ds[63] <= 2
            if name == "sc_recode4_hi8":   # a value below 2^(4m - 1) needs only m digits
                m = next(m for m in range(65) if 2 * x < 16 ** m)
                good = good and not any(ds[m:])
            if not good:
                fail(name, f"below 2^{limit.bit_length() - 1}", i, [R.words(x)], out[i], hex(x))
        return len(xs)
    wb = int(name[len("sc_recode_w"):])       # s < 2^253 -> ceil(254 / WB) digits in [-2^(WB-1), 2^(WB-1)), one a word
    nd = (254 + wb - 1) // wb
    xs = recode_inputs(2 ** 253, rng)
    out = probe_lib.run(where, name, [R.words(x) for x in xs])
    assert out.shape[1] == nd
    for i, x in enumerate(xs):
        ds = [int(w) - (1 << (wb - 1)) for w in out[i]]
        if sum(d << (wb * j) for j, d in enumerate(ds)) != x or not all(-(1 << (wb - 1)) <= d < 1 << (wb - 1) for d in ds):
            fail(name, "below 2^253", i, [R.words(x)], out[i], hex(x))
    return len(xs)


def lattice_tables():
    rng = random.Random(0x1A77)
    return [("corner", tl.corner_ks(), 4), ("near threshold", tl.near_threshold_ks(), 4),
            ("random", [(rng.randrange(L), rng.randrange(L)) for _ in range(4096)], 1)]


def lattice_records(where, pairs):
    out = probe_lib.run(where, "lattice", [R.words(k) + R.words(s) for k, s in pairs])
    return out, [(R.unwords(r[:8]), R.unwords(r[8:16]) * (-1 if r[16] else 1), int(r[17]), R.unwords(r[18:26])) for r in out]


def check_lattice(where):
    """the assertions of tests/test_lattice_host.py (its check()) on the record of lattice_reduce + sc_mul_signed; on the
    device also the same record as the host compile, word for word"""
    n = 0
    for site, pairs, slack in lattice_tables():
        raw, res = lattice_records(where, pairs)
        try:
            worst = tl.check(pairs, res, slack)
        except AssertionError as e:
            raise AssertionError(f"lattice [{site}]: {e}") from e
        assert worst <= (140 if site == "random" else 253), (site, worst)
        if where != probe_lib.HOST:
            host, _ = lattice_records(probe_lib.HOST, pairs)
            diff = np.nonzero((raw != host).any(axis=1))[0]
            if len(diff):
                i = int(diff[0])
                fail("lattice", f"{site}: device record differs from the host's", i, [R.words(pairs[i][0])], raw[i],
                     list(map(int, host[i])))
        n += len(pairs)
    return n
