"""References for the probe tests (tests/probe_cases.py), in Python integers: the limb forms of GF(2^255 - 19) elements
(radix 2^25.5, at2v_fu_base.h), affine twisted Edwards arithmetic, the test points, and 32-bit word helpers. The decode
reference is reason_ref.decode (dalek's sqrt_ratio_i), the lattice reference tools/halfscalar_proto.lattice."""
import importlib.util
import os
import random

import reason_ref as rr
import zip215_ref as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L, D = rr.P, rr.L, rr.D
N8 = 8 * L
D2 = 2 * D % P
SQRT_M1 = rr.SQRT_M1
OFF = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
W = [26, 25] * 5


def gen_fu():
    """tools/gen_fu.py as a module (its classes, constants and proofs)"""
    spec = importlib.util.spec_from_file_location("gen_fu", os.path.join(ROOT, "tools", "gen_fu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = gen_fu()
_D = GEN.derive()
CARRIED = list(_D["C"])                  # limb i <= 2^W[i] - 1, limb 1 <= 2^25 - 1 + kFuLimb1Spill
SPILL = _D["spill"]
KC, K2C = list(_D["K"]["C"]), list(_D["K"]["2C"])
assert CARRIED == [(1 << W[i]) - 1 + (SPILL if i == 1 else 0) for i in range(10)]


# ---- limbs

def val(limbs) -> int:
    return sum(int(v) << OFF[i] for i, v in enumerate(limbs))


def radix(v: int):
    """the limbs of the integer v itself: limb i < 2^W[i] for i < 9, everything above bit 230 in limb 9"""
    assert 0 <= v and (v >> 230) < 2 ** 32
    return [(v >> OFF[i]) & ((1 << W[i]) - 1) for i in range(9)] + [v >> 230]


def canon(x: int):
    """the canonical limbs of x mod p"""
    return radix(x % P)


def max_rep(x: int, cmax):
    """the representative of x mod p with the largest limbs inside the class `cmax` (per-limb maxima, each at least
    2^W[i] - 1): the largest integer V <= val(cmax) with V = x (mod p), as cmax minus the canonical limbs of the gap"""
    top = val(cmax)
    gap = (top - x) % P
    g = radix(gap)
    out = [cmax[i] - g[i] for i in range(10)]
    assert all(0 <= out[i] <= cmax[i] for i in range(10)) and (val(out) - x) % P == 0
    return out


def is_carried(limbs) -> bool:
    return all(0 <= int(v) <= CARRIED[i] for i, v in enumerate(limbs))


def words(v: int, n: int = 8):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def unwords(ws) -> int:
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def inv(x: int) -> int:
    return pow(x, -1, P)


# ---- affine twisted Edwards, -x^2 + y^2 = 1 + d x^2 y^2 (the addition law is complete: d is no square)

IDENT = (0, 1)


def on_curve(p) -> bool:
    x, y = p
    return (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def add(p, q):
    x1, y1 = p
    x2, y2 = q
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * inv(1 + t) % P, (y1 * y2 + x1 * x2) * inv(1 - t) % P)


def neg(p):
    return ((-p[0]) % P, p[1])


def mul(k: int, p):
    q = IDENT
    for bit in bin(k)[2:]:
        q = add(q, q)
        if bit == "1":
            q = add(q, p)
    return q


def affine(ext):
    """an extended point of zip215_ref -> (x, y)"""
    zi = inv(ext[2])
    return (ext[0] * zi % P, ext[1] * zi % P)


B = affine(zr.BASE)
TORSION = [affine(t) for t in zr.TORSION]      # [j]T8, j = 0..7: the eight points of order dividing 8


def in_torsion(p) -> bool:
    return mul(8, p) == IDENT


def points():
    """(name, (x, y)): the eight small-order points, B, 2B, a B + T for every small-order T (mixed order for T != 0),
    and 256 random points r B + T (seeded)"""
    rng = random.Random(0x9047)
    a_b = affine(zr.mul_base(zr.SECRET_A))
    out = [(f"[{j}]T8", t) for j, t in enumerate(TORSION)]
    out += [("B", B), ("2B", add(B, B))]
    out += [(f"aB+[{j}]T8", add(a_b, t)) for j, t in enumerate(TORSION)]
    for i in range(256):
        out.append((f"random#{i}", add(affine(zr.mul_base(rng.randrange(1, L))), TORSION[rng.randrange(8)])))
    assert all(on_curve(p) for _, p in out)
    return out
