"""A limb-exact model of dkg_amd/csrc/fe25519.h and sc25519.h ON VALUES, the big-integer reference next
to it, and the test vectors at the corners of the primitives' stated input ranges.

The model restates each primitive limb for limb with the code's 32- and 64-bit wrap-around.  The
products take their terms from the header text through tools/fe_bounds._parse_terms (the parse the
bound checker uses), followed by an exact product-scanning pass (FE_LIMB / FE_FOLD, flavour 1) or an
exact fe_carry64 pass (flavour 2).  The reference is plain integers mod p = 2^255 - 19 and mod l and
never looks at limbs.  tests/test_fe_model.py validates model and vectors on the CPU;
tests/test_gpu_field_ops.py and tests/test_gpu_scalar_ops.py run the same lists through the device
(dkg_fe_ops / dkg_sc_ops)."""
import functools
import json
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fe_bounds as F  # noqa: E402

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
W, OFF, MASK, P2 = F.W, F.OFF, F.MASK, F.P2
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
ZERO = [0] * 10
P_LIMBS = [0x3ffffed] + [MASK[i] for i in range(1, 10)]
TIGHT_MAX = [(1 << 26) + 63 if i % 2 == 0 else (1 << 25) + 4095 for i in range(10)]
SQRT_M1 = pow(2, (P - 1) // 4, P)


def value(limbs):
    return sum(x << OFF[i] for i, x in enumerate(limbs))


def split(v):
    """The limbs of v < 2^256 in their nominal widths (limb 9 takes what is left)."""
    return [(v >> OFF[i]) & MASK[i] for i in range(9)] + [v >> OFF[9]]


def is_tight(limbs):
    return all(x < ((1 << 26) + (1 << 6) if i % 2 == 0 else (1 << 25) + (1 << 12)) for i, x in enumerate(limbs))


# ------------------------------------------------------------------ the field model (fe25519.h)
def fe_add(a, b):
    return [(a[i] + b[i]) & M32 for i in range(10)]


def fe_sub(a, b):
    return [(a[i] + P2[i] - b[i]) & M32 for i in range(10)]


def fe_neg(a):
    return [(P2[i] - a[i]) & M32 for i in range(10)]


def fe_dbl(a):
    return [(2 * x) & M32 for x in a]


def fe_carry(a):
    c = [a[i] >> W[i] for i in range(10)]
    return [((a[0] & MASK[0]) + 19 * c[9]) & M32] + [((a[i] & MASK[i]) + c[i - 1]) & M32 for i in range(1, 10)]


@functools.lru_cache(maxsize=None)
def _plan(func):
    """The header's product terms of `func`, compiled: the distinct operands (source, limb, weight) and
    per column the index pairs."""
    cols = F._parse_terms(func)
    names = sorted({n for k in cols for t in cols[k] for n in t})
    spec = []
    for n in names:
        m = re.fullmatch(r"([fg])(\d)(?:_(\d+))?", n)
        assert m, n
        spec.append((m.group(1) == "g", int(m.group(2)), int(m.group(3) or 1)))
    idx = {n: i for i, n in enumerate(names)}
    return spec, [[(idx[x], idx[y]) for x, y in cols[k]] for k in range(10)]


def columns(func, f, g):
    """The ten column sums as the code forms them: 32-bit pre-multiplies (19u * g, dbl32), 32 x 32 -> 64
    products, 64-bit sums."""
    spec, plan = _plan(func)
    ops = [((g if isg else f)[i] * k) & M32 for isg, i, k in spec]
    return [sum(ops[a] * ops[b] for a, b in col) for col in plan]


def scan(cols, mutant=None, trace=None):
    """FE_LIMB per column on one 64-bit accumulator, then FE_FOLD."""
    r, h = [0] * 10, 0
    for k in range(10):
        h = (h + cols[k]) & M64
        r[k] = h & MASK[k]
        h >>= W[k]
    if trace is not None:
        trace["fold_carry"] = h
    t = (r[0] + (h & M32) * 19) & M64
    if mutant != "fold_hi":
        t = (t + (((19 * (h >> 32)) & M32) << 32)) & M64
    r[0] = t & 0x3ffffff
    r[1] = (r[1] + ((t >> 26) & M32)) & M32
    return r


_CARRY64 = [(0, 1), (4, 5), (1, 2), (5, 6), (2, 3), (6, 7), (3, 4), (7, 8), (4, 5), (8, 9)]


def carry64(cols, mutant=None, trace=None):
    """fe_carry64, statement by statement.  Mutants: "h4_second" leaves out the addition of the second
    carry out of h4 into h5; "signed" shifts the columns arithmetically (a port of the signed carry
    chain this one descends from)."""
    h = [x & M64 for x in cols]
    if trace is not None:
        trace["col_max"] = max(h)

    def shr(x, n):
        if mutant == "signed" and x >> 63:
            return ((x - (1 << 64)) >> n) & M64
        return x >> n

    for n, (i, j) in enumerate(_CARRY64):
        c = shr(h[i], W[i])
        if n == 8 and trace is not None:
            trace["h4_second"] = c
        if not (n == 8 and mutant == "h4_second"):
            h[j] = (h[j] + c) & M64
        h[i] &= MASK[i]
    c = shr(h[9], 25)
    h[0] = (h[0] + c * 19) & M64
    h[9] &= MASK[9]
    c = shr(h[0], 26)
    h[1] = (h[1] + c) & M64
    h[0] &= MASK[0]
    return [x & M32 for x in h]


def _reduce(flavour, cols, mutant, trace):
    return scan(cols, mutant, trace) if flavour == 1 else carry64(cols, mutant, trace)


def fe_mul(f, g, flavour, mutant=None, trace=None):
    return _reduce(flavour, columns("fe_mul_ps" if flavour == 1 else "fe_mul_cs", f, g), mutant, trace)


def fe_sq(f, flavour, mutant=None, trace=None):
    return _reduce(flavour, columns("fe_sq_ps" if flavour == 1 else "fe_sq_cs", f, f), mutant, trace)


def fe_mul_small(a, k, flavour, mutant=None, trace=None):
    cols = F._parse_terms("fe_mul_small_ps")
    assert all(c == [(f"a.v[{i}]", "k")] for i, c in cols.items())
    return _reduce(flavour, [a[i] * k for i in range(10)], mutant, trace)


def fe_sqn(a, n, fl):
    for _ in range(n):
        a = fe_sq(a, fl)
    return a


def fe_pow22523(z, fl):
    t0 = fe_sq(z, fl)
    t1 = fe_sqn(t0, 2, fl)
    t1 = fe_mul(z, t1, fl)
    t0 = fe_mul(t0, t1, fl)
    t0 = fe_sq(t0, fl)
    t0 = fe_mul(t1, t0, fl)
    t1 = fe_sqn(t0, 5, fl)
    t0 = fe_mul(t1, t0, fl)
    t1 = fe_sqn(t0, 10, fl)
    t1 = fe_mul(t1, t0, fl)
    t2 = fe_sqn(t1, 20, fl)
    t1 = fe_mul(t2, t1, fl)
    t1 = fe_sqn(t1, 10, fl)
    t0 = fe_mul(t1, t0, fl)
    t1 = fe_sqn(t0, 50, fl)
    t1 = fe_mul(t1, t0, fl)
    t2 = fe_sqn(t1, 100, fl)
    t1 = fe_mul(t2, t1, fl)
    t1 = fe_sqn(t1, 50, fl)
    t0 = fe_mul(t1, t0, fl)
    t0 = fe_sqn(t0, 2, fl)
    return fe_mul(t0, z, fl)


def fe_invert(z, fl):
    t0 = fe_sq(z, fl)
    t1 = fe_sqn(t0, 2, fl)
    t1 = fe_mul(z, t1, fl)
    t0 = fe_mul(t0, t1, fl)
    t2 = fe_sq(t0, fl)
    t1 = fe_mul(t1, t2, fl)
    t2 = fe_sqn(t1, 5, fl)
    t1 = fe_mul(t2, t1, fl)
    t2 = fe_sqn(t1, 10, fl)
    t2 = fe_mul(t2, t1, fl)
    t3 = fe_sqn(t2, 20, fl)
    t2 = fe_mul(t3, t2, fl)
    t2 = fe_sqn(t2, 10, fl)
    t1 = fe_mul(t2, t1, fl)
    t2 = fe_sqn(t1, 50, fl)
    t2 = fe_mul(t2, t1, fl)
    t3 = fe_sqn(t2, 100, fl)
    t2 = fe_mul(t3, t2, fl)
    t2 = fe_sqn(t2, 50, fl)
    t1 = fe_mul(t2, t1, fl)
    t1 = fe_sqn(t1, 5, fl)
    return fe_mul(t1, t0, fl)


def fe_tobytes32(a):
    t = fe_carry(fe_carry(a))
    q = ((t[0] + 19) & M32) >> 26
    for i in range(1, 10):
        q = ((t[i] + q) & M32) >> W[i]
    t[0] = (t[0] + 19 * q) & M32
    for i in range(9):
        t[i + 1] = (t[i + 1] + (t[i] >> W[i])) & M32
        t[i] &= MASK[i]
    t[9] &= MASK[9]
    sh = lambda x, n: (x << n) & M32  # noqa: E731
    return [t[0] | sh(t[1], 26), (t[1] >> 6) | sh(t[2], 19), (t[2] >> 13) | sh(t[3], 13), (t[3] >> 19) | sh(t[4], 6),
            t[5] | sh(t[6], 25), (t[6] >> 7) | sh(t[7], 19), (t[7] >> 13) | sh(t[8], 12), (t[8] >> 20) | sh(t[9], 6)]


def fe_frombytes32(s):
    sh = lambda x, n: (x << n) & M32  # noqa: E731
    return [s[0] & 0x3ffffff, ((s[0] >> 26) | sh(s[1], 6)) & 0x1ffffff, ((s[1] >> 19) | sh(s[2], 13)) & 0x3ffffff,
            ((s[2] >> 13) | sh(s[3], 19)) & 0x1ffffff, (s[3] >> 6) & 0x3ffffff, s[4] & 0x1ffffff,
            ((s[4] >> 25) | sh(s[5], 7)) & 0x3ffffff, ((s[5] >> 19) | sh(s[6], 13)) & 0x1ffffff,
            ((s[6] >> 12) | sh(s[7], 20)) & 0x3ffffff, (s[7] >> 6) & 0x1ffffff]


def fe_abs(a):
    return fe_carry(fe_neg(a)) if fe_tobytes32(a)[0] & 1 else list(a)


def words(v, k):
    return [(v >> (32 * i)) & M32 for i in range(k)]


def val(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


def fe_model(op, flavour, t, mutant=None):
    """The output words of dkg_fe_ops for op on the operand tuple t (a flat list of words)."""
    a, b, c, d = t[0:10], t[10:20], t[20:30], t[30:40]
    if op == "mul":
        return fe_mul(a, b, flavour, mutant)
    if op == "sq":
        return fe_sq(a, flavour, mutant)
    if op == "mul2":
        return fe_mul(a, b, flavour, mutant) + fe_mul(c, d, flavour, mutant)
    if op == "sq2":
        return fe_sq(a, flavour, mutant) + fe_sq(b, flavour, mutant)
    if op == "mul_small":
        return fe_mul_small(a, t[10], flavour, mutant)
    if op == "invert":
        return fe_invert(a, flavour)
    if op == "pow22523":
        return fe_pow22523(a, flavour)
    if op == "tobytes":
        s = fe_tobytes32(a)
        return s + [s[0] & 1, int(not any(s))]
    if op == "frombytes":
        return fe_frombytes32(t[0:8])
    return {"carry": lambda: fe_carry(a), "add": lambda: fe_add(a, b), "sub": lambda: fe_sub(a, b),
            "neg": lambda: fe_neg(a), "dbl": lambda: fe_dbl(a), "abs": lambda: fe_abs(a)}[op]()


def fe_ref(op, t):
    """The big-integer result: for the ops that return an element, its value mod p (a list for the pair
    ops); for tobytes the words and flags; for frombytes the exact limbs."""
    a, b, c, d = (value(t[10 * i:10 * i + 10]) for i in range(4))
    if op == "tobytes":
        v = a % P
        return words(v, 8) + [v & 1, int(v == 0)]
    if op == "frombytes":
        return split(val(t[0:8]) & ((1 << 255) - 1))
    if op == "abs":
        v = a % P
        return [P - v if v & 1 else v]
    return {"mul": lambda: [a * b % P], "sq": lambda: [a * a % P], "mul2": lambda: [a * b % P, c * d % P],
            "sq2": lambda: [a * a % P, b * b % P], "mul_small": lambda: [a * t[10] % P], "carry": lambda: [a % P],
            "add": lambda: [(a + b) % P], "sub": lambda: [(a - b) % P], "neg": lambda: [-a % P],
            "dbl": lambda: [2 * a % P], "invert": lambda: [pow(a, P - 2, P)],
            "pow22523": lambda: [pow(a, 2**252 - 3, P)]}[op]()


PRODUCT_OPS = ("mul", "sq", "mul2", "sq2", "mul_small")
TIGHT_OUT = PRODUCT_OPS + ("invert", "pow22523", "abs")


def violations(op, t):
    """The violations tools/fe_bounds.py finds with the vector's own limbs as the bounds (none: admissible)."""
    a, b, c, d = t[0:10], t[10:20], t[20:30], t[30:40]
    F.violations.clear()
    if op == "mul":
        F.fe_mul(a, b, "v")
    elif op == "sq":
        F.fe_sq(a, "v")
    elif op == "mul2":
        F.fe_mul(a, b, "v")
        F.fe_mul(c, d, "v")
    elif op == "sq2":
        F.fe_sq(a, "v")
        F.fe_sq(b, "v")
    elif op == "mul_small":
        assert t[10] < 1 << 12
        F.fe_mul_small(a, t[10], "v")
    elif op == "carry":
        F.fe_carry(a, "v")
    elif op in ("add", "dbl"):
        F.fe_add(a, b if op == "add" else a, "v")
    elif op == "sub":
        F.fe_sub(a, b, "v")
    elif op == "neg":
        F.fe_neg(a, "v")
    elif op in ("invert", "pow22523"):
        assert is_tight(a)
        F.fe_pow_chain(a, "v")
    elif op == "tobytes":
        F.fe_tobytes32(a, "v")
    elif op == "abs":
        assert is_tight(a)
        F.fe_abs(a, "v")
    out, F.violations[:] = list(F.violations), []
    return out


@functools.lru_cache(maxsize=None)
def sq_uniform_max():
    """The largest b for which fe_sq of ten limbs b is admissible, by bisection on the bound model."""
    lo, hi = 1 << 26, 1 << 30
    assert not violations("sq", [lo] * 10) and violations("sq", [hi] * 10)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if violations("sq", [mid] * 10):
            hi = mid
        else:
            lo = mid
    return lo


CORNERS = [(int(2 ** 28.0), int(2 ** 27.75)), (int(2 ** 28.32), int(2 ** 27.585)), (1 << 29, 1 << 26)]


def reps(v):
    """Limb representations of the integer v < 2^256: the nominal split, every split with one unit of a
    limb moved down into the limb below it, and the split plus p and plus 2p limb by limb."""
    base = split(v)
    out = [("split", base)]
    for i in range(9):
        if base[i + 1]:
            s = list(base)
            s[i] += 1 << W[i]
            s[i + 1] -= 1
            out.append((f"shift{i}", s))
    out.append(("+p", [base[i] + P_LIMBS[i] for i in range(10)]))
    out.append(("+2p", [base[i] + P2[i] for i in range(10)]))
    return out


@functools.lru_cache(maxsize=None)
def field_vectors():
    """op -> list of (class, flat operand words).  Deterministic; classes are mixed across lanes."""
    rng = random.Random(0x25519)
    canon = lambda: [rng.getrandbits(W[i]) for i in range(10)]  # noqa: E731
    tight = lambda: [rng.randrange(TIGHT_MAX[i] + 1) for i in range(10)]  # noqa: E731
    upto = lambda b: [rng.randrange(b + 1) for _ in range(10)]  # noqa: E731
    only = lambda i: [TIGHT_MAX[j] if j == i else 0 for j in range(10)]  # noqa: E731

    def with_max(i):
        t = tight()
        t[i] = TIGHT_MAX[i]
        return t

    bsq = sq_uniform_max()
    zero_reps = [ZERO, P_LIMBS, list(P2)]

    mul = [("canon", canon() + canon()) for _ in range(512)]
    mul.append(("tight_max", TIGHT_MAX + TIGHT_MAX))
    mul += [("tight_max:single", only(i) + only(j)) for i in range(10) for j in range(10)]
    mul += [("tight_max:single", only(i) + TIGHT_MAX) for i in range(10)]
    mul += [("tight_max:single", TIGHT_MAX + only(i)) for i in range(10)]
    for _ in range(3):
        mul += [("tight_max:single+random", with_max(i) + with_max(j)) for i in range(10) for j in (i, 9 - i)]
    for cf, cg in CORNERS:
        mul.append(("corner", [cf] * 10 + [cg] * 10))
        mul += [("corner:random", upto(cf) + upto(cg)) for _ in range(256)]
        ev = lambda c: [c if i % 2 == 0 else 0 for i in range(10)]  # noqa: E731
        od = lambda c: [c if i % 2 else 0 for i in range(10)]  # noqa: E731
        mul += [("corner:checker", x(cf) + y(cg)) for x in (ev, od) for y in (ev, od)]
    for _ in range(256):
        a, b, c, d = tight(), tight(), tight(), tight()
        mul.append(("formula", fe_sub(a, b) + fe_sub(d, c)))
    mul.append(("formula", fe_sub(TIGHT_MAX, ZERO) + fe_sub(TIGHT_MAX, ZERO)))
    for x in [ZERO, TIGHT_MAX] + [tight() for _ in range(62)]:
        mul.append(("formula:comb", fe_neg(x) + tight()))
        mul.append(("formula:comb", tight() + fe_neg(x)))
    for z in zero_reps:
        for o in zero_reps + [TIGHT_MAX, tight(), canon()]:
            mul.append(("zero_p", z + o))
            mul.append(("zero_p", o + z))

    sq = [("canon", canon()) for _ in range(512)]
    sq.append(("tight_max", TIGHT_MAX))
    sq += [("tight_max:single", only(i)) for i in range(10)]
    for _ in range(3):
        sq += [("tight_max:single+random", with_max(i)) for i in range(10)]
    sq += [("corner", [b] * 10) for b in (bsq, CORNERS[0][1], CORNERS[1][1], CORNERS[2][1])]
    sq += [("corner:random", upto(bsq)) for _ in range(512)]
    sq += [("corner:checker", [bsq if i % 2 == par else 0 for i in range(10)]) for par in (0, 1)]
    sq += [("formula", fe_sub(tight(), tight())) for _ in range(256)]
    sq.append(("formula", fe_sub(TIGHT_MAX, ZERO)))
    sq += [("formula:comb", fe_neg(x)) for x in [ZERO, TIGHT_MAX] + [tight() for _ in range(30)]]
    sq += [("zero_p", z) for z in zero_reps]

    def corner_mul(k):
        return [CORNERS[k][0]] * 10 + [CORNERS[k][1]] * 10

    mul2 = [("canon", canon() + canon() + canon() + canon()) for _ in range(256)]
    sq2 =[("canon", canon() + canon()) for _ in range(256)]
    for k in range(3):
        for _ in range(16):
            mul2.append(("pair:corner/tight", corner_mul(k) + tight() + tight()))
            mul2.append(("pair:tight/corner", tight() + tight() + corner_mul(k)))
        mul2 += [("pair:corner/corner", corner_mul(k) + corner_mul(j)) for j in range(3)]
    for b in (bsq, CORNERS[0][1], CORNERS[1][1]):
        for _ in range(16):
            sq2.append(("pair:corner/tight", [b] * 10 + tight()))
            sq2.append(("pair:tight/corner", tight() + [b] * 10))
        sq2 += [("pair:corner/corner", [b] * 10 + [c] * 10) for c in (bsq, CORNERS[0][1], CORNERS[1][1])]
    hard_mul = [v for v in mul if v[0] != "canon"]
    hard_sq = [v for v in sq if v[0] != "canon"]
    for _ in range(1024):
        x, y = rng.choice(hard_mul), rng.choice(hard_mul)
        mul2.append((f"pair:{x[0]}/{y[0]}", x[1] + y[1]))
        x, y = rng.choice(hard_sq), rng.choice(hard_sq)
        sq2.append((f"pair:{x[0]}/{y[0]}", x[1] + y[1]))

    small = []
    for a in [TIGHT_MAX, ZERO, P_LIMBS, list(MASK)] + [tight() for _ in range(28)] + [canon() for _ in range(32)]:
        small += [("tight", a + [k]) for k in (0, 1, 2, 19, 4095, rng.randrange(1 << 12), rng.randrange(1 << 12))]

    ones = [M32] * 10
    carry = [("ones", ones), ("tight_max", TIGHT_MAX), ("zero_p", ZERO), ("zero_p", P_LIMBS), ("zero_p", list(P2))]
    carry += [("random32", [rng.getrandbits(32) for _ in range(10)]) for _ in range(251)]
    add = [("tight_max", TIGHT_MAX + TIGHT_MAX), ("edge", [0x7fffffff] * 10 + [0x80000000] * 10), ("edge", ones + ZERO)]
    add += [("tight", tight() + tight()) for _ in range(125)]
    sub = [(c, a + b) for c, a in (("tight_max", TIGHT_MAX), ("zero", ZERO), ("tight", tight()), ("wide", [1 << 28] * 10))
           for b in (list(P2), TIGHT_MAX, ZERO, P_LIMBS)]
    sub += [("tight", tight() + tight()) for _ in range(112)]
    neg = [("2p", list(P2)), ("tight_max", TIGHT_MAX), ("zero_p", ZERO), ("zero_p", P_LIMBS)]
    neg += [("tight", tight()) for _ in range(124)]
    dbl = [("edge", [0x7fffffff] * 10), ("tight_max", TIGHT_MAX), ("zero_p", ZERO)] + [("tight", tight()) for _ in range(125)]

    powv = []
    for v in (0, 1, P - 1, 2, SQRT_M1):
        powv += [(f"special:{name}", r) for name, r in reps(v)[:-2] if is_tight(r)]
    powv += [("tight_max", TIGHT_MAX), ("zero_p", P_LIMBS)]
    powv += [("tight_max:single+random", with_max(i)) for i in range(10)]
    powv += [("canon", canon()) for _ in range(256)]

    tob = []
    for v in (0, 1, P - 1, P, P + 1, 2 * P - 1, 2**255 - 1, 2**255 + 18):
        tob += [(f"value:{name}", r) for name, r in reps(v)]
    tob += [("ones", ones), ("tight_max", TIGHT_MAX)]
    tob += [("random32", [rng.getrandbits(32) for _ in range(10)]) for _ in range(512)]
    tob += [("canon", canon()) for _ in range(256)]

    fromb = [("edge", words(v, 8)) for v in (2**256 - 1, 1 << 255, P, P + 18, (1 << 255) + P, 0, 1, 2**255 - 1)]
    fromb += [("random", [rng.getrandbits(32) for _ in range(8)]) for _ in range(248)]

    absv = [("tight_max", TIGHT_MAX), ("zero_p", ZERO), ("zero_p", P_LIMBS)]
    for v in (1, 2, P - 1, P - 2):
        absv += [(f"value:{name}", r) for name, r in reps(v)[:-2] if is_tight(r)]
    absv += [("tight", tight()) for _ in range(256)]

    out = {"mul": mul, "sq": sq, "mul2": mul2, "sq2": sq2, "mul_small": small, "carry": carry, "add": add, "sub": sub,
           "neg": neg, "dbl": dbl, "invert": list(powv), "pow22523": list(powv), "tobytes": tob, "frombytes": fromb,
           "abs": absv}
    for name in sorted(out):  # classes mixed across the lanes of every wave
        random.Random(name).shuffle(out[name])
    return out


# ------------------------------------------------------------------ the scalar model (sc25519.h)
DELTA = L - 2**252
LW, DW = words(L, 8), words(DELTA, 4)
R = 2**256
RR = R * R % L
RINV = pow(R, -1, L)
LINV = (-pow(L, -1, 1 << 32)) & M32


def _add_l_if(r, cond):
    c, out = 0, []
    for i in range(8):
        c += r[i] + (LW[i] if cond else 0)
        out.append(c & M32)
        c >>= 32
    return out


def sc_reduce9(x, trace=None):
    q = ((x[7] >> 28) | (x[8] << 4)) & M32
    lo = list(x[:7]) + [x[7] & 0x0fffffff]
    t, c = [], 0
    for i in range(4):
        c += q * DW[i]
        t.append(c & M32)
        c >>= 32
    t.append(c & M32)
    r, b = [], 0
    for i in range(8):
        d = lo[i] - (t[i] if i < 5 else 0) + b
        r.append(d & M32)
        b = d >> 32
    if trace is not None:
        trace["borrow"] = b < 0
    return _add_l_if(r, b < 0)


def _row(a, x, c, n):
    w, acc = [], 0
    for i in range(n):
        acc += a[i] * x + (c[i] if i < 8 else 0)
        w.append(acc & M32)
        acc >>= 32
    return w, acc & M32


def sc_mul_small_add(a, x, c):
    w, top = _row(a, x, c, 8)
    return sc_reduce9(w + [top])


def sc_horner2(a, x, c1, c0):
    w, top = _row(a, x, c1, 8)
    w, _ = _row(w + [top], x, c0, 9)
    return sc_reduce9(w)


def sc_lazy_step(v, x, c):
    t, out = 0, []
    for i in range(10):
        t = (v[i] * x + (c[i] if i < 8 else 0) + (t >> 32)) & M64
        out.append(t & M32)
    return out


def sc_lazy_fold(v):
    h = [((v[7] >> 28) | (v[8] << 4)) & M32, ((v[8] >> 28) | (v[9] << 4)) & M32, v[9] >> 28]
    p, acc, hiacc = [], 0, 0
    for k in range(7):
        for i in range(3):
            if 0 <= k - i < 4:
                m = h[i] * DW[k - i]
                acc = (acc + (m & M32)) & M64
                hiacc += m >> 32
        p.append(acc & M32)
        acc, hiacc = (acc >> 32) + hiacc, 0
    c, out = 0, []
    for i in range(8):
        c += (v[i] if i < 7 else v[7] & 0x0fffffff) + LW[i] - (p[i] if i < 7 else 0)
        out.append(c & M32)
        c >>= 32
    return out + [0, 0]


def sc_add(a, b):
    w, top = _row(a, 1, b, 8)
    return sc_reduce9(w + [top])


def sc_sub(a, b):
    w, acc = [], 0
    for i in range(8):
        acc += a[i] - b[i]
        w.append(acc & M32)
        acc >>= 32
    return _add_l_if(w, acc < 0)


def sc_neg(a):
    nz, b, r = any(a), 0, []
    for i in range(8):
        d = LW[i] - a[i] + b
        r.append((d & M32) if nz else 0)
        b = d >> 32
    return r


def sc_mont_mul(a, b):
    t = [0] * 10
    for i in range(8):
        c = 0
        for j in range(8):
            c += a[j] * b[i] + t[j]
            t[j] = c & M32
            c >>= 32
        c += t[8]
        t[8], t[9] = c & M32, (c >> 32) & M32
        m = (t[0] * LINV) & M32
        c = (m * LW[0] + t[0]) >> 32
        for j in range(1, 8):
            c += m * LW[j] + t[j]
            t[j - 1] = c & M32
            c >>= 32
        c += t[8]
        t[7] = c & M32
        t[8] = (t[9] + (c >> 32)) & M32
    d, bb = [], 0
    for i in range(8):
        x = t[i] - LW[i] + bb
        d.append(x & M32)
        bb = x >> 32
    return d if (t[8] != 0 or bb == 0) else t[:8]


def sc_mul(a, b):
    return sc_mont_mul(sc_mont_mul(a, b), words(RR, 8))


def sc_mont_inv(am):
    e, r = L - 2 - 2**252, list(am)
    for bit in range(251, -1, -1):
        r = sc_mont_mul(r, r)
        if bit < 128 and (e >> bit) & 1:
            r = sc_mont_mul(r, am)
    return r


def sc_reduce512(w):
    a = sc_reduce9(list(w[:8]) + [0])
    b = sc_mont_mul(sc_reduce9(list(w[8:]) + [0]), words(RR, 8))
    return sc_add(a, b)


def sc_radix16(s):
    d = [(s[i // 8] >> (4 * (i % 8))) & 15 for i in range(64)]
    for i in range(63):
        carry = (d[i] + 8) >> 4
        d[i] -= carry << 4
        d[i + 1] += carry
    return d


def sc_model(op, t):
    """The output words of dkg_sc_ops for op on the operand tuple t."""
    a, b = t[0:8], t[8:16]
    if op == "lazy":
        v = list(t[0:10])
        for _ in range(t[10]):
            v = sc_lazy_step(v, t[11], t[12:20])
        v = sc_lazy_fold(v)
        return v + sc_reduce9(v[:9])
    if op == "radix16":
        d = [x & 0xff for x in sc_radix16(a)]
        return [d[4 * i] | d[4 * i + 1] << 8 | d[4 * i + 2] << 16 | d[4 * i + 3] << 24 for i in range(16)]
    return {"reduce9": lambda: sc_reduce9(t), "reduce256": lambda: sc_reduce9(list(a) + [0]),
            "reduce512": lambda: sc_reduce512(t), "add": lambda: sc_add(a, b), "sub": lambda: sc_sub(a, b),
            "neg": lambda: sc_neg(a), "mul_small_add": lambda: sc_mul_small_add(a, t[8], t[9:17]),
            "horner2": lambda: sc_horner2(a, t[8], t[9:17], t[17:25]), "mont_mul": lambda: sc_mont_mul(a, b),
            "mul": lambda: sc_mul(a, b), "mont_inv": lambda: sc_mont_inv(a)}[op]()


def sc_ref(op, t):
    """The big-integer result in canonical form (8 words); None where the check is a property (lazy's
    folded state, radix16's digits: sc_check)."""
    a, b = val(t[0:8]), val(t[8:16])
    r = {"reduce9": lambda: val(t), "reduce256": lambda: a, "reduce512": lambda: val(t), "add": lambda: a + b,
         "sub": lambda: a - b, "neg": lambda: -a, "mul_small_add": lambda: a * t[8] + val(t[9:17]),
         "horner2": lambda: (a * t[8] + val(t[9:17])) * t[8] + val(t[17:25]), "mont_mul": lambda: a * b * RINV,
         "mul": lambda: a * b, "mont_inv": lambda: pow(a * RINV % L, -1, L) * R}[op]()
    return words(r % L, 8)


def sc_check(op, t, out):
    """Assert that `out` (the aid's or the model's words) is the big-integer result for the tuple t."""
    if op == "lazy":
        want = val(t[0:10])
        for _ in range(t[10]):
            want = want * t[11] + val(t[12:20])
        folded = val(out[0:10])
        assert folded < 2**254 and folded % L == want % L, (t, out)
        assert out[10:18] == words(want % L, 8), (t, out)
    elif op == "radix16":
        d = [((out[i // 4] >> (8 * (i % 4))) & 0xff) for i in range(64)]
        d = [x - 256 if x >= 128 else x for x in d]
        assert sum(x << (4 * i) for i, x in enumerate(d)) == val(t), (t, d)
        assert all(-8 <= x < 8 for x in d[:63]) and 0 <= d[63] <= 8, (t, d)
    else:
        assert out == sc_ref(op, t), (op, t, out)


@functools.lru_cache(maxsize=None)
def scalar_vectors():
    """op -> list of (label, flat operand words), each within the range the primitive's comment states."""
    rng = random.Random(0x5c25519)
    w8 = lambda v: words(v, 8)  # noqa: E731
    rs = lambda: rng.randrange(L)  # noqa: E731
    top = (2**277 - 1) // L * L
    r9 = [0, L - 1, L, L + 1, 2**252 - 1, 2**252, top - 1, top, top + 1, 2**277 - 1]
    for k in (1, 2, 15, 16, 1 << 24):
        r9 += [k * L - 1, k * L, k * L + 1]
    for q in (1, (1 << 25) - 1):
        x = q * 2**252 + q * DELTA
        r9 += [x - 1, x, x + 1]
    r9 += [rng.randrange(2**277) for _ in range(256)] + [rng.randrange(1, top // L) * L + rng.randrange(3) - 1 for _ in range(64)]
    edge = [0, 1, L - 1]
    pairs = [(a, b) for a in edge for b in edge]
    mm = [0, 1, L - 1, R % L, RR]
    wide = [2**512 - 1, (L - 1) * R + (L - 1), L - 1, (L - 1) * R, (2**256 - 1) * R, 2**256 - 1, 0]
    with open(os.path.join(ROOT, "tests", "golden", "kat_scalar.json")) as fh:
        wide += [int.from_bytes(bytes.fromhex(e["in"]), "little") for e in json.load(fh)["reduce_wide"]]
    nib = [int(c * 64, 16) & (2**255 - 1) for c in "78f"] + [int("7f" * 32, 16), int("f7" * 32, 16) & (2**255 - 1)]
    return {
        "reduce9": [("x", words(x, 9)) for x in r9],
        "reduce256": [("x", w8(x)) for x in [2**256 - 1, 0, L - 1] + [k * L for k in range(1, 16)] +
                      [k * L + e for k in (1, 15) for e in (-1, 1)] + [rng.getrandbits(256) for _ in range(64)]],
        "reduce512": [("x", words(x, 16)) for x in wide + [rng.getrandbits(512) for _ in range(64)]],
        "add": [("x", w8(a) + w8(b)) for a, b in pairs + [(rs(), rs()) for _ in range(64)]],
        "sub": [("x", w8(a) + w8(b)) for a, b in pairs + [(rs(), rs()) for _ in range(64)]],
        "neg": [("x", w8(a)) for a in edge + [rs() for _ in range(64)]],
        "mul_small_add": [("x", w8(a) + [x] + w8(c)) for a, x, c in
                          [(L - 1, x, L - 1) for x in (0, 1, (1 << 24) - 1)] +
                          [(rs(), rng.randrange(1 << 24), rs()) for _ in range(128)]],
        "horner2": [("x", w8(a) + [x] + w8(c1) + w8(c0)) for a, x, c1, c0 in
                    [(L - 1, x, L - 1, L - 1) for x in (0, 1, 2047)] +
                    [(rs(), rng.randrange(1 << 11), rs(), rs()) for _ in range(128)]],
        "lazy": [("x", words(s, 10) + [k, x] + w8(c)) for k in range(6) for s, x, c in
                 [(2**254 - 1, 8191, L - 1), (0, 8191, L - 1), (L - 1, 1, 0), (2**254 - 1, 0, 0)] +
                 [(rng.randrange(2**254), rng.randrange(1 << 13), rs()) for _ in range(16)]],
        "mont_mul": [("x", w8(a) + w8(b)) for a, b in [(a, b) for a in mm for b in mm] + [(rs(), rs()) for _ in range(128)]],
        "mul": [("x", w8(a) + w8(b)) for a, b in [(a, b) for a in mm for b in mm] + [(rs(), rs()) for _ in range(128)]],
        "mont_inv": [("x", w8(a * R % L)) for a in [1, 2, L - 1, (L + 1) // 2] + [1 + rng.randrange(L - 1) for _ in range(60)]],
        "radix16": [("x", w8(s)) for s in nib + [0, 1, L - 1, 2**255 - 1] + [rng.getrandbits(255) for _ in range(64)]],
    }


# the lengths of the lists above, asserted wherever they are consumed: no case is dropped on the way
FIELD_COUNTS = {"mul": 1897, "sq": 1363, "mul2": 1385, "sq2": 1385, "mul_small": 448, "carry": 256, "add": 128,
                "sub": 128, "neg": 128, "dbl": 128, "invert": 273, "pow22523": 273, "tobytes": 840, "frombytes": 256,
                "abs": 263}
SCALAR_COUNTS = {"reduce9": 351, "reduce256": 86, "reduce512": 83, "add": 73, "sub": 73, "neg": 67,
                 "mul_small_add": 131, "horner2": 131, "lazy": 120, "mont_mul": 153, "mul": 153, "mont_inv": 64,
                 "radix16": 73}
