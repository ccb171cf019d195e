"""Coefficient vectors whose difference tables meet an exceptional pair of the dedicated addition
(points.h ge_add_ded_lds) at one chosen place, and a big-integer model of what the kernels do there.

The stepping (kernels.hip k_stepping) holds Delta^m Q(0) at position m of a table, adds position
m + 1 into position m once per receiver, and so forms Delta^m Q(j) + Delta^(m+1) Q(j) at loop index
j.  The binomial Horner (k_binom_step, k_binom_wave) builds that table by e'_0 = C_k, e'_m =
m (e_(m-1) + e_m).  Every entry is an INTEGER combination of the decoded commitments, so one linear
condition mod l on the scalar coefficients makes two entries equal (or opposite) as ristretto255
elements while their curve points still differ by a 4-torsion point: the decoded representative of
a commitment is the prime-order point plus some T in E[4], and the integer weights carry T along.

Pure Python over tests/ristretto_ref.py; imports neither the library under test nor the C oracle.
"""
from math import comb

from tests import ristretto_ref as R

L = R.L
P = R.P


# ---- weights of the difference tables
def delta_weight(m, j, k, mod=None):
    """The integer Delta^m [x^k] (j) = sum_i (-1)^(m-i) C(m, i) (j + i)^k (reduced when mod is given)."""
    if mod is None:
        return sum((-1) ** (m - i) * comb(m, i) * (j + i) ** k for i in range(m + 1))
    return sum((-1) ** (m - i) * comb(m, i) * pow(j + i, k, mod) for i in range(m + 1)) % mod


def delta_weights(m, j, length, mod):
    """[delta_weight(m, j, k, mod) for k < length] with running powers (length * (m + 1) products)."""
    sgn = [(-1) ** (m - i) * comb(m, i) % mod for i in range(m + 1)]
    pw = [1] * (m + 1)
    out = []
    for _ in range(length):
        out.append(sum(s * p for s, p in zip(sgn, pw)) % mod)
        pw = [p * (j + i) % mod for i, p in enumerate(pw)]
    return out


def relation_weights(m, j, length, sign=+1, mod=L):
    """w_k with sum_k c_k w_k = Delta^m Q(j) - sign Delta^(m+1) Q(j) for Q = sum_k c_k x^k."""
    a, b = delta_weights(m, j, length, mod), delta_weights(m + 1, j, length, mod)
    return [(x - sign * y) % mod for x, y in zip(a, b)]


def craft_stepping(rng, length, m, j, sign=+1):
    """`length` coefficients mod l, random but for c_m, with Delta^m Q(j) = sign Delta^(m+1) Q(j):
    positions m and m + 1 of Q's table are equal (opposite) when loop index j adds them.  The solved
    coefficient is c_m (Delta^m x^m = m!, Delta^(m+1) x^m = 0: its weight m! is a unit mod l), so
    c_m + 1 breaks the relation.  Needs m <= length - 2 (position m + 1 exists)."""
    c = [rng.randrange(1, L) for _ in range(length)]
    solve_stepping(c, m, j, sign)
    return c


def solve_stepping(c, m, j, sign=+1):
    """Sets c[m] so that Delta^m Q(j) = sign Delta^(m+1) Q(j) holds with the other coefficients kept."""
    length = len(c)
    assert 0 <= m <= length - 2 and j >= 0 and sign in (1, -1)
    w = relation_weights(m, j, length, sign)
    assert w[m] % L != 0
    rest = sum(ck * wk for k, (ck, wk) in enumerate(zip(c, w)) if k != m) % L
    c[m] = -rest * pow(w[m], L - 2, L) % L


def stepping_relation(c, m, j, sign=+1):
    """Delta^m Q(j) - sign Delta^(m+1) Q(j) mod l: zero on a crafted vector."""
    return sum(ck * wk for ck, wk in zip(c, relation_weights(m, j, len(c), sign))) % L


def crafted_row(seed, N, plen, pairs, sign=+1, control=False, binom=()):
    """One dealer's (a, b): N random coefficients each, both with the relations `pairs` = [(piece, m,
    j)] inside pieces of `plen` coefficients (the last one shorter) and `binom` = [(piece, r, m)]
    (craft_binomial's relation in that piece; its stepping pairs must have m < piece length - r).
    control: every solved coefficient incremented by one, which breaks every relation."""
    import random

    assert len({u for u, _, _ in pairs}) == len(pairs)  # one solved coefficient per piece
    rng = random.Random(seed)
    out = []
    for _ in range(2):
        c = [rng.randrange(1, L) for _ in range(N)]
        for u, r, m in binom:
            lo, hi = u * plen, min((u + 1) * plen, N)
            c[lo:hi] = craft_binomial(rng, hi - lo, r, m, sign)
        for u, m, j in pairs:
            lo, hi = u * plen, min((u + 1) * plen, N)
            assert all(bu != u or m < hi - lo - r for bu, r, _ in binom)
            piece = c[lo:hi]
            solve_stepping(piece, m, j, sign)
            c[lo:hi] = piece
        if control:
            for u, r, m in binom:
                k = u * plen + binomial_pivot(min((u + 1) * plen, N) - u * plen, r, m)
                c[k] = (c[k] + 1) % L
            for u, m, j in pairs:
                c[u * plen + m] = (c[u * plen + m] + 1) % L
        out.append(c)
    return out[0], out[1]


# ---- the binomial recurrence on scalars
def binom_tables(c, mod=None):
    """tables[r] = the r + 1 entries after Horner step r (tables[0] = [c_(N-1)]): e'_0 = c_(N-1-r),
    e'_m = m (e_(m-1) + e_m) with e_r = 0.  tables[N-1][m] = Delta^m P(0)."""
    N = len(c)
    e = [c[N - 1]]
    tables = [list(e)]
    for r in range(1, N):
        old = e + [0]
        e = [c[N - 1 - r]] + [m * (old[m - 1] + old[m]) for m in range(1, r + 1)]
        if mod:
            e = [x % mod for x in e]
        tables.append(list(e))
    return tables


def binomial_pivot(length, r, m):
    """The coefficient craft_binomial solves for (incrementing it breaks the relation)."""
    return length - r + m - 1


def craft_binomial(rng, length, r, m, sign=+1):
    """`length` coefficients whose step-r input has e_(m-1) = sign e_m, 1 <= m <= r - 1 < length - 1.
    The input of step r is the table of Q(x) = sum_(i<r) c_(length-r+i) x^i at 0, so the relation is
    craft_stepping's at (m - 1, 0) on the top r coefficients."""
    assert 1 <= m <= r - 1 and r <= length - 1
    c = [rng.randrange(1, L) for _ in range(length)]
    c[length - r:] = craft_stepping(rng, r, m - 1, 0, sign)
    return c


def sc_bytes(c):
    return b"".join(R.sc(x) for x in c)


# ---- curve points with their torsion
def mul_full(k, p):
    """k p for an integer k >= 0 that is NOT reduced mod l (torsion components survive)."""
    r = R.IDENTITY
    for i in reversed(range(k.bit_length())):
        r = R.double(r)
        if (k >> i) & 1:
            r = R.add(r, p)
    return r


def combo(weights, pts):
    """sum_k weights[k] pts[k] with the weights taken mod 8 l (the group's exponent)."""
    r = R.IDENTITY
    for w, p in zip(weights, pts):
        r = R.add(r, mul_full(w % (8 * L), p))
    return r


def torsion_class(p):
    """'O', 'T2' or 'T4' for a point of E[4] (T4: either point of order 4, Y = 0); None otherwise."""
    x, y, z = p[0] % P, p[1] % P, p[2] % P
    if x == 0 and y == z:
        return "O"
    if x == 0 and (y + z) % P == 0:
        return "T2"
    if y == 0 and (x * x + z * z) % P == 0:
        return "T4"
    return None


def _points(commitment_bytes):
    if isinstance(commitment_bytes, (bytes, bytearray)):
        commitment_bytes = [bytes(commitment_bytes[i:i + 32]) for i in range(0, len(commitment_bytes), 32)]
    pts = [R.decode(b) for b in commitment_bytes]
    assert all(p is not None for p in pts)
    return pts


def table_entries(commitment_bytes, m, j):
    """(Delta^m Q(j), Delta^(m+1) Q(j)) as curve points over the decoded commitments of one piece,
    with the integer weights the binomial and the stepping apply."""
    pts = _points(commitment_bytes)
    n = len(pts)
    M = 8 * L
    return combo(delta_weights(m, j, n, M), pts), combo(delta_weights(m + 1, j, n, M), pts)


def classify(commitment_bytes, m, j, sign=+1):
    """The 4-torsion class of Delta^m Q(j) - Delta^(m+1) Q(j) (of their sum when sign = -1) over the
    decoded commitments of one piece: 'O', 'T2' or 'T4'; None when the entries are not related."""
    a, b = table_entries(commitment_bytes, m, j)
    return torsion_class(R.add(a, R.neg(b) if sign > 0 else b))


def binomial_entries(commitment_bytes, r, m):
    """(e_(m-1), e_m) of the input of Horner step r over the decoded commitments of one piece."""
    pts = _points(commitment_bytes)
    top = pts[len(pts) - r:]
    M = 8 * L
    return combo(delta_weights(m - 1, 0, r, M), top), combo(delta_weights(m, 0, r, M), top)


def classify_binomial(commitment_bytes, r, m, sign=+1):
    a, b = binomial_entries(commitment_bytes, r, m)
    return torsion_class(R.add(a, R.neg(b) if sign > 0 else b))


# ---- the dedicated addition and the m-chain, as the kernels run them
def ded_add(p, q):
    """points.h ge_add_ded_lds: p + q by HWCD 2008's dedicated formula on (X, Y, Z, T) and the cached
    (Y+X, Y-X, 2Z, 2T) of q.  Z3 = F G with F = 2 (X1 Y2 - Y1 X2), G = 2 (Y1 Y2 - X1 X2)."""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 + x2) % P
    b = (y1 + x1) * (y2 - x2) % P
    f, g = (b - a) % P, (b + a) % P
    c, d = z1 * 2 * t2 % P, t1 * 2 * z2 % P
    e, h = (d + c) % P, (d - c) % P
    return e * f % P, g * h % P, f * g % P, e * h % P


def ded_factors(p, q):
    """(F == 0, G == 0) of the dedicated addition p + q."""
    x1, y1 = p[0], p[1]
    x2, y2 = q[0], q[1]
    a = (y1 - x1) * (y2 + x2) % P
    b = (y1 + x1) * (y2 - x2) % P
    return (b - a) % P == 0, (b + a) % P == 0


def ded_meets_zero(p, q):
    return ded_add(p, q)[2] == 0


def small_recode(m):
    """points.h small_recode: (length, pos, neg) of the signed digits the m-chains run (the NAF, with
    a leading 1 0 -1 rewritten as 0 1 1)."""
    pos = neg = ln = 0
    v = m
    while v:
        if v & 1:
            if v & 3 == 1:
                pos |= 1 << ln
                v -= 1
            else:
                neg |= 1 << ln
                v += 1
        v >>= 1
        ln += 1
    if ln >= 3 and not ((pos | neg) >> (ln - 2) & 1) and (neg >> (ln - 3) & 1):
        pos = (pos & ~(1 << (ln - 1))) | (3 << (ln - 3))
        neg &= ~(1 << (ln - 3))
        ln -= 1
    assert pos - neg == m
    return ln, pos, neg


def chain_meets_zero(x, m):
    """kernels.hip mul_small_ded_lds: does the chain m x (doublings, dedicated additions of +-x)
    produce a sum with Z = 0?  Returns (met, m x by the complete formula)."""
    ln, pos, neg = small_recode(m)
    y, met = x, False
    for i in range(ln - 2, -1, -1):
        y = R.double(y)
        bit = 1 << i
        if (pos | neg) & bit:
            q = R.neg(x) if neg & bit else x
            met = met or ded_meets_zero(y, q)
            y = R.add(y, q)  # what the chain holds whenever Z != 0; after Z = 0 the redo replaces all
    return met, y


def binomial_item_meets_zero(a, b, m):
    """One item of a Horner step, m (a + b) as k_binom_step / k_binom_wave run it with the dedicated
    formula: True when the addition or the chain meets Z = 0 (the item's wave marks its flag)."""
    if ded_meets_zero(a, b):
        return True
    return chain_meets_zero(R.add(a, b), m)[0]
