"""Plain big-integer reference of the group and scalar operations the kernels implement.

Python ints only, written from RFC 9496 (ristretto255) and the documented semantics of
include/dkg_amd.h: points are 32-byte ristretto255 encodings, scalars 32-byte little-endian values
read as Scalar::from_bits reads them (bit 255 dropped) and taken mod l.  Independent of the library
under test and of the C oracle: it imports neither.  One scalar multiplication costs about 2 ms.
"""

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493


# ---- field mod 2^255 - 19
def inv(x):
    return pow(x, P - 2, P)


D = -121665 * inv(121666) % P
D2 = 2 * D % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
assert SQRT_M1 * SQRT_M1 % P == P - 1


def is_negative(x):
    return (x % P) & 1


def fabs(x):
    x %= P
    return P - x if x & 1 else x


def sqrt_ratio_m1(u, v):
    """RFC 9496 section 4.2: (was_square, r) with r the non-negative root of u/v, or of
    SQRT_M1 * u/v when u/v is not a square."""
    u %= P
    v %= P
    v3 = v * v % P * v % P
    v7 = v3 * v3 % P * v % P
    r = u * v3 % P * pow(u * v7 % P, (P - 5) // 8, P) % P
    check = v * r % P * r % P
    correct = check == u
    flipped = check == (-u) % P
    flipped_i = check == (-u) * SQRT_M1 % P
    if flipped or flipped_i:
        r = r * SQRT_M1 % P
    return (correct or flipped), fabs(r)


INVSQRT_A_MINUS_D = sqrt_ratio_m1(1, -1 - D)[1]
assert INVSQRT_A_MINUS_D * INVSQRT_A_MINUS_D % P * ((-1 - D) % P) % P == 1


# ---- points: extended coordinates (X, Y, Z, T) on -x^2 + y^2 = 1 + d x^2 y^2, T = XY/Z
IDENTITY = (0, 1, 1, 0)


def decode_why(b):
    """RFC 9496 section 4.3.1: (point, None), or (None, reason) for a rejected encoding.  The
    reasons are tested in the RFC's order; an encoding is listed under the first that applies."""
    b = bytes(b)
    if len(b) != 32:
        return None, "length"
    s = int.from_bytes(b, "little")
    if s >= P:
        return None, "non-canonical"
    if s & 1:
        return None, "negative s"
    ss = s * s % P
    u1 = (1 - ss) % P
    u2 = (1 + ss) % P
    u2_sqr = u2 * u2 % P
    v = (-(D * u1 % P * u1) - u2_sqr) % P
    was_square, invsqrt = sqrt_ratio_m1(1, v * u2_sqr % P)
    den_x = invsqrt * u2 % P
    den_y = invsqrt * den_x % P * v % P
    x = fabs(2 * s * den_x % P)
    y = u1 * den_y % P
    t = x * y % P
    if not was_square:
        return None, "not square"
    if is_negative(t):
        return None, "negative t"
    if y == 0:
        return None, "y = 0"
    return (x, y, 1, t), None


def decode(b):
    return decode_why(b)[0]


def encode(p):
    """RFC 9496 section 4.3.2."""
    x0, y0, z0, t0 = p
    u1 = (z0 + y0) * (z0 - y0) % P
    u2 = x0 * y0 % P
    _, invsqrt = sqrt_ratio_m1(1, u1 * u2 % P * u2 % P)
    den1 = invsqrt * u1 % P
    den2 = invsqrt * u2 % P
    z_inv = den1 * den2 % P * t0 % P
    ix0 = x0 * SQRT_M1 % P
    iy0 = y0 * SQRT_M1 % P
    enchanted = den1 * INVSQRT_A_MINUS_D % P
    if is_negative(t0 * z_inv % P):
        x, y, den_inv = iy0, ix0, enchanted
    else:
        x, y, den_inv = x0, y0, den2
    if is_negative(x * z_inv % P):
        y = (-y) % P
    return fabs(den_inv * (z0 - y) % P).to_bytes(32, "little")


def equals(p, q):
    """RFC 9496 section 4.3.3."""
    return (p[0] * q[1] - p[1] * q[0]) % P == 0 or (p[1] * q[1] - p[0] * q[0]) % P == 0


def add(p, q):
    """Unified addition (Hisil-Wong-Carter-Dawson 2008, a = -1): complete on this curve."""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = t1 * D2 % P * t2 % P
    d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return e * f % P, g * h % P, f * g % P, e * h % P


def double(p):
    x1, y1, z1, _ = p
    a = x1 * x1 % P
    b = y1 * y1 % P
    c = 2 * z1 * z1 % P
    e = ((x1 + y1) * (x1 + y1) - a - b) % P
    g = b - a
    f = g - c
    h = -a - b
    return e * f % P, g * h % P, f * g % P, e * h % P


def neg(p):
    return (-p[0]) % P, p[1], p[2], (-p[3]) % P


def mul(k, p):
    """k * p by left-to-right double-and-add; k any non-negative int (taken mod l)."""
    k %= L
    r = IDENTITY
    for i in reversed(range(k.bit_length())):
        r = double(r)
        if (k >> i) & 1:
            r = add(r, p)
    return r


def doublings(p):
    """[p, 2p, 4p, .., 2^252 p]: a base that serves many scalars pays its doublings once."""
    tab = [p]
    for _ in range(252):
        tab.append(double(tab[-1]))
    return tab


def mul_doublings(k, tab):
    """k * p from doublings(p): the additions of double-and-add alone."""
    k %= L
    r = IDENTITY
    for i in range(k.bit_length()):
        if (k >> i) & 1:
            r = add(r, tab[i])
    return r


def msm(ks, ps):
    r = IDENTITY
    for k, p in zip(ks, ps):
        r = add(r, mul(k, p))
    return r


def _base():
    y = 4 * inv(5) % P
    ok, x = sqrt_ratio_m1(y * y - 1, D * y * y + 1)
    assert ok
    return x, y, 1, x * y % P


BASE = _base()
BASE_BYTES = encode(BASE)


# ---- scalars mod l
def from_bits(b):
    """Scalar::from_bits of a 32-byte string (bit 255 dropped), as an int mod l."""
    return (int.from_bytes(bytes(b), "little") & (2**255 - 1)) % L


def sc(k):
    """The canonical 32-byte encoding of k mod l."""
    return (k % L).to_bytes(32, "little")


def poly_eval(coeffs, x):
    """sum_k coeffs[k] x^k mod l by Horner's rule."""
    r = 0
    for c in reversed(coeffs):
        r = (r * x + c) % L
    return r
