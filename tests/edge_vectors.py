"""Deterministic edge-case inputs for the scalar recodings, the decoder and the share checks.

Random scalars reach the rare branches of the recodings (the last entry of a comb window, a zero
digit in a middle window, a carry into the top window, a saturated wNAF) with probability 2^-18 or
less per window; these generators place them in every window.  Seeded random.Random, no I/O, no
import of the library: the recodings are modelled here from their descriptions in
dkg_amd/csrc/points.h and hybrid.hip.
"""
import random

from tests import ristretto_ref as ref

L = ref.L
P = ref.P


# ---- models of the recodings
def comb_windows(B):
    """Windows of the radix-2^B comb: the top one absorbs the signed recoding's carry."""
    return 256 // B + 1


def comb_radix(windows):
    """The radix 2^B of a comb of `windows` windows (dkg_fixed_base_windows / dkg_key_comb_windows)."""
    rs = [B for B in range(2, 33) if comb_windows(B) == windows]
    assert len(rs) == 1, (windows, rs)
    return rs[0]


def comb_low_windows(B):
    """Windows that lie wholly below bit 253, i.e. that a canonical scalar fills freely."""
    return 253 // B


def comb_recode(k, B):
    """Signed radix-2^B digits of k in [-2^(B-1), 2^(B-1) - 1], lowest window first, and the carry
    out of each window: d = raw + carry_in; carry_out = (d + 2^(B-1)) >> B; d -= carry_out << B."""
    E = 1 << (B - 1)
    digits, carries, carry = [], [], 0
    for w in range(comb_windows(B)):
        d = ((k >> (B * w)) & ((1 << B) - 1)) + carry
        carry = (d + E) >> B
        d -= carry << B
        digits.append(d)
        carries.append(carry)
    assert carry == 0 and sum(d << (B * w) for w, d in enumerate(digits)) == k
    return digits, carries


def naf(k):
    """Bitwise non-adjacent form, lowest digit first."""
    out = []
    while k:
        d = 0
        if k & 1:
            d = 2 - (k & 3)
            k -= d
        out.append(d)
        k >>= 1
    return out


def wnaf4(k):
    """Width-4 wNAF (digits 0, +-1, +-3, +-5, +-7; three zeros after a nonzero one), lowest first."""
    out = []
    while k:
        d = 0
        if k & 1:
            d = k & 15
            if d >= 8:
                d -= 16
            k -= d
        out.append(d)
        k >>= 1
    return out


def _unique(values):
    seen, out = set(), []
    for v in values:
        assert 0 <= v < L
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


# ---- scalars for the signed combs
def comb_scalars(B, seed=1):
    """Scalars < l that put the comb recoding's edge values in every window below bit 253 with both
    carries in: raw window values 0, 1, E-1, E, E+1, 2^B-2, 2^B-1 (E = 2^(B-1)), the other bits
    random; then the saturated scalars and the ends of the range."""
    rng = random.Random(1000 * B + seed)
    E, mask = 1 << (B - 1), (1 << B) - 1
    nw = comb_low_windows(B)
    raws = (0, 1, E - 1, E, E + 1, mask - 1, mask)
    out = []
    for w in range(nw):
        for cin in ((0,) if w == 0 else (0, 1)):
            for raw in raws:
                k = rng.getrandbits(252)
                k = (k & ~(mask << (B * w))) | (raw << (B * w))
                if w:  # the window below decides the carry in: raw + carry < E gives 0, >= E gives 1
                    below = rng.randrange(E + 1, mask + 1) if cin else rng.randrange(0, E - 1)
                    k = (k & ~(mask << (B * (w - 1)))) | (below << (B * (w - 1)))
                out.append(k)
    rep = lambda v: sum(v << (B * w) for w in range(nw))  # noqa: E731
    out += [rep(E), rep(E) - 1, rep(mask), 0, 1, L - 1, L - 2, 2**252, 2**252 - 1]
    assert all(0 <= k < L for k in out)
    return out


# ---- scalars for the NAF and width-4 window chains
def naf_scalars(seed=2):
    rng = random.Random(seed)
    out = [0, 1, 2, 3]
    for k in (31, 32, 33, 63, 64, 251, 252):
        out += [2**k, 2**k - 1, 2**k + 1]
    out += [L - 1, L - 2]
    out += [2**252 - 2**k for k in (1, 4, 100)]  # a run of ones from bit k to the top: one long carry
    for nib in (0x5, 0xA, 0x3, 0x7, 0x9, 0x1, 0xF):
        out.append(int(("%x" % nib) * 64, 16) & (2**252 - 1))
    # saturated width-4 wNAFs: a nonzero digit every fourth bit.  Bits 0, 4, .., 252 is the most a
    # scalar below l can hold (64 digits, the bound behind the kernels' nzb[96] / nzd[96]): the top
    # digit +1 at bit 252 and a negative digit below it keep the value under 2^252.
    odd = (1, 3, 5, 7)
    out.append(2**252 - sum(rng.choice(odd) << (4 * i) for i in range(63)))
    out.append(2**252 - (7 << 248) - sum(rng.choice((-7, -5, -3, -1, 1, 3, 5, 7)) << (4 * i) for i in range(62)))
    out.append((1 << 248) + sum(rng.choice((-7, -5, -3, -1, 1, 3, 5, 7)) << (4 * i) for i in range(62)))
    out.append(sum(7 << (4 * i + 1) for i in range(62)) + (1 << 249))  # digits on bits 1, 5, .., 249
    out.append(sum(rng.choice(odd) << (4 * i + 3) for i in range(62)))  # bits 3, 7, .., 247
    return _unique(out)


# ---- encodings for the decoder
def _le(v):
    return v.to_bytes(32, "little")


def decode_edges(seed=3, invalid_fixture=()):
    """[(class, encoding, expected)]: expected True / False where the class fixes it, None where only
    the reference can tell (small even s, p-3, p-5).  invalid_fixture: further known-bad encodings
    (the RFC 9496 vectors of tests/golden/kat_group.json)."""
    rng = random.Random(seed)
    out = [("small-even", _le(s), None) for s in range(0, 65, 2)]
    out.append(("p-1", _le(P - 1), False))  # even and canonical: only y = 0 rejects it
    out += [("p-3", _le(P - 3), None), ("p-5", _le(P - 5), None)]
    out += [("non-canonical", _le(P + k), False) for k in range(19)]  # p .. 2^255 - 1
    valid = [ref.encode(ref.mul(k, ref.BASE)) for k in
             [1, 2, 3, 7, 8, L - 1, L - 2, 2**252] + [rng.randrange(L) for _ in range(42)]]
    out += [("valid", v, True) for v in valid]
    out += [("negated", _le(P - int.from_bytes(v, "little")), False) for v in valid[:10]]  # odd
    out += [("bit255", bytes(v[:31]) + bytes([v[31] | 0x80]), False) for v in valid[:10]]
    out += [("bit255", _le(2**255), False), ("bit255", b"\x00" + b"\xff" * 31, False), ("bit255", b"\xff" * 32, False)]
    # the rest of RFC 9496 appendix A.3 by its rules: negative s, non-square, negative x*y
    out += [("negative-s", _le(1), False), ("negative-s", _le(2**255 - 255), False)]
    want = {"not square": 8, "negative t": 8}
    while any(want.values()):
        s = rng.randrange(P) & ~1
        why = ref.decode_why(_le(s))[1]
        if want.get(why):
            want[why] -= 1
            out.append((why, _le(s), False))
    out += [("fixture", bytes(x), False) for x in invalid_fixture]
    return out


# ---- polynomials through a chosen share
def share_at(e, x, t, rng, pool=None):
    """Coefficients a_0..a_t (ints mod l) of a polynomial with f(x) = e: a_1..a_t random (drawn from
    `pool` when given), a_0 = e - sum_k a_k x^k."""
    hi = [rng.choice(pool) if pool else rng.randrange(L) for _ in range(t)]
    a0 = (e - sum(a * pow(x, k + 1, L) for k, a in enumerate(hi))) % L
    return [a0] + hi
