#!/usr/bin/env python3
"""Numeric check of the stepping's dedicated addition (points.h ge_add_ded_lds, HWCD 2008
"add-2008-hwcd-4" for a = -1) against the complete group law (tools/r255.py add):

  * on random pairs of points (random projective scaling) it returns p + q with Z != 0;
  * over every pair of 8-torsion offsets T1, T2 and the relations q = p, q = -p, q = 2p, q random
    (p = a g + T1, q = b g + T2), it either returns p + q exactly or a point with Z = 0 -- never a
    wrong point with Z != 0.  That is what makes the stepping's redo rule exact: a workgroup whose
    sums all came out with Z != 0 holds the complete formula's values.
  * the scaled-state addition (points.h ge_add_sc_lds: the same products on (X, Y, 2Z, T/2) and the
    published (Y+X, Y-X, 2Z, T/2)) returns, on every one of those pairs, exactly (X3/2, Y3/2, Z3, T3/4)
    of the dedicated result (X3, Y3, Z3, T3): again a scaled state, of the same point, with Z3' = 0
    exactly where Z3 = 0; ge_to_scaled's (2X, 2Y, 4Z, T) is a scaled state of the same point; and the
    normalisations' folded constants (k_affine_pieces<SC>, k_affine_pairs<SC>) give the affine Niels
    slots of the proper records.
  * which factor of Z3 = F G vanishes is recorded per relation and order of the torsion offset
    (stats["factors"]): F exactly when q - p is the identity or the point of order 2, G exactly when
    q - p has order 4, neither for an offset of order 8 -- and neither for q = -p + T, q = 2p + T or a
    random q whatever T is: opposite points are not exceptional.
Usage: python tools/ded_check.py   (exit status 1 on a wrong sum); tests/test_bounds.py runs it.
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import r255 as R  # noqa: E402

P = R.P


def ded_fg(p, q):
    """F = B - A and G = B + A of ge_add_ded_lds (Z3 = F G)."""
    A = (p.Y - p.X) * ((q.Y + q.X) % P) % P
    B = (p.Y + p.X) * ((q.Y - q.X) % P) % P
    return (B - A) % P, (B + A) % P


def ded(p, q):
    """ge_add_ded_lds on (X, Y, Z, T) and the cached (Y+X, Y-X, 2Z, 2T) of q."""
    z2, t2 = 2 * q.Z % P, 2 * q.T % P
    F, G = ded_fg(p, q)
    C, Dd = p.Z * t2 % P, p.T * z2 % P
    E, H = (Dd + C) % P, (Dd - C) % P
    return R.Pt(E * F, G * H, G * F, E * H)


INV2, INV4 = pow(2, P - 2, P), pow(4, P - 2, P)


def to_scaled(p):
    """points.h ge_to_scaled: (2X, 2Y, 4Z, T), the scaled state of the representative 2 (X, Y, Z, T)."""
    return R.Pt(2 * p.X % P, 2 * p.Y % P, 4 * p.Z % P, p.T % P)


def from_scaled(s):
    """The proper point (X, Y, Z~/2, 2T^) a scaled state stands for."""
    return R.Pt(s.X, s.Y, s.Z * INV2 % P, 2 * s.T % P)


def ded_sc(p, q):
    """ge_add_sc_lds on scaled states: ge_add_ded_lds's products, q published without doublings."""
    ypx, ymx = (q.Y + q.X) % P, (q.Y - q.X) % P
    A = (p.Y - p.X) * ypx % P
    B = (p.Y + p.X) * ymx % P
    F, G = (B - A) % P, (B + A) % P
    C, Dd = p.Z * q.T % P, p.T * q.Z % P
    E, H = (Dd + C) % P, (Dd - C) % P
    return R.Pt(E * F, G * H, G * F, E * H)


def niels(x, y):
    return ((y + x) % P, (y - x) % P, 2 * R.D * x * y % P)


def affine_niels(p):
    zi = pow(p.Z, P - 2, P)
    return niels(p.X * zi % P, p.Y * zi % P)


def norm_pieces_sc(s):
    """k_affine_pieces<SC> on a scaled record: zi = 2 / Z~, 2dxy = (T^ zi) 4d."""
    zi = 2 * pow(s.Z, P - 2, P) % P
    x, y = s.X * zi % P, s.Y * zi % P
    return ((y + x) % P, (y - x) % P, s.T * zi % P * (4 * R.D % P) % P)


def norm_pairs_sc(s0, s1):
    """k_affine_pairs<SC> on two scaled records: the Niels slots of Q0, Q1, Q0 + Q1, Q0 - Q1."""
    z01 = s0.Z * s1.Z % P
    c = s0.T * s1.T % P * (16 * R.D % P) % P
    f, g = (z01 - c) % P, (z01 + c) % P
    zs = f * g % P
    t = 2 * pow(z01 * zs % P, P - 2, P) % P   # the doubled inverse of this receiver's product
    i01, izs = t * zs % P, t * z01 % P
    iz0, iz1 = i01 * s1.Z % P, i01 * s0.Z % P
    ig, i_f = f * izs % P, g * izs % P
    out = [niels(s0.X * iz0 % P, s0.Y * iz0 % P), niels(s1.X * iz1 % P, s1.Y * iz1 % P)]
    ym0, yp0, ym1, yp1 = (s0.Y - s0.X) % P, (s0.Y + s0.X) % P, (s1.Y - s1.X) % P, (s1.Y + s1.X) % P
    for qa, qb, ix, iy in ((ym1, yp1, ig, i_f), (yp1, ym1, i_f, ig)):
        a, b = ym0 * qa % P, yp0 * qb % P
        out.append(niels((b - a) * ix % P, (b + a) * iy % P))
    return out


def same(a, b):
    return all((u * b.Z - v * a.Z) % P == 0 for u, v in ((a.X, b.X), (a.Y, b.Y), (a.T, b.T)))


def scaled(p, s):
    return R.Pt(p.X * s, p.Y * s, p.Z * s, p.T * s)


def mul_full(p, k):  # k * p without reducing k mod l (torsion survives)
    r = R.IDENTITY
    while k:
        if k & 1:
            r = R.add(r, p)
        p = R.add(p, p)
        k >>= 1
    return r


def torsion(rng):
    """The 8 points of E[8] as l * (random curve points)."""
    out = {}
    while len(out) < 8:
        y = rng.randrange(P)
        x2 = (1 - y * y) * pow((-1 - R.D * y * y) % P, P - 2, P) % P
        x = pow(x2, (P + 3) // 8, P)
        if x * x % P != x2:
            x = x * pow(2, (P - 1) // 4, P) % P
        if x * x % P != x2:
            continue
        t = mul_full(R.Pt(x, y, 1, x * y), R.L)
        zi = pow(t.Z, P - 2, P)
        out[(t.X * zi % P, t.Y * zi % P)] = None
    return [R.Pt(x, y, 1, x * y) for x, y in out]


def order(t):
    """The order (1, 2, 4 or 8) of a point of E[8]."""
    k, r = 1, t
    while not same(r, R.IDENTITY):
        r, k = R.add(r, r), 2 * k
    return k


RELATIONS = ("q = p + T", "q = -p + T", "q = 2p + T", "q random")


def run(seed=1, nrand=64):
    rng = random.Random(seed)
    g = R.from_uniform_bytes(bytes(range(64)))
    stats = {"sum": 0, "Z=0": 0, "wrong": 0, "scaled wrong": 0, "factors": {}}

    def one(p, q):
        r = ded(p, q)
        ps, qs = to_scaled(p), to_scaled(q)
        rs = ded_sc(ps, qs)
        r2 = ded(R.Pt(2 * p.X, 2 * p.Y, 2 * p.Z, 2 * p.T), R.Pt(2 * q.X, 2 * q.Y, 2 * q.Z, 2 * q.T))
        ok = (rs.X % P, rs.Y % P, rs.Z % P, rs.T % P) == (r2.X * INV2 % P, r2.Y * INV2 % P, r2.Z % P, r2.T * INV4 % P)
        ok = ok and same(from_scaled(ps), p) and ((rs.Z % P == 0) == (r.Z % P == 0))
        if r.Z % P != 0:  # the records the normalisations read: the slots of the complete sum
            ok = ok and same(from_scaled(rs), R.add(p, q)) and norm_pieces_sc(rs) == affine_niels(R.add(p, q))
            if p.Z % P and q.Z % P:
                neg_q = R.Pt(-q.X % P, q.Y, q.Z, -q.T % P)
                ok = ok and norm_pairs_sc(ps, qs) == [affine_niels(p), affine_niels(q), affine_niels(R.add(p, q)),
                                                      affine_niels(R.add(p, neg_q))]
        stats["scaled wrong"] += 0 if ok else 1
        if r.Z % P == 0:
            stats["Z=0"] += 1
        elif same(r, R.add(p, q)):
            stats["sum"] += 1
        else:
            stats["wrong"] += 1

    for _ in range(nrand):
        one(scaled(R.mul(g, rng.randrange(1, R.L)), rng.randrange(1, P)), R.mul(g, rng.randrange(1, R.L)))
    rand_exc = stats["Z=0"]
    for t1 in torsion(rng):
        for t2 in torsion(rng):
            for rel in range(4):
                a = rng.randrange(1, R.L)
                b = (a, R.L - a, 2 * a % R.L, rng.randrange(1, R.L))[rel]
                p, q = scaled(R.add(R.mul(g, a), t1), rng.randrange(1, P)), R.add(R.mul(g, b), t2)
                one(p, q)
                # T = q - (b/a) p: the offset t2 - t1 for q = p + T, t2 + t1 for q = -p + T, t2 - 2 t1 ..
                neg1 = R.Pt(-t1.X % P, t1.Y, t1.Z, -t1.T % P)
                off = (R.add(t2, neg1), R.add(t2, t1), R.add(t2, R.add(neg1, neg1)), R.IDENTITY)[rel]
                F, G = ded_fg(p, q)
                stats["factors"].setdefault((RELATIONS[rel], order(off) if rel < 3 else 0), set()).add(
                    ("F" if F == 0 else "") + ("G" if G == 0 else ""))
    one(R.IDENTITY, R.IDENTITY)
    one(g, R.IDENTITY)
    return stats, rand_exc


if __name__ == "__main__":
    st, rx = run()
    fac = st.pop("factors")
    print(st, "exceptional among random pairs:", rx)
    for (rel, o), v in sorted(fac.items()):
        print(f"  {rel:11s} offset of order {o}: vanishing factor {sorted(v)}")
    sys.exit(1 if st["wrong"] or st["scaled wrong"] or rx else 0)
