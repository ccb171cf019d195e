"""The fused pair normalisation (kernels.hip k_affine_pairs) on the CPU: the limb bounds of its four
affine addends under tools/fe_bounds.py, and the identity it rests on -- one inverse of Z_S = f g
gives the affine sum AND difference of a pair -- against the affine addition law."""
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fe_bounds as F  # noqa: E402


def test_pair_addends_are_bounded():
    """From TIGHT coordinates every product, sum and difference of the kernel stays inside its
    limits, the four addends are bounded as k_affine_pieces' are (y + x, y - x uncarried below
    2^27 and 2^27.585, 2dxy tight), and a mixed addition of each gives TIGHT coordinates again."""
    tight = F.run()
    assert F.violations == [], F.violations
    pt = (tight, tight, tight, tight)
    outs = F.affine_pair(pt, pt)
    assert len(outs) == 4
    for q in outs:
        ypx, ymx, xy2d = q
        assert max(ypx) <= 2 ** 27 + 2 ** 14 and math.log2(max(ymx)) < 27.586
        assert all(xy2d[i] <= tight[i] for i in range(10))
        r = F.ge_madd_signed(pt, q, "pairnorm madd")
        assert all(c[i] <= tight[i] for c in r for i in range(10))
    assert F.violations == [], F.violations


P = F.P
D = (-121665 * pow(121666, -1, P)) % P


def _inv(x):
    return pow(x, P - 2, P)


def _rand_point(rng):
    """A random curve point in extended coordinates with a random Z."""
    while True:
        y = rng.randrange(P)
        x2 = (y * y - 1) * _inv(D * y * y + 1) % P
        x = pow(x2, (P + 3) // 8, P)
        if (x * x - x2) % P:
            x = x * pow(2, (P - 1) // 4, P) % P
        if (x * x - x2) % P:
            continue
        z = rng.randrange(1, P)
        return (x * z % P, y * z % P, z, x * y % P * z % P)


def _aff(p):
    zi = _inv(p[2])
    return (p[0] * zi % P, p[1] * zi % P)


def _aff_add(a, b):
    (x1, y1), (x2, y2) = a, b
    k = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * _inv(1 + k) % P, (y1 * y2 + x1 * x2) * _inv(1 - k) % P)


def test_shared_inverse_gives_sum_and_difference():
    """x_S = e f / Z_S, y_S = h g / Z_S, x_D = e' g / Z_S, y_D = h' f / Z_S with Z_S = f g != 0, on
    random pairs, on Q_1 = Q_0, Q_1 = -Q_0 and identity + identity."""
    rng = random.Random(11)
    for k in range(40):
        a, b = _rand_point(rng), _rand_point(rng)
        if k == 0:
            b = a
        elif k == 1:
            b = (-a[0] % P, a[1], a[2], -a[3] % P)
        elif k == 2:
            a = b = (0, 1, 1, 0)
        elif k == 3:
            a, b = (0, 7, 7, 0), b          # identity (Z = 7) + a random point
        X0, Y0, Z0, T0 = a
        X1, Y1, Z1, T1 = b
        c, d = T0 * T1 * 2 * D % P, 2 * Z0 * Z1 % P
        f, g = (d - c) % P, (d + c) % P
        zs = f * g % P
        assert zs != 0
        izs = _inv(zs)
        ig, i_f = f * izs % P, g * izs % P
        ym0, yp0, ym1, yp1 = (Y0 - X0) % P, (Y0 + X0) % P, (Y1 - X1) % P, (Y1 + X1) % P
        e, h = (yp0 * yp1 - ym0 * ym1) % P, (yp0 * yp1 + ym0 * ym1) % P
        e2, h2 = (yp0 * ym1 - ym0 * yp1) % P, (yp0 * ym1 + ym0 * yp1) % P
        A, B = _aff(a), _aff(b)
        assert (e * ig % P, h * i_f % P) == _aff_add(A, B), k
        assert (e2 * i_f % P, h2 * ig % P) == _aff_add(A, (-B[0] % P, B[1])), k
