"""CPU checks of tests/crafted_pairs.py and of the seeds tests/test_gpu_crafted_pairs.py commits: the
scalar relations hold, the C oracle accepts every crafted row in both rounds, and the pairs fall into
the 4-torsion classes -- and zero the factor of the dedicated addition -- stated next to each seed."""
import random

import pytest

from tests import crafted_pairs as CP
from tests import oracle_lib as O
from tests import ristretto_ref as R
from tests import test_gpu_crafted_pairs as G

L = CP.L
ACCEPT, SELF = 1, 2
N = 32  # t = 31: every classified case


@pytest.fixture(scope="module")
def h():
    return O.call32("or_pt_hash_to_group", G.CK, len(G.CK))[0]


def _commit(h, a, b, n=64):
    return O.share_gen(1, n, len(a) - 1, CP.sc_bytes(a), CP.sc_bytes(b), h)


def _accepts(h, n, E, A, s, sp, d=3):
    """The oracle's per-pair MSM checks accept the whole row in both rounds (dealer index d: SELF there)."""
    want = bytes(SELF if j == d else ACCEPT for j in range(n))
    for rnd, C in ((2, E), (4, A)):
        acc, rc = O.verify_rows(n, len(E) // 32 - 1, rnd, C, h, s, sp if rnd == 2 else None, d, d + 1, 0, n)
        assert rc == 0 and acc == want, rnd


def test_delta_weights():
    for m, j, k in ((0, 5, 3), (1, 0, 1), (3, 2, 3), (3, 2, 2), (4, 7, 9), (6, 1, 6)):
        w = CP.delta_weight(m, j, k)
        assert CP.delta_weight(m + 1, j, k) == CP.delta_weight(m, j + 1, k) - w  # Delta^(m+1) = Delta Delta^m
        assert w % L == CP.delta_weight(m, j, k, L) == CP.delta_weights(m, j, k + 1, L)[k]
    import math
    assert all(CP.delta_weight(m, 9, m) == math.factorial(m) and CP.delta_weight(m + 1, 9, m) == 0 for m in range(8))
    # m! divides Delta^m [x^k]: why the torsion offsets thin out with m
    assert all(CP.delta_weight(m, j, k) % math.factorial(m) == 0 for m in range(6) for j in (0, 3) for k in range(9))


def test_binom_tables_end_in_the_differences_at_zero():
    rng = random.Random(1)
    for n in (1, 2, 5, 16, 32):
        c = [rng.randrange(L) for _ in range(n)]
        tabs = CP.binom_tables(c)
        assert [len(x) for x in tabs] == list(range(1, n + 1))
        assert tabs[-1] == [sum(ck * CP.delta_weight(m, 0, k) for k, ck in enumerate(c)) for m in range(n)]
        assert [x % L for x in tabs[-1]] == CP.binom_tables(c, L)[-1]


def test_crafted_relations_hold_on_scalars():
    rng = random.Random(2)
    poly = lambda c, x: sum(ck * x ** k for k, ck in enumerate(c))  # noqa: E731

    def delta(c, m, j):
        return sum((-1) ** (m - i) * CP.comb(m, i) * poly(c, j + i) for i in range(m + 1))

    for length, m, j, sign in ((32, 5, 10, 1), (32, 0, 62, 1), (32, 1, 58, 1), (16, 14, 3, 1), (42, 40, 77, 1),
                               (32, 0, 20, -1), (64, 0, 20, -1), (43, 2, 90, -1)):
        c = CP.craft_stepping(rng, length, m, j, sign)
        assert (delta(c, m, j) - sign * delta(c, m + 1, j)) % L == 0
        assert CP.stepping_relation(c, m, j, sign) == 0
        c[m] += 1
        assert CP.stepping_relation(c, m, j, sign) != 0
    for length, r, m, sign in ((32, 20, 7, 1), (32, 20, 1, 1), (16, 10, 4, 1), (16, 15, 14, 1), (32, 12, 4, -1),
                               (32, 31, 2, -1)):
        c = CP.craft_binomial(rng, length, r, m, sign)
        e = CP.binom_tables(c, L)[r - 1]
        assert len(e) == r and (e[m - 1] - sign * e[m]) % L == 0
        c[CP.binomial_pivot(length, r, m)] += 1
        e = CP.binom_tables(c, L)[r - 1]
        assert (e[m - 1] - sign * e[m]) % L != 0


def test_crafted_row_pieces_and_control():
    """crafted_row on the split shapes of the GPU file: every relation holds inside its piece, and
    the control breaks each."""
    for Ntot, plen, pairs in ((128, 64, [(1, 2, 90), (0, 20, 3)]), (128, 43, [(2, 17, 100)]),
                              (128, 32, [(2, 2, 90), (3, 20, 3)]), (1030, 515, [(1, 257, 300)]),
                              (1030, 515, [(0, 258, 300)]), (600, 600, [(0, 299, 300)])):
        for control in (False, True):
            for c in CP.crafted_row(7, Ntot, plen, pairs, +1, control):
                for u, m, j in pairs:
                    rel = CP.stepping_relation(c[u * plen:min((u + 1) * plen, Ntot)], m, j)
                    assert (rel != 0) == control
    row = G.BATCH_ROW
    for control in (False, True):
        for c in CP.crafted_row(row["seed"], N, N, row["pairs"], +1, control, row["binom"]):
            (_, r, m), (_, ms, js) = row["binom"][0], row["pairs"][0]
            e = CP.binom_tables(c, L)[r - 1]
            assert ((e[m - 1] - e[m]) % L != 0) == control
            assert (CP.stepping_relation(c, ms, js) != 0) == control


def test_recoding_and_chain_model():
    for m in range(1, 600):
        ln, pos, neg = CP.small_recode(m)
        assert pos - neg == m and pos & neg == 0 and (pos >> (ln - 1)) == 1
    x = R.mul(12345, R.BASE)
    for m in (1, 2, 3, 7, 12, 31, 100):
        met, y = CP.chain_meets_zero(x, m)
        assert not met and R.equals(y, R.mul(m, x)) and R.encode(y) == R.encode(R.mul(m, x))
    # on a pure torsion point every addition of the chain is exceptional; doublings alone are not
    for tor in (R.IDENTITY, (0, R.P - 1, 1, 0), (R.SQRT_M1, 0, 1, 0)):
        assert [CP.chain_meets_zero(tor, m)[0] for m in (1, 2, 4, 8, 3, 6, 7, 20)] == [False] * 4 + [True] * 4
    # the dedicated addition: exact where Z != 0, Z = 0 on p + p
    p, q = R.mul(5, R.BASE), R.mul(11, R.BASE)
    assert R.encode(CP.ded_add(p, q)) == R.encode(R.mul(16, R.BASE)) and not CP.ded_meets_zero(p, q)
    assert CP.ded_meets_zero(p, p) and CP.ded_factors(p, p) == (True, False)
    assert CP.ded_factors(p, R.neg(p)) == (False, False)  # opposite points are not exceptional


def _stepping_case(h, n, spec, sign):
    seed, m, j, cls_e, cls_a = spec
    a, b = CP.crafted_row(seed, N, N, [(0, m, j)], sign)
    E, A, s, sp = _commit(h, a, b, n)
    _accepts(h, n, E, A, s, sp)
    out = []
    for C, cls in ((E, cls_e), (A, cls_a)):
        assert CP.classify(C, m, j, sign) == cls, (spec, sign)
        x, y = CP.table_entries(C, m, j)
        f, g = CP.ded_factors(x, y)
        if sign > 0:  # F = 0 across O and T2, G = 0 across an offset of order 4
            assert (f, g) == ((False, True) if cls == "T4" else (True, False)), spec
            assert (x[0] % R.P, x[1] % R.P, x[2] % R.P) != (y[0] % R.P, y[1] % R.P, y[2] % R.P)  # never the same limbs
        else:  # opposite entries: the addition is not exceptional; its sum is the pure torsion point
            assert (f, g) == (False, False), spec
            assert CP.torsion_class(CP.ded_add(x, y)) == cls
            zero = bytes(32)
            assert s[32 * j:32 * j + 32] == zero and sp[32 * j:32 * j + 32] == zero  # receiver j's shares
            if cls == "T4":
                assert CP.ded_add(x, y)[1] == 0
        out.append(cls)
    return out


def test_stepping_seeds_cover_every_class(h):
    """The committed stepping seeds: the oracle accepts the rows, the classes are as stated, and for
    the E and the A table each there is an O case at m >= 4 (different representations, F = 0), a T2
    case and a T4 case (G = 0)."""
    specs = list(G.STEP_SEEDS) + list(G.SHAPE1.values())
    for spec in specs:
        _stepping_case(h, 64, spec, +1)
    for spec in G.SHAPE1R.values():
        _stepping_case(h, 70, spec, +1)
    for col in (3, 4):
        assert any(s[col] == "O" and s[1] >= 4 for s in G.STEP_SEEDS)
        assert any(s[col] == "T2" for s in G.STEP_SEEDS)
        assert any(s[col] == "T4" for s in G.STEP_SEEDS)
    # the placement of shape 1's pairs in the tail phases (J_k = n - 32 / 2^k + 1)
    for n, table in ((64, G.SHAPE1), (70, G.SHAPE1R)):
        J = [0] + [n - (32 >> k) + 1 for k in (1, 2, 3)] + [n]
        phase = lambda m, j: next(k for k in range(4) if J[k] <= j < J[k + 1])  # noqa: E731
        assert sorted(phase(m, j) for _, m, j, _, _ in table.values()) == [0, 0, 2, 3]
        assert all(m + 1 < (32 >> phase(m, j)) and m + j < n for _, m, j, _, _ in table.values())


def test_opposite_seeds(h):
    """Opposite entries at m = 0: never exceptional, sums O, T2 and an order-4 point with Y = 0."""
    got = [_stepping_case(h, 64, spec, -1) for spec in G.OPP_SEEDS]
    assert {c for pair in got for c in pair} == {"O", "T2", "T4"}
    assert {pair[0] for pair in got} == {"O", "T2", "T4"}  # each of them on the E table


def test_binomial_seeds(h):
    """The committed binomial seeds (and the second dealer's, seed + 100): the oracle accepts the rows,
    the classes are as stated, and the item m (e_(m-1) + e_m) meets Z = 0 exactly where the GPU file
    expects a rerun.  An equal pair at m >= 2 and an equal pair at m = 1 of class T4 are present for the
    E and the A table each."""
    for seed, r, m, sign, cls_e, cls_a, rerun in G.BINOM_SEEDS:
        for sd, check_cls in ((seed, True), (seed + 100, False)):
            a, b = CP.crafted_row(sd, N, N, [], sign, binom=[(0, r, m)])
            E, A, s, sp = _commit(h, a, b)
            _accepts(h, 64, E, A, s, sp)
            for C, cls in ((E, cls_e), (A, cls_a)):
                x, y = CP.binomial_entries(C, r, m)
                assert CP.classify_binomial(C, r, m, sign) == cls or not check_cls
                assert CP.binomial_item_meets_zero(x, y, m) == rerun, (seed, r, m, sign)
                assert CP.ded_meets_zero(x, y) == (sign > 0)
    eq = [s for s in G.BINOM_SEEDS if s[3] > 0]
    for col in (4, 5):
        assert any(s[2] >= 2 for s in eq) and any(s[2] == 1 and s[col] == "T4" for s in eq)
    assert {s[6] for s in G.BINOM_SEEDS if s[3] < 0 and s[2] >= 2} == {True, False}


def test_wave_and_batch_rows(h):
    """The per-wave cases' rows (relation inside piece 1 of a 2-way split of 16 + 16) and the batch's
    row: accepted by the oracle, related as group elements, exceptional for the dedicated addition."""
    for seed, piece, r, m in G.WAVE_SEEDS:
        for sd in (seed, seed + 100):
            a, b = CP.crafted_row(sd, N, 16, [], +1, binom=[(piece, r, m)])
            E, A, s, sp = _commit(h, a, b)
            _accepts(h, 64, E, A, s, sp)
            for C in (E, A):
                x, y = CP.binomial_entries(C[32 * 16 * piece:32 * 16 * (piece + 1)], r, m)
                assert CP.ded_meets_zero(x, y)
    row = G.BATCH_ROW
    for sd in (row["seed"], row["seed"] + 100):
        a, b = CP.crafted_row(sd, N, N, row["pairs"], +1, False, row["binom"])
        E, A, s, sp = _commit(h, a, b)
        _accepts(h, 64, E, A, s, sp)
        (_, r, m), (_, ms, js) = row["binom"][0], row["pairs"][0]
        for C in (E, A):
            assert CP.ded_meets_zero(*CP.binomial_entries(C, r, m))
            assert CP.ded_meets_zero(*CP.table_entries(C, ms, js))
