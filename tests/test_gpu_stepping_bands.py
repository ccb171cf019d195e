"""The stepping's banded lane map (dkg_amd/csrc/step_map.h, kernels.hip k_stepping<.., BAND>) at the
smallest shapes that reach each of its branches, through dkg_share_gen + dkg_verify_pairs with the
split forced.  The shapes put t + 1 = 2 P or 4 P positions on n barely above it so that bands die at
several different steps; they lie outside the ceremony's t < (n + 1) / 2 (committee.rs:73), which
the pair verification does not need, so what is compared are the decision rows of both rounds (a
ceremony's final shares and mpk follow from them and the inputs alone).

Every case tampers a few shares of dealer 0, one E coefficient of dealer 1 and one A coefficient of
dealer 2; the whole rows of those dealers and of the last dealer come from the C oracle's per-pair
MSM checks (committee.rs:287-305, 532-548) as in tests/test_gpu_scale.py, every other row must
accept everywhere but its SELF diagonal.  The dedicated stepping's outputs equal the complete
formula's (dkg_ctx_set_stepping_formula 1) byte for byte."""
import random

import pytest

import dkg_amd
from dkg_amd import ACCEPT, REJECT, SELF
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

L = 2**252 + 27742317777372353535851937790883648493
CK = b"Example of a shared string."


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


def _bump(buf, off):
    v = (int.from_bytes(buf[off:off + 32], "little") + 1) % L
    buf[off:off + 32] = v.to_bytes(32, "little")


def _committee(be, n, t, D, seed):
    """D dealers' broadcasts for n receivers with the faults above; {(dealer, round): oracle row}."""
    N = t + 1
    h = be.env_init(1, n, CK)  # the commitment key only: h does not depend on (t, n)
    a, b = dkg_amd.dealer_coefficients(bytes([seed]) * 32, 5, 0, D, t)
    E, A, s, sp = (bytearray(x) for x in be.share_gen(a, b, D, n, t))
    rng = random.Random(seed)
    for j in sorted({1, n // 2, n - 1, rng.randrange(1, n)}):  # dealer 0: shares of receivers in every band
        _bump(s, 32 * (0 * n + j))
    k = rng.randrange(N)
    E[32 * (1 * N + k):32 * (1 * N + k) + 32] = O.base_mul(rng.randrange(1, L).to_bytes(32, "little"))
    A[32 * (2 * N + N - 1):32 * (2 * N + N)] = O.base_mul(rng.randrange(1, L).to_bytes(32, "little"))
    exp = {}
    row = lambda buf, w, i: bytes(buf[w * i:w * (i + 1)])  # noqa: E731
    for i, rnd in ((0, 2), (0, 4), (1, 2), (2, 4), (D - 1, 2), (D - 1, 4)):
        C = E if rnd == 2 else A
        acc, rc = O.verify_rows(n, t, rnd, row(C, 32 * N, i), h, row(s, 32 * n, i),
                                row(sp, 32 * n, i) if rnd == 2 else None, i, i + 1, 0, n)
        assert rc == 0
        exp[(i, rnd)] = acc
    # the faults are visible: an all-accept answer cannot pass
    assert exp[(0, 2)].count(REJECT) >= 3 and exp[(0, 4)].count(REJECT) >= 3
    assert exp[(1, 2)].count(REJECT) >= n - 2 and exp[(2, 4)].count(REJECT) >= n - 2
    return E, A, s, sp, exp


def _verify(be, n, t, D, E, A, s, sp, split, stepping=0, formula=0):
    """(dec2, dec4, redos of round 2, redos of round 4) with the split and the slot mode forced."""
    be.set_split(split)
    be.set_stepping(stepping)
    be.set_stepping_formula(formula)
    try:
        d2 = be.verify_pairs(n, t, 2, 0, D, bytes(E), bytes(s), bytes(sp))
        r2 = be.stepping_redos()
        assert be.last_split() == split
        d4 = be.verify_pairs(n, t, 4, 0, D, bytes(A), bytes(s))
        r4 = be.stepping_redos()
        assert be.last_split() == split
    finally:
        be.set_split(0)
        be.set_stepping(0)
        be.set_stepping_formula(0)
    return d2, d4, r2, r4


def _check(n, D, d2, d4, exp, ctx):
    for i in range(D):
        for rnd, dec in ((2, d2), (4, d4)):
            want = exp.get((i, rnd), bytes(SELF if j == i else ACCEPT for j in range(n)))
            assert dec[i * n:(i + 1) * n] == want, (ctx, i, rnd)


# n, t, U, dealers, stepping slot modes (dkg_ctx_set_stepping: 0 cost model, 1 per column, 2 per piece)
CASES = [
    (300, 255, 2, 300, (0,)),    # P = 128, two segments per 256-lane workgroup (the n = 1024 headline's
                                 # stepping shape), band 32; nrecv = 300: bands die at four different steps
    (130, 127, 2, 130, (0,)),    # P = 64, four segments per workgroup, band 16, nrecv barely above 2 P
    (300, 255, 4, 300, (1, 2)),  # four pieces of 64: the whole-column form (one slot per column) against
                                 # per-piece launches
    (300, 200, 2, 300, (0,)),    # a short last piece: ragged Plast, Nlive < P (contiguous map)
    (70, 63, 2, 70, (0, 1, 2)),  # P = 32, band 8, nrecv < 2 P + 8: upper bands dead for most of the launch
    (300, 255, 2, 70, (0,)),     # a ragged dealer count: identity padding columns must not mark
]


@pytest.mark.parametrize("n,t,U,D,modes", CASES)
def test_banded_stepping_matches_oracle(be, n, t, U, D, modes):
    E, A, s, sp, exp = _committee(be, n, t, D, seed=(n + t + U + D) % 251)
    outs = []
    for mode in modes:
        d2, d4, r2, r4 = _verify(be, n, t, D, E, A, s, sp, U, stepping=mode)
        assert (r2, r4) == (0, 0), (mode, r2, r4)  # no exceptional pair: nothing marks, padding included
        _check(n, D, d2, d4, exp, (n, t, U, D, mode))
        outs.append((d2, d4))
    assert all(o == outs[0] for o in outs)  # the slot modes' outputs are identical
    c2, c4, r2, r4 = _verify(be, n, t, D, E, A, s, sp, U, stepping=modes[-1], formula=1)
    assert (c2, c4) == outs[0] and (r2, r4) == (0, 0)


def test_banded_stepping_redo(be):
    """n = 300, t = 255, U = 2 with one dealer's E row all identity (committee.rs:1127; the recipe of
    test_gpu_scale.test_stepping_redo_at_scale): its dedicated additions are exceptional, the marked
    workgroup is redone by the complete formula on the same grid and lane map, and the outputs equal
    the complete formula's; the same committee without the crafted row redoes nothing."""
    n, t, U, D = 300, 255, 2, 300
    N = t + 1
    E, A, s, sp, exp = _committee(be, n, t, D, seed=77)
    d2, d4, r2, r4 = _verify(be, n, t, D, E, A, s, sp, U)
    assert (r2, r4) == (0, 0)
    _check(n, D, d2, d4, exp, "control")
    d = D - 2  # a dealer of the last stepping workgroup
    E[32 * d * N:32 * (d + 1) * N] = bytes(32 * N)
    x2, x4, r2, r4 = _verify(be, n, t, D, E, A, s, sp, U)
    c2, c4, q2, q4 = _verify(be, n, t, D, E, A, s, sp, U, formula=1)
    assert (x2, x4) == (c2, c4)
    assert r2 > 0 and r4 == 0 and (q2, q4) == (0, 0)
    exp[(d, 2)] = bytes(SELF if j == d else REJECT for j in range(n))  # identity commitments: all reject
    _check(n, D, x2, x4, exp, "identity row")
