"""The fused pair normalisation (k_affine_pairs: the affine addends of a pair's pieces, sum and
difference from one shared inverse) at the shapes tests/test_gpu_jsf.py does not reach: identity
padding columns next to real ones, receiver counts around the point where the lanes per run halve,
a receiver range of more than one run, exceptional pairs in a padded group, and two chunk streams.
Bit-exact at the level of outputs (decisions, sets, shares, master public key) against the CPU
oracle and against mode 3 (per-scalar NAF chains over k_affine_pieces); the affine limbs themselves
are not compared."""
import pytest

import dkg_amd
from dkg_amd import ACCEPT, REJECT, SELF
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

ELL = 2**252 + 27742317777372353535851937790883648493
CK = b"Example of a shared string."


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


def _outputs(r):
    return (bytes(r.dec2), bytes(r.dec4), r.qualified, r.reconstruct, r.complaints2, r.final_share, r.public_share,
            r.mpk)


def _both_modes(be, pieces, run):
    """run() under the default recombination and under mode 3 (pieces = 0: the schedule's own split)."""
    out = []
    try:
        be.set_split(pieces)
        for mode in (0, 3):
            be.set_combine(mode)
            out.append(run())
            assert be.last_combine() == 2 and (be.last_split() == pieces if pieces else mode or be.last_split() in (2, 4))
    finally:
        be.set_combine(0)
        be.set_split(0)
    return out


def _shares(be, n, t, seed):
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(bytes(range(32)), seed, 0, n, t)
    return (h, a, b) + tuple(bytearray(x) for x in be.share_gen(a, b, n, n, t))


def _flip(s, n, i, j):
    assert i != j
    s[32 * (i * n + j)] ^= 1


def _oracle_rows(n, t, h, E, A, s, sp, dealers, r, skip4=()):
    """Rows `dealers` of r's decision matrices against the oracle (a dealer disqualified in round 2 has
    no round-4 row: skip4)."""
    N = t + 1
    for i in dealers:
        for rnd, C, dec in ((2, E, r.dec2), (4, A, r.dec4)):
            if rnd == 4 and i in skip4:
                continue
            acc, rc = O.verify_rows(n, t, rnd, bytes(C[32 * N * i:32 * N * (i + 1)]), h, bytes(s[32 * n * i:32 * n * (i + 1)]),
                                    bytes(sp[32 * n * i:32 * n * (i + 1)]) if rnd == 2 else None, i, i + 1, 0, n)
            assert bytes(dec[i * n:(i + 1) * n]) == bytes(acc), (i, rnd)


# n = 65: the second dealer group is one real column and 63 identity padding columns (Z = 0) per
# segment; n = 33 and 31: just over and under the receiver count where the lanes per run double (launches
# this small run 8 receivers per lane: 4 lanes cover 32), with lanes of fewer receivers than the
# others and a last block of lanes that is partly empty.  t = 7: pieces of 4 and 2 positions.
@pytest.mark.parametrize("pieces", [2, 4])
@pytest.mark.parametrize("n", [65, 33, 31])
def test_pairnorm_small_against_oracle(be, n, pieces):
    t = 7
    h, a, b, E, A, s, sp = _shares(be, n, t, 40 + n)
    flipped, ident = n - 1, 2                   # n = 65: the lone dealer of the padded group rejects
    _flip(s, n, flipped, 1)
    E[32 * (t + 1) * ident:32 * (t + 1) * (ident + 1)] = bytes(32 * (t + 1))    # an all-identity E row
    r0, r3 = _both_modes(be, pieces, lambda: be.ceremony_verify(bytes(E), bytes(A), bytes(s), bytes(sp), n, t))
    assert _outputs(r0) == _outputs(r3)
    _oracle_rows(n, t, h, E, A, s, sp, range(n), r0, skip4=(flipped, ident))
    assert r0.dec2[flipped * n + 1] == REJECT and r0.dec2[flipped * n + 2] == ACCEPT
    assert bytes(r0.dec2[ident * n:(ident + 1) * n]) == bytes(SELF if j == ident else REJECT for j in range(n))
    assert r0.qualified == [int(i not in (flipped, ident)) for i in range(n)]


def test_pairnorm_two_runs_n1100(be):
    """1100 receivers: a full run of 1024 and a short one of 76 per (pair, column).  Tampered shares
    with receivers in both runs and on both sides of the boundary; the whole decision matrices equal
    mode 3's, and the tampered dealers' and three honest dealers' rows equal the oracle's."""
    n, t = 1100, 7
    h, a, b, E, A, s, sp = _shares(be, n, t, 77)
    bad = {3: (5, 1050), 700: (1023, 1024), 1099: (0, 1098)}
    for i, js in bad.items():
        for j in js:
            _flip(s, n, i, j)
    r0, r3 = _both_modes(be, 2, lambda: be.ceremony_verify(bytes(E), bytes(A), bytes(s), bytes(sp), n, t))
    assert _outputs(r0) == _outputs(r3)
    _oracle_rows(n, t, h, E, A, s, sp, list(bad) + [0, 512, 1098], r0, skip4=tuple(bad))
    for i, js in bad.items():
        assert [j for j in range(n) if r0.dec2[i * n + j] == REJECT] == list(js)
    assert r0.qualified == [int(i not in bad) for i in range(n)]


@pytest.mark.parametrize("pieces", [2, 4])
@pytest.mark.parametrize("eq,neg", [(64, 5), (5, 64)])
def test_pairnorm_crafted_pairs_n65(be, pieces, eq, neg):
    """Dealer `eq` has piece 1 = piece 0 (Q_0 - Q_1 is the identity at every receiver), dealer `neg`
    piece 1 = -piece 0 (the sum is); one of them is dealer 64, alone among the identity padding
    columns of the second group.  Honestly shared, so every check accepts through the exceptional
    pair and the shared inverse of f g."""
    n, t = 65, 31
    N, Lp = t + 1, (t + 1) // pieces
    h = be.env_init(t, n, CK)
    a, b = (bytearray(x) for x in dkg_amd.dealer_coefficients(bytes(range(32)), 23, 0, n, t))
    for buf in (a, b):
        for dealer, sign in ((eq, 1), (neg, -1)):
            for k in range(Lp):
                v = int.from_bytes(buf[32 * (dealer * N + k):32 * (dealer * N + k) + 32], "little")
                buf[32 * (dealer * N + Lp + k):32 * (dealer * N + Lp + k) + 32] = (sign * v % ELL).to_bytes(32, "little")
    E, A, s, sp = (bytearray(x) for x in be.share_gen(bytes(a), bytes(b), n, n, t))
    assert E[32 * (eq * N + Lp):32 * (eq * N + 2 * Lp)] == E[32 * eq * N:32 * (eq * N + Lp)]
    r0, r3 = _both_modes(be, pieces, lambda: be.ceremony_verify(bytes(E), bytes(A), bytes(s), bytes(sp), n, t))
    assert _outputs(r0) == _outputs(r3)
    _oracle_rows(n, t, h, E, A, s, sp, (eq, neg, 0, 63), r0)
    for i in (eq, neg):
        honest = bytes(SELF if j == i else ACCEPT for j in range(n))
        assert bytes(r0.dec2[i * n:(i + 1) * n]) == honest and bytes(r0.dec4[i * n:(i + 1) * n]) == honest
    assert r0.qualified == [1] * n


def test_pairnorm_chunk_streams_n512(be):
    """n = 512, t = 255 under the default schedule: 1024 padded columns in 8 dealer groups, and a
    stepping of over 5e7 lane-steps, so verify_device runs two chunk streams (its long_stepping rule)
    and the second chunk's normalisation starts at column offset 512 of planes 1024 columns apart.
    One tampered share per chunk; the outputs equal mode 3's."""
    n, t = 512, 255
    h, a, b, E, A, s, sp = _shares(be, n, t, 9)
    bad = {3: 5, 300: 400}
    for i, j in bad.items():
        _flip(s, n, i, j)
    r0, r3 = _both_modes(be, 0, lambda: be.ceremony_verify(bytes(E), bytes(A), bytes(s), bytes(sp), n, t))
    assert _outputs(r0) == _outputs(r3)
    for i, j in bad.items():
        assert [k for k in range(n) if r0.dec2[i * n + k] == REJECT] == [j]
    assert r0.qualified == [int(i not in bad) for i in range(n)]
    assert sum(r0.qualified) == n - 2
    assert bytes(r0.dec2[:n]) == bytes(SELF if j == 0 else ACCEPT for j in range(n))
