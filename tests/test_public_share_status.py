"""dkg_public_share_status (host only, no GPU): the status dkg_public_shares reports per (ceremony, index),
against the rule of tests/public_share_ref.py on the libsodium fixtures and on random draws; the precedence,
`which` and every DKG_E_ARG case."""
import ctypes
import random

import pytest

import dkg_amd
from dkg_amd import DkgError
from tests import public_share_ref as PR

FIXTURES = ["ceremony_n10_t4", "fault_recon_only_n10_t4", "fault_share_flip_n10_t4", "fault_a_generator_n10_t4",
            "fault_self_share_n10_t4", "fault_e_identity_n10_t4", "fault_recon_r2err_n16_t3"]


def test_constants():
    assert (dkg_amd.DKG_PS_OK, dkg_amd.DKG_PS_NO_COMMITMENT, dkg_amd.DKG_PS_NO_DISCLOSURE) == (0, 1, 2)
    assert (PR.OK, PR.NO_COMMITMENT, PR.NO_DISCLOSURE) == (0, 1, 2)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(golden, name):
    c = golden(name + ".json")
    n, q, r = c["n"], c["qualified"], c["reconstruct"]
    pairs = [(j + 1, i + 1) for i in range(n) if r[i] for j in range(n)]
    for j in range(n):
        assert dkg_amd.public_share_status(n, q, r, j, pairs) == (dkg_amd.DKG_PS_OK, -1)
        assert dkg_amd.public_share_status(n, q, None if not any(r) else r, j, pairs) == (dkg_amd.DKG_PS_OK, -1)
        for drop in pairs:
            less = [p for p in pairs if p != drop]
            want = PR.status(n, q, r, j, less)
            assert want == ((PR.NO_DISCLOSURE, drop[1] - 1) if drop[0] == j + 1 else (PR.OK, -1))
            assert dkg_amd.public_share_status(n, q, r, j, less) == want
        for i in range(n):
            ap = [1] * n
            ap[i] = 0
            want = PR.status(n, q, r, j, pairs, ap)
            assert want == ((PR.NO_COMMITMENT, i) if q[i] and not r[i] else (PR.OK, -1))
            assert dkg_amd.public_share_status(n, q, r, j, pairs, ap) == want


def test_random_draws():
    rng = random.Random(2024)
    seen = set()
    for _ in range(400):
        n = rng.randint(1, 12)
        q = [int(rng.random() < 0.8) for _ in range(n)]
        r = [int(q[i] and rng.random() < 0.3) for i in range(n)]
        ap = None if rng.random() < 0.4 else [int(rng.random() < 0.9) for _ in range(n)]
        every = [(s + 1, d + 1) for s in range(n) for d in range(n)]
        pairs = [p for p in every if rng.random() < rng.choice([0.5, 0.9, 1.0])]
        rng.shuffle(pairs)
        j = rng.randrange(n)
        want = PR.status(n, q, r, j, pairs, ap)
        assert dkg_amd.public_share_status(n, q, r, j, pairs, ap) == want, (n, q, r, ap, pairs, j)
        if not any(r):
            assert dkg_amd.public_share_status(n, q, None, j, pairs, ap) == want
        seen.add(want[0])
    assert seen == {PR.OK, PR.NO_COMMITMENT, PR.NO_DISCLOSURE}


def test_precedence_and_which():
    n, q, r = 6, [1, 1, 1, 1, 0, 1], [0, 1, 0, 1, 0, 0]
    full = [(3, 2), (3, 4)]
    assert dkg_amd.public_share_status(n, q, r, 2, full) == (dkg_amd.DKG_PS_OK, -1)
    assert dkg_amd.public_share_status(n, q, r, 2, [(3, 4)]) == (dkg_amd.DKG_PS_NO_DISCLOSURE, 1)
    assert dkg_amd.public_share_status(n, q, r, 2, [(3, 2), (2, 4)]) == (dkg_amd.DKG_PS_NO_DISCLOSURE, 3)
    # a missing commitment wins over a missing disclosure, the lowest used dealer first
    assert dkg_amd.public_share_status(n, q, r, 2, [], [1, 1, 0, 1, 1, 0]) == (dkg_amd.DKG_PS_NO_COMMITMENT, 2)
    # absent rows of dealers the sum does not use (reconstructed 1, 3; disqualified 4) change nothing
    assert dkg_amd.public_share_status(n, q, r, 2, full, [1, 0, 1, 0, 0, 1]) == (dkg_amd.DKG_PS_OK, -1)
    # entries of other senders and of dealers that are not reconstructed are ignored
    assert dkg_amd.public_share_status(n, q, r, 2, full + [(1, 1), (6, 5), (3, 3)]) == (dkg_amd.DKG_PS_OK, -1)


def test_arguments():
    q, r = [1, 1, 1], [0, 1, 0]
    for args in [(0, [], [], 0, []),                 # n == 0
                 (3, q, r, 3, []),                   # j >= n
                 (3, [1, 0, 1], r, 0, []),           # reconstruct without qualified
                 (3, q, r, 0, [(0, 2)]),             # sender outside 1..n
                 (3, q, r, 0, [(4, 2)]),
                 (3, q, r, 0, [(1, 0)]),             # dealer outside 1..n
                 (3, q, r, 0, [(1, 4)]),
                 (3, q, r, 0, [(1, 2), (2, 2), (1, 2)])]:  # a duplicate pair
        with pytest.raises(DkgError):
            dkg_amd.public_share_status(*args)
    # NULL required pointers, through the C entry point
    fn = dkg_amd.lib().dkg_public_share_status
    which = ctypes.c_int32(7)
    one = (ctypes.c_uint32 * 1)(1)
    assert fn(3, None, bytes(r), None, 0, 0, None, None, ctypes.byref(which)) == -1
    assert fn(3, bytes(q), bytes(r), None, 0, 1, None, one, ctypes.byref(which)) == -1
    assert fn(3, bytes(q), bytes(r), None, 0, 1, one, None, ctypes.byref(which)) == -1
    # a NULL `which` is allowed
    assert fn(3, bytes(q), bytes(r), None, 0, 0, None, None, None) == dkg_amd.DKG_PS_NO_DISCLOSURE
