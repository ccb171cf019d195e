"""CPU-only checks of the joint-sparse-form recoding behind the pairwise recombination chain
(lattice.cpp jsf_digits through dkg_jsf_digits, runtime.hip short_digit_words through
dkg_split_digits): Solinas' properties on random and structured pairs, and the digit words of
every receiver against the short multipliers they encode."""
import ctypes
import random

import pytest

import dkg_amd
from dkg_amd import _lib


def jsf(a: int, b: int):
    da = ctypes.create_string_buffer(256)
    db = ctypes.create_string_buffer(256)
    top = ctypes.c_int16(-2)
    rc = _lib.lib().dkg_jsf_digits(a.to_bytes(32, "little"), b.to_bytes(32, "little"), da, db, ctypes.byref(top))
    assert rc == _lib.DKG_OK, (hex(a), hex(b))
    sg = lambda raw: [x - 256 if x > 127 else x for x in raw]  # noqa: E731
    return sg(da.raw), sg(db.raw), top.value


def naf_weight(k: int) -> int:
    return bin((3 * k ^ k) >> 1).count("1")


def check_pair(a: int, b: int):
    da, db, top = jsf(a, b)
    assert set(da) <= {-1, 0, 1} and set(db) <= {-1, 0, 1}
    assert sum(d << i for i, d in enumerate(da)) == a
    assert sum(d << i for i, d in enumerate(db)) == b
    # of any three consecutive positions at least one column is zero
    for i in range(254):
        assert any(da[i + k] == 0 and db[i + k] == 0 for k in range(3)), (hex(a), hex(b), i)
    nz = [i for i in range(256) if da[i] or db[i]]
    assert top == (nz[-1] if nz else -1)
    # a JSF is at most one position longer than the longer binary expansion
    assert top <= max(a.bit_length(), b.bit_length())
    assert len(nz) <= naf_weight(a) + naf_weight(b)
    return len(nz)


def test_jsf_random_pairs():
    rng = random.Random(0x4a5346)
    joint = naf = 0
    for k in range(1000):
        bits = (189, 126, 253, 64)[k % 4] if k % 10 else rng.randrange(1, 254)
        a, b = rng.getrandbits(bits), rng.getrandbits(bits)
        joint += check_pair(a, b)
        naf += naf_weight(a) + naf_weight(b)
    # the joint form has every second column nonzero, two NAFs two thirds of them
    assert joint < 0.8 * naf


@pytest.mark.parametrize("x", [1, 2, 3, 0x5a5a5a5a5a5a5a5a, (1 << 189) - 1, (1 << 252) + 12345, (1 << 253) - 1])
def test_jsf_edges_with_x(x):
    check_pair(0, x)
    check_pair(x, 0)
    check_pair(x, x)
    if x + 1 < 1 << 253:
        check_pair(x, x + 1)
        check_pair(x + 1, x)


def test_jsf_edges():
    for k in (1, 2, 3, 31, 32, 63, 64, 65, 127, 128, 189, 251, 252):
        check_pair((1 << k) - 1, (1 << k) + 1)
        check_pair((1 << k) + 1, (1 << k) - 1)
    check_pair((1 << 252) - 1, (1 << 252) - 1)
    check_pair(1, 0)
    check_pair(0, 1)
    check_pair(0, 0)
    assert jsf(0, 0)[2] == -1
    check_pair((1 << 253) - 1, (1 << 253) - 1)   # both maximal below 2^253
    check_pair((1 << 253) - 1, (1 << 253) - 2)
    check_pair((1 << 253) - 1, 1 << 252)


def test_jsf_rejects_a_form_that_does_not_fit():
    da = ctypes.create_string_buffer(256)
    db = ctypes.create_string_buffer(256)
    top = ctypes.c_int16(0)
    big = ((1 << 256) - 1).to_bytes(32, "little")
    assert _lib.lib().dkg_jsf_digits(big, big, da, db, ctypes.byref(top)) == _lib.DKG_E_ARG
    assert _lib.lib().dkg_jsf_digits(None, big, da, db, ctypes.byref(top)) == _lib.DKG_E_ARG


def split_digits(n, L, U, mode):
    dig = ctypes.create_string_buffer(n * U * 256)
    top = (ctypes.c_int16 * n)()
    assert _lib.lib().dkg_split_digits(n, L, U, mode, dig, top) == _lib.DKG_OK
    raw = dig.raw
    rows = [[[x - 256 if x > 127 else x for x in raw[(j * U + u) * 256:(j * U + u + 1) * 256]] for u in range(U)]
            for j in range(n)]
    return rows, list(top)


@pytest.mark.parametrize("L", [8, 128])
@pytest.mark.parametrize("U", [2, 4])
def test_mode_aware_digits_rebuild_the_multipliers(L, U):
    """Every receiver's digit words of the default mode are the signed multipliers that
    dkg_split_multipliers reports (its rows are the default mode's), pair by pair in JSF."""
    n = 64
    mults = dkg_amd.split_multipliers(n, L, U)
    rows, top = split_digits(n, L, U, 0)
    assert split_digits(n, L, U, 2) == (rows, top)
    ell = (1 << 252) + 27742317777372353535851937790883648493
    for j in range(n):
        assert [sum(d << i for i, d in enumerate(rows[j][u])) for u in range(U)] == mults[j]
        nz = [i for i in range(256) if any(rows[j][u][i] for u in range(U))]
        assert top[j] == nz[-1]
        y = pow(j + 1, L, ell)
        assert all((mults[j][u] - mults[j][0] * pow(y, u, ell)) % ell == 0 for u in range(U)) and mults[j][0] > 0
        for p in range(U // 2):  # the pair's columns obey the JSF property whatever the signs
            a, b = rows[j][2 * p], rows[j][2 * p + 1]
            for i in range(254):
                assert any(a[i + k] == 0 and b[i + k] == 0 for k in range(3))


@pytest.mark.parametrize("U", [2, 3, 4])
def test_mode_3_digits_are_nafs(U):
    """Mode 3 keeps one NAF per scalar (no two adjacent nonzero digits) of rows that satisfy the same
    lattice relation; U = 3 has no pairwise chain, so its default digits are those of mode 3."""
    n, L = 64, 8
    rows, top = split_digits(n, L, U, 3)
    ell = (1 << 252) + 27742317777372353535851937790883648493
    for j in range(n):
        v = [sum(d << i for i, d in enumerate(rows[j][u])) for u in range(U)]
        y = pow(j + 1, L, ell)
        assert v[0] > 0 and all((v[u] - v[0] * pow(y, u, ell)) % ell == 0 for u in range(U))
        for u in range(U):
            assert all(not (rows[j][u][i] and rows[j][u][i + 1]) for i in range(255))
    if U == 3:
        assert split_digits(n, L, U, 0) == (rows, top)
    assert _lib.lib().dkg_split_digits(n, L, U, 1, None, None) == _lib.DKG_E_ARG
