"""The signed radix-4 recoding of the dealing seats' joint chain (seat_deal.h seat_enc_digit through
dkg_seat_enc_digits; k_seat_enc_mul runs the same routine): exact value, digit range and window count
on structured scalars, and the argument rules of the pure function.  CPU only.

Range as the header states it: 128 windows always; digits in {-2, -1, 0, 1} below the top window (127),
which keeps bits 254.. plus the carry: {0, 1, 2} for k < 2^255 and {0, 1} for k < 2^254, so for every
canonical scalar.  "The top" of a canonical scalar's own bits is window 126 (bits 252, 253): single
digits 2 and 3 are set there; window 127 takes the values that fit below 2^255 (digit 1), and 2^255 --
digit 2 there -- is outside the function's domain."""
import ctypes
import random

import pytest

import dkg_amd
from dkg_amd import _lib

L = 2**252 + 27742317777372353535851937790883648493
WINDOWS = 128


def check(k: int):
    d = dkg_amd.seat_enc_digits(k)
    assert len(d) == WINDOWS <= 128
    assert sum(v * 4**i for i, v in enumerate(d)) == k
    assert all(-2 <= v <= 1 for v in d[:-1]), d
    assert 0 <= d[-1] <= (1 if k < 2**254 else 2), d
    return d


EDGES = [0, 1, 2, 3, L - 1, L - 2, 2**252, 2**252 + 1, 2**252 - 1]


@pytest.mark.parametrize("k", EDGES)
def test_small_and_group_order_edges(k):
    check(k)


def test_carry_chains():
    """0xAA..A (every window 2: each gives -2 and carries) and 0x55..5 (every window 1: no carry at all),
    reduced below l."""
    a = int.from_bytes(b"\xaa" * 32, "little") % L
    f = int.from_bytes(b"\x55" * 32, "little") % L
    check(a)
    check(f)
    # the unreduced patterns below 2^255 show the chains themselves
    a2 = int.from_bytes(b"\xaa" * 31 + b"\x2a", "little")  # windows 0..126 hold 2
    d = check(a2)
    assert d[0] == -2 and all(v == -1 for v in d[1:127]) and d[127] == 1
    f2 = int.from_bytes(b"\x55" * 31 + b"\x15", "little")  # windows 0..126 hold 1
    d = check(f2)
    assert d[:127] == [1] * 127 and d[127] == 0


@pytest.mark.parametrize("w", [0, 63, 125, 126])
@pytest.mark.parametrize("v", [2, 3])
def test_single_digit(w, v):
    d = check(v * 4**w)
    want = [0] * WINDOWS
    want[w], want[w + 1] = v - 4, 1
    assert d == want


def test_top_window():
    d = check(4**127)  # bit 254
    assert d == [0] * 127 + [1]
    d = check(4**127 + 2 * 4**126)  # a carry into the top window: it keeps 2
    assert d[126] == -2 and d[127] == 2
    d = check(2**255 - 1)
    assert d[0] == -1 and all(v == 0 for v in d[1:127]) and d[127] == 2


def test_random_scalars():
    rng = random.Random(20260521)
    for _ in range(200):
        check(rng.randrange(L))
    for _ in range(50):
        check(rng.randrange(2**255))


def test_argument_rules():
    lib = _lib.lib()
    d = (ctypes.c_int8 * 128)(*([7] * 128))
    w = ctypes.c_int(-5)
    one = (1).to_bytes(32, "little")
    assert lib.dkg_seat_enc_digits(None, d, ctypes.byref(w)) == _lib.DKG_E_ARG
    assert lib.dkg_seat_enc_digits(one, None, ctypes.byref(w)) == _lib.DKG_E_ARG
    assert lib.dkg_seat_enc_digits(one, d, None) == _lib.DKG_E_ARG
    for big in (2**255, 2**256 - 1):  # the top window would leave its range
        assert lib.dkg_seat_enc_digits(big.to_bytes(32, "little"), d, ctypes.byref(w)) == _lib.DKG_E_ARG
    assert list(d) == [7] * 128 and w.value == -5  # a refused call writes nothing
    assert lib.dkg_seat_enc_digits(one, d, ctypes.byref(w)) == _lib.DKG_OK
    assert w.value == 128 and list(d) == [1] + [0] * 127
    with pytest.raises(dkg_amd.DkgError):
        dkg_amd.seat_enc_digits(2**255)
