"""dkg_commitment_eval_pairs: P_row(x) for a list of (row, index) pairs, one wave per pair (receivers.hip
k_pair_eval).  Expected values are the CPU oracle's multiscalar multiplication with the powers of x, as
tests/test_gpu_receivers.msm_eval computes them; every listed pair is compared, bit for bit."""
import ctypes
import random

import pytest

import dkg_amd
from dkg_amd import DkgError
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

H = bytes.fromhex
L = 2**252 + 27742317777372353535851937790883648493
E_ARG = -1


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


def msm_eval(row, N, x):
    return O.msm(b"".join(pow(x, k, L).to_bytes(32, "little") for k in range(N)), row)


def row_of(C, N, i):
    return C[32 * N * i:32 * N * (i + 1)]


def expect(C, N, pairs, cache):
    out = []
    for i, j in pairs:
        if (i, j) not in cache:
            cache[(i, j)] = msm_eval(row_of(C, N, i), N, j + 1)
        out.append(cache[(i, j)])
    return b"".join(out)


def run(be, D, t, pairs, C):
    return be.commitment_eval_pairs(D, t, [i for i, _ in pairs], [j for _, j in pairs], C)


# ---------------------------------------------------------------- the n = 16, t = 7 ceremony, E and A
@pytest.mark.parametrize("which", ["E", "A"])
def test_ceremony_all_pairs(be, golden, which):
    """All 256 (dealer, receiver) pairs, shuffled, 20 of them listed twice; the shapes 8 lanes / 3 stages
    (automatic), 4 / 2, 3 lanes with a ragged last chunk, and one lane without a stage (8 and 64)."""
    c = golden("ceremony_n16_t7.json")
    n, t = c["n"], c["t"]
    N = t + 1
    C = H(c[which])
    rng = random.Random(16)
    pairs = [(i, j) for i in range(n) for j in range(n)]
    pairs += rng.sample(pairs, 20)
    rng.shuffle(pairs)
    cache = {}
    exp = expect(C, N, pairs, cache)
    assert dkg_amd.pair_eval_shape(t, 0) == {"chunk": 1, "lanes": 8, "stages": 3}
    assert dkg_amd.pair_eval_shape(t, 3) == {"chunk": 3, "lanes": 3, "stages": 2}
    try:
        for chunk in (0, 2, 3, 8, 64):
            be.set_receiver_chunk(chunk)
            P, ok = run(be, n, t, pairs, C)
            assert ok == b"\x01" * len(pairs), chunk
            assert P == exp, chunk
            assert be.last_receiver_chunk() == min(chunk or 1, N)
        # one undecodable coefficient: ok and the zero bytes land on exactly the pairs that name row 6
        bad = bytearray(C)
        k = 32 * (N * 6 + 3)
        bad[k:k + 32] = H(golden("kat_group.json")["invalid_encodings"][1])
        # an all-identity row: every evaluation is the identity, whose encoding is 32 zero bytes, and ok = 1
        bad[32 * N * 9:32 * N * 10] = bytes(32 * N)
        for chunk in (0, 3):
            be.set_receiver_chunk(chunk)
            P, ok = run(be, n, t, pairs, bytes(bad))
            assert ok == bytes(int(i != 6) for i, _ in pairs), chunk
            for p, (i, _) in enumerate(pairs):
                assert P[32 * p:32 * p + 32] == (bytes(32) if i in (6, 9) else exp[32 * p:32 * p + 32]), (chunk, p)
    finally:
        be.set_receiver_chunk(0)


# ---------------------------------------------------------------- two rows of 128 coefficients
def test_spot_rows(be, golden):
    """Automatic chunk: L = 2, the full 64 lanes, 6 stages; forced 3 (43 lanes, ragged), 5 (26 lanes) and
    128 (one lane, no stage)."""
    sp = golden("spot_n256_t127.json")
    t = sp["t"]
    N = t + 1
    C = b"".join(H(d["E"]) for d in sp["dealers"])
    js = [0, 1, 170, 254, 255]
    pairs = [(d, j) for j in js for d in range(2)]
    random.Random(5).shuffle(pairs)
    exp = expect(C, N, pairs, {})
    covered = 0
    for d, drow in enumerate(sp["dealers"]):  # the fixture's own right-hand sides where they cover a pair
        for pr in drow["pairs"]:
            if (d, pr["receiver"]) in pairs:
                p = pairs.index((d, pr["receiver"]))
                assert exp[32 * p:32 * p + 32].hex() == pr["rhs2"]
                covered += 1
    assert covered
    assert dkg_amd.pair_eval_shape(t, 0) == {"chunk": 2, "lanes": 64, "stages": 6}
    try:
        for chunk in (0, 3, 5, 128):
            be.set_receiver_chunk(chunk)
            P, ok = run(be, 2, t, pairs, C)
            assert ok == b"\x01" * len(pairs), chunk
            assert P == exp, chunk
    finally:
        be.set_receiver_chunk(0)


# ---------------------------------------------------------------- lengths around the wave boundary
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 129, 256])
def test_lengths_around_the_wave(be, golden, N):
    """Prefixes and suffixes of the two spot rows concatenated (a run of commitment points is a commitment
    row) at x = 1 (the empty chain), a power of two, and 2^24, the largest index js admits, whose
    multipliers pass l from the first stage on."""
    sp = golden("spot_n256_t127.json")
    cat = b"".join(H(d["E"]) for d in sp["dealers"])
    assert len(cat) == 32 * 256
    C = cat[:32 * N] + cat[32 * (256 - N):]
    pairs = [(i, x - 1) for x in (1, 4096, 1 << 24) for i in range(2)]
    exp = expect(C, N, pairs, {})
    P, ok = run(be, 2, N - 1, pairs, C)
    assert ok == b"\x01" * len(pairs)
    for p in range(len(pairs)):
        assert P[32 * p:32 * p + 32] == exp[32 * p:32 * p + 32], pairs[p]


# ---------------------------------------------------------------- both copies of k_pair_eval
def test_field_modes(be, golden):
    """k_pair_eval is compiled with both field multiplications and the runtime picks one per launch: the
    product-scanning copy (dkg_ctx_set_field_mode 1) and the column-sum copy (2) give the bytes of the
    default, at N = 65 (one past a wave) and on the n = 16 ceremony's shuffled pairs with a forced chunk."""
    sp = golden("spot_n256_t127.json")
    cat = b"".join(H(d["E"]) for d in sp["dealers"])
    N = 65
    C65 = cat[:32 * N] + cat[32 * (256 - N):]
    pairs65 = [(i, x - 1) for x in (1, 4096, 1 << 24) for i in range(2)]
    c = golden("ceremony_n16_t7.json")
    n, t = c["n"], c["t"]
    CE = H(c["E"])
    rng = random.Random(16)
    pairs = [(i, j) for i in range(n) for j in range(n)]
    rng.shuffle(pairs)
    exp65, exp = expect(C65, N, pairs65, {}), expect(CE, t + 1, pairs, {})
    try:
        for mode in (0, 1, 2):
            be.set_field_mode(mode)
            be.set_receiver_chunk(0)
            assert run(be, 2, N - 1, pairs65, C65) == (exp65, b"\x01" * len(pairs65)), mode
            for chunk in (0, 3):
                be.set_receiver_chunk(chunk)
                assert run(be, n, t, pairs, CE) == (exp, b"\x01" * len(pairs)), (mode, chunk)
    finally:
        be.set_field_mode(0)
        be.set_receiver_chunk(0)


# ---------------------------------------------------------------- order, slots, arguments
def test_order_independence(be, golden):
    """The same pairs permuted give the permuted outputs: an item's slot among the call's distinct indices
    (its digit record) and its row's place among the gathered rows belong to that item alone."""
    c = golden("ceremony_n16_t7.json")
    n, t = c["n"], c["t"]
    N = t + 1
    C = H(c["A"])
    rng = random.Random(77)
    idx = [0, 1, 2, 15, 682, 4095, (1 << 20) + 2, (1 << 24) - 1]
    pairs = [(rng.randrange(n), rng.choice(idx)) for _ in range(40)]
    exp = expect(C, N, pairs, {})
    P, ok = run(be, n, t, pairs, C)
    assert P == exp and ok == b"\x01" * 40
    perm = list(range(40))
    rng.shuffle(perm)
    P2, _ = run(be, n, t, [pairs[p] for p in perm], C)
    assert P2 == b"".join(P[32 * p:32 * p + 32] for p in perm)
    for p in (0, 17, 39):  # and alone, in slot 0 of its own call
        assert run(be, n, t, [pairs[p]], C)[0] == exp[32 * p:32 * p + 32]


def test_argument_errors(be, golden):
    c = golden("ceremony_n16_t7.json")
    n, t = c["n"], c["t"]
    C = H(c["E"])
    for pairs in ([(n, 0)], [(0, 0), (n + 5, 3)], [(0, 1 << 24)], [(3, 2), (3, 0xffffffff)]):
        with pytest.raises(DkgError) as e:
            run(be, n, t, pairs, C)
        assert e.value.code == E_ARG
    sp = golden("spot_n256_t127.json")
    row = H(sp["dealers"][0]["E"])
    try:
        be.set_receiver_chunk(1)  # 128 lanes
        with pytest.raises(DkgError) as e:
            run(be, 1, sp["t"], [(0, 0)], row)
        assert e.value.code == E_ARG
        be.set_receiver_chunk(2)
        assert run(be, 1, sp["t"], [(0, 0)], row)[1] == b"\x01"
    finally:
        be.set_receiver_chunk(0)
    lib = dkg_amd.lib()
    one = (ctypes.c_uint32 * 1)(0)
    assert lib.dkg_commitment_eval_pairs(be._ctx, n, t, 1, one, one, C, None, None) == E_ARG  # NULL P
    assert lib.dkg_commitment_eval_pairs(be._ctx, n, t, 1, None, one, C, None, None) == E_ARG
    P = ctypes.create_string_buffer(b"\xaa" * 32, 32)
    ok = ctypes.create_string_buffer(b"\xaa", 1)
    assert lib.dkg_commitment_eval_pairs(be._ctx, n, t, 0, None, None, None, P, ok) == 0  # count = 0
    assert P.raw == b"\xaa" * 32 and ok.raw == b"\xaa"
    assert run(be, n, t, [], C) == (b"", b"")
    assert lib.dkg_commitment_eval_pairs(be._ctx, n, t, 1, one, one, C, P, None) == 0  # ok may be NULL
    assert P.raw == msm_eval(row_of(C, t + 1, 0), t + 1, 1)
