"""Hosted seats deal round 1 (dkg_party_round1_seats: k_commit / k_share_eval with D = S, e1 on the shared
comb, K = pk r by the joint radix-4 chain k_seat_enc_mul or by a radix-16 comb per key slot): against the
full-mode fixtures, against share_gen(D = 1) + encrypt_shares(D = 1) per seat, against the CPU oracle's
hybrid_encrypt item by item on edge keys and edge scalars, and through party_round2_seats -- bit for bit,
under both routes and the automatic one."""
import ctypes
import random

import pytest

import dkg_amd
from dkg_amd import ACCEPT, SELF, DkgError, _lib
from dkg_amd import broadcast as BC
from tests import oracle_lib as O
from tests.test_gpu import CK, H, L

pytestmark = pytest.mark.gpu

BAD = b"\xff" * 32  # not a point
KEYS = ("E", "A", "e1", "ct", "s", "s_prime", "own")


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


def sc(v: int) -> bytes:
    return (v % L).to_bytes(32, "little")


def scalars(rng, count) -> bytes:
    return b"".join(sc(rng.randrange(L)) for _ in range(count))


def keys(rng, count) -> bytes:
    return b"".join(O.base_mul(sc(rng.randrange(1, L))) for _ in range(count))


def deal(be, B, n, t, cer, js, a, b, r, pk):
    """party_round1_seats under the joint chain, the comb route and the automatic mode: equal outputs."""
    out = {}
    try:
        for mode in (2, 1):
            be.set_seat_deal(mode)
            out[mode] = be.party_round1_seats(B, n, t, cer, js, a, b, r, pk)
            assert be.last_seat_deal() == mode
    finally:
        be.set_seat_deal(0)
    out[0] = be.party_round1_seats(B, n, t, cer, js, a, b, r, pk)
    assert be.last_seat_deal() in (1, 2)
    for k in KEYS:
        assert out[1][k] == out[2][k], (k, "routes 1 and 2 differ")
        assert out[0][k] == out[2][k], (k, "automatic differs")
    return out[2]


def per_seat(be, n, t, cer, js, a, b, r, pk):
    """The same rows by one share_gen(D = 1) + one encrypt_shares(D = 1) per seat."""
    N = t + 1
    out = {k: b"" for k in KEYS}
    for p, (c, j) in enumerate(zip(cer, js)):
        E, A, s, sp = be.share_gen(a[32 * N * p:32 * N * (p + 1)], b[32 * N * p:32 * N * (p + 1)], 1, n, t)
        e1, ct = be.encrypt_shares(pk[32 * n * c:32 * n * (c + 1)], s, sp, r[64 * n * p:64 * n * (p + 1)], 1, n)
        own = sp[32 * j:32 * j + 32] + s[32 * j:32 * j + 32]
        for k, v in zip(KEYS, (E, A, e1, ct, s, sp, own)):
            out[k] += v
    return out


def random_case(seed, B, n, t, seats, bad_ceremonies=()):
    rng = random.Random(seed)
    S, N = len(seats), t + 1
    pk = b"".join(BAD * n if c in bad_ceremonies else keys(rng, n) for c in range(B))
    return ([c for c, _ in seats], [j for _, j in seats], scalars(rng, S * N), scalars(rng, S * N),
            scalars(rng, 2 * S * n), pk)


# ---------------------------------------------------------------- fixtures: every dealer a seat, shuffled
@pytest.mark.parametrize("name", ["full_n4_t1.json", "full_n8_t3.json", "full_n10_t4.json"])
def test_goldens(be, golden, name):
    c = golden(name)
    n, t = c["n"], c["t"]
    N = t + 1
    assert H(c["ck_bytes"]) == CK
    be.env_init(t, n, CK)
    order = list(range(n))
    random.Random(n).shuffle(order)
    row = lambda key, w, i: H(c[key])[w * i:w * (i + 1)]  # noqa: E731
    a = b"".join(row("a", 32 * N, i) for i in order)
    b = b"".join(row("b", 32 * N, i) for i in order)
    r = b"".join(row("enc_r", 64 * n, i) for i in order)
    out = deal(be, 1, n, t, [0] * n, order, a, b, r, H(c["member_pk"]))
    for key, fx, w in (("E", "E", 32 * N), ("A", "A", 32 * N), ("s", "s", 32 * n), ("s_prime", "s_prime", 32 * n),
                       ("e1", "e1", 64 * n), ("ct", "ct", 64 * n)):
        assert out[key] == b"".join(row(fx, w, i) for i in order), key
    assert out["own"] == b"".join(row("s_prime", 32 * n, i)[32 * i:32 * i + 32] + row("s", 32 * n, i)[32 * i:32 * i + 32]
                                  for i in order)
    # the seats' broadcasts, in dealer order, are what the committee's intake reads
    msgs = [None] * n
    for p, i in enumerate(order):
        m = BC.seat_phase1(n, out["E"][32 * N * p:32 * N * (p + 1)], out["e1"][64 * n * p:64 * n * (p + 1)],
                           out["ct"][64 * n * p:64 * n * (p + 1)])
        msgs[i] = BC.BroadcastPhase1.from_bytes(m.to_bytes())
        assert msgs[i] == m and [e.recipient_index for e in m.encrypted_shares] == list(range(1, n + 1))
    p1 = BC.intake_phase1(n, t, msgs, mode=1)
    assert p1.fetched1 == bytes([1] * n) and p1.fetch_invalid == bytes(n) and p1.E == H(c["E"])
    assert BC._hybrid_items(n, p1) == (H(c["e1"]), H(c["ct"]))


# ---------------------------------------------------------------- equality with the per-seat calls
SHAPES = [
    ("one_coefficient", 1, 2, 0, [(0, 0), (0, 1)], ()),
    ("n3", 2, 3, 1, [(1, 2), (0, 0)], ()),
    ("wave_boundary_65_slots", 2, 13, 6, [(0, 0), (1, 12), (0, 5), (1, 1), (1, 7)], ()),
    ("one_wave", 1, 64, 31, [(0, 63)], ()),
    ("ragged_140_slots", 2, 70, 34, [(1, 69), (0, 3)], ()),
    ("only_ceremony_1_named", 3, 5, 2, [(1, 4), (1, 0)], (0, 2)),
    ("shared_ceremony_and_repeat", 2, 6, 2, [(1, 3), (1, 4), (0, 2), (1, 3)], ()),
]


@pytest.mark.parametrize("name,B,n,t,seats,bad", SHAPES, ids=[s[0] for s in SHAPES])
def test_equals_per_seat_calls(be, name, B, n, t, seats, bad):
    be.env_init(t, n, CK)
    cer, js, a, b, r, pk = random_case(len(name) * 100 + n, B, n, t, seats, bad)
    got = deal(be, B, n, t, cer, js, a, b, r, pk)
    want = per_seat(be, n, t, cer, js, a, b, r, pk)
    for k in KEYS:
        assert got[k] == want[k], k
    if name == "shared_ceremony_and_repeat":  # the same seat twice: the same row twice (its inputs differ here,
        cer2, js2 = cer + [cer[0]], js + [js[0]]  # so append a true repeat)
        N = t + 1
        rep = deal(be, B, n, t, cer2, js2, a + a[:32 * N], b + b[:32 * N], r + r[:64 * n], pk)
        for k, w in (("E", 32 * N), ("e1", 64 * n), ("ct", 64 * n), ("s", 32 * n), ("own", 64)):
            assert rep[k][:-w] == got[k] and rep[k][-w:] == got[k][:w], k


def test_forced_chunk(be):
    """Seats per chunk forced to 2 (5 seats: chunks of 2, 2, 1) and to 1: the outputs do not move."""
    B, n, t = 2, 13, 6
    be.env_init(t, n, CK)
    seats = [(0, 0), (1, 12), (0, 5), (1, 1), (1, 7)]
    cer, js, a, b, r, pk = random_case(77, B, n, t, seats)
    whole = deal(be, B, n, t, cer, js, a, b, r, pk)
    try:
        for chunk in (2, 1):
            be.set_batch_full_chunk(chunk)
            got = deal(be, B, n, t, cer, js, a, b, r, pk)
            for k in KEYS:
                assert got[k] == whole[k], (chunk, k)
    finally:
        be.set_batch_full_chunk(0)
    want = per_seat(be, n, t, cer, js, a, b, r, pk)
    assert all(whole[k] == want[k] for k in KEYS)


# ---------------------------------------------------------------- edges against the CPU oracle, item by item
def radix4_edges():
    """The recoding's structured scalars (tests/test_seat_deal_digits.py), canonical."""
    e = [0, 1, 2, 3, L - 1, L - 2, 2**252, 2**252 + 1, 2**252 - 1,
         int.from_bytes(b"\xaa" * 32, "little") % L, int.from_bytes(b"\x55" * 32, "little") % L]
    e += [v * 4**w for w in (0, 63, 125) for v in (2, 3)] + [2 * 4**126 % L, 3 * 4**126 % L]
    return e


def test_edge_keys_and_scalars_against_oracle(be):
    n, t = 11, 5
    be.env_init(t, n, CK)
    rng = random.Random(5)
    edges = radix4_edges()
    S = 2 * ((len(edges) + n - 1) // n)  # every edge scalar once in each w position
    slots = S * n // 2
    edges = edges + [rng.randrange(L) for _ in range(slots - len(edges))]
    r = bytearray()
    for p in range(S):
        for q in range(n):
            e = sc(edges[(p // 2) * n + q])
            other = sc(rng.randrange(L))
            r += (e + other) if p % 2 == 0 else (other + e)
    r = bytes(r)
    # ceremony 0: the identity, g and (l - 1) g among random keys; ceremony 1: random keys
    pk0 = [bytes(32), O.base_mul(sc(1)), O.base_mul(sc(L - 1))] + [keys(rng, 1) for _ in range(n - 3)]
    rng.shuffle(pk0)
    pk = b"".join(pk0) + keys(rng, n)
    cer = [(p // 2) % 2 for p in range(S)]  # seats 0 and 1: both w positions of the first edges meet the edge keys
    js = [rng.randrange(n) for _ in range(S)]
    a, b = scalars(rng, S * (t + 1)), scalars(rng, S * (t + 1))
    out = deal(be, 2, n, t, cer, js, a, b, r, pk)
    for p in range(S):
        for q in range(n):
            for w, msg in enumerate((out["s_prime"], out["s"])):
                k = (p * n + q) * 2 + w
                want = O.hybrid_encrypt(pk[32 * (cer[p] * n + q):32 * (cer[p] * n + q + 1)], r[32 * k:32 * k + 32],
                                        msg[32 * (p * n + q):32 * (p * n + q + 1)])
                assert want is not None
                assert (out["e1"][32 * k:32 * k + 32], out["ct"][32 * k:32 * k + 32]) == want, (p, q, w)


def test_round2_on_dealt_ceremony(be, golden):
    """Every party of a small ceremony deals as a seat; every party then runs round 2 as a seat on what was
    dealt: ACCEPT or SELF everywhere, and the decrypted shares are the dealt ones."""
    c = golden("full_n8_t3.json")
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    rng = random.Random(9)
    a, b, r = scalars(rng, n * (t + 1)), scalars(rng, n * (t + 1)), scalars(rng, 2 * n * n)
    seats = list(range(n))
    out = deal(be, 1, n, t, [0] * n, seats, a, b, r, H(c["member_pk"]))
    col = lambda buf, j: b"".join(buf[64 * (i * n + j):64 * (i * n + j + 1)] for i in range(n))  # noqa: E731
    e1c = b"".join(col(out["e1"], j) for j in seats)
    ctc = b"".join(col(out["ct"], j) for j in seats)
    r2 = be.party_round2_seats(1, n, t, [0] * n, seats, out["E"], e1c, ctc, H(c["member_sk"]))
    assert all(r2["dec"][j * n + i] == (SELF if i == j else ACCEPT) for j in seats for i in range(n))
    assert r2["complaints"] == [0] * n and r2["r2_error"] == [0] * n
    scol = lambda buf, j: b"".join(buf[32 * (i * n + j):32 * (i * n + j + 1)] for i in range(n))  # noqa: E731
    assert r2["s"] == b"".join(scol(out["s"], j) for j in seats)
    assert r2["s_prime"] == b"".join(scol(out["s_prime"], j) for j in seats)


# ---------------------------------------------------------------- arguments, errors, phase times
def raw_call(b, B, n, t, cer, js, a, bb, r, pk, E, A, e1, ct, s=None, sp=None, own=None):
    S = len(cer)
    ca, ja = (ctypes.c_uint32 * max(S, 1))(*cer), (ctypes.c_uint32 * max(S, 1))(*js)
    return _lib.lib().dkg_party_round1_seats(b._ctx, B, n, t, S, ca, ja, a, bb, r, pk, E, A, e1, ct, s, sp, own)


def test_arguments(golden):
    c = golden("full_n4_t1.json")
    n, t = c["n"], c["t"]
    N = t + 1
    a, bb, r, pk = H(c["a"])[:32 * N], H(c["b"])[:32 * N], H(c["enc_r"])[:64 * n], H(c["member_pk"])
    sks = H(c["member_sk"])[:32]
    b = dkg_amd.Backend(0)
    try:
        outs = [ctypes.create_string_buffer(b"\x5a" * w, w) for w in (32 * N, 32 * N, 64 * n, 64 * n, 32 * n, 32 * n, 64)]
        # without dkg_env_init: what party_round2_seats answers
        with pytest.raises(DkgError) as e2:
            b.party_round2_seats(1, n, t, [0], [0], H(c["E"]), H(c["e1"])[:64 * n], H(c["ct"])[:64 * n], sks)
        with pytest.raises(DkgError) as e1:
            b.party_round1_seats(1, n, t, [0], [0], a, bb, r, pk)
        assert e1.value.code == e2.value.code == _lib.DKG_E_ARG and "dkg_env_init" in str(e1.value)
        b.env_init(t, n, CK)
        # (t, n) that dkg_env_check refuses
        with pytest.raises(DkgError) as e2:
            b.party_round2_seats(1, n, 2, [0], [0], H(c["E"]), H(c["e1"])[:64 * n], H(c["ct"])[:64 * n], sks)
        with pytest.raises(DkgError) as e1:
            b.party_round1_seats(1, n, 2, [0], [0], a + a, bb + bb, r, pk)
        assert e1.value.code == e2.value.code == _lib.DKG_E_ARG
        # S == 0: DKG_OK, nothing touched, nothing required
        assert raw_call(b, 1, n, t, [], [], None, None, None, None, *outs) == _lib.DKG_OK
        assert all(o.raw == b"\x5a" * len(o.raw) for o in outs)
        # indices out of range, B == 0
        for cer, js, B in (([1], [0], 1), ([0], [n], 1), ([0], [0], 0)):
            with pytest.raises(DkgError) as e:
                b.party_round1_seats(B, n, t, cer, js, a, bb, r, pk)
            assert e.value.code == _lib.DKG_E_ARG
        # a NULL required pointer: each of a, b, r, pk, E, A, e1, ct
        args = [a, bb, r, pk] + outs[:4]
        for k in range(8):
            assert raw_call(b, 1, n, t, [0], [0], *(args[:k] + [None] + args[k + 1:])) == _lib.DKG_E_ARG, k
        # the optional outputs may be NULL
        assert raw_call(b, 1, n, t, [0], [0], *args) == _lib.DKG_OK
        assert outs[0].raw == H(c["E"])[:32 * N] and outs[2].raw == H(c["e1"])[:64 * n]
        # an undecodable key in a named ceremony: DKG_E_DECODE naming ceremony and recipient; in an unnamed
        # one it is never read
        pk3 = pk + pk[:64] + BAD + pk[96:] + pk
        for mode in (1, 2):
            b.set_seat_deal(mode)
            with pytest.raises(DkgError) as e:
                b.party_round1_seats(3, n, t, [2, 1], [0, 0], a + a, bb + bb, r + r, pk3)
            assert e.value.code == _lib.DKG_E_DECODE
            assert "ceremony 1" in str(e.value) and "recipient 2" in str(e.value)
            ok = b.party_round1_seats(3, n, t, [2, 0], [0, 0], a + a, bb + bb, r + r, pk3)
            assert ok["e1"] == H(c["e1"])[:64 * n] * 2 and ok["ct"] == H(c["ct"])[:64 * n] * 2
        with pytest.raises(DkgError):
            b.set_seat_deal(3)
    finally:
        b.close()


def test_phase_times(be, golden):
    c = golden("full_n4_t1.json")
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    names = ("commit", "deal_e1", "deal_mul", "deal_encode", "deal_sym")
    args = (1, n, t, [0], [1], H(c["a"])[:32 * (t + 1)], H(c["b"])[:32 * (t + 1)], H(c["enc_r"])[:64 * n],
            H(c["member_pk"]))
    be.party_round1_seats(*args)
    assert all(be.phase_times("seats")[k] == -1 for k in names)  # recorded on one stream only
    try:
        be.set_streams(1)
        be.party_round1_seats(*args)
        ph = be.phase_times("seats")
        assert all(ph[k] > 0 for k in names), ph
    finally:
        be.set_streams(2)
