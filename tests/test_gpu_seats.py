"""Hosted seats: one operator's share checks across many ceremonies (k_seat_horner and its runtime):
dkg_commitment_eval_seats, dkg_verify_seats and dkg_party_round2_seats against the fixtures, the CPU
oracle and the per-ceremony calls (commitment_eval, verify_receivers, party_round2), bit for bit, under
both kernel copies (set_field_mode 1 and 2)."""
import ctypes
import glob
import json
import os
import random

import pytest

import dkg_amd
from dkg_amd import ACCEPT, MISSING, REJECT, SELF, SKIPPED, DkgError
from tests.test_gpu import CK, H, dec_str
from tests.test_gpu_receivers import INVALID, columns, party_column

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


def both(be, call):
    """call() under the product-scanning and the column-sum copy of the kernel: identical outputs."""
    try:
        be.set_field_mode(1)
        r1 = call()
        be.set_field_mode(2)
        r2 = call()
    finally:
        be.set_field_mode(0)
    assert r1 == r2
    assert call() == r1  # the default copy
    return r1


def seat_cols(mats, n, seats):
    """[S][n][32]: column j of ceremony c's [n][n][32] share matrix, per seat (c, j)."""
    return b"".join(mats[c][32 * (i * n + j):32 * (i * n + j) + 32] for c, j in seats for i in range(n))


def seat_dec(decs, n, seats):
    return "".join(decs[c][i * n + j] for c, j in seats for i in range(n))


class Stack:
    """B fixtures of one (n, t) as one batch: row c * n + i is dealer i of fixture c."""

    def __init__(self, fixtures):
        self.f = fixtures
        self.B, self.n, self.t = len(fixtures), fixtures[0]["n"], fixtures[0]["t"]
        assert all((c["n"], c["t"]) == (self.n, self.t) for c in fixtures)
        self.E = b"".join(H(c["E"]) for c in fixtures)
        self.A = b"".join(H(c["A"]) for c in fixtures)
        self.s = [H(c["s"]) for c in fixtures]
        self.sp = [H(c["s_prime"]) for c in fixtures]
        self.qual = b"".join(bytes(1 if q else 0 for q in c["qualified"]) for c in fixtures)
        self.rowlen = 32 * self.n * (self.t + 1)  # bytes of one ceremony's commitments

    def ceremony(self, buf, c):
        return buf[self.rowlen * c:self.rowlen * (c + 1)]

    def expect(self, rnd, seats):
        return seat_dec([c["dec2" if rnd == 2 else "dec4"] for c in self.f], self.n, seats)

    def run(self, be, seats, E=None, A=None):
        """(dec2, dec4, dec4 without the qualified sets, (P, ok) of E) of the seats calls, both copies."""
        n, t, B = self.n, self.t, self.B
        cer, js = [c for c, _ in seats], [j for _, j in seats]
        E, A = E or self.E, A or self.A
        sc, spc = seat_cols(self.s, n, seats), seat_cols(self.sp, n, seats)
        d2 = both(be, lambda: be.verify_seats(B, n, t, 2, cer, js, E, sc, spc))
        d4 = both(be, lambda: be.verify_seats(B, n, t, 4, cer, js, A, sc, None, self.qual))
        d4u = both(be, lambda: be.verify_seats(B, n, t, 4, cer, js, A, sc))
        ev = both(be, lambda: be.commitment_eval_seats(B, n, t, cer, js, E))
        return d2, d4, d4u, ev

    def per_ceremony(self, be, seats, E=None, A=None):
        """The same through verify_receivers / commitment_eval, one call per seat."""
        n, t = self.n, self.t
        E, A = E or self.E, A or self.A
        d2 = d4 = d4u = P = ok = b""
        for c, j in seats:
            Ec, Ac = self.ceremony(E, c), self.ceremony(A, c)
            sc, spc = columns(self.s[c], n, [j]), columns(self.sp[c], n, [j])
            d2 += be.verify_receivers(n, t, 2, [j], Ec, sc, spc)
            d4 += be.verify_receivers(n, t, 4, [j], Ac, sc, None, self.qual[n * c:n * (c + 1)])
            d4u += be.verify_receivers(n, t, 4, [j], Ac, sc)
            p, o = be.commitment_eval(n, t, [j], Ec)
            P, ok = P + p, ok + o
        return d2, d4, d4u, (P, ok)


@pytest.fixture(scope="module")
def stack10(golden):
    """The ten n = 10, t = 4 fixtures that carry dec2, one commitment key."""
    names = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*_n10_t4.json"))):
        with open(path) as f:
            if "dec2" in json.load(f):
                names.append(os.path.basename(path))
    assert len(names) == 10
    fx = [golden(nm) for nm in names]
    assert len({c["h"] for c in fx}) == 1
    return Stack(fx)


# ---------------------------------------------------------------- the golden stack: all 100 seats, shuffled
def test_golden_stack(be, stack10):
    st = stack10
    be.env_init(st.t, st.n, CK)
    seats = [(c, j) for c in range(st.B) for j in range(st.n)]
    random.Random(1).shuffle(seats)
    d2, d4, d4u, ev = st.run(be, seats)
    assert dec_str(d2) == st.expect(2, seats)
    assert dec_str(d4) == st.expect(4, seats)
    assert SKIPPED in d4 and REJECT in d4 and REJECT in d2 and SELF in d2  # the fixtures exercise them
    assert (d2, d4, d4u, ev) == st.per_ceremony(be, seats)


# ---------------------------------------------------------------- shapes where the kernel can go wrong
@pytest.mark.parametrize("name, xs", [
    ("ceremony_n16_t7.json", (3, 3, 3, 3, 3, 7, 7, 1, 16)),  # W = 16: a full wave, a partly filled one, x = 1, x = n
    ("ceremony_n10_t4.json", (10, 1, 5, 5, 5, 5, 5, 2)),     # W = 16 with dead lanes inside every slot
    ("ceremony_n64_t31.json", (1, 43, 64)),                  # W = 64: one seat per wave
    ("ceremony_n2_t0.json", (1, 2, 2)),                      # N = 1: no step
    ("ceremony_n3_t1.json", (3, 1, 2, 3)),                   # N = 2
])
def test_fixture_shapes(be, golden, name, xs):
    st = Stack([golden(name)])
    be.env_init(st.t, st.n, CK)
    seats = [(0, x - 1) for x in xs]
    d2, d4, d4u, ev = st.run(be, seats)
    assert dec_str(d2) == st.expect(2, seats)
    assert dec_str(d4) == st.expect(4, seats)
    assert (d2, d4, d4u, ev) == st.per_ceremony(be, seats)
    assert ev[1] == b"\x01" * (len(seats) * st.n)


def test_two_tiles_ragged(be):
    """n = 70, t = 34: two 64-dealer tiles per seat, the second ragged; tampered dealers 0..4 as the scale
    tests inject them, expectations from the oracle's rows."""
    from tests.test_gpu_scale import _expected_rows, _inject
    n, t = 70, 34
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x5a" * 32, 3, 0, n, t)
    E, A, s, sp = (bytearray(v) for v in be.share_gen(a, b, n, n, t))
    _inject(random.Random(70), n, t, E, A, s, sp)
    exp = _expected_rows(n, t, h, E, A, s, sp)
    E, A, s, sp = bytes(E), bytes(A), bytes(s), bytes(sp)
    js = [69, 3, 34, 3, 0, 66, 7]

    def oracle(rnd):
        out = bytearray()
        for j in js:
            out += bytes(exp[(i, rnd)][j] if i < 5 else (SELF if i == j else ACCEPT) for i in range(n))
        return bytes(out)

    sc, spc = columns(s, n, js), columns(sp, n, js)
    d2 = both(be, lambda: be.verify_seats(1, n, t, 2, [0] * len(js), js, E, sc, spc))
    d4 = both(be, lambda: be.verify_seats(1, n, t, 4, [0] * len(js), js, A, sc))
    assert d2 == oracle(2) and d4 == oracle(4)
    assert MISSING in d2 and REJECT in d2 and REJECT in d4
    assert d2 == be.verify_receivers(n, t, 2, js, E, sc, spc)
    assert d4 == be.verify_receivers(n, t, 4, js, A, sc)
    assert both(be, lambda: be.commitment_eval_seats(1, n, t, [0] * len(js), js, E)) == tuple(
        b"".join(be.commitment_eval(n, t, [j], E)[k] for j in js) for k in (0, 1))


# ---------------------------------------------------------------- seat lists
def test_seat_lists(be, stack10):
    st = Stack(stack10.f[:4])
    be.env_init(st.t, st.n, CK)
    # the same seat twice, two seats in one ceremony, ceremony 1 named by no seat
    seats = [(2, 5), (0, 1), (2, 5), (3, 9), (0, 7), (3, 0), (2, 5)]
    base = st.run(be, seats)
    assert dec_str(base[0]) == st.expect(2, seats) and dec_str(base[1]) == st.expect(4, seats)
    assert base == st.per_ceremony(be, seats)
    n = st.n
    for a, b_ in ((0, 2), (0, 6)):  # the repeated seat reads the same in every place
        for k in (0, 1, 2):
            assert base[k][n * a:n * (a + 1)] == base[k][n * b_:n * (b_ + 1)]
    # a ceremony no seat names is never interpreted: 0xFF rows change nothing
    ff = b"\xff" * st.rowlen
    E = st.E[:st.rowlen] + ff + st.E[2 * st.rowlen:]
    A = st.A[:st.rowlen] + ff + st.A[2 * st.rowlen:]
    assert st.run(be, seats, E, A) == base
    # ... and it does not decode where a seat does name it
    d2 = be.verify_seats(st.B, n, st.t, 2, [1], [4], E, seat_cols(st.s, n, [(1, 4)]), seat_cols(st.sp, n, [(1, 4)]))
    assert d2 == bytes(SELF if i == 4 else MISSING for i in range(n))


def test_undecodable_row(be, stack10, golden):
    """One non-canonical coefficient of dealer 6 in ceremony 2: MISSING (round 2) / REJECT (round 4) for
    that ceremony's seats only, ok = 0 and P zero there."""
    st = Stack(stack10.f[:3])
    n, t, N = st.n, st.t, st.t + 1
    be.env_init(t, n, CK)
    seats = [(c, j) for j in range(n) for c in (2, 0)]
    base = st.run(be, seats)
    bad = H(golden("kat_group.json")["invalid_encodings"][1])
    k = 2 * st.rowlen + 32 * (N * 6 + 3)
    E = st.E[:k] + bad + st.E[k + 32:]
    A = st.A[:k] + bad + st.A[k + 32:]
    d2, d4, d4u, (P, ok) = st.run(be, seats, E, A)
    assert (d2, d4, d4u, (P, ok)) == st.per_ceremony(be, seats, E, A)
    for p, (c, j) in enumerate(seats):
        for i in range(n):
            e = p * n + i
            if c == 2 and i == 6:
                assert d2[e] == (SELF if j == 6 else MISSING)
                assert d4u[e] == (SELF if j == 6 else REJECT)
                assert d4[e] == (SELF if j == 6 else (REJECT if st.qual[n * c + i] else SKIPPED))
                assert ok[e] == 0 and P[32 * e:32 * e + 32] == bytes(32)
            else:
                assert (d2[e], d4[e], d4u[e], ok[e]) == (base[0][e], base[1][e], base[2][e], 1)
                assert P[32 * e:32 * e + 32] == base[3][0][32 * e:32 * e + 32]


# ---------------------------------------------------------------- party_round2_seats
def party_inputs(fixtures, seats, rng):
    n = fixtures[0]["n"]
    e1, ct, sk = b"", b"", b""
    for c, j in seats:
        a, b_ = party_column(fixtures[c], n, j)
        e1, ct = e1 + a, ct + b_
        sk += H(fixtures[c]["member_sk"])[32 * j:32 * j + 32]
    w = bytearray(rng.randrange(256) for _ in range(64 * n * len(seats)))
    for k in range(31, len(w), 32):
        w[k] &= 0x0f  # canonical nonces
    return e1, ct, sk, bytes(w)


def party_compare(be, fixtures, seats, e1, ct, sk, w):
    """party_round2_seats against party_round2 per seat, every output byte for byte."""
    st = Stack(fixtures)
    n, t = st.n, st.t
    cer, js = [c for c, _ in seats], [j for _, j in seats]
    r = both(be, lambda: be.party_round2_seats(st.B, n, t, cer, js, st.E, e1, ct, sk, w))
    for p, (c, j) in enumerate(seats):
        one = be.party_round2(n, t, j, st.ceremony(st.E, c), e1[64 * n * p:64 * n * (p + 1)],
                              ct[64 * n * p:64 * n * (p + 1)], sk[32 * p:32 * p + 32], w[64 * n * p:64 * n * (p + 1)])
        assert r["s"][32 * n * p:32 * n * (p + 1)] == one["s"]
        assert r["s_prime"][32 * n * p:32 * n * (p + 1)] == one["s_prime"]
        assert r["dec"][n * p:n * (p + 1)] == one["dec"]
        assert (r["complaints"][p], r["r2_error"][p]) == (one["complaints"], one["r2_error"])
        assert r["proofs"][192 * n * p:192 * n * (p + 1)] == one["proofs"]
    return r


@pytest.mark.parametrize("names", [["full_n10_t4.json"], ["full_faults_n10_t4.json"], ["full_n8_t3.json"],
                                   ["full_n4_t1.json"], ["full_faults_n10_t4.json", "full_n10_t4.json"]])
def test_party_round2_seats(be, golden, names):
    fx = [golden(nm) for nm in names]
    n, t = fx[0]["n"], fx[0]["t"]
    be.env_init(t, n, CK)
    seats = [(c, j) for c in range(len(fx)) for j in range(n)]
    random.Random(len(names)).shuffle(seats)
    e1, ct, sk, w = party_inputs(fx, seats, random.Random(n))
    r = party_compare(be, fx, seats, e1, ct, sk, w)
    assert dec_str(r["dec"]) == seat_dec([c["dec2"] for c in fx], n, seats)
    for p, (c, j) in enumerate(seats):
        assert r["s"][32 * n * p:32 * n * (p + 1)] == columns(H(fx[c]["s"]), n, [j])
        assert r["complaints"][p] == fx[c]["complaints2"][j] and bool(r["r2_error"][p]) == fx[c]["r2_error"][j]
        for i in range(n):
            proven = r["proofs"][192 * (p * n + i):192 * (p * n + i + 1)] != bytes(192)
            assert proven == (r["dec"][p * n + i] == REJECT)
    if "faults" in names[0]:
        assert REJECT in r["dec"]
    nop = be.party_round2_seats(len(fx), n, t, [c for c, _ in seats], [j for _, j in seats], b"".join(H(c["E"]) for c in fx),
                                e1, ct, sk)
    assert nop["proofs"] is None and nop["dec"] == r["dec"]


def test_party_round2_seats_undecodable_e1(be, golden):
    fx = [golden("full_faults_n10_t4.json")]
    n, t = fx[0]["n"], fx[0]["t"]
    be.env_init(t, n, CK)
    seats = [(0, j) for j in (2, 5, 2)]
    e1, ct, sk, w = party_inputs(fx, seats, random.Random(3))
    base = party_compare(be, fx, seats, e1, ct, sk, w)
    i = 7
    k = 64 * (n * 2 + i) + 32  # the share's e1 of dealer 7, third seat only
    bad = e1[:k] + INVALID + e1[k + 32:]
    r = party_compare(be, fx, seats, bad, ct, sk, w)
    e = 2 * n + i
    assert r["dec"][e] == MISSING and r["proofs"][192 * e:192 * e + 192] == bytes(192)
    assert r["complaints"][2] == base["complaints"][2] - (1 if base["dec"][e] == REJECT else 0)
    assert bytes(v for q, v in enumerate(r["dec"]) if q != e) == bytes(v for q, v in enumerate(base["dec"]) if q != e)
    assert r["dec"][i] == base["dec"][i]  # the same seat listed first keeps its own pair


# ---------------------------------------------------------------- arguments and phases
def test_arguments_and_phases(golden):
    c = golden("ceremony_n10_t4.json")
    st = Stack([c, c])
    n, t = st.n, st.t
    sc, spc = seat_cols(st.s, n, [(1, 1)]), seat_cols(st.sp, n, [(1, 1)])
    b = dkg_amd.Backend(0)
    try:
        with pytest.raises(DkgError) as e:  # round 2 without dkg_env_init
            b.verify_seats(2, n, t, 2, [1], [1], st.E, sc, spc)
        assert e.value.code == -1 and "dkg_env_init" in str(e.value)
        P, ok = b.commitment_eval_seats(2, n, t, [1], [1], st.E)  # needs none
        assert (P, ok) == b.commitment_eval(n, t, [1], H(c["E"]))
        # S == 0 touches nothing
        L = dkg_amd.lib()
        out = ctypes.create_string_buffer(b"\x07" * 32, 32)
        assert L.dkg_verify_seats(b._ctx, 2, n, t, 2, 0, None, None, None, None, None, None, out) == 0
        assert L.dkg_commitment_eval_seats(b._ctx, 2, n, t, 0, None, None, None, out, out) == 0
        assert L.dkg_party_round2_seats(b._ctx, 2, n, t, 0, None, None, None, None, None, None, None, out, out, out,
                                        None, None, None) == 0
        assert out.raw == b"\x07" * 32
        assert b.verify_seats(2, n, t, 2, [], [], st.E, b"", b"") == b""
        b.env_init(t, n, CK)
        for rnd, cer, js, spc_ in ((3, [1], [1], spc), (2, [2], [1], spc), (2, [1], [n], spc), (2, [1], [1], None)):
            with pytest.raises(DkgError) as e:
                b.verify_seats(2, n, t, rnd, cer, js, st.E, sc, spc_)
            assert e.value.code == -1
        with pytest.raises(DkgError):
            b.commitment_eval_seats(2, n, t, [0, 2], [1, 1], st.E)
        with pytest.raises(DkgError):
            b.party_round2_seats(2, n, t, [0], [n], st.E, bytes(64 * n), bytes(64 * n), bytes(32))
        assert dec_str(b.verify_seats(2, n, t, 2, [1], [1], st.E, sc, spc)) == st.expect(2, [(1, 1)])
        assert set(b.phase_times("seats").values()) == {-1}  # phases are recorded on one stream only
        b.set_streams(1)
        assert dec_str(b.verify_seats(2, n, t, 2, [1], [1], st.E, sc, spc)) == st.expect(2, [(1, 1)])
        ph = b.phase_times("seats")
        assert ph["decrypt"] == -1 and ph["prove"] == -1
        assert ph["decode"] >= 0 and ph["eval"] > 0 and ph["check"] > 0
    finally:
        b.close()
