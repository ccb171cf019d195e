"""Hosted seats of large committees: the chunked evaluation (k_seat_chunks, k_seat_fold) behind
set_seat_eval.  Every case runs both kernel copies (set_field_mode 1, 2) and is compared with the serial
walk (mode 1) byte for byte, with the libsodium fixtures' dec2 / dec4, and, where there is no fixture,
with the per-ceremony calls and the CPU oracle's rows.  The chunks named are the smallest shapes at which
the new code can go wrong: odd chunk counts, a short last chunk, one stage, several x in one launch,
x = 1 (empty fold chain), x = n, three tiles, and a fold multiplier that is reduced mod l."""
import random

import pytest

import dkg_amd
from dkg_amd import ACCEPT, MISSING, REJECT, SELF, SKIPPED, DkgError
from tests import ristretto_ref as R
from tests.test_gpu import CK, H, dec_str
from tests.test_gpu_receivers import columns
from tests.test_gpu_seats import Stack, both, party_inputs, seat_cols, stack10  # noqa: F401 (stack10: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.set_seat_eval(0, 0)
    b.close()


def routes(be, call, N, chunks):
    """call() under mode 1 and under mode 2 with every chunk, both kernel copies each: one result, and the
    route each call reports.  chunk 0 under mode 2 is the rule's choice (either route)."""
    try:
        be.set_seat_eval(1)
        base = both(be, call)
        assert be.last_seat_eval() == (1, N)
        for L in chunks:
            be.set_seat_eval(2, L)
            assert both(be, call) == base, L
            mode, ran = be.last_seat_eval()
            if L == 0:
                assert (mode, ran) == (1, N) or (mode == 2 and ran < N)
            else:
                assert (mode, ran) == ((2, L) if L < N else (1, N)), L
    finally:
        be.set_seat_eval(0, 0)
    return base


def run_stack(be, st, seats, chunks, E=None, A=None):
    """Stack.run's four outputs, each through routes()."""
    n, t, B, N = st.n, st.t, st.B, st.t + 1
    cer, js = [c for c, _ in seats], [j for _, j in seats]
    E, A = E or st.E, A or st.A
    sc, spc = seat_cols(st.s, n, seats), seat_cols(st.sp, n, seats)
    d2 = routes(be, lambda: be.verify_seats(B, n, t, 2, cer, js, E, sc, spc), N, chunks)
    d4 = routes(be, lambda: be.verify_seats(B, n, t, 4, cer, js, A, sc, None, st.qual), N, chunks)
    d4u = routes(be, lambda: be.verify_seats(B, n, t, 4, cer, js, A, sc), N, chunks)
    ev = routes(be, lambda: be.commitment_eval_seats(B, n, t, cer, js, E), N, chunks)
    return d2, d4, d4u, ev


# ---------------------------------------------------------------- fixture shapes
@pytest.mark.parametrize("name, xs, chunks", [
    # N = 5.  L = 1: G = 5, 3 stages, an odd count at two of them, no step in the chunk kernel; L = 2: G = 3, a
    # last chunk of one coefficient; L = 3, 4: G = 2, a short last chunk; L = 5, 9: the serial walk
    ("ceremony_n10_t4.json", (10, 1, 5, 5, 5, 5, 5, 2), (1, 2, 3, 4, 5, 9)),
    ("ceremony_n3_t1.json", (3, 1, 2, 3), (1,)),            # N = 2: one stage, nothing else
    ("ceremony_n2_t0.json", (1, 2, 2), (1, 2)),             # N = 1: any chunk is the serial walk
    # W = 16: a full wave, a partly filled one, several x in one launch (per-wave digit slots)
    ("ceremony_n16_t7.json", (3, 3, 3, 3, 3, 7, 7, 1, 16), (1, 2, 3)),
    ("ceremony_n64_t31.json", (1, 43, 64), (1, 8, 0)),      # L = 1: 5 stages
])
def test_fixture_shapes(be, golden, name, xs, chunks):
    st = Stack([golden(name)])
    be.env_init(st.t, st.n, CK)
    seats = [(0, x - 1) for x in xs]
    d2, d4, d4u, ev = run_stack(be, st, seats, chunks)
    assert dec_str(d2) == st.expect(2, seats)
    assert dec_str(d4) == st.expect(4, seats)
    assert ev[1] == b"\x01" * (len(seats) * st.n)
    if st.n == 10:  # P of three (seat, dealer) pairs against the Python reference
        N = st.t + 1
        for p, i in ((0, 0), (1, 9), (3, 4)):
            x = xs[p]
            pts = [R.decode(st.E[32 * (i * N + k):32 * (i * N + k) + 32]) for k in range(N)]
            want = R.encode(R.msm([pow(x, k, R.L) for k in range(N)], pts))
            assert ev[0][32 * (p * st.n + i):32 * (p * st.n + i) + 32] == want


def test_three_tiles_reduced_multiplier(be):
    """n = 130, t = 64: three 64-dealer tiles per seat, the last with 2 live lanes; with L = 1 and x = 130
    the last fold multiplier x^64 exceeds l and is reduced.  Tampered dealers 0..4 as the scale tests inject
    them, expectations from the oracle's rows."""
    from tests.test_gpu_scale import _expected_rows, _inject
    n, t = 130, 64
    N = t + 1
    assert 130 ** 64 > R.L > 130 ** 32
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x5a" * 32, 3, 0, n, t)
    E, A, s, sp = (bytearray(v) for v in be.share_gen(a, b, n, n, t))
    _inject(random.Random(130), n, t, E, A, s, sp)
    exp = _expected_rows(n, t, h, E, A, s, sp)
    E, A, s, sp = bytes(E), bytes(A), bytes(s), bytes(sp)
    js = [129, 3, 64, 3, 0, 127]

    def oracle(rnd):
        out = bytearray()
        for j in js:
            out += bytes(exp[(i, rnd)][j] if i < 5 else (SELF if i == j else ACCEPT) for i in range(n))
        return bytes(out)

    sc, spc = columns(s, n, js), columns(sp, n, js)
    cer = [0] * len(js)
    chunks = (1, 16, 0)
    d2 = routes(be, lambda: be.verify_seats(1, n, t, 2, cer, js, E, sc, spc), N, chunks)
    d4 = routes(be, lambda: be.verify_seats(1, n, t, 4, cer, js, A, sc), N, chunks)
    assert d2 == oracle(2) and d4 == oracle(4)
    assert MISSING in d2 and REJECT in d2 and REJECT in d4
    assert d2 == be.verify_receivers(n, t, 2, js, E, sc, spc)
    assert d4 == be.verify_receivers(n, t, 4, js, A, sc)
    ev = routes(be, lambda: be.commitment_eval_seats(1, n, t, cer, js, E), N, chunks)
    assert ev == tuple(b"".join(be.commitment_eval(n, t, [j], E)[k] for j in js) for k in (0, 1))


# ---------------------------------------------------------------- the golden stack and the seat lists
def test_golden_stack(be, stack10):
    st = stack10
    be.env_init(st.t, st.n, CK)
    seats = [(c, j) for c in range(st.B) for j in range(st.n)]
    random.Random(1).shuffle(seats)
    d2, d4, d4u, ev = run_stack(be, st, seats, (2,))
    assert dec_str(d2) == st.expect(2, seats)
    assert dec_str(d4) == st.expect(4, seats)
    assert SKIPPED in d4 and REJECT in d4 and REJECT in d2 and SELF in d2
    be.set_seat_eval(0, 0)  # the automatic choice computes the same
    assert st.run(be, seats) == (d2, d4, d4u, ev)


def test_seat_lists(be, stack10):
    st = Stack(stack10.f[:4])
    be.env_init(st.t, st.n, CK)
    n = st.n
    seats = [(2, 5), (0, 1), (2, 5), (3, 9), (0, 7), (3, 0), (2, 5)]  # a repeated seat; ceremony 1 unnamed
    base = run_stack(be, st, seats, (2,))
    assert dec_str(base[0]) == st.expect(2, seats) and dec_str(base[1]) == st.expect(4, seats)
    for a, b_ in ((0, 2), (0, 6)):
        for k in (0, 1, 2):
            assert base[k][n * a:n * (a + 1)] == base[k][n * b_:n * (b_ + 1)]
    ff = b"\xff" * st.rowlen  # a ceremony no seat names is never interpreted
    E = st.E[:st.rowlen] + ff + st.E[2 * st.rowlen:]
    A = st.A[:st.rowlen] + ff + st.A[2 * st.rowlen:]
    assert run_stack(be, st, seats, (2,), E, A) == base
    sc, spc = seat_cols(st.s, n, [(1, 4)]), seat_cols(st.sp, n, [(1, 4)])
    d2 = routes(be, lambda: be.verify_seats(st.B, n, st.t, 2, [1], [4], E, sc, spc), st.t + 1, (2,))
    assert d2 == bytes(SELF if i == 4 else MISSING for i in range(n))


def test_undecodable_row(be, stack10, golden):
    """One non-canonical coefficient of dealer 6 in ceremony 2: MISSING / REJECT, ok = 0 and zero P there."""
    st = Stack(stack10.f[:3])
    n, t, N = st.n, st.t, st.t + 1
    be.env_init(t, n, CK)
    seats = [(c, j) for j in range(n) for c in (2, 0)]
    bad = H(golden("kat_group.json")["invalid_encodings"][1])
    k = 2 * st.rowlen + 32 * (N * 6 + 3)
    E = st.E[:k] + bad + st.E[k + 32:]
    A = st.A[:k] + bad + st.A[k + 32:]
    d2, d4, d4u, (P, ok) = run_stack(be, st, seats, (2,), E, A)
    for p, (c, j) in enumerate(seats):
        e = p * n + 6
        if c == 2:
            assert d2[e] == (SELF if j == 6 else MISSING)
            assert d4u[e] == (SELF if j == 6 else REJECT)
            assert d4[e] == (SELF if j == 6 else (REJECT if st.qual[n * c + 6] else SKIPPED))
            assert ok[e] == 0 and P[32 * e:32 * e + 32] == bytes(32)
        else:
            assert ok[e] == 1 and P[32 * e:32 * e + 32] != bytes(32)


def test_identity_rows(be, golden):
    """A dealer whose every coefficient is the identity (32 zero bytes), and one whose top chunk alone is:
    the complete additions need no special case, the chunked routes equal the serial walk."""
    st = Stack([golden("ceremony_n10_t4.json")])
    n, t, N = st.n, st.t, st.t + 1
    E = bytearray(st.E)
    E[32 * N * 2:32 * N * 3] = bytes(32 * N)            # dealer 2: all identity
    E[32 * (N * 5 + N - 1):32 * (N * 5 + N)] = bytes(32)  # dealer 5: the top coefficient (the top chunk at L = 1, 2)
    E[32 * (N * 7 + 2):32 * (N * 7 + 4)] = bytes(64)      # dealer 7: the middle chunk at L = 2
    E = bytes(E)
    js = [9, 0, 4, 4, 1]
    P, ok = routes(be, lambda: be.commitment_eval_seats(1, n, t, [0] * len(js), js, E), N, (1, 2, 3))
    assert ok == b"\x01" * (len(js) * n)
    for p in range(len(js)):
        assert P[32 * (p * n + 2):32 * (p * n + 3)] == bytes(32)  # the identity's encoding
    assert (P, ok) == tuple(b"".join(be.commitment_eval(n, t, [j], E)[k] for j in js) for k in (0, 1))


def test_party_round2_seats(be, golden):
    fx = [golden("full_faults_n10_t4.json")]
    st = Stack(fx)
    n, t = st.n, st.t
    be.env_init(t, n, CK)
    seats = [(0, j) for j in range(n)]
    random.Random(2).shuffle(seats)
    e1, ct, sk, w = party_inputs(fx, seats, random.Random(n))
    cer, js = [c for c, _ in seats], [j for _, j in seats]
    r = routes(be, lambda: be.party_round2_seats(1, n, t, cer, js, st.E, e1, ct, sk, w), t + 1, (2,))
    assert REJECT in r["dec"] and any(r["proofs"][192 * e:192 * e + 192] != bytes(192) for e in range(n * n))
    assert dec_str(r["dec"]) == "".join(fx[0]["dec2"][i * n + j] for _, j in seats for i in range(n))


# ---------------------------------------------------------------- the switch
def test_switch_and_phases(golden):
    c = golden("ceremony_n10_t4.json")
    st = Stack([c])
    n, t, N = st.n, st.t, st.t + 1
    sc, spc = seat_cols(st.s, n, [(0, 1)]), seat_cols(st.sp, n, [(0, 1)])
    b = dkg_amd.Backend(0)
    try:
        assert b.last_seat_eval() == (0, 0)
        for mode, chunk in ((0, 3), (3, 0), (-1, 0), (2, -1), (1, 2)):
            with pytest.raises(DkgError) as e:
                b.set_seat_eval(mode, chunk)
            assert e.value.code == -1
        b.env_init(t, n, CK)
        b.set_streams(1)
        call = lambda: b.verify_seats(1, n, t, 2, [0], [1], st.E, sc, spc)  # noqa: E731
        b.set_seat_eval(2, 2)
        d = call()
        assert dec_str(d) == st.expect(2, [(0, 1)]) and b.last_seat_eval() == (2, 2)
        ph = b.phase_times("seats")
        assert 0 < ph["fold"] < ph["eval"] and ph["decode"] >= 0 and ph["check"] > 0
        b.set_seat_eval(1)
        assert call() == d and b.last_seat_eval() == (1, N)
        ph = b.phase_times("seats")
        assert ph["fold"] == -1 and ph["eval"] > 0
        b.set_seat_eval(2, 2)
        b.set_streams(2)  # phases are recorded on one stream only
        assert call() == d and b.phase_times("seats")["fold"] == -1
        # a forced shape above 1 GiB of scratch: 42,000 seats of one x are 10,500 waves, G = 5
        S = 42000
        b.set_seat_eval(2, 1)
        with pytest.raises(DkgError) as e:
            b.commitment_eval_seats(1, n, t, [0] * S, [0] * S, st.E)
        assert e.value.code == -1 and str(2 * 160 * 5 * 64 * 10500) in str(e.value)
        b.set_seat_eval(0, 0)  # the rule never selects such a shape
        P, ok = b.commitment_eval_seats(1, n, t, [0] * S, [0] * S, st.E)
        assert P[:32 * n] == b.commitment_eval(n, t, [0], st.E)[0] and P == P[:32 * n] * S
    finally:
        b.close()
