"""Complaint evaluation mode 4: every (row, index) item of dkg_complaints_verify / dkg_complaints3_verify
and of the proven ceremony driver goes to the wave evaluator (receivers.hip k_pair_eval) in the per-pair
Horner walk's place.  Verdicts, qualified and reconstruct must equal modes 1 and 2 and the CPU oracle
(tests/oracle_lib.py complaint1_verify / complaint3_verify), bit for bit; every complaint is compared."""
import random

import pytest

import dkg_amd
from dkg_amd import COMPLAINT_IGNORED, COMPLAINT_NO_PHASE3, DkgError
from tests import oracle_lib as O
from tests.test_gpu_ceremony_proven import honest_complaints, lists, no_times
from tests.test_gpu_complaints import enc_of, fixture_inputs
from tests.test_oracle import VERDICT

pytestmark = pytest.mark.gpu

H = bytes.fromhex
L = 2**252 + 27742317777372353535851937790883648493
CK = b"Example of a shared string."
MODES = (1, 2, 4)


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.set_complaint_eval(0)
    b.close()


def sc(v):
    return (v % L).to_bytes(32, "little")


def row(C, N, i):
    return C[32 * N * i:32 * N * (i + 1)]


def pair(s, sp, n, i, q):
    k = 32 * (i * n + q)
    return s[k:k + 32], sp[k:k + 32]


def bad_coefficient(C, N, i, k, point):
    C = bytearray(C)
    C[32 * (N * i + k):32 * (N * i + k + 1)] = point
    return bytes(C)


def test_mode_values(be):
    for mode in (0, 1, 2, 4):
        be.set_complaint_eval(mode)
    for mode in (3, 5, 6, -1):
        with pytest.raises(DkgError) as e:
            be.set_complaint_eval(mode)
        assert e.value.code == -1
    be.set_complaint_eval(0)


# ---------------------------------------------------------------- round 2, n = 10, t = 4
def test_round2_fixture_and_forgeries(be, golden):
    """The fixture's five complaints over full_faults_n10_t4.json (verdicts 0, 0, 0, 2, 1) and, in the same
    call: a forged complaint of every verdict code (an honest proof against an honest dealer: 2; a tampered
    response: 1; a share key that does not decode: -1; a true one: 0), an accused row that does not decode
    (-1), an accused without a phase-1 broadcast (IGNORED)."""
    c, full, _, enc, proof, _ = fixture_inputs(golden)
    n, t = full["n"], full["t"]
    N = t + 1
    h = be.env_init(t, n, CK)
    assert h.hex() == full["h"]
    E, pk, sk = H(full["E"]), H(full["member_pk"]), H(full["member_sk"])
    e1, ct = H(full["e1"]), H(full["ct"])
    rng = random.Random(404)
    comp = [(x["accuser"], x["accused"], proof[192 * b:192 * b + 192]) for b, x in enumerate(c["round1"])]
    assert [VERDICT[x["verdict"]] for x in c["round1"]] == [0, 0, 0, 2, 1]

    def prove(i, q):
        return O.misbehaviour_prove(sk[32 * q:32 * q + 32], enc_of(e1, ct, n, i, q),
                                    sc(rng.randrange(L)) + sc(rng.randrange(L)))

    q0, i0 = comp[0][0] - 1, comp[0][1] - 1  # a complaint that holds
    tampered = bytearray(prove(i0, q0))
    tampered[160 + 5] ^= 1
    comp.append((q0 + 1, i0 + 1, prove(i0, q0)))                       # 0 again, other nonces
    comp.append((q0 + 1, i0 + 1, bytes(tampered)))                     # 1
    comp.append((2, 1, prove(0, 1)))                                   # 2: dealer 1 is honest to receiver 2
    comp.append((q0 + 1, i0 + 1, b"\xff" * 32 + prove(i0, q0)[32:]))   # -1
    Ebad = bad_coefficient(E, N, 6, 2, b"\xff" * 32)
    comp.append((3, 7, prove(6, 2)))                                   # the accused row does not decode
    comp.append((4, 10, prove(9, 3)))                                  # no phase-1 broadcast of dealer 10
    fetched1 = bytes(int(i != 9) for i in range(n))
    accuser, accused = [x[0] for x in comp], [x[1] for x in comp]
    encs = b"".join(enc_of(e1, ct, n, i - 1, q - 1) for q, i, _ in comp)
    proofs = b"".join(x[2] for x in comp)
    oracle = [O.complaint1_verify(h, t, q, pk[32 * (q - 1):32 * q], enc_of(e1, ct, n, i - 1, q - 1), row(Ebad, N, i - 1), p)
              for q, i, p in comp]
    assert oracle == [0, 0, 0, 2, 1, 0, 1, 2, -1, -1, 2]  # the last: the oracle knows no fetched1
    exp = oracle[:-1] + [COMPLAINT_IGNORED]
    qual = [1] * n
    qual[6] = qual[9] = 0
    for (q, i, _), v in zip(comp, exp):
        if v == 0:
            qual[i - 1] = 0
    got = {}
    for mode in MODES:
        be.set_complaint_eval(mode)
        got[mode] = be.complaints_verify(n, t, accuser, accused, pk, Ebad, encs, proofs, fetched1)
        # and the fixture's own five, whose qualified set is the golden's
        v, ql = be.complaints_verify(n, t, accuser[:5], accused[:5], pk, E, encs[:128 * 5], proofs[:192 * 5])
        assert v == [0, 0, 0, 2, 1] and ql == full["qualified"], mode
    be.set_complaint_eval(0)
    for mode in MODES:
        assert got[mode] == (exp, qual), mode


# ---------------------------------------------------------------- round 4, n = 10, t = 4
def test_round4_fixture_and_forgeries(be, golden):
    """The eleven round3 records of complaints_n10_t4.json (nine valid, FalseClaimedInequality,
    FalseClaimedEquality) and, in the same call: a randomness + 1 (3), an accused whose A row does not
    decode (NO_PHASE3), whose E row does not decode (-1), a disqualified accused (IGNORED)."""
    c = golden("complaints_n10_t4.json")
    p3 = golden(c["round3_source"])
    n, t = p3["n"], p3["t"]
    N = t + 1
    h = be.env_init(t, n, CK)
    E, A, s, sp = H(p3["E"]), H(p3["A"]), H(p3["s"]), H(p3["s_prime"])
    comp = [(x["accuser"], x["accused"], H(x["share"]), H(x["randomness"])) for x in c["round3"]]
    fixture_exp = [VERDICT[x["verdict"]] for x in c["round3"]]
    assert fixture_exp == [0] * 9 + [2, 3]
    q, i, sh, rn = comp[0]
    comp.append((q, i, sh, sc(int.from_bytes(rn, "little") + 1)))
    A2 = bad_coefficient(A, N, 3, 4, b"\xff" * 32)
    E2 = bad_coefficient(E, N, 7, 0, b"\xff" * 32)
    comp.append((5, 4) + pair(s, sp, n, 3, 4))
    comp.append((6, 8) + pair(s, sp, n, 7, 5))
    comp.append((7, 9) + pair(s, sp, n, 8, 6))
    qualified = bytes(int(k != 8) for k in range(n))
    oracle = [O.complaint3_verify(h, t, q, sh, rn, row(E2, N, i - 1), row(A2, N, i - 1)) for q, i, sh, rn in comp]
    assert oracle == fixture_exp + [3, -1, -1, 2]  # the oracle knows neither the rule for A rows nor qualified
    exp = fixture_exp + [3, COMPLAINT_NO_PHASE3, -1, COMPLAINT_IGNORED]
    rec = [int(k in (5, 3)) for k in range(n)]
    got = {}
    for mode in MODES:
        be.set_complaint_eval(mode)
        got[mode] = be.complaints3_verify(n, t, *lists(comp), E2, A2, qualified)
        v, r = be.complaints3_verify(n, t, *lists(comp[:11]), E, A)
        assert v == fixture_exp and r == p3["reconstruct"], mode
    be.set_complaint_eval(0)
    for mode in MODES:
        assert got[mode] == (exp, rec), mode


# ---------------------------------------------------------------- n = 256, t = 127: 64 lanes, 6 stages
CHEATS = [3, 100, 200]
RECEIVERS = [0, 1, 170, 255]  # receivers 1, 2, 171 and 256


@pytest.fixture(scope="module")
def big(be):
    n, t = 256, 127
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x4d" * 32, 0, 0, n, t)
    E, A, s, sp = be.share_gen(a, b, n, n, t)
    return dict(n=n, t=t, N=t + 1, h=h, E=E, A=A, s=s, sp=sp)


def test_round2_n256(be, big):
    d = big
    n, t, N, h = d["n"], d["t"], d["N"], d["h"]
    assert dkg_amd.pair_eval_shape(t) == {"chunk": 2, "lanes": 64, "stages": 6}
    be.env_init(t, n, CK)
    rng = random.Random(256)
    sk, pk = be.member_keys(b"\x4e" * 32, 0, n)
    s2 = bytearray(d["s"])
    pairs = [(i, q) for i in CHEATS for q in RECEIVERS if q != i]
    for i, q in pairs:
        k = 32 * (i * n + q)
        s2[k:k + 32] = sc(int.from_bytes(d["s"][k:k + 32], "little") + 1 + q)
    e1, ct = be.encrypt_shares(pk, bytes(s2), d["sp"], dkg_amd.enc_randomness(b"\x4d" * 32, 0, 0, n, n, t), n, n)
    pairs.append((7, 170))  # a false complaint: dealer 8 is honest
    encs = [enc_of(e1, ct, n, i, q) for i, q in pairs]
    proofs = [O.misbehaviour_prove(sk[32 * q:32 * q + 32], e, sc(rng.randrange(L)) + sc(rng.randrange(L)))
              for (i, q), e in zip(pairs, encs)]
    oracle = [O.complaint1_verify(h, t, q + 1, pk[32 * q:32 * q + 32], e, row(d["E"], N, i), p)
              for (i, q), e, p in zip(pairs, encs, proofs)]
    assert oracle == [0] * (len(pairs) - 1) + [2]
    qual = [int(i not in CHEATS) for i in range(n)]
    for mode in MODES:
        be.set_complaint_eval(mode)
        got = be.complaints_verify(n, t, [q + 1 for _, q in pairs], [i + 1 for i, _ in pairs], pk, d["E"],
                                   b"".join(encs), b"".join(proofs))
        assert got == (oracle, qual), mode
    be.set_complaint_eval(0)


def test_round4_n256(be, big):
    d = big
    n, t, N, h = d["n"], d["t"], d["N"], d["h"]
    be.env_init(t, n, CK)
    A = d["A"]
    for i in CHEATS:
        A = bad_coefficient(A, N, i, (37 * i) % N, O.base_mul(sc(5000 + i)))
    pairs = [(i, q) for i in CHEATS for q in RECEIVERS if q != i] + [(7, 170)]
    comp = [(q + 1, i + 1) + pair(d["s"], d["sp"], n, i, q) for i, q in pairs]
    oracle = [O.complaint3_verify(h, t, q, sh, rn, row(d["E"], N, i - 1), row(A, N, i - 1)) for q, i, sh, rn in comp]
    assert oracle == [0] * (len(pairs) - 1) + [2]
    rec = [int(i in CHEATS) for i in range(n)]
    try:
        for mode, chunk in ((1, 0), (2, 0), (4, 0), (4, 3), (4, 128)):
            be.set_complaint_eval(mode)
            be.set_receiver_chunk(chunk)
            assert be.complaints3_verify(n, t, *lists(comp), d["E"], A) == (oracle, rec), (mode, chunk)
        be.set_receiver_chunk(1)  # 128 lanes: rejected where the wave evaluator runs, ignored elsewhere
        with pytest.raises(DkgError) as e:
            be.complaints3_verify(n, t, *lists(comp), d["E"], A)
        assert e.value.code == -1
        be.set_complaint_eval(1)
        assert be.complaints3_verify(n, t, *lists(comp[:2]), d["E"], A) == (oracle[:2], [int(i == CHEATS[0]) for i in range(n)])
    finally:
        be.set_receiver_chunk(0)
        be.set_complaint_eval(0)


# ---------------------------------------------------------------- the proven ceremony driver
def test_full_proven_mode4_equals_mode0(be, golden):
    """ceremony_verify_full_proven on full_faults_n10_t4.json (dealer 2's A_20 replaced, so that round 4 has
    complaints too, as tests/test_gpu_ceremony_proven.py builds it): every output field under mode 4 is
    mode 0's."""
    c, f, _, _, proof, _ = fixture_inputs(golden)
    n, t = f["n"], f["t"]
    N = t + 1
    be.env_init(t, n, CK)
    A = bytearray(H(f["A"]))
    A[32 * N:32 * N + 32] = O.base_mul(sc(321))
    args = (H(f["E"]), bytes(A), H(f["e1"]), H(f["ct"]), H(f["member_sk"]), H(f["member_pk"]))
    accuser = [x["accuser"] for x in c["round1"]]
    accused = [x["accused"] for x in c["round1"]]
    ref, v, _ = be.ceremony_verify_full_complaints(*args, accuser, accused, proof, n, t)
    comp = honest_complaints(ref, ref.s, ref.s_prime, n)
    assert v == [0, 0, 0, 2, 1] and len(comp) == 9
    out = {}
    for mode in (0, 4):
        be.set_complaint_eval(mode)
        out[mode] = no_times(be.ceremony_verify_full_proven(*args, accuser, accused, proof, *lists(comp), n, t))
    be.set_complaint_eval(0)
    assert out[4] == out[0]
    assert (out[4].verdict, out[4].verdict4) == ([0, 0, 0, 2, 1], [0] * 9)
