"""Round-2 complaints on the GPU (complaints.hip) and the qualified set by PROVEN complaints
(Phases<Phase2>::compute_qualified_set, committee.rs:370-398).

Expected values come from the CPU oracle (tests/oracle_lib.py misbehaviour_prove / complaint1_verify),
the libsodium fixtures, and tests/finalise_ref.py; the parent's host-side primitives
(Backend.misbehaviour_prove / complaint1_verify) serve as a second opinion.  Bit-exact throughout.
"""
import random

import pytest

import dkg_amd
from dkg_amd import ACCEPT, REJECT
from tests import finalise_ref as FR
from tests import oracle_lib as O
from tests.test_oracle import VERDICT, _complaint_inputs

pytestmark = pytest.mark.gpu

H = bytes.fromhex
L = 2**252 + 27742317777372353535851937790883648493
CK = b"Example of a shared string."
G = H("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
IGNORED = 4


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.set_complaint_eval(0)
    b.close()


def sc(v):
    return (v % L).to_bytes(32, "little")


def enc_of(e1, ct, n, i, q):
    """The pair dealer i (0-based) broadcast to receiver q: e1_rand || ct_rand || e1_share || ct_share."""
    k = 2 * (i * n + q)
    return e1[32 * k:32 * k + 32] + ct[32 * k:32 * k + 32] + e1[32 * k + 32:32 * k + 64] + ct[32 * k + 32:32 * k + 64]


def row(E, N, i):
    return E[32 * N * i:32 * N * (i + 1)]


def fixture_inputs(golden):
    c = golden("complaints_n10_t4.json")
    full = golden(c["source"])
    rows = [_complaint_inputs(c, full, x) for x in c["round1"]]
    sk, pk, enc, E, proof = (b"".join(r[k] for r in rows) for k in range(5))
    w = b"".join(H(v) for x in c["round1"] for v in x["w"])
    return c, full, sk, enc, proof, w


# ---------------- 1. fixture, primitives ----------------
def test_fixture_primitives(be, golden):
    """The five round-1 records of complaints_n10_t4.json over full_faults_n10_t4.json: proofs byte for
    byte, verdicts [0, 0, 0, 2, 1] (three honest, the forged honest pair, the tampered r1), the golden's
    qualified set, in every evaluation mode."""
    c, full, sk, enc, proof, w = fixture_inputs(golden)
    n, t = full["n"], full["t"]
    assert full["h"] == be.env_init(t, n, CK).hex()
    got = be.complaints_prove(sk, enc, w)
    untampered = [b for b, x in enumerate(c["round1"]) if x["verdict"] != "InvalidProofOfMisbehaviour"]
    assert len(untampered) == 4
    for b in untampered:
        assert got[192 * b:192 * b + 192] == proof[192 * b:192 * b + 192], c["round1"][b]
    assert be.complaints_prove(b"", b"", b"") == b""
    accuser = [x["accuser"] for x in c["round1"]]
    accused = [x["accused"] for x in c["round1"]]
    assert [VERDICT[x["verdict"]] for x in c["round1"]] == [0, 0, 0, 2, 1]
    for mode in (0, 1, 2):
        be.set_complaint_eval(mode)
        v, q = be.complaints_verify(n, t, accuser, accused, H(full["member_pk"]), H(full["E"]), enc, proof)
        assert v == [0, 0, 0, 2, 1], mode
        assert q == [1, 1, 0, 1, 1, 0, 1, 1, 0, 1] == full["qualified"], mode
    be.set_complaint_eval(0)


# ---------------- 2. fixture, ceremony ----------------
def _ceremony_fields(r):
    return (bytes(r.dec2), bytes(r.dec4), r.qualified, r.r2_error, r.complaints2, r.reconstruct, r.r4_error,
            r.phase4_error, r.n_qualified, r.final_share, r.public_share, r.mpk, r.s, r.s_prime)


def test_fixture_ceremony(be, golden):
    """With all of its receivers' complaints broadcast, the ceremony by proven complaints is the
    ceremony by rejections: every field equals ceremony_verify_full's and the golden's."""
    from tests.test_gpu import _check_ceremony
    c, full, _, _, proof, _ = fixture_inputs(golden)
    n, t = full["n"], full["t"]
    be.env_init(t, n, CK)
    args = (H(full["E"]), H(full["A"]), H(full["e1"]), H(full["ct"]), H(full["member_sk"]))
    accuser = [x["accuser"] for x in c["round1"]]
    accused = [x["accused"] for x in c["round1"]]
    for mode in (1, 2):
        be.set_complaint_eval(mode)
        r, v, dis = be.ceremony_verify_full_complaints(*args, H(full["member_pk"]), accuser, accused, proof, n, t)
        assert v == [0, 0, 0, 2, 1]
        assert dis == [0] * n
        assert r.s.hex() == full["s"] and r.s_prime.hex() == full["s_prime"]
        _check_ceremony(full, r, n)
        ref = be.ceremony_verify_full(*args, n, t)
        assert _ceremony_fields(r) == _ceremony_fields(ref)
    be.set_complaint_eval(0)


# ---------------- 3. a silent receiver ----------------
def test_silent_receiver(be, golden):
    """Receiver 5 rejects dealer 3 (flipped share ciphertext) but broadcasts no complaint: dealer 3 stays
    qualified for everyone else, round 4 checks its row, the flipped share is an accusation there and
    dealer 3 is reconstructed.  Expected outputs restated from the golden's decrypted shares and A."""
    c, full, _, _, proof, _ = fixture_inputs(golden)
    n, t = full["n"], full["t"]
    N = t + 1
    be.env_init(t, n, CK)
    keep = [b for b, x in enumerate(c["round1"]) if (x["accuser"], x["accused"]) != (5, 3)]
    assert len(keep) == 4
    accuser = [c["round1"][b]["accuser"] for b in keep]
    accused = [c["round1"][b]["accused"] for b in keep]
    proofs = b"".join(proof[192 * b:192 * b + 192] for b in keep)
    r, v, dis = be.ceremony_verify_full_complaints(H(full["E"]), H(full["A"]), H(full["e1"]), H(full["ct"]),
                                                   H(full["member_sk"]), H(full["member_pk"]), accuser, accused,
                                                   proofs, n, t)
    assert v == [0, 0, 2, 1]
    qualified = [1, 1, 1, 1, 1, 0, 1, 1, 0, 1]
    assert r.qualified == qualified and r.n_qualified == 8
    assert dis == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert "".join(str(x) for x in r.dec2) == full["dec2"] and r.complaints2 == full["complaints2"]
    # round 4: dealer 3's row is checked now; receiver 5 holds the flipped share
    dec4 = [[2 if i == j else (ACCEPT if qualified[i] else 3) for j in range(n)] for i in range(n)]
    dec4[2][4] = REJECT
    assert list(r.dec4) == [x for rw in dec4 for x in rw]
    recon = [0, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    assert r.reconstruct == recon and r.r4_error == [0] * n and r.r2_error == [0] * n and r.phase4_error == 0
    s = H(full["s"])

    def share(i, j):
        return int.from_bytes(s[32 * (i * n + j):32 * (i * n + j) + 32], "little")

    fs = [sum(share(i, j) for i in range(n) if qualified[i]) % L for j in range(n)]
    assert r.final_share == b"".join(sc(x) for x in fs)
    assert r.public_share == b"".join(O.base_mul(sc(x)) for x in fs)
    A0 = [H(full["A"])[32 * N * i:32 * N * i + 32] for i in range(n)]
    assert r.mpk == FR.final_party_mpk(n, qualified, recon, A0, share, [0] * n, [0] * n, t)


# ---------------- 4. the swapped-role dealer ----------------
def test_swapped_role_dealer(be):
    """Dealer 4 sends receiver 9 its share and randomness exchanged.  The receiver rejects
    (committee.rs:292-305) and its proof is honest, but ProofOfMisbehaviour::verify tests h*share +
    g*randomness (broadcast.rs:271-283), which equals the commitment for exchanged values: everyone else
    gets InvalidProofOfMisbehaviour and keeps dealer 4.  The receivers' own rule disqualifies it."""
    n, t = 16, 7
    N = t + 1
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x11" * 32, 0, 0, n, t)
    E, A, s, sp = O.share_gen(n, n, t, a, b, h)
    sk, pk = be.member_keys(b"\x21" * 32, 0, n)
    i, q = 3, 8
    k = 32 * (i * n + q)
    s2, sp2 = bytearray(s), bytearray(sp)
    s2[k:k + 32], sp2[k:k + 32] = sp[k:k + 32], s[k:k + 32]
    r_enc = dkg_amd.enc_randomness(b"\x11" * 32, 0, 0, n, n, t)
    e1, ct = be.encrypt_shares(pk, bytes(s2), bytes(sp2), r_enc, n, n)
    enc = enc_of(e1, ct, n, i, q)
    proof = O.misbehaviour_prove(sk[32 * q:32 * q + 32], enc, sc(1234567) + sc(7654321))
    assert O.complaint1_verify(h, t, q + 1, pk[32 * q:32 * q + 32], enc, row(E, N, i), proof) == 1
    assert be.complaint1_verify(t, [q + 1], pk[32 * q:32 * q + 32], enc, row(E, N, i), proof) == [1]
    for mode in (1, 2):
        be.set_complaint_eval(mode)
        r, v, dis = be.ceremony_verify_full_complaints(E, A, e1, ct, sk, pk, [q + 1], [i + 1], proof, n, t)
        assert r.dec2[i * n + q] == REJECT and list(r.dec2).count(REJECT) == 1
        assert v == [1]
        assert r.qualified == [1] * n
        assert dis == [int(j == q) for j in range(n)]
        # round 4 checks dealer 4's row: g * (the randomness) is not P_A(9)
        assert r.dec4[i * n + q] == REJECT and r.reconstruct == [int(d == i) for d in range(n)]
    be.set_complaint_eval(0)
    ref = be.ceremony_verify_full(E, A, e1, ct, sk, n, t)
    assert ref.qualified == [int(d != i) for d in range(n)]  # the two rules differ exactly here


# ---------------- 5. random batch against the oracle ----------------
@pytest.fixture(scope="module")
def batch(be):
    """n = 40, t = 19: seven dealers cheat all 39 other receivers (273 complaints: past a 256-lane
    workgroup and five waves), plus the odd ones.  Inputs and oracle verdicts, computed once."""
    rng = random.Random(2024)
    n, t = 40, 19
    N = t + 1
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x31" * 32, 0, 0, n, t)
    E, A, s, sp = O.share_gen(n, n, t, a, b, h)
    sk, pk = be.member_keys(b"\x32" * 32, 0, n)
    cheats = [2, 5, 11, 17, 23, 31, 38]
    s2 = bytearray(s)
    for i in cheats + [29, 34]:  # 29: one bad E coefficient; 34: no phase-1 broadcast
        for q in range(n):
            if q != i:
                k = 32 * (i * n + q)
                s2[k:k + 32] = sc(int.from_bytes(s[k:k + 32], "little") + 1 + q)
    r_enc = dkg_amd.enc_randomness(b"\x31" * 32, 0, 0, n, n, t)
    e1, ct = be.encrypt_shares(pk, bytes(s2), sp, r_enc, n, n)
    E = bytearray(E)
    E[32 * (N * 29 + 3):32 * (N * 29 + 4)] = b"\xff" * 32
    E = bytes(E)
    fetched1 = bytearray([1] * n)
    fetched1[34] = 0

    def prove(i, q):
        return O.misbehaviour_prove(sk[32 * q:32 * q + 32], enc_of(e1, ct, n, i, q),
                                    sc(rng.randrange(L)) + sc(rng.randrange(L)))

    comp = [(q + 1, i + 1, prove(i, q)) for i in cheats for q in range(n) if q != i]
    assert len(comp) == 273

    def tamper(p, off):
        p = bytearray(p)
        p[off] ^= 1
        return bytes(p)

    comp.append((4, 3, tamper(prove(2, 3), 64)))                   # c1
    comp.append((5, 3, tamper(prove(2, 4), 160 + 5)))              # r2
    comp.append((6, 3, O.base_mul(sc(5)) + prove(2, 5)[32:]))      # a wrong but decodable share_key
    comp.append((7, 1, prove(0, 6)))                               # a false complaint: dealer 1 is honest
    comp.append((9, 12, prove(11, 8)))                             # (9, 12) again, other nonces
    comp.append((10, 12, b"\xff" * 32 + prove(11, 9)[32:]))        # a key that does not decode
    comp.append((2, 30, prove(29, 1)))                             # accused row with a bad coefficient
    comp.append((3, 35, prove(34, 2)))                             # accused without a phase-1 broadcast
    accuser = [c[0] for c in comp]
    accused = [c[1] for c in comp]
    proofs = b"".join(c[2] for c in comp)
    enc = b"".join(enc_of(e1, ct, n, i - 1, q - 1) for q, i, _ in comp)
    oracle = [O.complaint1_verify(h, t, q, pk[32 * (q - 1):32 * q], enc_of(e1, ct, n, i - 1, q - 1), row(E, N, i - 1), p)
              for q, i, p in comp]
    return dict(n=n, t=t, N=N, pk=pk, E=E, fetched1=bytes(fetched1), accuser=accuser, accused=accused, proofs=proofs,
                enc=enc, oracle=oracle)


def test_batch_oracle_is_as_intended(batch):
    o = batch["oracle"]
    assert o[:273] == [0] * 273
    assert o[273:] == [1, 1, 1, 2, 0, -1, -1, 0]  # the last: the oracle knows no fetched1


def test_batch_parent_agrees(be, batch):
    """The parent's host-side primitive on the decodable complaints: the same verdicts as the oracle."""
    d = batch
    be.env_init(d["t"], d["n"], CK)
    idx = [c for c, v in enumerate(d["oracle"]) if v >= 0]
    res = be.complaint1_verify(d["t"], [d["accuser"][c] for c in idx],
                               b"".join(d["pk"][32 * (d["accuser"][c] - 1):32 * d["accuser"][c]] for c in idx),
                               b"".join(d["enc"][128 * c:128 * c + 128] for c in idx),
                               b"".join(row(d["E"], d["N"], d["accused"][c] - 1) for c in idx),
                               b"".join(d["proofs"][192 * c:192 * c + 192] for c in idx))
    assert res == [d["oracle"][c] for c in idx]


@pytest.mark.parametrize("mode", [1, 2, 0])
def test_batch_against_oracle(be, batch, mode):
    d = batch
    n = d["n"]
    be.env_init(d["t"], n, CK)
    be.set_complaint_eval(mode)
    v, q = be.complaints_verify(n, d["t"], d["accuser"], d["accused"], d["pk"], d["E"], d["enc"], d["proofs"],
                                d["fetched1"])
    be.set_complaint_eval(0)
    exp = [IGNORED if not d["fetched1"][i - 1] else o for i, o in zip(d["accused"], d["oracle"])]
    assert v == exp
    qual = [1] * n
    qual[29] = 0  # E row does not decode
    qual[34] = 0  # not fetched
    for i, o in zip(d["accused"], exp):
        if o == 0:
            qual[i - 1] = 0
    assert q == qual
    assert sum(qual) == n - 9


def test_automatic_mode_mixes_both_paths(be):
    """n = 130, t = 12: dealer 1 cheats all 129 other receivers, for which the automatic mode's chain
    model (runtime.hip complaint_tables_pay: 13 N + 3.7 n = 650 against 3.6 N (8 + 8 + 1) = 796) takes the
    difference tables, and dealer 7 cheats one receiver, a Horner walk (3.6 N (8 + 2 + 1) = 515) in the
    same call; dealer 4's false complaint is another."""
    rng = random.Random(77)
    n, t = 130, 12
    N = t + 1
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x41" * 32, 0, 0, n, t)
    E, A, s, sp = O.share_gen(n, n, t, a, b, h)
    sk, pk = be.member_keys(b"\x42" * 32, 0, n)
    pairs = [(0, q) for q in range(1, n)] + [(6, 99)]
    s2 = bytearray(s)
    for i, q in pairs:
        k = 32 * (i * n + q)
        s2[k:k + 32] = sc(int.from_bytes(s[k:k + 32], "little") + 1)
    e1, ct = be.encrypt_shares(pk, bytes(s2), sp, dkg_amd.enc_randomness(b"\x41" * 32, 0, 0, n, n, t), n, n)
    pairs.append((3, 4))  # and a false complaint
    encs = [enc_of(e1, ct, n, i, q) for i, q in pairs]
    proofs = [O.misbehaviour_prove(sk[32 * q:32 * q + 32], e, sc(rng.randrange(L)) + sc(rng.randrange(L)))
              for (i, q), e in zip(pairs, encs)]
    exp = [O.complaint1_verify(h, t, q + 1, pk[32 * q:32 * q + 32], e, row(E, N, i), p)
           for (i, q), e, p in zip(pairs, encs, proofs)]
    assert exp == [0] * 130 + [2]
    for mode in (0, 1, 2):
        be.set_complaint_eval(mode)
        v, qual = be.complaints_verify(n, t, [q + 1 for _, q in pairs], [i + 1 for i, _ in pairs], pk, E,
                                       b"".join(encs), b"".join(proofs))
        assert v == exp, mode
        assert qual == [int(i not in (0, 6)) for i in range(n)], mode
    be.set_complaint_eval(0)


# ---------------- 6. edges ----------------
def _small_case(be, n, t, cheat, seed):
    """One committee with the pairs `cheat` [(dealer, receiver)] given a wrong share: inputs and oracle verdicts."""
    rng = random.Random(seed)
    N = t + 1
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(bytes([seed]) * 32, 0, 0, n, t)
    E, A, s, sp = O.share_gen(n, n, t, a, b, h)
    sk, pk = be.member_keys(bytes([seed + 1]) * 32, 0, n)
    s2 = bytearray(s)
    for i, q in cheat:
        k = 32 * (i * n + q)
        s2[k:k + 32] = sc(int.from_bytes(s[k:k + 32], "little") + 1)
    e1, ct = be.encrypt_shares(pk, bytes(s2), sp, dkg_amd.enc_randomness(bytes([seed]) * 32, 0, 0, n, n, t), n, n)
    encs = [enc_of(e1, ct, n, i, q) for i, q in cheat]
    proofs = [O.misbehaviour_prove(sk[32 * q:32 * q + 32], e, sc(rng.randrange(L)) + sc(rng.randrange(L)))
              for (i, q), e in zip(cheat, encs)]
    exp = [O.complaint1_verify(h, t, q + 1, pk[32 * q:32 * q + 32], e, row(E, N, i), p)
           for (i, q), e, p in zip(cheat, encs, proofs)]
    return pk, E, encs, proofs, exp


@pytest.mark.parametrize("n,t,cheat", [(2, 0, [(0, 1)]), (3, 1, [(2, 0), (1, 0)]), (5, 2, [(4, 1)])])
def test_small_committees(be, n, t, cheat):
    """C = 1 and the smallest committees: a constant polynomial (t = 0), and t = 1."""
    pk, E, encs, proofs, exp = _small_case(be, n, t, cheat, 0x51)
    assert exp == [0] * len(cheat)
    for mode in (0, 1, 2):
        be.set_complaint_eval(mode)
        v, q = be.complaints_verify(n, t, [q + 1 for _, q in cheat], [i + 1 for i, _ in cheat], pk, E, b"".join(encs),
                                    b"".join(proofs))
        assert v == exp, mode
        assert q == [int(i not in [d for d, _ in cheat]) for i in range(n)], mode
        # C = 1, and C = 0
        v, q = be.complaints_verify(n, t, [cheat[0][1] + 1], [cheat[0][0] + 1], pk, E, encs[0], proofs[0])
        assert v == [0] and q == [int(i != cheat[0][0]) for i in range(n)]
        assert be.complaints_verify(n, t, [], [], pk, E, b"", b"") == ([], [1] * n)
    be.set_complaint_eval(0)


def test_index_range_and_env(be):
    pk, E, encs, proofs, _ = _small_case(be, 3, 1, [(2, 0)], 0x53)
    for acc, acd in [([0], [3]), ([4], [3]), ([1], [0]), ([1], [4])]:
        with pytest.raises(dkg_amd.DkgError) as e:
            be.complaints_verify(3, 1, acc, acd, pk, E, encs[0], proofs[0])
        assert e.value.code == -1
    fresh = dkg_amd.Backend(0)
    try:
        with pytest.raises(dkg_amd.DkgError) as e:
            fresh.complaints_verify(3, 1, [1], [3], pk, E, encs[0], proofs[0])
        assert e.value.code == -1
    finally:
        fresh.close()


def test_accuser_index_13_bits(be):
    """Accusers 4095 (all twelve low bits) and 4096 (only bit 12) at n = 4096, t = 3: the index walk of the
    Horner path and the last table positions.  E is 512 KB: dealer 1's row real, the rest the generator."""
    rng = random.Random(91)
    n, t = 4096, 3
    N = t + 1
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x61" * 32, 0, 0, 1, t)
    E1, _, s, sp = O.share_gen(1, n, t, a, b, h)
    E = E1 + G * (N * (n - 1))
    accusers = [4095, 4096]
    sks = [sc(rng.randrange(1, L)) for _ in accusers]
    pk = bytearray(G * n)
    encs, proofs, exp = [], [], []
    for j, x in zip(accusers, sks):
        pkj = O.base_mul(x)
        pk[32 * (j - 1):32 * j] = pkj
        k = 32 * (j - 1)
        bad = sc(int.from_bytes(s[k:k + 32], "little") + 1)
        er, cr = O.hybrid_encrypt(pkj, sc(rng.randrange(L)), sp[k:k + 32])
        es, cs = O.hybrid_encrypt(pkj, sc(rng.randrange(L)), bad)
        enc = er + cr + es + cs
        p = O.misbehaviour_prove(x, enc, sc(rng.randrange(L)) + sc(rng.randrange(L)))
        encs.append(enc)
        proofs.append(p)
        exp.append(O.complaint1_verify(h, t, j, pkj, enc, E1, p))
    # and a false complaint by 4096 about the true share
    k = 32 * 4095
    er, cr = O.hybrid_encrypt(bytes(pk[k:k + 32]), sc(3), sp[k:k + 32])
    es, cs = O.hybrid_encrypt(bytes(pk[k:k + 32]), sc(4), s[k:k + 32])
    enc = er + cr + es + cs
    p = O.misbehaviour_prove(sks[1], enc, sc(5) + sc(6))
    assert O.complaint1_verify(h, t, 4096, bytes(pk[k:k + 32]), enc, E1, p) == 2
    assert exp == [0, 0]
    for mode in (1, 2):
        be.set_complaint_eval(mode)
        v, q = be.complaints_verify(n, t, accusers, [1, 1], bytes(pk), E, b"".join(encs), b"".join(proofs))
        assert v == [0, 0], mode
        assert q == [0] + [1] * (n - 1), mode
        v, q = be.complaints_verify(n, t, [4096], [1], bytes(pk), E, enc, p)
        assert v == [2] and q == [1] * n, mode
    be.set_complaint_eval(0)
