"""Ceremonies whose reconstructable set follows the PROVEN round-4 complaints (Phases<Phase4>::proceed,
committee.rs:625-688): dkg_ceremony_verify_fetched_proven and dkg_ceremony_verify_full_proven.

Where every receiver files its complaint the outcome is the rejection rule's, which passes its goldens;
where the rules differ the expected sets, mpk and status are restated with tests/finalise_ref.py.
The last section pins what all six verify entry points share through their one driver (verify_ceremony).
"""
import ctypes
import dataclasses

import pytest

import dkg_amd
from dkg_amd import COMPLAINT_IGNORED, COMPLAINT_NO_PHASE3, REJECT, _lib
from dkg_amd import broadcast as B
from dkg_amd._lib import DKG_E_ARG, DKG_OK, FIN_INSUFFICIENT, FIN_OK, FIN_PANIC, FIN_PHASE4_ERROR
from dkg_amd.api import CeremonyResult, ProvenResult
from tests import finalise_ref as FR
from tests import oracle_lib as O
from tests.test_gpu import _check_ceremony
from tests.test_gpu_complaints import _ceremony_fields, fixture_inputs

pytestmark = pytest.mark.gpu

H = bytes.fromhex
L = 2**252 + 27742317777372353535851937790883648493
CK = b"Example of a shared string."
ZERO = bytes(32)


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


def sc(v):
    return (v % L).to_bytes(32, "little")


def pair(s, sp, n, i, q):
    k = 32 * (i * n + q)
    return s[k:k + 32], sp[k:k + 32]


def honest_complaints(r, s, sp, n):
    """One complaint per round-4 rejection of a qualified dealer, with the pair the receiver holds."""
    return [(j + 1, i + 1) + pair(s, sp, n, i, j) for i in range(n) for j in range(n)
            if r.qualified[i] and r.dec4[i * n + j] == REJECT]


def lists(comp):
    return ([c[0] for c in comp], [c[1] for c in comp], b"".join(c[2] for c in comp), b"".join(c[3] for c in comp))


def proven(be, c, comp, fetched1=None, fetched3=None, A=None, s=None):
    n, t = c["n"], c["t"]
    return be.ceremony_verify_fetched_proven(H(c["E"]), A or H(c["A"]), s or H(c["s"]), H(c["s_prime"]),
                                             fetched1 or bytes([1] * n), fetched3 or bytes([1] * n), *lists(comp), n, t)


def status_of(r):
    if r.phase4_error:
        return FIN_PHASE4_ERROR
    return FIN_INSUFFICIENT if any(r.reconstruct) and r.mpk == ZERO else FIN_OK


def fin_inputs(c, A=None):
    n, N = c["n"], c["t"] + 1
    A = A or H(c["A"])
    s = H(c["s"])
    return [A[32 * N * i:32 * N * i + 32] for i in range(n)], lambda i, j: int.from_bytes(
        s[32 * (i * n + j):32 * (i * n + j) + 32], "little")


# ---------------- 7. everyone files: the rejection rule's outcome ----------------
@pytest.mark.parametrize("name", ["fault_a_generator_n10_t4.json", "fault_a_many_n10_t4.json",
                                  "fault_recon_only_n10_t4.json", "fault_recon_insufficient_n16_t3.json",
                                  "fault_recon_r2err_n16_t3.json"])
def test_agrees_with_rejection_rule(be, golden, name):
    c = golden(name)
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    ones = bytes([1] * n)
    ref = be.ceremony_verify_fetched(H(c["E"]), H(c["A"]), H(c["s"]), H(c["s_prime"]), ones, ones, n, t)
    comp = honest_complaints(ref, H(c["s"]), H(c["s_prime"]), n)
    assert comp and {x[1] - 1 for x in comp} == {i for i in range(n) if ref.reconstruct[i]}
    p = proven(be, c, comp)
    assert _ceremony_fields(p.result) == _ceremony_fields(ref)
    assert p.verdict4 == [0] * len(comp)
    assert p.finalise_status == status_of(ref)
    first = next(i for i in range(n) if ref.reconstruct[i])
    assert p.recovery_index == (first if p.finalise_status == FIN_INSUFFICIENT else -1)


def test_insufficient_fixture_is_insufficient(be, golden):
    """The status the previous test derives from mpk is the one the fixture was built for."""
    c = golden("fault_recon_insufficient_n16_t3.json")
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    ones = bytes([1] * n)
    ref = be.ceremony_verify_fetched(H(c["E"]), H(c["A"]), H(c["s"]), H(c["s_prime"]), ones, ones, n, t)
    assert status_of(ref) == FIN_INSUFFICIENT
    c = golden("fault_a_many_n10_t4.json")
    assert c["phase4_error"]


# ---------------- 8. where the rules differ ----------------
@pytest.fixture(scope="module")
def agen(be, golden):
    """fault_a_generator_n10_t4: dealer 6's A row is the generator, every other receiver rejects it."""
    c = golden("fault_a_generator_n10_t4.json")
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    ones = bytes([1] * n)
    ref = be.ceremony_verify_fetched(H(c["E"]), H(c["A"]), H(c["s"]), H(c["s_prime"]), ones, ones, n, t)
    assert ref.reconstruct == [int(i == 5) for i in range(n)] and ref.mpk.hex() == c["mpk"]
    return c, ref, honest_complaints(ref, H(c["s"]), H(c["s_prime"]), n)


def check_unreconstructed(c, p, ref):
    n, t = c["n"], c["t"]
    A0, share = fin_inputs(c)
    r = p.result
    assert r.reconstruct == [0] * n and r.phase4_error == 0
    mpk = FR.final_party_mpk(n, r.qualified, [0] * n, A0, share, r.r2_error, r.r4_error, t)
    assert mpk == FR.gsum(A0)  # every qualified A_i0, the bad dealer's g included
    assert r.mpk == mpk != ref.mpk
    assert FR.party_finalise(0, n, t, r.qualified, r.reconstruct, A0, share) == ("OK", -1, mpk)
    assert (p.finalise_status, p.recovery_index) == (FIN_OK, -1)
    # the receivers' own view is unchanged
    assert (bytes(r.dec2), bytes(r.dec4), r.qualified, r.r4_error, r.final_share, r.public_share) == (
        bytes(ref.dec2), bytes(ref.dec4), ref.qualified, ref.r4_error, ref.final_share, ref.public_share)


def test_no_complaints(be, agen):
    """(a) Nobody files: the reference keeps dealer 6's A_60 in the key.  Fails on the rejection rule."""
    c, ref, _ = agen
    be.env_init(c["t"], c["n"], CK)
    p = proven(be, c, [])
    assert p.verdict4 == []
    check_unreconstructed(c, p, ref)


def test_forged_complaints_only(be, agen):
    """(b) A wrong share (FalseClaimedEquality) and an honest pair (FalseClaimedInequality) prove nothing."""
    c, ref, comp = agen
    n = c["n"]
    be.env_init(c["t"], n, CK)
    q, i, sh, rn = comp[0]
    forged = [(q, i, sc(int.from_bytes(sh, "little") + 1), rn), (3, 2) + pair(H(c["s"]), H(c["s_prime"]), n, 1, 2)]
    p = proven(be, c, forged)
    assert p.verdict4 == [3, 2]
    check_unreconstructed(c, p, ref)


@pytest.mark.parametrize("k", [0, 8])
def test_one_valid_complaint_suffices(be, agen, k):
    """(c) Any one of the nine possible complaints reconstructs dealer 6 for everyone."""
    c, ref, comp = agen
    assert len(comp) == 9
    be.env_init(c["t"], c["n"], CK)
    p = proven(be, c, [comp[k]])
    assert p.verdict4 == [0]
    assert _ceremony_fields(p.result) == _ceremony_fields(ref)
    assert (p.finalise_status, p.recovery_index) == (FIN_OK, -1)


def test_no_phase3_broadcast(be, agen):
    """(d) Dealer 3 publishes no phase-3 broadcast.  One complaint, whatever it carries, reconstructs it
    (committee.rs:643); with none its committed shares were never stored (:527-530) and every party's
    finalise panics at dealer 3 (:791-795), before it reaches the reconstructed dealer 6."""
    c, _, comp = agen
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    f3 = bytes([int(i != 2) for i in range(n)])
    ones = bytes([1] * n)
    ref = be.ceremony_verify_fetched(H(c["E"]), H(c["A"]), H(c["s"]), H(c["s_prime"]), ones, f3, n, t)
    assert ref.reconstruct == [int(i in (2, 5)) for i in range(n)]
    p = proven(be, c, comp + [(7, 3, sc(12345), sc(67890))], fetched3=f3)
    assert p.verdict4 == [0] * 9 + [COMPLAINT_NO_PHASE3]
    assert _ceremony_fields(p.result) == _ceremony_fields(ref)
    assert (p.finalise_status, p.recovery_index) == (FIN_OK, -1)
    p = proven(be, c, comp, fetched3=f3)
    assert p.verdict4 == [0] * 9
    assert p.result.reconstruct == [int(i == 5) for i in range(n)] and p.result.phase4_error == 0
    assert (p.finalise_status, p.recovery_index) == (FIN_PANIC, 2)
    assert p.result.mpk == ZERO


def test_complaint_against_disqualified(be, agen):
    """(e) Dealer 9's share to receiver 2 is wrong: round 2 disqualifies it, a round-4 complaint against it is
    ignored (committee.rs:639)."""
    c, _, comp = agen
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    s = bytearray(H(c["s"]))
    k = 32 * (8 * n + 1)
    s[k:k + 32] = sc(int.from_bytes(s[k:k + 32], "little") + 1)
    s = bytes(s)
    ones = bytes([1] * n)
    ref = be.ceremony_verify_fetched(H(c["E"]), H(c["A"]), s, H(c["s_prime"]), ones, ones, n, t)
    assert ref.qualified == [int(i != 8) for i in range(n)]
    p = proven(be, c, comp + [(4, 9) + pair(s, H(c["s_prime"]), n, 8, 3)], s=s)
    assert p.verdict4 == [0] * 9 + [COMPLAINT_IGNORED]
    assert p.result.reconstruct == [int(i == 5) for i in range(n)]
    assert _ceremony_fields(p.result) == _ceremony_fields(ref)
    assert (p.finalise_status, p.recovery_index) == (FIN_OK, -1)


def test_phase4_error_needs_proven_complaints(be, agen):
    """(f) Six bad A rows, one proven complaint each: qualified - reconstruct = 4 <= t, Phases<Phase4>::proceed
    fails for everyone (committee.rs:673-677).  The same rows with no complaint: no such error."""
    c, _, _ = agen
    n, t = c["n"], c["t"]
    N = t + 1
    be.env_init(t, n, CK)
    A = bytearray(H(c["A"]))
    bad = [0, 2, 4, 5, 7, 9]
    for i in bad:
        A[32 * N * i:32 * N * i + 32] = O.base_mul(sc(500 + i))
    A = bytes(A)
    comp = [((i + 1) % n + 1, i + 1) + pair(H(c["s"]), H(c["s_prime"]), n, i, (i + 1) % n) for i in bad]
    p = proven(be, c, comp, A=A)
    assert p.verdict4 == [0] * 6
    assert p.result.reconstruct == [int(i in bad) for i in range(n)]
    assert p.result.phase4_error == 1 and p.result.mpk == ZERO
    assert (p.finalise_status, p.recovery_index) == (FIN_PHASE4_ERROR, -1)
    p = proven(be, c, [], A=A)
    assert p.result.reconstruct == [0] * n and p.result.phase4_error == 0
    ones = bytes([1] * n)
    ref = be.ceremony_verify_fetched(H(c["E"]), A, H(c["s"]), H(c["s_prime"]), ones, ones, n, t)
    assert ref.phase4_error == 1  # the rejection rule reconstructs all six
    assert (bytes(p.result.dec4), p.result.r4_error) == (bytes(ref.dec4), ref.r4_error)  # the receivers' own checks


# ---------------- 9. full mode ----------------
@pytest.fixture(scope="module")
def full(be, golden):
    """full_faults_n10_t4.json (three round-2 faults, five phase-2 complaints) with dealer 2's A_20 replaced,
    so that round 4 has rejections too."""
    c, f, _, _, proof, _ = fixture_inputs(golden)
    n, t = f["n"], f["t"]
    N = t + 1
    be.env_init(t, n, CK)
    A = bytearray(H(f["A"]))
    A[32 * N:32 * N + 32] = O.base_mul(sc(321))
    args = (H(f["E"]), bytes(A), H(f["e1"]), H(f["ct"]), H(f["member_sk"]), H(f["member_pk"]))
    accuser = [x["accuser"] for x in c["round1"]]
    accused = [x["accused"] for x in c["round1"]]
    ref, v, dis = be.ceremony_verify_full_complaints(*args, accuser, accused, proof, n, t)
    assert v == [0, 0, 0, 2, 1] and ref.reconstruct == [int(i == 1) for i in range(n)]
    comp = honest_complaints(ref, ref.s, ref.s_prime, n)
    assert len(comp) == 9
    return dict(c=c, f=f, n=n, t=t, args=args, accuser=accuser, accused=accused, proof=proof, ref=ref, v=v, dis=dis,
                comp=comp)


def test_full_agrees_with_rejection_rule(be, full):
    d = full
    be.env_init(d["t"], d["n"], CK)
    p = be.ceremony_verify_full_proven(*d["args"], d["accuser"], d["accused"], d["proof"], *lists(d["comp"]),
                                       d["n"], d["t"])
    assert _ceremony_fields(p.result) == _ceremony_fields(d["ref"])
    assert (p.verdict, p.dissent, p.verdict4) == (d["v"], d["dis"], [0] * 9)
    assert (p.finalise_status, p.recovery_index) == (FIN_OK, -1)


def test_full_silent_round4(be, full):
    """Nobody files in round 4: dealer 2 stays a final party and its A_20 in the key."""
    d = full
    n, t, N = d["n"], d["t"], d["t"] + 1
    be.env_init(t, n, CK)
    p = be.ceremony_verify_full_proven(*d["args"], d["accuser"], d["accused"], d["proof"], [], [], b"", b"", n, t)
    r, ref = p.result, d["ref"]
    assert (p.verdict, p.dissent, p.verdict4) == (d["v"], d["dis"], [])
    assert r.reconstruct == [0] * n and r.qualified == ref.qualified and r.phase4_error == 0
    A = d["args"][1]
    A0 = [A[32 * N * i:32 * N * i + 32] for i in range(n)]
    mpk = FR.gsum([A0[i] for i in range(n) if r.qualified[i]])
    assert r.mpk == mpk != ref.mpk
    assert (bytes(r.dec2), bytes(r.dec4), r.final_share, r.public_share, r.s, r.s_prime) == (
        bytes(ref.dec2), bytes(ref.dec4), ref.final_share, ref.public_share, ref.s, ref.s_prime)
    assert (p.finalise_status, p.recovery_index) == (FIN_OK, -1)


def test_full_from_wire_bytes(be, full):
    """The same call fed by intake_phase4 / verify_broadcasts_proven from serialised broadcasts."""
    d = full
    n, t, N = d["n"], d["t"], d["t"] + 1
    be.env_init(t, n, CK)
    E, A, e1, ct, sk, pk = d["args"]

    def hybrid(i, q, w):
        k = 32 * (2 * (i * n + q) + w)
        return e1[k:k + 32] + ct[k:k + 32]

    p1 = [B.BroadcastPhase1([E[32 * (N * i + k):32 * (N * i + k + 1)] for k in range(N)],
                            [B.EncryptedShares(q + 1, hybrid(i, q, 1), hybrid(i, q, 0)) for q in range(n)])
          for i in range(n)]
    p3 = [B.BroadcastPhase3([A[32 * (N * i + k):32 * (N * i + k + 1)] for k in range(N)]) for i in range(n)]
    p2 = [None] * n
    for b, (q, i) in enumerate(zip(d["accuser"], d["accused"])):
        m = B.MisbehavingPartiesRound1(i, 0, hybrid(i - 1, q - 1, 0) + hybrid(i - 1, q - 1, 1),
                                       d["proof"][192 * b:192 * b + 192])
        p2[q - 1] = B.BroadcastPhase2((p2[q - 1].misbehaving_parties if p2[q - 1] else []) + [m])
    p4 = [None] * n
    for q, i, sh, rn in d["comp"]:
        p4[q - 1] = B.BroadcastPhase4([B.MisbehavingPartiesRound3(i, sh, rn)])

    def wire(cls, msgs):
        return [None if m is None else cls.from_bytes(m.to_bytes()) for m in msgs]

    # intake_phase2 flattens by sender: the fixture's records are not in that order
    order = sorted(range(len(d["accuser"])), key=lambda b: d["accuser"][b])
    p = B.verify_broadcasts_proven(be, n, t, wire(B.BroadcastPhase1, p1), wire(B.BroadcastPhase3, p3),
                                   wire(B.BroadcastPhase4, p4), phase2=wire(B.BroadcastPhase2, p2), sk=sk, pk=pk)
    assert _ceremony_fields(p.result) == _ceremony_fields(d["ref"])
    assert p.verdict == [d["v"][b] for b in order] and p.dissent == d["dis"]
    assert sorted(B.intake_phase4(n, p4)[0]) == sorted(x[0] for x in d["comp"])
    assert p.verdict4 == [0] * 9
    assert (p.finalise_status, p.recovery_index) == (FIN_OK, -1)


# ---------------- 10. the one verify driver behind the entry points ----------------
@pytest.fixture(scope="module")
def amany(be, golden):
    """fault_a_many_n10_t4 (six reconstructed dealers, phase4_error) with every receiver's round-4 complaint."""
    c = golden("fault_a_many_n10_t4.json")
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    ones = bytes([1] * n)
    ref = be.ceremony_verify_fetched(H(c["E"]), H(c["A"]), H(c["s"]), H(c["s_prime"]), ones, ones, n, t)
    comp = honest_complaints(ref, H(c["s"]), H(c["s_prime"]), n)
    assert comp and ref.phase4_error
    return c, comp


def u32s(xs):
    return (ctypes.c_uint32 * max(len(xs), 1))(*xs)


def raw_proven(be, n, t, fn, args, verdicts, C4, null=()):
    """fn(ctx, n, t, *args, out, *verdicts, status, index) through the C ABI, the out struct's `null`
    arrays absent: what the call reports beside the per-party arrays (verdicts[-1] the round-4 ones)."""
    o, _bufs = be._ceremony_out(n, t, True)
    for k in null:
        setattr(o, k, None)
    st, ri = ctypes.c_int32(-9), ctypes.c_int32(-9)
    rc = fn(be.ctx, n, t, *args, ctypes.byref(o), *verdicts, ctypes.byref(st), ctypes.byref(ri))
    assert rc == DKG_OK
    return bytes(o.mpk), o.n_qualified, o.phase4_error, list(verdicts[-1])[:C4], st.value, ri.value


FLAG_ARRAYS = ("qualified", "reconstruct", "r2_error", "r4_error")


def test_null_flag_arrays_fetched(be, amany):
    """The proven outcome needs the four per-party flag vectors whether or not the caller asked for them."""
    c, comp = amany
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    acc, acd, sh, rn = lists(comp)
    ones = bytes([1] * n)
    args = (H(c["E"]), H(c["A"]), H(c["s"]), H(c["s_prime"]), ones, ones, len(comp), u32s(acc), u32s(acd), sh, rn)
    fn = _lib.lib().dkg_ceremony_verify_fetched_proven
    got = [raw_proven(be, n, t, fn, args, ((ctypes.c_int32 * len(comp))(),), len(comp), null)
           for null in ((), FLAG_ARRAYS)]
    assert got[0] == got[1]
    p = proven(be, c, comp)
    assert got[0] == (p.result.mpk, p.result.n_qualified, p.result.phase4_error, p.verdict4, p.finalise_status,
                      p.recovery_index)
    assert got[0][2] == 1 and got[0][4] == FIN_PHASE4_ERROR


def test_null_flag_arrays_full(be, full):
    d = full
    n, t, comp = d["n"], d["t"], d["comp"]
    be.env_init(t, n, CK)
    acc4, acd4, sh, rn = lists(comp)
    C = len(d["accuser"])
    args = d["args"] + (C, u32s(d["accuser"]), u32s(d["accused"]), d["proof"], None, len(comp), u32s(acc4),
                        u32s(acd4), sh, rn)
    fn = _lib.lib().dkg_ceremony_verify_full_proven
    got = []
    for null in ((), FLAG_ARRAYS):
        verdicts = ((ctypes.c_int32 * C)(), (ctypes.c_int32 * n)(), (ctypes.c_int32 * len(comp))())
        got.append(raw_proven(be, n, t, fn, args, verdicts, len(comp), null) + (list(verdicts[0]), list(verdicts[1])))
    assert got[0] == got[1]
    r = d["ref"]
    assert got[0] == (r.mpk, r.n_qualified, r.phase4_error, [0] * 9, FIN_OK, -1, d["v"], d["dis"])


@pytest.mark.parametrize("fetched", [False, True])
@pytest.mark.parametrize("missing", ["E", "A", "s", "s_prime"])
def test_null_required_pointer(be, golden, fetched, missing):
    """A null E, A, s or s_prime is DKG_E_ARG, and the context serves the next call."""
    c = golden("fault_a_generator_n10_t4.json")
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    ones = bytes([1] * n)
    vals = [None if k == missing else H(c[k]) for k in ("E", "A", "s", "s_prime")]
    o, _bufs = be._ceremony_out(n, t, True)
    if fetched:
        rc = _lib.lib().dkg_ceremony_verify_fetched(be.ctx, n, t, *vals, ones, ones, ctypes.byref(o))
    else:
        rc = _lib.lib().dkg_ceremony_verify(be.ctx, n, t, *vals, ctypes.byref(o))
    assert rc == DKG_E_ARG
    good = [H(c[k]) for k in ("E", "A", "s", "s_prime")]
    r = be.ceremony_verify_fetched(*good, ones, ones, n, t) if fetched else be.ceremony_verify(*good, n, t)
    _check_ceremony(c, r, n)


def no_times(x):
    if isinstance(x, CeremonyResult):
        return dataclasses.replace(x, ms=None)
    if isinstance(x, ProvenResult):
        return dataclasses.replace(x, result=no_times(x.result))
    if isinstance(x, tuple):
        return tuple(no_times(v) for v in x)
    return x


def test_entry_points_share_one_context(be, amany, full):
    """The six verify entry points one after the other on one context, then in reverse order: every one
    returns what it returned before (no device buffer of one call is another's under the same name)."""
    c, comp = amany
    d = full
    n, t = c["n"], c["t"]
    assert (d["n"], d["t"]) == (n, t)
    be.env_init(t, n, CK)
    plain = tuple(H(c[k]) for k in ("E", "A", "s", "s_prime"))
    ones, f3 = bytes([1] * n), bytes([int(i != 2) for i in range(n)])
    calls = [
        lambda: be.ceremony_verify(*plain, n, t),
        lambda: be.ceremony_verify_fetched(*plain, ones, f3, n, t),
        lambda: be.ceremony_verify_full(*d["args"][:5], n, t),
        lambda: be.ceremony_verify_full_complaints(*d["args"], d["accuser"], d["accused"], d["proof"], n, t),
        lambda: be.ceremony_verify_fetched_proven(*plain, ones, f3, *lists(comp), n, t),
        lambda: be.ceremony_verify_full_proven(*d["args"], d["accuser"], d["accused"], d["proof"],
                                               *lists(d["comp"]), n, t),
    ]
    first = [no_times(f()) for f in calls]
    again = [no_times(f()) for f in reversed(calls)][::-1]
    for k, (x, y) in enumerate(zip(first, again)):
        assert x == y, k
    _check_ceremony(c, first[0], n)
    assert no_times(first[3]) == no_times((d["ref"], d["v"], d["dis"]))
