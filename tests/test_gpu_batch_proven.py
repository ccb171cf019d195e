"""Batches of ceremonies that decide by the PROVEN complaints: dkg_ceremony_batch_verify_proven and
dkg_ceremony_batch_verify_full_proven, with the complaint stage on the device.

The reference is the single-ceremony call (ceremony_verify_fetched_proven / ceremony_verify_full_proven,
pinned by tests/test_gpu_complaints*.py and tests/test_gpu_ceremony_proven.py) on each ceremony's
slices and its own complaints in their relative order; every comparison is bit-exact.  Tests 1 and 4
also check each verdict 0-3 against the CPU oracle's per-complaint verification.
"""
import ctypes
import dataclasses

import pytest

import dkg_amd
from dkg_amd import COMPLAINT_IGNORED, COMPLAINT_NO_PHASE3, MISSING, _lib
from dkg_amd import api
from dkg_amd import broadcast as BC
from dkg_amd._lib import DKG_E_ARG, DKG_OK, FIN_OK, FIN_PANIC, FIN_PHASE4_ERROR
from tests import oracle_lib as O
from tests.test_gpu_complaints import enc_of, fixture_inputs, row

gpu = pytest.mark.gpu

H = bytes.fromhex
L = 2**252 + 27742317777372353535851937790883648493
CK = b"Example of a shared string."
ZERO = bytes(32)
N10, T4 = 10, 4
BATCH_FIELDS = ("mpk", "n_qualified", "phase4_error", "qualified", "r2_error", "r4_error", "complaints2",
                "reconstruct", "final_share", "public_share", "dec2", "dec4")


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.set_batch_full_chunk(0)
    b.close()


def sc(v):
    return (v % L).to_bytes(32, "little")


def bump(x):
    return sc(int.from_bytes(x, "little") + 1)


def pair(s, sp, n, i, q):
    k = 32 * (i * n + q)
    return s[k:k + 32], sp[k:k + 32]


# ---------------- ceremonies and their complaints ----------------
# A ceremony is a dict: n, t, the call's arrays, c2 = [(accuser, accused, proof)] (full mode) and
# c4 = [(accuser, accused, share, randomness)], fetched1 / fetched3 (None = all present).
def interleave(cers, key):
    """The ceremonies' complaints round-robin: [(ceremony, complaint)], each ceremony's in their order."""
    out, k = [], 0
    while any(k < len(c[key]) for c in cers):
        out += [(g, c[key][k]) for g, c in enumerate(cers) if k < len(c[key])]
        k += 1
    return out


def cat(cers, key):
    return b"".join(c[key] for c in cers)


def masks(cers, key):
    if all(c.get(key) is None for c in cers):
        return None
    return b"".join(c.get(key) or bytes([1] * c["n"]) for c in cers)


def single_full(be, c):
    c2, c4 = c["c2"], c["c4"]
    return be.ceremony_verify_full_proven(
        c["E"], c["A"], c["e1"], c["ct"], c["sk"], c["pk"], [x[0] for x in c2], [x[1] for x in c2],
        b"".join(x[2] for x in c2), [x[0] for x in c4], [x[1] for x in c4], b"".join(x[2] for x in c4),
        b"".join(x[3] for x in c4), c["n"], c["t"], fetched3=c.get("fetched3"))


def single_plain(be, c):
    n, c4 = c["n"], c["c4"]
    ones = bytes([1] * n)
    return be.ceremony_verify_fetched_proven(
        c["E"], c["A"], c["s"], c["s_prime"], c.get("fetched1") or ones, c.get("fetched3") or ones,
        [x[0] for x in c4], [x[1] for x in c4], b"".join(x[2] for x in c4), b"".join(x[3] for x in c4), n, c["t"])


def full_args(cers):
    n, t = cers[0]["n"], cers[0]["t"]
    i2, i4 = interleave(cers, "c2"), interleave(cers, "c4")
    return dict(B=len(cers), n=n, t=t, E=cat(cers, "E"), A=cat(cers, "A"), e1=cat(cers, "e1"), ct=cat(cers, "ct"),
                sk=cat(cers, "sk"), pk=cat(cers, "pk"), ceremony=[g for g, _ in i2], accusers=[x[0] for _, x in i2],
                accused=[x[1] for _, x in i2], proofs=b"".join(x[2] for _, x in i2), ceremony4=[g for g, _ in i4],
                accusers4=[x[0] for _, x in i4], accused4=[x[1] for _, x in i4],
                share4=b"".join(x[2] for _, x in i4), randomness4=b"".join(x[3] for _, x in i4),
                fetched3=masks(cers, "fetched3"))


def plain_args(cers):
    n, t = cers[0]["n"], cers[0]["t"]
    i4 = interleave(cers, "c4")
    return dict(B=len(cers), n=n, t=t, E=cat(cers, "E"), A=cat(cers, "A"), s=cat(cers, "s"),
                s_prime=cat(cers, "s_prime"), ceremony4=[g for g, _ in i4], accusers4=[x[0] for _, x in i4],
                accused4=[x[1] for _, x in i4], share4=b"".join(x[2] for _, x in i4),
                randomness4=b"".join(x[3] for _, x in i4), fetched1=masks(cers, "fetched1"),
                fetched3=masks(cers, "fetched3"))


def same_as_single(d, p, full):
    """One ceremony's view of a BatchProvenResult against the single call's ProvenResult."""
    r = p.result
    assert d["mpk"] == r.mpk and d["n_qualified"] == r.n_qualified and d["phase4_error"] == r.phase4_error
    for k in ("qualified", "r2_error", "r4_error", "complaints2", "reconstruct"):
        assert list(d[k]) == getattr(r, k), k
    for k in ("final_share", "public_share", "dec2", "dec4"):
        assert d[k] == bytes(getattr(r, k)), k
    assert d["verdict4"] == p.verdict4
    assert (d["finalise_status"], d["recovery_index"]) == (p.finalise_status, p.recovery_index)
    if full:
        assert d["verdict"] == p.verdict and d["dissent"] == p.dissent
        assert d["s"] == r.s and d["s_prime"] == r.s_prime


def no_times(r):
    return dataclasses.replace(r, result=dataclasses.replace(r.result, ms=None, complaints2=list(r.result.complaints2)))


def oracle2(h, c, verdicts):
    """Each round-1 verdict 0-3 of ceremony c against the oracle's MisbehavingPartiesRound1::verify."""
    n, t = c["n"], c["t"]
    for (q, i, proof), v in zip(c["c2"], verdicts):
        if 0 <= v <= 3:
            assert O.complaint1_verify(h, t, q, c["pk"][32 * (q - 1):32 * q], enc_of(c["e1"], c["ct"], n, i - 1, q - 1),
                                       row(c["E"], t + 1, i - 1), proof) == v, (q, i)


def oracle4(h, c, verdicts):
    t = c["t"]
    for (q, i, sh, rn), v in zip(c["c4"], verdicts):
        if 0 <= v <= 3:
            assert O.complaint3_verify(h, t, q, sh, rn, row(c["E"], t + 1, i - 1), row(c["A"], t + 1, i - 1)) == v, (q, i)


def golden_full(golden, name):
    f = golden(name)
    return dict(n=f["n"], t=f["t"], E=H(f["E"]), A=H(f["A"]), e1=H(f["e1"]), ct=H(f["ct"]), sk=H(f["member_sk"]),
                pk=H(f["member_pk"]), c2=[], c4=[])


def faulted_ceremony(golden):
    """full_faults_n10_t4 (three round-2 faults) with dealer 2's A_20 replaced, its five round-1 complaints
    (verdicts 0, 0, 0, 2, 1) and the nine honest round-4 complaints against dealer 2 -- the `full` fixture
    of tests/test_gpu_ceremony_proven.py, built on the host from the golden's decrypted shares."""
    c, f, _, _, proof, _ = fixture_inputs(golden)
    cer = golden_full(golden, c["source"])
    n, N = cer["n"], cer["t"] + 1
    A = bytearray(cer["A"])
    A[32 * N:32 * N + 32] = O.base_mul(sc(321))
    cer["A"] = bytes(A)
    cer["c2"] = [(x["accuser"], x["accused"], proof[192 * b:192 * b + 192]) for b, x in enumerate(c["round1"])]
    s, sp = H(f["s"]), H(f["s_prime"])
    cer["c4"] = [(j + 1, 2) + pair(s, sp, n, 1, j) for j in range(n) if j != 1]
    cer["shares"] = (s, sp)
    return cer


def stacked(golden, bad_e1=b"\xff" * 32):
    """Test 1's four ceremonies."""
    n = N10
    c0 = golden_full(golden, "full_n10_t4.json")
    c1 = faulted_ceremony(golden)
    s, sp = c1.pop("shares")
    valid = c1["c4"]
    q, i, sh, rn = valid[0]
    # one valid complaint twice; a forged one (wrong share, FalseClaimedEquality) against the same dealer
    c1["c4"] = valid[:4] + [valid[2]] + [(q, i, bump(sh), rn)] + valid[4:]
    c2 = dict(c1)
    # forged only: a wrong share, and an honest pair (FalseClaimedInequality): dealer 2 stays a final party
    c2["c4"] = [(q, i, bump(sh), rn), (4, 5) + pair(s, sp, n, 4, 3)]
    c3 = golden_full(golden, "full_n10_t4.json")
    k = 2 * (5 * n + 3)  # dealer 6 -> receiver 4, the randomness: e1 does not decode
    c3["e1"] = c3["e1"][:32 * k] + bad_e1 + c3["e1"][32 * k + 32:]
    c3["c4"] = [(2, 6, sc(11), sc(12))]  # against the dealer with missing data: ignored
    return [c0, c1, c2, c3]


@pytest.fixture(scope="module")
def stack(be, golden):
    """Test 1's ceremonies, the single calls on each, and the batch call."""
    cers = stacked(golden)
    h = be.env_init(T4, N10, CK)
    assert be.points_valid(b"\xff" * 32) == b"\x00"
    singles = [single_full(be, c) for c in cers]
    args = full_args(cers)
    r = dkg_amd.ceremony_batch_verify_full_proven(be, **args)
    return dict(cers=cers, h=h, singles=singles, args=args, r=r)


# ---------------- 1. stacked goldens, full mode ----------------
@gpu
def test_stacked_goldens_full(be, golden, stack):
    cers, singles, r, args = stack["cers"], stack["singles"], stack["r"], stack["args"]
    n = N10
    # the complaints are interleaved, not grouped
    assert args["ceremony"][:2] == [1, 2] and args["ceremony4"][:3] == [1, 2, 3]
    # what the single calls say about these ceremonies
    assert singles[1].verdict == [0, 0, 0, 2, 1] and singles[1].verdict4 == [0] * 5 + [3] + [0] * 5
    assert singles[1].result.reconstruct == [int(i == 1) for i in range(n)]
    assert singles[2].verdict4 == [3, 2] and singles[2].result.reconstruct == [0] * n
    assert singles[2].result.mpk != singles[1].result.mpk
    assert singles[3].verdict4 == [COMPLAINT_IGNORED] and singles[3].result.qualified == [int(i != 5) for i in range(n)]
    assert MISSING in singles[3].result.dec2
    assert singles[0].result.mpk.hex() == golden("full_n10_t4.json")["mpk"]
    for c in range(4):
        same_as_single(r.ceremony(c), singles[c], True)
        oracle2(stack["h"], cers[c], r.ceremony(c)["verdict"])
        oracle4(stack["h"], cers[c], r.ceremony(c)["verdict4"])
    assert r.finalise_status == [FIN_OK] * 4 and r.recovery_index == [-1] * 4


# ---------------- 2. chunk independence ----------------
@gpu
def test_chunk_independence(be, stack):
    be.env_init(T4, N10, CK)
    want = no_times(stack["r"])
    try:
        for chunk in (1, 2, 0):
            be.set_batch_full_chunk(chunk)
            assert no_times(dkg_amd.ceremony_batch_verify_full_proven(be, **stack["args"])) == want, chunk
    finally:
        be.set_batch_full_chunk(0)


# ---------------- 3. plaintext variant ----------------
def golden_plain(golden, name):
    c = golden(name)
    return dict(n=c["n"], t=c["t"], E=H(c["E"]), A=H(c["A"]), s=H(c["s"]), s_prime=H(c["s_prime"]), c4=[])


def rejections(c, golden_c, skip=()):
    """One complaint per round-4 rejection the golden records, with the pair the receiver holds."""
    n = c["n"]
    return [(j + 1, i + 1) + pair(c["s"], c["s_prime"], n, i, j) for i in range(n) for j in range(n)
            if golden_c["dec4"][i * n + j] == "0" and i not in skip]


@gpu
def test_plaintext_variant(be, golden):
    n, t = N10, T4
    be.env_init(t, n, CK)
    names = ["fault_a_generator_n10_t4.json", "fault_a_many_n10_t4.json", "fault_recon_only_n10_t4.json",
             "fault_a_generator_n10_t4.json"]
    cers = [golden_plain(golden, x) for x in names]
    for c, x in zip(cers, names):
        c["c4"] = rejections(c, golden(x))
        assert c["c4"]
    # ceremony 0: dealer 9's share to receiver 2 is wrong, round 2 disqualifies it; a complaint against it
    s = bytearray(cers[0]["s"])
    k = 32 * (8 * n + 1)
    s[k:k + 32] = bump(bytes(s[k:k + 32]))
    cers[0]["s"] = bytes(s)
    cers[0]["c4"].append((4, 9) + pair(cers[0]["s"], cers[0]["s_prime"], n, 8, 3))
    # ceremony 1: dealer 4's phase-1 broadcast was not fetched
    cers[1]["fetched1"] = bytes([int(i != 3) for i in range(n)])
    # ceremony 2: dealer 1 has no phase-3 broadcast and one complaint, whatever it carries
    cers[2]["fetched3"] = bytes([int(i != 0) for i in range(n)])
    cers[2]["c4"].insert(1, (7, 1, sc(12345), sc(67890)))
    # ceremony 3: dealer 3 has no phase-3 broadcast and nobody complains about it
    cers[3]["fetched3"] = bytes([int(i != 2) for i in range(n)])
    singles = [single_plain(be, c) for c in cers]
    assert singles[0].verdict4[-1] == COMPLAINT_IGNORED and singles[0].finalise_status == FIN_OK
    assert singles[1].finalise_status == FIN_PHASE4_ERROR and singles[1].result.qualified[3] == 0
    assert singles[2].verdict4[1] == COMPLAINT_NO_PHASE3 and singles[2].result.reconstruct[0] == 1
    assert (singles[3].finalise_status, singles[3].recovery_index) == (FIN_PANIC, 2)
    r = dkg_amd.ceremony_batch_verify_proven(be, **plain_args(cers))
    for c in range(4):
        same_as_single(r.ceremony(c), singles[c], False)
    assert r.finalise_status == [FIN_OK, FIN_PHASE4_ERROR, FIN_OK, FIN_PANIC] and r.recovery_index == [-1, -1, -1, 2]
    # only the panicking ceremony's key is zeroed (and the one nobody finalises)
    assert r.result.mpk[3] == ZERO and r.result.mpk[1] == ZERO and ZERO not in (r.result.mpk[0], r.result.mpk[2])
    assert dkg_amd.lib().dkg_ctx_phase_ms(be.ctx, b"bproven.c4") >= 0
    assert dkg_amd.lib().dkg_ctx_phase_ms(be.ctx, b"bproven.c2") == -1.0
    # the other schedules of the rounds (protocol order, interpolation) report the usable phase-3
    # broadcasts from other flags: the same outcome, the panic included
    for switch, on, off in ((be.set_overlap, False, True), (be.set_verify_mode, 1, 0)):
        switch(on)
        try:
            assert no_times(dkg_amd.ceremony_batch_verify_proven(be, **plain_args(cers))) == no_times(r)
        finally:
            switch(off)


# ---------------- 4. wave boundaries: n = 64, more than one wave of complaints ----------------
@pytest.fixture(scope="module")
def wave(be):
    n, t = 64, 31
    master = bytes(range(32))
    h = be.env_init(t, n, CK)
    cers = []
    for g in range(2):
        a, b = dkg_amd.dealer_coefficients(master, g, 0, n, t)
        E, A, s, sp = be.share_gen(a, b, n, n, t)
        sk, pk = be.member_keys(master, g, n)
        cers.append(dict(n=n, t=t, E=E, A=A, s=s, s_prime=sp, sk=sk, pk=pk, c2=[], c4=[]))
    # ceremony 0: dealer 11 encrypts wrong shares to all 63 others
    d0 = 10
    s2 = bytearray(cers[0]["s"])
    for q in range(n):
        if q != d0:
            k = 32 * (d0 * n + q)
            s2[k:k + 32] = bump(bytes(s2[k:k + 32]))
    sent = [bytes(s2), cers[1]["s"]]
    for g, c in enumerate(cers):
        c["e1"], c["ct"] = be.encrypt_shares(c["pk"], sent[g], c["s_prime"], dkg_amd.enc_randomness(master, g, 0, n, n, t),
                                             n, n)

    def prove(c, pairs, seed):
        """dkg_complaints_prove for (accuser q, accused i) pairs of ceremony c, 0-based."""
        sks = b"".join(c["sk"][32 * q:32 * q + 32] for q, _ in pairs)
        enc = b"".join(enc_of(c["e1"], c["ct"], n, i, q) for q, i in pairs)
        w = b"".join(sc(seed + 2 * k) + sc(seed + 2 * k + 1) for k in range(len(pairs)))
        proofs = be.complaints_prove(sks, enc, w)
        return [(q + 1, i + 1, proofs[192 * k:192 * k + 192]) for k, (q, i) in enumerate(pairs)]

    cers[0]["c2"] = prove(cers[0], [(q, d0) for q in range(n) if q != d0], 1000)
    # forged: honest pairs (FalseClaimedInequality), one by accuser 64, and a tampered response (invalid proof)
    cers[0]["c2"].insert(5, prove(cers[0], [(63, 1)], 5000)[0])
    f1, f2 = prove(cers[1], [(2, 4), (63, 20)], 6000)
    f2 = f2[:2] + (f2[2][:160] + bump(f2[2][160:192]),)
    cers[1]["c2"] = [f1, f2]
    # ceremony 1: dealer 31's A_0 is wrong, every other receiver's round-4 check fails
    d1, N = 30, t + 1
    A = bytearray(cers[1]["A"])
    A[32 * N * d1:32 * N * d1 + 32] = O.base_mul(sc(777))
    cers[1]["A"] = bytes(A)
    cers[1]["c4"] = [(q + 1, d1 + 1) + pair(cers[1]["s"], cers[1]["s_prime"], n, d1, q) for q in range(n) if q != d1]
    # forged: an honest pair (2) and wrong shares (3), spread over both ceremonies, accuser 64 among them
    sh, rn = pair(sent[0], cers[0]["s_prime"], n, 6, 63)
    cers[0]["c4"] = [(64, 7, sh, rn)]
    sh, rn = pair(sent[0], cers[0]["s_prime"], n, 8, 4)
    cers[0]["c4"].append((5, 9, bump(sh), rn))
    sh, rn = pair(cers[1]["s"], cers[1]["s_prime"], n, 2, 63)
    cers[1]["c4"].insert(40, (64, 3, bump(sh), rn))
    return h, cers


@gpu
def test_wave_boundaries(be, wave):
    h, cers = wave
    n, t = 64, 31
    be.env_init(t, n, CK)
    args = full_args(cers)
    assert len(args["accusers"]) >= 65 and len(args["accusers4"]) >= 65
    assert 64 in args["accusers"] and 64 in args["accusers4"]
    assert args["ceremony"][:4] == [0, 1, 0, 1] and args["ceremony4"][:4] == [0, 1, 0, 1]
    singles = [single_full(be, c) for c in cers]
    assert singles[0].verdict == [0] * 5 + [2] + [0] * 58 and singles[1].verdict == [2, 1]
    assert singles[0].verdict4 == [2, 3] and singles[1].verdict4 == [0] * 40 + [3] + [0] * 23
    assert singles[0].result.qualified == [int(i != 10) for i in range(n)]
    assert singles[1].result.reconstruct == [int(i == 30) for i in range(n)]
    r = dkg_amd.ceremony_batch_verify_full_proven(be, **args)
    for c in range(2):
        same_as_single(r.ceremony(c), singles[c], True)
        oracle2(h, cers[c], r.ceremony(c)["verdict"])
        oracle4(h, cers[c], r.ceremony(c)["verdict4"])


# ---------------- 5. no complaints ----------------
def u32s(xs):
    return (ctypes.c_uint32 * max(len(xs), 1))(*xs)


def raw_full(be, a, **over):
    """dkg_ceremony_batch_verify_full_proven through the C ABI with full_args' dictionary; `over` replaces
    C-level arguments (None = a null pointer).  Returns (rc, BatchProvenResult or None)."""
    a = dict(a)
    B, n, t = a["B"], a["n"], a["t"]
    C, C4 = len(a["accusers"]), len(a["accusers4"])
    o, bufs = api._batch_out(B, n, True)
    size = 32 * B * n * n
    s, sp = ctypes.create_string_buffer(max(size, 1)), ctypes.create_string_buffer(max(size, 1))
    i32 = ctypes.c_int32
    c = dict(E=a["E"], A=a["A"], e1=a["e1"], ct=a["ct"], sk=a["sk"], pk=a["pk"], C=C, ceremony=u32s(a["ceremony"]),
             accuser=u32s(a["accusers"]), accused=u32s(a["accused"]), proofs=a["proofs"], fetched3=a["fetched3"], C4=C4,
             ceremony4=u32s(a["ceremony4"]), accuser4=u32s(a["accusers4"]), accused4=u32s(a["accused4"]),
             share4=a["share4"], randomness4=a["randomness4"], verdict=(i32 * max(C, 1))(),
             dissent=(i32 * max(B * n, 1))(), verdict4=(i32 * max(C4, 1))(), status=(i32 * max(B, 1))(),
             index=(i32 * max(B, 1))(), s_out=s, s_prime_out=sp)
    c.update(over)
    rc = _lib.lib().dkg_ceremony_batch_verify_full_proven(
        be.ctx, B, n, t, c["E"], c["A"], c["e1"], c["ct"], c["sk"], c["pk"], c["C"], c["ceremony"], c["accuser"],
        c["accused"], c["proofs"], c["fetched3"], c["C4"], c["ceremony4"], c["accuser4"], c["accused4"], c["share4"],
        c["randomness4"], ctypes.byref(o), c["s_out"], c["s_prime_out"], c["verdict"], c["dissent"], c["verdict4"],
        c["status"], c["index"])
    if rc != DKG_OK or B == 0:
        return rc, None
    r = api._batch_result(B, n, t, o, bufs)
    r.s, r.s_prime = (x and x.raw[:size] for x in (c["s_out"], c["s_prime_out"]))
    return rc, api.BatchProvenResult(r, a["ceremony4"][:c["C4"]], list(c["verdict4"] or [])[:c["C4"]],
                                     list(c["status"] or [])[:B], list(c["index"] or [])[:B], a["ceremony"][:c["C"]],
                                     list(c["verdict"] or [])[:c["C"]], list(c["dissent"] or [])[:B * n])


def raw_plain(be, a, **over):
    """dkg_ceremony_batch_verify_proven through the C ABI with plain_args' dictionary, as raw_full."""
    B, n, t, C4 = a["B"], a["n"], a["t"], len(a["accusers4"])
    o, bufs = api._batch_out(B, n, True)
    i32 = ctypes.c_int32
    c = dict(E=a["E"], A=a["A"], s=a["s"], s_prime=a["s_prime"], fetched1=a["fetched1"], fetched3=a["fetched3"], C4=C4,
             ceremony4=u32s(a["ceremony4"]), accuser4=u32s(a["accusers4"]), accused4=u32s(a["accused4"]),
             share4=a["share4"], randomness4=a["randomness4"], verdict4=(i32 * max(C4, 1))(),
             status=(i32 * max(B, 1))(), index=(i32 * max(B, 1))())
    c.update(over)
    rc = _lib.lib().dkg_ceremony_batch_verify_proven(
        be.ctx, B, n, t, c["E"], c["A"], c["s"], c["s_prime"], c["fetched1"], c["fetched3"], c["C4"], c["ceremony4"],
        c["accuser4"], c["accused4"], c["share4"], c["randomness4"], ctypes.byref(o), c["verdict4"], c["status"],
        c["index"])
    if rc != DKG_OK or B == 0:
        return rc, None
    return rc, api.BatchProvenResult(api._batch_result(B, n, t, o, bufs), a["ceremony4"][:c["C4"]],
                                     list(c["verdict4"] or [])[:c["C4"]], list(c["status"] or [])[:B],
                                     list(c["index"] or [])[:B])


@gpu
def test_empty(be, stack):
    n, t = N10, T4
    be.env_init(t, n, CK)
    cers = [dict(c, c2=[], c4=[]) for c in stack["cers"]]
    singles = [single_full(be, c) for c in cers]
    null = dict(C=0, ceremony=None, accuser=None, accused=None, proofs=None, verdict=None, C4=0, ceremony4=None,
                accuser4=None, accused4=None, share4=None, randomness4=None, verdict4=None)
    rc, r = raw_full(be, full_args(cers), **null)
    assert rc == DKG_OK
    for c in range(4):
        same_as_single(r.ceremony(c), singles[c], True)
    # no complaint disqualifies nobody but the rows with missing data, and reconstructs nobody
    assert r.result.qualified == bytes([1] * 35 + [0] + [1] * 4) and r.result.reconstruct == bytes(4 * n)
    # the rejection rule decides ceremony 1 otherwise
    a = stack["args"]
    old = dkg_amd.ceremony_batch_verify_full(be, 4, n, t, a["E"], a["A"], a["e1"], a["ct"], a["sk"])
    assert old.ceremony(1)["qualified"] == [1, 1, 0, 1, 1, 0, 1, 1, 0, 1] != r.ceremony(1)["qualified"]
    assert old.ceremony(1)["reconstruct"] == [int(i == 1) for i in range(n)] != r.ceremony(1)["reconstruct"]
    assert old.mpk[1] != r.result.mpk[1] and old.mpk[0] == r.result.mpk[0]
    # B = 0
    empty = dict(full_args(cers), B=0)
    assert raw_full(be, empty, **null)[0] == DKG_OK
    o, _bufs = api._batch_out(0, n, True)
    assert _lib.lib().dkg_ceremony_batch_verify_proven(be.ctx, 0, n, t, b"", b"", b"", b"", None, None, 0, None, None,
                                                       None, None, None, ctypes.byref(o), None, None, None) == DKG_OK


# ---------------- 6. arguments ----------------
@gpu
def test_arguments(be, stack):
    n, t = N10, T4
    be.env_init(t, n, CK)
    a = stack["args"]
    C, C4 = len(a["accusers"]), len(a["accusers4"])

    def with_entry(key, k, v):
        xs = list(a[key])
        xs[k] = v
        return u32s(xs)

    bad = [dict(ceremony=with_entry("ceremony", C - 1, 4)), dict(ceremony4=with_entry("ceremony4", 0, 4)),
           dict(accuser=with_entry("accusers", 2, 0)), dict(accuser4=with_entry("accusers4", C4 - 1, 0)),
           dict(accused=with_entry("accused", 0, n + 1)), dict(accused4=with_entry("accused4", 3, n + 1)),
           dict(proofs=None), dict(E=None)]
    for over in bad:
        assert raw_full(be, a, **over)[0] == DKG_E_ARG, sorted(over)
    # the context serves the next call
    rc, r = raw_full(be, a)
    assert rc == DKG_OK and no_times(r) == no_times(stack["r"])


# ---------------- 7. one context ----------------
@gpu
def test_one_context(be, stack):
    be.env_init(T4, N10, CK)
    first = dkg_amd.ceremony_batch_verify_full_proven(be, **stack["args"])
    one = single_full(be, stack["cers"][1])
    third = dkg_amd.ceremony_batch_verify_full_proven(be, **stack["args"])
    assert no_times(first) == no_times(third) == no_times(stack["r"])
    ref = stack["singles"][1]
    assert dataclasses.replace(one, result=dataclasses.replace(one.result, ms=None)) == \
        dataclasses.replace(ref, result=dataclasses.replace(ref.result, ms=None))


# ---------------- 8. wire bytes ----------------
def broadcasts(c):
    """Ceremony c's serialised phase-1 .. phase-4 broadcasts, parsed back."""
    n, N = c["n"], c["t"] + 1
    E, A, e1, ct = c["E"], c["A"], c["e1"], c["ct"]

    def hybrid(i, q, w):
        k = 32 * (2 * (i * n + q) + w)
        return e1[k:k + 32] + ct[k:k + 32]

    p1 = [BC.BroadcastPhase1([E[32 * (N * i + k):32 * (N * i + k + 1)] for k in range(N)],
                             [BC.EncryptedShares(q + 1, hybrid(i, q, 1), hybrid(i, q, 0)) for q in range(n)])
          for i in range(n)]
    p3 = [BC.BroadcastPhase3([A[32 * (N * i + k):32 * (N * i + k + 1)] for k in range(N)]) for i in range(n)]
    p2, p4 = [None] * n, [None] * n
    for q, i, proof in c["c2"]:
        m = BC.MisbehavingPartiesRound1(i, 0, hybrid(i - 1, q - 1, 0) + hybrid(i - 1, q - 1, 1), proof)
        p2[q - 1] = BC.BroadcastPhase2((p2[q - 1].misbehaving_parties if p2[q - 1] else []) + [m])
    for q, i, sh, rn in c["c4"]:
        m = BC.MisbehavingPartiesRound3(i, sh, rn)
        p4[q - 1] = BC.BroadcastPhase4((p4[q - 1].misbehaving_parties if p4[q - 1] else []) + [m])

    def wire(cls, msgs):
        return [None if m is None else cls.from_bytes(m.to_bytes()) for m in msgs]

    return (wire(BC.BroadcastPhase1, p1), wire(BC.BroadcastPhase3, p3), wire(BC.BroadcastPhase4, p4),
            wire(BC.BroadcastPhase2, p2))


def by_sender(c):
    """Ceremony c with its complaints in broadcast order (by sender, each sender's in their order)."""
    return dict(c, c2=sorted(c["c2"], key=lambda x: x[0]), c4=sorted(c["c4"], key=lambda x: x[0]))


def wire_case(golden):
    cers = [by_sender(c) for c in stacked(golden)[1:3]]
    msgs = [broadcasts(c) for c in cers]
    got = BC.batch_proven_arguments(N10, T4, *([m[k] for m in msgs] for k in range(4)), sk=[c["sk"] for c in cers],
                                    pk=[c["pk"] for c in cers])
    return cers, msgs, got


def test_wire_arguments(golden):
    """The helper's call arguments from serialised broadcasts are the ceremonies' own, grouped by ceremony."""
    cers, _, got = wire_case(golden)
    want = full_args(cers)
    for key, lst in (("c2", ("ceremony", "accusers", "accused")), ("c4", ("ceremony4", "accusers4", "accused4"))):
        flat = [(g, x) for g, c in enumerate(cers) for x in c[key]]
        want[lst[0]] = [g for g, _ in flat]
        want[lst[1]] = [x[0] for _, x in flat]
        want[lst[2]] = [x[1] for _, x in flat]
        if key == "c2":
            want["proofs"] = b"".join(x[2] for _, x in flat)
        else:
            want["share4"] = b"".join(x[2] for _, x in flat)
            want["randomness4"] = b"".join(x[3] for _, x in flat)
    want["fetched3"] = bytes([1] * 2 * N10)
    assert got == want
    assert len(got["accusers"]) == 10 and len(got["accusers4"]) == 13


@gpu
def test_wire_call(be, golden):
    cers, msgs, got = wire_case(golden)
    be.env_init(T4, N10, CK)
    r = BC.verify_broadcasts_batch_proven(be, N10, T4, *([m[k] for m in msgs] for k in range(4)),
                                          sk=[c["sk"] for c in cers], pk=[c["pk"] for c in cers])
    assert no_times(r) == no_times(dkg_amd.ceremony_batch_verify_full_proven(be, **got))
    for g, c in enumerate(cers):
        same_as_single(r.ceremony(g), single_full(be, c), True)
    assert sorted(r.ceremony(0)["verdict"]) == [0, 0, 0, 1, 2] and r.ceremony(1)["verdict4"] == [3, 2]


# ---------------- 9. the four verify entry points behind one driver ----------------
def stripped(r):
    """A BatchResult or BatchProvenResult without its times."""
    if isinstance(r, api.BatchProvenResult):
        return no_times(r)
    return dataclasses.replace(r, ms=None, complaints2=list(r.complaints2))


def stack_plain_args(stack):
    """The stack as a plaintext batch: the shares its full-mode call decrypted, the round-4 complaints."""
    a, r = stack["args"], stack["r"].result
    return dict({k: a[k] for k in ("B", "n", "t", "E", "A", "ceremony4", "accusers4", "accused4", "share4",
                                   "randomness4", "fetched3")}, s=r.s, s_prime=r.s_prime, fetched1=None)


def four_calls(stack):
    """[(name, call(backend))]: dkg_ceremony_batch_verify, _full, _proven, _full_proven on the stack's inputs."""
    a, p = stack["args"], stack_plain_args(stack)
    shape = (a["B"], a["n"], a["t"], a["E"], a["A"])
    return [("verify", lambda b: dkg_amd.ceremony_batch_verify(b, *shape, p["s"], p["s_prime"])),
            ("verify_full", lambda b: dkg_amd.ceremony_batch_verify_full(b, *shape, a["e1"], a["ct"], a["sk"])),
            ("verify_proven", lambda b: dkg_amd.ceremony_batch_verify_proven(b, **p)),
            ("verify_full_proven", lambda b: dkg_amd.ceremony_batch_verify_full_proven(b, **a))]


@pytest.fixture(scope="module")
def four_refs(stack):
    """Each of the four calls on a context that has served nothing else."""
    fresh = dkg_amd.Backend(0)
    try:
        fresh.env_init(T4, N10, CK)
        return {name: stripped(call(fresh)) for name, call in four_calls(stack)}
    finally:
        fresh.close()


@gpu
def test_four_entry_points_one_context(be, stack, four_refs):
    be.env_init(T4, N10, CK)
    calls = four_calls(stack)
    got = {}
    for name, call in calls + calls[::-1]:
        got[name] = stripped(call(be))
        assert got[name] == four_refs[name], name
    assert got["verify_full_proven"] == no_times(stack["r"])
    p = stack_plain_args(stack)
    sz = 32 * N10 * N10
    for c, cer in enumerate(stack["cers"]):
        same_as_single(got["verify_full_proven"].ceremony(c), stack["singles"][c], True)
        one = dict(cer, s=p["s"][sz * c:sz * (c + 1)], s_prime=p["s_prime"][sz * c:sz * (c + 1)])
        same_as_single(got["verify_proven"].ceremony(c), single_plain(be, one), False)


# ---------------- 10. the announcement buffers, shared by one ceremony's and the batch's complaints ----------------
def more_complaints(cer, times):
    """complaints_verify's arguments for ceremony `cer` with its round-1 complaints listed `times` times."""
    n, c2 = cer["n"], cer["c2"] * times
    return dict(n=n, t=cer["t"], accusers=[x[0] for x in c2], accused=[x[1] for x in c2], pk=cer["pk"], E=cer["E"],
                enc=b"".join(enc_of(cer["e1"], cer["ct"], n, i - 1, q - 1) for q, i, _ in c2),
                proofs=b"".join(x[2] for x in c2))


@gpu
def test_shared_announcement_buffers(be, stack):
    cer, want = stack["cers"][1], no_times(stack["r"])
    C2 = len(stack["args"]["accusers"])
    own, more = more_complaints(cer, 1), more_complaints(cer, 3)
    # fewer than the batch's, and more: the buffers grow from either side
    assert len(own["accusers"]) < C2 < len(more["accusers"])
    verdicts = stack["singles"][1].verdict
    assert verdicts == [0, 0, 0, 2, 1]
    proven = {i for (_, i, _), v in zip(cer["c2"], verdicts) if v == 0}
    qualified = [int(i + 1 not in proven) for i in range(N10)]  # every row decodes
    assert sum(qualified) < N10

    def batch(b):
        assert no_times(dkg_amd.ceremony_batch_verify_full_proven(b, **stack["args"])) == want

    def single(b, a, times):
        assert b.complaints_verify(**a) == (verdicts * times, qualified)

    be.env_init(T4, N10, CK)
    batch(be)
    single(be, more, 3)
    batch(be)
    fresh = dkg_amd.Backend(0)
    try:
        fresh.env_init(T4, N10, CK)
        single(fresh, own, 1)
        batch(fresh)
        single(fresh, more, 3)
        batch(fresh)
        single(fresh, own, 1)
    finally:
        fresh.close()


# ---------------- 11. null optional outputs with complaints present ----------------
@gpu
def test_null_optional_outputs(be, stack):
    be.env_init(T4, N10, CK)
    a, want = stack["args"], no_times(stack["r"])
    assert a["accusers"] and a["accusers4"]
    rc, r = raw_full(be, a, dissent=None, status=None, index=None, s_out=None, s_prime_out=None)
    assert rc == DKG_OK
    assert (r.result.s, r.result.s_prime, r.dissent, r.finalise_status, r.recovery_index) == (None, None, [], [], [])
    r.result.s, r.result.s_prime = want.result.s, want.result.s_prime
    assert no_times(r) == dataclasses.replace(want, dissent=[], finalise_status=[], recovery_index=[])
    p = stack_plain_args(stack)
    rc, full = raw_plain(be, p)
    assert rc == DKG_OK and no_times(full) == no_times(dkg_amd.ceremony_batch_verify_proven(be, **p))
    rc, r = raw_plain(be, p, status=None, index=None)
    assert rc == DKG_OK
    assert no_times(r) == dataclasses.replace(no_times(full), finalise_status=[], recovery_index=[])


# ---------------- 12. required pointers of the four entry points ----------------
@gpu
def test_required_pointers(be, stack):
    n, t = N10, T4
    be.env_init(t, n, CK)
    a, p = stack["args"], stack_plain_args(stack)
    B = a["B"]
    L_ = _lib.lib()

    def verify(**over):
        c = dict(p, **over)
        o, _bufs = api._batch_out(B, n, True)
        return L_.dkg_ceremony_batch_verify(be.ctx, B, n, t, c["E"], c["A"], c["s"], c["s_prime"], ctypes.byref(o))

    def verify_full(**over):
        c = dict(a, **over)
        o, _bufs = api._batch_out(B, n, True)
        return L_.dkg_ceremony_batch_verify_full(be.ctx, B, n, t, c["E"], c["A"], c["e1"], c["ct"], c["sk"],
                                                 ctypes.byref(o), None, None)

    entries = [(verify, ("E", "A", "s", "s_prime")), (verify_full, ("E", "A", "e1", "ct", "sk")),
               (lambda **over: raw_plain(be, p, **over)[0], ("E", "A", "s", "s_prime")),
               (lambda **over: raw_full(be, a, **over)[0], ("E", "A", "e1", "ct", "sk", "pk"))]
    for call, required in entries:
        for key in required:
            assert call(**{key: None}) == DKG_E_ARG, (required, key)
        assert call() == DKG_OK, required  # the context serves a correct call afterwards
    rc, r = raw_full(be, a)
    assert rc == DKG_OK and no_times(r) == no_times(stack["r"])
    # an empty batch is done before its complaint arrays are looked at
    none4 = dict(ceremony4=None, accuser4=None, accused4=None, share4=None, randomness4=None, verdict4=None)
    none2 = dict(ceremony=None, accuser=None, accused=None, proofs=None, verdict=None)
    assert raw_full(be, dict(a, B=0), **none2, **none4)[0] == DKG_OK
    assert raw_plain(be, dict(p, B=0), **none4)[0] == DKG_OK
    # .. and only then: the same arrays with B > 0
    assert raw_full(be, a, **none2, **none4)[0] == DKG_E_ARG
    assert raw_plain(be, p, **none4)[0] == DKG_E_ARG
